"""Progressive distillation on the GPU (v_diffusion/distill.py over vd_distill_mid / vd_distill_loss_fwd / vd_distill_loss_bwd)
against the float64 restatement of tests/distill_ref.py.  Teacher and student of the kernel tests are pointwise stand-ins,
a(t) x + b(t) tanh(x) + g y, the same function in fp64 on the CPU and in fp32 on the GPU.  The yardstick for the kernels' error is
the same arithmetic as a plain fp32 torch composition on the GPU (convex form, same coefficient table): kernels and composition
differ in summation order and FMA contraction only, so the kernels may be at most 2x as far from fp64.  (Both assemble the residual
x_student - x_tilde from differences against z_t: see csrc/diffusion.hip.)  Needs an MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distill_ref as R                                           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {"75": (3, 3, 5, 5), "972": (2, 3, 18, 18)}            # C*HW = 75: odd, below one block; 972: above 256, no multiple of it
STEPS = (2, 1024)
REWEIGHTS = ("constant", "snr", "snr_trunc", "snr_1plus")
TYPE_PAIRS = (("v", "v"), ("eps", "v"), ("both", "x0"))          # (student, teacher)
W_GUIDE = 1.5
QUANTITIES = ("x_tilde", "loss", "dout")
# A single run's errors are often 1-2 ulp of the result, where the ratio of two fp32 evaluations is chance (measured: loss off by
# 1.4e-7 from the kernels and 3.2e-8 from the composition in one run, 8.0e-8 against 1.1e-7 in another).  The 2x bound is therefore
# asserted on the maxima over a parametrisation's runs; so that a regression in an easy run cannot hide under the hardest one, each
# run is ALSO held to 2x the composition plus 4 ulp (relative to the row's scale): both evaluations start from the same fp32 z_t,
# network outputs and coefficient table and end in one fp32 rounding, each worth up to half an ulp that the comparison cannot see.
FLOOR = 4 * 2.0 ** -24


@pytest.fixture(scope="module")
def vd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import v_diffusion
    from v_diffusion import _hip
    _hip.lib()
    return v_diffusion


class Stub:
    """pointwise stand-in network; ``extra`` (a leaf) is added to the output so that autograd delivers d loss / d output"""

    training = False

    def __init__(self, a, b, g, both=False, extra=None):
        self.a, self.b, self.g, self.both, self.extra = a, b, g, both, extra

    def __call__(self, x, t, y):
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        if self.both:
            out = torch.cat([out, 0.5 * out - 0.25 * x], dim=1)
        return out if self.extra is None else out + self.extra


def teacher_stub(out_type):
    return Stub((0.3, -0.5), (0.4, 0.3), 0.07, both=out_type == "both")


def student_stub(out_type, extra=None):
    return Stub((-0.2, 0.6), (0.5, -0.2), 0.03, both=out_type == "both", extra=extra)


def data(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(shape, generator=g, dtype=torch.float64).clamp(-1, 1).float()
    noise = torch.randn(shape, generator=g, dtype=torch.float64).float()
    y = torch.arange(1, shape[0] + 1, dtype=torch.float32)
    gw = (torch.rand(shape[0], generator=g, dtype=torch.float64) + 0.5).float()
    return x0, noise, y, gw


def step_sets(B, N):
    """per-sample step indices covering i = 1, i = N and an interior i (N = 2 has none)"""
    mid = 300 if N > 2 else 1
    return [[1, N, mid]] if B == 3 else [[1, N], [mid, N]]


def make_dd(vd, teacher, N, s, te, rw, w, clip):
    dd = vd.DistillationDiffusion(teacher, N, teacher_out_type=te, teacher_w_guide=w, clip_teacher=clip,
                                  logsnr_fn=vd.get_logsnr_schedule("cosine", -20.0, 20.0), model_out_type=s,
                                  model_var_type="fixed_large", reweight_type=rw)
    dd.keep_target = True
    return dd


def reference(coef, times, x0, noise, y, gw, s, te, rw, w, clip, D):
    """fp64 on the CPU: (x_tilde, loss, d (sum gw*loss) / d student output)"""
    l = coef[:, D.LOGSNR_T].cpu().double()
    tt, tm, tend = (v.cpu() for v in times)
    fn = __import__("v_diffusion").get_logsnr_schedule("cosine", -20.0, 20.0)
    ls = (l, fn(tm.clone()).float().double(), fn(tend.clone()).float().double())
    a, sg = R.alpha_sigma(R.col(l))
    z = a * x0.double() + sg * noise.double()
    yd = None if y is None else y.double()
    xt = R.target(teacher_stub(te), z, (tt, tm, tend), ls, yd, te, w, clip)
    extra = torch.zeros((x0.shape[0], (2 if s == "both" else 1) * x0.shape[1]) + tuple(x0.shape[2:]), dtype=torch.float64,
                        requires_grad=True)
    loss = R.loss(student_stub(s, extra)(z, tt, yd), z, xt, l, s, rw)
    (loss * gw.double()).sum().backward()
    return xt, loss.detach(), extra.grad, z, ls


def composition(coef, times, x0, noise, y, gw, s, te, cfg, clip, D):
    """the kernels' arithmetic as fp32 tensor ops on the GPU, from the same table: the target in the convex form, the residual from
    the difference forms (every prediction minus the state it was made from)"""
    k = lambda j: coef[:, j].reshape(-1, 1, 1, 1)
    tt, tm, _ = times
    l = k(D.LOGSNR_T)
    z = x0 * torch.sigmoid(l).sqrt() + noise * torch.sigmoid(-l).sqrt()
    C = x0.shape[1]

    def pred(out, zz, c0, m1, both, rep=lambda v: v):
        """(prediction, prediction - zz): the direct form and the difference form, weights from columns c0.. and m1"""
        tail = rep(k(c0 + 1)) * out[:, :C] + rep(k(c0 + 2)) * out[:, C:] if both else rep(k(c0 + 1)) * out
        return rep(k(c0)) * zz + tail, rep(k(m1)) * zz + tail

    def tpred(zz, tnet, c0, m1):
        rep = (lambda v: v.repeat_interleave(2, dim=0)) if cfg else (lambda v: v)
        y_in = y
        if cfg:
            y_in = rep(y).clone()
            y_in[1::2] = 0
        p, d = pred(teacher_stub(te)(rep(zz), rep(tnet), y_in), rep(zz), c0, m1, te == "both", rep)
        if clip:
            pc = p.clamp(-1.0, 1.0)
            p, d = pc, torch.where(pc != p, pc - rep(zz), d)
        if cfg:
            w_ = k(D.W_GUIDE)
            return p[0::2] + w_ * (p[0::2] - p[1::2]), d[0::2] + w_ * (d[0::2] - d[1::2])
        return p, d

    xh, dh = tpred(z, tt, D.T_A0, D.T_A0M1)
    zm = k(D.C1) * z + k(D.C2) * xh
    xh2, dp = tpred(zm, tm, D.U_A0, D.U_A0M1)
    xt = k(D.W1) * xh + k(D.W2) * xh2
    dz = k(D.C12M1) * z + k(D.C2) * dh
    dt = k(D.W1) * dh + k(D.W2) * (dp + dz)
    extra = torch.zeros((x0.shape[0], (2 if s == "both" else 1) * C) + tuple(x0.shape[2:]), device=DEV, requires_grad=True)
    _, ds = pred(student_stub(s, extra)(z, tt, y), z, D.S_A0, D.S_A0M1, s == "both")
    loss = coef[:, D.OMEGA] * ((ds - dt) ** 2).flatten(1).mean(1)
    (loss * gw).sum().backward()
    return xt.detach(), loss.detach(), extra.grad, (z, zm, xh2)


def quotient32(coef, times, zs, ls, D):
    """the paper's quotient evaluated in fp32 (for the record in FINDINGS.md, not asserted): z_t'' by a second fp32 DDIM step, then
    (z_t'' - r z_t)/(alpha_t'' - r alpha_t)"""
    from v_diffusion.diffusion import logsnr_to_posterior_ddim
    z, zm, xh2 = zs
    l, lm, le = (v.float().to(DEV) for v in ls)
    c1, c2, _ = logsnr_to_posterior_ddim(le, lm, eta=0.)
    col = lambda v: v.reshape(-1, 1, 1, 1)
    ze = col(c1) * zm + col(c2) * xh2
    a_t, s_t = torch.sigmoid(col(l)).sqrt(), torch.sigmoid(-col(l)).sqrt()
    a_e, s_e = torch.sigmoid(col(le)).sqrt(), torch.sigmoid(-col(le)).sqrt()
    r = s_e / s_t
    return torch.where(col(times[2]) == 0, xh2, (ze - r * z) / (a_e - r * a_t))


def row_err(got, ref):
    """max over rows of the row's max error relative to the row's own scale (rows differ by many orders at the ends of the schedule)"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.detach().double().reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1).clamp(min=1e-300)
    return float(((got - ref).abs().amax(dim=1) / scale).max())


def run_kernels(dd, x0, noise, y, gw, t, s):
    extra = torch.zeros((x0.shape[0], (2 if s == "both" else 1) * x0.shape[1]) + tuple(x0.shape[2:]), device=DEV, requires_grad=True)
    y0 = None if y is None else y.clone()
    loss = dd.train_loss(student_stub(s, extra), x0, t, y, noise)
    (loss * gw).sum().backward()
    assert y is None or torch.equal(y, y0)                         # no label drop
    return dd.last_target, loss.detach(), extra.grad


@pytest.mark.parametrize("types", TYPE_PAIRS, ids=lambda p: f"{p[0]}-from-{p[1]}")
@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_target_loss_and_gradient_against_fp64(vd, shape, guided, types):
    """x_tilde, loss and d loss / d student output over N, step indices, clip and the four reweights: per quantity, the largest error
    of the kernels against fp64 (each row relative to its own scale) may be at most twice the largest error of the fp32 composition."""
    from v_diffusion import distill as D
    s, te = types
    shp = SHAPES[shape]
    w = W_GUIDE if guided else 0.0
    x0, noise, y, gw = data(shp, seed=11 + shp[0])
    xd, nd, yd, gd = x0.to(DEV), noise.to(DEV), y.to(DEV), gw.to(DEV)
    kmax, cmax, qmax, where = ({q: 0.0 for q in QUANTITIES} for _ in range(4))
    for N in STEPS:
        for idx in step_sets(shp[0], N):
            t = torch.tensor(idx, dtype=torch.float64) / N
            for clip in (False, True):
                for rw in REWEIGHTS:
                    dd = make_dd(vd, teacher_stub(te), N, s, te, rw, w, clip)
                    coef, times = D.distill_coefs(dd.logsnr_fn, t.to(DEV), N, s, te, rw, w)
                    got = run_kernels(dd, xd, nd, yd, gd, t.to(DEV), s)
                    ref = reference(coef, times, x0, noise, y, gw, s, te, rw, w, clip, D)
                    cmp = composition(coef, times, xd, nd, yd, gd, s, te, guided, clip, D)
                    if N == 1024:
                        qmax["x_tilde"] = max(qmax["x_tilde"], row_err(quotient32(coef, times, cmp[3], ref[4], D), ref[0]))
                    for q, g_, r_, c_ in zip(QUANTITIES, got, ref[:3], cmp[:3]):
                        ek, ec = row_err(g_, r_), row_err(c_, r_)
                        # beside the maxima below, every single run: within 2x the composition plus FLOOR (see there)
                        assert ek <= 2.0 * ec + FLOOR, f"{q} N={N} i={idx} clip={clip} {rw}: kernels {ek:.3e}, composition {ec:.3e}"
                        if ek > kmax[q]:
                            kmax[q], where[q] = ek, f"N={N} i={idx} clip={clip} {rw}"
                        cmax[q] = max(cmax[q], ec)
    for q in QUANTITIES:
        print(f"[distill {shape} {'guided' if guided else 'plain'} {s}<-{te}] {q}: kernels {kmax[q]:.3e}  composition {cmax[q]:.3e}"
              + (f"  fp32 quotient at N=1024 {qmax[q]:.3e}" if q == "x_tilde" else "") + f"  (kernels' worst at {where[q]})")
    for q in QUANTITIES:
        assert kmax[q] <= 2.0 * cmax[q], f"{q}: kernels {kmax[q]:.3e} > 2 x composition {cmax[q]:.3e} (at {where[q]})"


@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("N", STEPS)
def test_point_mass_teacher_gives_its_point_back(vd, N, guided):
    """an x0-teacher that answers c whatever it is shown: x_tilde = w1 c + w2 c must be c to 1 ulp, at every step index"""
    g = torch.Generator().manual_seed(3)
    c = (torch.randn((1, 3, 5, 5), generator=g, dtype=torch.float64) * 0.7).float().to(DEV)
    teacher = lambda x, t, y: c.expand(x.shape[0], -1, -1, -1).contiguous()
    teacher.training = False
    dd = make_dd(vd, teacher, N, "v", "x0", "constant", W_GUIDE if guided else 0.0, False)
    t = (torch.arange(1, N + 1, dtype=torch.float64) / N).to(DEV)
    x0, noise, _, _ = data((N, 3, 5, 5), seed=4)
    y = torch.ones(N, device=DEV)
    dd.train_loss(student_stub("v"), x0.to(DEV), t, y, noise.to(DEV))
    ulp = torch.nextafter(c.abs(), torch.full_like(c, float("inf"))) - c.abs()
    err = (dd.last_target - c).abs()
    assert bool((err <= ulp).all()), float((err / ulp).max())
    assert torch.equal(dd.last_target[0:1], c)                      # i = 1: (w1, w2) = (0, 1), exactly x_hat'


@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_one_student_step_lands_where_two_teacher_steps_do(vd, shape, N, guided):
    """the existing sampler, twice at T = 2N with the teacher, against once at T = N with a student that answers the v of the kernels'
    x_tilde.  Tolerance: twice what the two fp32 sampler calls themselves are off their fp64 restatement."""
    from v_diffusion import distill as D
    from v_diffusion.diffusion import q_sample
    shp = SHAPES[shape]
    B = shp[0]
    w = W_GUIDE if guided else 0.0
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    x0, noise, y, _ = data(shp, seed=23)
    xd, nd, yd = x0.to(DEV), noise.to(DEV), y.to(DEV)
    for i in sorted({1, N, 300 if N > 2 else 1}):
        t = torch.full((B,), i / N, dtype=torch.float64, device=DEV)
        dd = make_dd(vd, teacher_stub("v"), N, "v", "v", "constant", w, False)
        coef, times = D.distill_coefs(fn, t, N, "v", "v", "constant", w)
        l32 = coef[:, D.LOGSNR_T].contiguous()
        z = q_sample(xd, l32, nd)
        dd.train_loss(student_stub("v"), xd, t, yd, nd)
        xt = dd.last_target
        # teacher side: two reverse steps on the 2N grid
        big = vd.GaussianDiffusion(fn, 2 * N, "v", "fixed_large", "constant", "mse", w_guide=w, p_uncond=0.0)
        step = lambda k: torch.full((B,), k, device=DEV)
        zm = big.p_sample_step(teacher_stub("v"), z, step(2 * i - 1), yd, clip_denoised=False, use_ddim=True)
        ze = big.p_sample_step(teacher_stub("v"), zm, step(2 * i - 2), yd, clip_denoised=False, use_ddim=True)
        # student side: one reverse step on the N grid, unguided, the network answering v(x_tilde)
        small = vd.GaussianDiffusion(fn, N, "v", "fixed_large", "constant", "mse", w_guide=0.0, p_uncond=0.0)
        a0, b0x = small._step_coefs(i - 1, True)[0][:2]             # x0_hat = a0 z + b0x v is what this sampler evaluates: invert THAT
        v = ((a0 * z.double() - xt.double()) / -b0x).float()
        zs = small.p_sample_step(lambda a, b, c: v, z, step(i - 1), yd, clip_denoised=False, use_ddim=True)
        # fp64 restatement of the two teacher calls, from the same z_t
        tt, tm, te = (u.cpu() for u in times)
        ls = tuple(fn(u.clone()).float().double() for u in (tt, tm, te))
        ref = R.two_steps(teacher_stub("v"), z.cpu().double(), (tt, tm, te), ls, y.double(), "v", w, False)[3]
        own = float((ze.cpu().double() - ref).abs().max())
        gap = float((zs - ze).abs().max())
        print(f"[distill sampler {shape} N={N} i={i} {'guided' if guided else 'plain'}] student vs teacher {gap:.3e}  "
              f"teacher's two calls vs fp64 {own:.3e}")
        assert gap <= 2.0 * own, (i, gap, own)


def test_networks_are_called_with_the_snapped_and_rewritten_times(vd):
    """off-grid t and a rescaling schedule: the teacher sees the grid times t, t - 1/(2N) as the schedule rewrote them (on 2B rows when
    guided), the student sees t; neither sees the caller's tensor, which is left as it was"""
    from v_diffusion import distill as D
    N, shp = 4, SHAPES["75"]
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0, rescale=True)
    x0, noise, y, _ = data(shp, seed=41)
    t = torch.tensor([0.05, 0.55, 0.80], dtype=torch.float64, device=DEV)
    t0 = t.clone()
    _, (tt, tm, _) = D.distill_coefs(fn, t, N, "v", "v", "constant", W_GUIDE)
    grid = torch.tensor([1, 3, 4], dtype=torch.float64, device=DEV) / N
    assert not torch.equal(tt, grid) and not torch.equal(tt, t)                      # rewritten, and not the caller's values
    seen = {"teacher": [], "student": []}

    def recording(stub, who):
        def net(x, tnet, lab):
            seen[who].append(tnet.clone())
            return stub(x, tnet, lab)
        net.training = False
        return net

    dd = vd.DistillationDiffusion(recording(teacher_stub("v"), "teacher"), N, teacher_w_guide=W_GUIDE, logsnr_fn=fn, model_out_type="v",
                                  model_var_type="fixed_large", reweight_type="constant")
    dd.train_loss(recording(student_stub("v"), "student"), x0.to(DEV), t, y.to(DEV), noise.to(DEV))
    assert torch.equal(t, t0)
    assert len(seen["teacher"]) == 2 and len(seen["student"]) == 1
    assert torch.equal(seen["teacher"][0], tt.repeat_interleave(2)) and torch.equal(seen["teacher"][1], tm.repeat_interleave(2))
    assert torch.equal(seen["student"][0], tt)


@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_run_to_run_bitwise(vd, shape):
    shp = SHAPES[shape]
    x0, noise, y, gw = data(shp, seed=31)
    t = (torch.tensor(step_sets(shp[0], 1024)[0], dtype=torch.float64) / 1024).to(DEV)
    runs = []
    for _ in range(2):
        dd = make_dd(vd, teacher_stub("x0"), 1024, "both", "x0", "snr_trunc", W_GUIDE, True)
        runs.append(run_kernels(dd, x0.to(DEV), noise.to(DEV), y.to(DEV), gw.to(DEV), t, "both"))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_entry_points_refuse_bad_arguments(vd):
    from v_diffusion import _hip
    z = torch.zeros((2, 3, 4, 4), device=DEV)
    coef = torch.zeros((2, 20), device=DEV)
    loss = torch.zeros(2, device=DEV)
    with pytest.raises(_hip.HipError, match="null"):
        _hip.distill_mid(z, None, coef, 0, False, False, z.clone(), z.clone(), z.clone(), None, 2, 3, 16)
    with pytest.raises(_hip.HipError, match="empty"):
        _hip.distill_mid(z, z, coef, 0, False, False, z.clone(), z.clone(), z.clone(), None, 0, 3, 16)
    with pytest.raises(_hip.HipError, match="model_out_type"):
        _hip.distill_loss_fwd(z, z, z, z, z, z, coef, 4, 0, False, False, loss, z.clone(), None, 2, 3, 16)
    with pytest.raises(_hip.HipError, match="null"):
        _hip.distill_loss_bwd(z, coef, None, 0, z.clone(), 2, 3, 16)


def _tiny(vd, train):
    from oracle.cases import TINY, make_weights
    case = TINY["tinyA"]
    model = vd.UNet(**case["cfg"])
    model.load_state_dict(make_weights(case["cfg"]))
    model.to(DEV)
    return (model.train() if train else model.eval()), case


def test_one_trainer_step_through_the_real_network(vd):
    from oracle.cases import make_inputs
    from v_diffusion import _hip, distill as D
    from v_diffusion.trainer import HotPathTrainer
    N, B = 4, 4
    student, case = _tiny(vd, train=True)
    teacher, _ = _tiny(vd, train=False)
    teacher.requires_grad_(False)
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    start = {k: v.detach().clone() for k, v in student.named_parameters()}
    x0, _, y = make_inputs(case["cfg"], B, case["R"], case["label"], seed=3)
    x0, y = x0.clamp(-1, 1).to(DEV), y.clamp(min=1).to(DEV)
    t = (torch.tensor([1, 2, 3, 4], dtype=torch.float64) / N).to(DEV)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    dd = make_dd(vd, teacher, N, "v", "v", "snr_trunc", 1.0, False)
    trainer = HotPathTrainer(student, dd, lr=1e-3, warmup=0, use_ema=False, timesteps=N)
    y0 = y.clone()
    loss = trainer.step(x0, y, t=t, noise=noise)
    assert torch.isfinite(loss) and float(loss) > 0 and torch.equal(y, y0)
    grads = {k: v.clone() for k, v in trainer.flat.grad_views.items()}
    assert all(torch.equal(v, before[k]) for k, v in teacher.state_dict().items())      # the teacher is frozen
    assert all(p.grad is None for p in teacher.parameters())
    assert any(not torch.equal(p.detach(), start[k]) for k, p in student.named_parameters())
    # the same gradients without the autograd.Function: the launches by hand, dout fed to the network's own backward
    ref, _ = _tiny(vd, train=True)
    coef, (tt, tm, _) = D.distill_coefs(dd.logsnr_fn, t, N, "v", "v", "snr_trunc", 1.0)
    C, HW = x0.shape[1], case["R"] ** 2
    z, xhat, dhat, zmid = (torch.empty_like(x0) for _ in range(4))
    zdup = torch.empty((2 * B,) + tuple(x0.shape[1:]), device=DEV)
    y_in = y.repeat_interleave(2).clone()
    y_in[1::2] = 0
    with torch.no_grad():
        _hip.q_sample(x0, noise, coef[:, D.LOGSNR_T].contiguous(), z, B, C, HW)
        o1 = teacher(z.repeat_interleave(2, dim=0), tt.repeat_interleave(2), y_in)
        _hip.distill_mid(z, o1, coef, 0, True, False, xhat, dhat, zmid, zdup, B, C, HW)
        o2 = teacher(zdup, tm.repeat_interleave(2), y_in)
    out = ref(z, tt, y)
    lossv, resid, dout = torch.empty(B, device=DEV), torch.empty_like(x0), torch.empty_like(x0)
    _hip.distill_loss_fwd(None, dhat, zmid, o2, z, out.detach().contiguous(), coef, 0, 0, True, False, lossv, resid, None, B, C, HW)
    _hip.distill_loss_bwd(resid, coef, torch.full((B,), 1.0 / B, device=DEV), 0, dout, B, C, HW)
    assert float((lossv.mean() - loss).abs()) <= 1e-6 * float(loss)
    out.backward(dout)
    # (the bound of smoke() for gradients of this network; the two paths run the same kernels)
    gmax = max(float(p.grad.norm()) for p in ref.parameters())
    for k, p in ref.named_parameters():
        err = float((grads[k] - p.grad).norm())
        assert err <= 1e-4 * float(p.grad.norm()) + 1e-6 * gmax, (k, err)


def test_next_stage_down_to_one_step(vd):
    student, case = _tiny(vd, train=True)
    teacher, _ = _tiny(vd, train=False)
    dd = make_dd(vd, teacher.requires_grad_(False), 4, "v", "v", "snr_trunc", 1.0, False)
    # a student that has been through a flat-buffer trainer (its parameters are views of the flat store, its engine is built)
    from v_diffusion.trainer import HotPathTrainer
    x = torch.rand((2, 3, case["R"], case["R"]), device=DEV) * 2 - 1
    HotPathTrainer(student, dd, use_ema=False, timesteps=4).step(x, torch.tensor([2.0, 5.0], device=DEV))
    two = dd.next_stage(student)
    one = two.next_stage(student)
    assert (two.student_steps, one.student_steps) == (2, 1) and two.teacher_w_guide == one.teacher_w_guide == 0.0
    for st in (two, one):
        tch = st.teacher_fn
        assert tch is not student and not tch.training and all(not p.requires_grad for p in tch.parameters())
        assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(tch.parameters(), student.parameters()))
        assert all(p.untyped_storage().nbytes() == 4 * p.numel() for p in tch.parameters())     # compact copies, not copies of the flat store
    R_ = case["R"]
    noise = torch.randn((2, 3, R_, R_), generator=torch.Generator().manual_seed(1))
    xs = one.p_sample(student.eval(), (2, 3, R_, R_), noise=noise, label=torch.tensor([1.0, 4.0]), use_ddim=True)
    assert xs.shape == (2, 3, R_, R_) and bool(torch.isfinite(xs).all())
    xs2 = one.p_sample(student, (2, 3, R_, R_), noise=noise, label=torch.tensor([1.0, 4.0]), use_ddim=True)
    assert torch.equal(xs, xs2)
