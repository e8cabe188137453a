"""Consistency distillation / training and multistep consistency sampling on the GPU (v_diffusion/consistency.py over vd_consist_mid /
vd_consist_pair / vd_consist_loss_fwd / vd_consist_loss_bwd / vd_ema_track_batched and the existing vd_sample_step) against the float64
restatement of tests/consist_ref.py.  The networks of the kernel tests are the pointwise stand-ins of tests/test_distill_gpu.py,
a(t) x + b(t) tanh(x) + g y, the same function in fp64 on the CPU and in fp32 on the GPU.  The yardstick for the kernels' error is that
file's: the same arithmetic as a plain fp32 torch composition on the GPU from the same coefficient table, the residual in difference
form; kernels and composition differ in summation order and FMA contraction only, so the kernels may be at most 2x as far from fp64
over a parametrisation's runs, and each run at most 2x the composition plus 4 ulp of the row's scale (reasoning: there).  Needs an MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consist_ref as R                                           # noqa: E402
from test_distill_gpu import FLOOR, SHAPES, STEPS, REWEIGHTS, TYPE_PAIRS, W_GUIDE, Stub, data, row_err, step_sets, student_stub, \
    teacher_stub                                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
METRICS = ("l2", "huber")
QUANTITIES = ("target", "loss", "dout")


@pytest.fixture(scope="module")
def vd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import v_diffusion
    from v_diffusion import _hip
    _hip.lib()
    return v_diffusion


def target_stub(out_type):
    return Stub((-0.25, 0.55), (0.45, -0.15), 0.04, both=out_type == "both")


def schedule(vd):
    return vd.get_logsnr_schedule("cosine", -20.0, 20.0)


def make_cd(vd, N, s, rw, metric, teacher=None, te=None, w=0.0, clip=False, target="stub"):
    cd = vd.ConsistencyDiffusion(N, teacher_fn=teacher, target_fn=target_stub(s) if target == "stub" else target, teacher_out_type=te,
                                 teacher_w_guide=w, clip_teacher=clip, metric=metric, logsnr_fn=schedule(vd), model_out_type=s,
                                 model_var_type="fixed_large", reweight_type=rw)
    cd.keep_target = True
    return cd


def zeros_out(x0, s, **kw):
    return torch.zeros((x0.shape[0], (2 if s == "both" else 1) * x0.shape[1]) + tuple(x0.shape[2:]), requires_grad=True, **kw)


def reference(vd, coef, times, x0, noise, y, gw, s, te, rw, metric, w, clip, D, distil):
    """fp64 on the CPU: (target, loss, d (sum gw*loss) / d student output)"""
    l = coef[:, D.LOGSNR_T].cpu().double()
    tt, ts = (v.cpu() for v in times)
    ls = schedule(vd)(ts.clone()).float().double()
    a, sg = R.alpha_sigma(R.col(l))
    xd, nd = x0.double(), noise.double()
    z = a * xd + sg * nd
    yd = None if y is None else y.double()
    zs = R.z_down(teacher_stub(te) if distil else None, z, xd, nd, (tt, ts), (l, ls), yd, te, w, clip)
    tgt = R.target(target_stub(s), zs, ts, ls, yd, s)
    extra = zeros_out(x0, s, dtype=torch.float64)
    loss = R.loss(student_stub(s, extra)(z, tt, yd), z, tgt, l, s, rw, metric)
    (loss * gw.double()).sum().backward()
    return tgt, loss.detach(), extra.grad


def composition(coef, times, x0, noise, y, gw, s, te, metric, cfg, clip, D, distil, huber_c=0.00054):
    """the kernels' arithmetic as fp32 tensor ops on the GPU, from the same table: the residual from the difference forms"""
    k = lambda j: coef[:, j].reshape(-1, 1, 1, 1)
    tt, ts = times
    l = k(D.LOGSNR_T)
    C = x0.shape[1]
    last = k(D.LAST) != 0
    z = x0 * torch.sigmoid(l).sqrt() + noise * torch.sigmoid(-l).sqrt()

    def pred(out, zz, c0, m1, both, rep=lambda v: v):
        tail = rep(k(c0 + 1)) * out[:, :C] + rep(k(c0 + 2)) * out[:, C:] if both else rep(k(c0 + 1)) * out
        return rep(k(c0)) * zz + tail, rep(k(m1)) * zz + tail

    if distil:
        rep = (lambda v: v.repeat_interleave(2, dim=0)) if cfg else (lambda v: v)
        y_in = y
        if cfg:
            y_in = rep(y).clone()
            y_in[1::2] = 0
        p, d = pred(teacher_stub(te)(rep(z), rep(tt), y_in), rep(z), D.T_A0, D.T_A0M1, te == "both", rep)
        if clip:
            pc = p.clamp(-1.0, 1.0)
            p, d = pc, torch.where(pc != p, pc - rep(z), d)
        if cfg:
            w_ = k(D.W_GUIDE)
            p, d = p[0::2] + w_ * (p[0::2] - p[1::2]), d[0::2] + w_ * (d[0::2] - d[1::2])
        zs = torch.where(last, p, k(D.C1) * z + k(D.C2) * p)
        dz = torch.where(last, d, k(D.C12M1) * z + k(D.C2) * d)
    else:
        zs = k(D.ALPHA_S) * x0 + k(D.SIGMA_S) * noise
        dz = k(D.D_ALPHA) * x0 + k(D.D_SIGMA) * noise
    pt, dt = pred(target_stub(s)(zs, ts, y), zs, D.G_A0, D.G_A0M1, s == "both")
    tgt = torch.where(last, zs, pt)
    dt = torch.where(last, torch.zeros_like(dt), dt)
    extra = zeros_out(x0, s, device=DEV)
    _, ds = pred(student_stub(s, extra)(z, tt, y), z, D.S_A0, D.S_A0M1, s == "both")
    S = (((ds - dt) - dz) ** 2).flatten(1).sum(1)
    n = x0[0].numel()
    if metric == "l2":
        loss = coef[:, D.OMEGA] * S / n
    else:
        c = huber_c * n ** 0.5
        loss = coef[:, D.OMEGA] * S / (torch.sqrt(S + c * c) + c)
    (loss * gw).sum().backward()
    return tgt.detach(), loss.detach(), extra.grad


def run_kernels(cd, x0, noise, y, gw, t, s):
    extra = zeros_out(x0, s, device=DEV)
    y0 = None if y is None else y.clone()
    loss = cd.train_loss(student_stub(s, extra), x0, t, y, noise)
    (loss * gw).sum().backward()
    assert y is None or torch.equal(y, y0)                         # no label drop
    return cd.last_target, loss.detach(), extra.grad


def parity(vd, shape, types, distil, guided, tag):
    from v_diffusion import consistency as D
    s, te = types
    shp = SHAPES[shape]
    w = W_GUIDE if guided else 0.0
    x0, noise, y, gw = data(shp, seed=13 + shp[0])
    xd, nd, yd, gd = x0.to(DEV), noise.to(DEV), y.to(DEV), gw.to(DEV)
    kmax, cmax, where = ({q: 0.0 for q in QUANTITIES} for _ in range(3))
    at1024 = {q: [0.0, 0.0] for q in QUANTITIES}
    for N in STEPS:
        for idx in step_sets(shp[0], N):
            t = torch.tensor(idx, dtype=torch.float64) / N
            for clip in ((False, True) if distil else (False,)):
                for rw in REWEIGHTS:
                    for metric in METRICS:
                        cd = make_cd(vd, N, s, rw, metric, teacher_stub(te) if distil else None, te, w, clip)
                        coef, times = D.consistency_coefs(cd.logsnr_fn, t.to(DEV), N, s, te, rw, w, teacher=distil)
                        got = run_kernels(cd, xd, nd, yd, gd, t.to(DEV), s)
                        ref = reference(vd, coef, times, x0, noise, y, gw, s, te, rw, metric, w, clip, D, distil)
                        cmp = composition(coef, times, xd, nd, yd, gd, s, te, metric, guided and distil, clip, D, distil)
                        for q, g_, r_, c_ in zip(QUANTITIES, got, ref, cmp):
                            ek, ec = row_err(g_, r_), row_err(c_, r_)
                            assert ek <= 2.0 * ec + FLOOR, f"{q} N={N} i={idx} clip={clip} {rw} {metric}: kernels {ek:.3e}, composition {ec:.3e}"
                            if ek > kmax[q]:
                                kmax[q], where[q] = ek, f"N={N} i={idx} clip={clip} {rw} {metric}"
                            cmax[q] = max(cmax[q], ec)
                            if N == 1024:
                                at1024[q] = [max(at1024[q][0], ek), max(at1024[q][1], ec)]
    for q in QUANTITIES:
        print(f"[consistency {tag} {shape} {'guided' if guided else 'plain'} {s}<-{te}] {q}: kernels {kmax[q]:.3e}  composition {cmax[q]:.3e}"
              f"  at N=1024: {at1024[q][0]:.3e} / {at1024[q][1]:.3e}  (kernels' worst at {where[q]})")
    for q in QUANTITIES:
        assert kmax[q] <= 2.0 * cmax[q], f"{q}: kernels {kmax[q]:.3e} > 2 x composition {cmax[q]:.3e} (at {where[q]})"


@pytest.mark.parametrize("types", TYPE_PAIRS, ids=lambda p: f"{p[0]}-from-{p[1]}")
@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_distillation_target_loss_and_gradient_against_fp64(vd, shape, guided, types):
    """target image, loss and d loss / d student output over N, step indices (i = 1, i = N, interior), clip, the four reweights and both
    metrics: per quantity, the largest error of the kernels against fp64 (each row relative to its own scale) may be at most twice the
    largest error of the fp32 composition"""
    parity(vd, shape, types, True, guided, "distillation")


@pytest.mark.parametrize("types", TYPE_PAIRS, ids=lambda p: p[0])
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_training_target_loss_and_gradient_against_fp64(vd, shape, types):
    """the same without a teacher: z_s = alpha_s x_0 + sigma_s eps from vd_consist_pair"""
    parity(vd, shape, types, False, False, "training")


def _bases(aligned, *shapes):
    """fp32 device buffers whose bases are 16-byte aligned, or 4 bytes past such an address"""
    out = []
    for shp in shapes:
        n = int(torch.tensor(shp).prod())
        buf = torch.empty(n + 4, device=DEV)
        assert buf.data_ptr() % 16 == 0
        out.append(buf[0 if aligned else 1: n + (0 if aligned else 1)].view(shp))
    return out


@pytest.mark.parametrize("s", ("v", "both"))
def test_wide_and_scalar_paths_agree_bit_for_bit(vd, s):
    """C*HW = 972 on aligned bases takes the dwordx4 kernels, the same buffers 4 bytes further the scalar ones; C*HW = 75 is scalar
    whatever the bases: every output of the four kernels has the same bits either way"""
    from v_diffusion import _hip, consistency as D
    for shape in SHAPES.values():
        B, C = shape[:2]
        HW = shape[2] * shape[3]
        Co = 2 if s == "both" else 1
        oshape = (B, Co * C) + tuple(shape[2:])
        x0, noise, y, gw = data(shape, seed=51)
        t = (torch.tensor(step_sets(B, 1024)[0], dtype=torch.float64) / 1024).to(DEV)
        coef, (tt, ts) = D.consistency_coefs(schedule(vd), t, 1024, s, s, "snr_trunc", W_GUIDE)
        g = torch.Generator().manual_seed(52)
        tout2, sout, tout = (torch.randn(shp, generator=g) for shp in ((2 * B, Co * C) + tuple(shape[2:]), oshape, oshape))
        results = []
        for aligned in (True, False):
            x0b, nb, zt, zs, dz, zt2, zs2, dz2, xh, resid, tgt = _bases(aligned, *([shape] * 11))
            to2, so, to, dout = _bases(aligned, tout2.shape, oshape, oshape, oshape)
            for dst, src in ((x0b, x0), (nb, noise), (to2, tout2), (so, sout), (to, tout)):
                dst.copy_(src)
            loss, aux = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
            _hip.consist_pair(x0b, nb, coef, zt, zs, dz, B, C, HW)
            _hip.consist_mid(zt, to2, coef, _hip.OUT_TYPES[s], True, True, zs2, dz2, xh, B, C, HW)
            _hip.consist_loss_fwd(zt, zs2, dz2, so, to, coef, _hip.OUT_TYPES[s], 1, 0.01, loss, resid, aux, tgt, B, C, HW)
            _hip.consist_loss_bwd(resid, coef, gw.to(DEV), aux, _hip.OUT_TYPES[s], dout, B, C, HW)
            results.append([v.clone() for v in (zt, zs, dz, zs2, dz2, xh, loss, resid, aux, tgt, dout)])
        for a, b in zip(*results):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(results[0][6]).all())


@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_run_to_run_bitwise(vd, shape):
    shp = SHAPES[shape]
    x0, noise, y, gw = data(shp, seed=31)
    t = (torch.tensor(step_sets(shp[0], 1024)[0], dtype=torch.float64) / 1024).to(DEV)
    for distil in (True, False):
        runs = []
        for _ in range(2):
            cd = make_cd(vd, 1024, "both", "snr_trunc", "huber", teacher_stub("x0") if distil else None, "x0", W_GUIDE, True)
            runs.append(run_kernels(cd, x0.to(DEV), noise.to(DEV), y.to(DEV), gw.to(DEV), t, "both"))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_pair_gives_q_samples_bits(vd, shape):
    """vd_consist_pair's z_t is vd_q_sample's, bit for bit, aligned or not; z_s and dz are what the table says"""
    from v_diffusion import _hip, consistency as D
    shp = SHAPES[shape]
    B, C, HW = shp[0], shp[1], shp[2] * shp[3]
    x0, noise, _, _ = data(shp, seed=61)
    for N in STEPS:
        t = (torch.tensor(step_sets(B, N)[0], dtype=torch.float64) / N).to(DEV)
        coef, _ = D.consistency_coefs(schedule(vd), t, N, "v", None, "constant", teacher=False)
        for aligned in (True, False):
            x0b, nb, zt, zs, dz, zq = _bases(aligned, *([shp] * 6))
            x0b.copy_(x0)
            nb.copy_(noise)
            _hip.consist_pair(x0b, nb, coef, zt, zs, dz, B, C, HW)
            _hip.q_sample(x0b, nb, coef[:, D.LOGSNR_T].contiguous(), zq, B, C, HW)
            assert torch.equal(zt, zq)
            k = lambda j: coef[:, j].double().reshape(-1, 1, 1, 1)
            for got, ca, cs in ((zs, D.ALPHA_S, D.SIGMA_S), (dz, D.D_ALPHA, D.D_SIGMA)):
                want = k(ca) * x0b.double() + k(cs) * nb.double()
                scale = (k(ca).abs() * x0b.double().abs() + k(cs).abs() * nb.double().abs())
                assert bool(((got.double() - want).abs() <= 2.0 ** -23 * scale).all())      # two roundings of the fused form


def _poisoned(stub, rows):
    def net(x, t, y):
        out = stub(x, t, y).clone()
        out[rows] = float("nan")
        return out
    net.training = False
    return net


@pytest.mark.parametrize("distil", (True, False), ids=("distillation", "training"))
@pytest.mark.parametrize("metric", METRICS)
def test_boundary_rows_select_and_other_rows_propagate(vd, metric, distil):
    """NaN in the target network's output on the i = 1 row leaves target, loss and dout finite and unchanged, bit for bit; NaN on
    another row makes that row's loss NaN and no other"""
    shp = SHAPES["75"]
    x0, noise, y, gw = data(shp, seed=71)
    args = [v.to(DEV) for v in (x0, noise, y, gw)]
    N = 1024
    t = (torch.tensor([1, N, 300], dtype=torch.float64) / N).to(DEV)
    teacher = teacher_stub("v") if distil else None
    clean = run_kernels(make_cd(vd, N, "v", "snr", metric, teacher, "v"), *args, t, "v")
    cd = make_cd(vd, N, "v", "snr", metric, teacher, "v", target=_poisoned(target_stub("v"), [0]))
    got = run_kernels(cd, *args, t, "v")
    for a, b in zip(got, clean):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    cd = make_cd(vd, N, "v", "snr", metric, teacher, "v", target=_poisoned(target_stub("v"), [2]))
    tgt, loss, dout = run_kernels(cd, *args, t, "v")
    assert bool(torch.isnan(loss[2])) and torch.equal(loss[:2], clean[1][:2])
    assert torch.equal(dout[:2], clean[2][:2]) and torch.equal(tgt[:2], clean[0][:2])


def test_distillation_i1_target_is_the_teachers_prediction(vd):
    """rows with i = 1 carry (c1, c2) = (0, 1) and are selected: z_0 and the target are the teacher's (clipped, guided) x0 prediction
    bit for bit, and dz its difference from z_t -- the image the samplers return on their last step (to rounding: the sampler's
    prediction weights are fp32 evaluations, the table's are rounded from fp64)"""
    from v_diffusion import _hip, consistency as D
    from v_diffusion.diffusion import q_sample
    shp = SHAPES["75"]
    B, C, HW = shp[0], shp[1], shp[2] * shp[3]
    x0, noise, y, gw = data(shp, seed=73)
    xd, nd, yd = x0.to(DEV), noise.to(DEV), y.to(DEV)
    N = 4
    t = torch.full((B,), 1 / N, dtype=torch.float64, device=DEV)
    for w in (0.0, W_GUIDE):
        cd = make_cd(vd, N, "v", "constant", "l2", teacher_stub("v"), "v", w, True)
        cd.train_loss(student_stub("v"), xd, t, yd, nd)
        coef, (tt, _) = D.consistency_coefs(cd.logsnr_fn, t, N, "v", "v", "constant", w)
        z = q_sample(xd, coef[:, D.LOGSNR_T].contiguous(), nd)
        zs, dz, xh = (torch.empty_like(z) for _ in range(3))
        cfg = w > 0
        y_in = yd.repeat_interleave(2).clone() if cfg else yd
        if cfg:
            y_in[1::2] = 0
        rep = (lambda v: v.repeat_interleave(2, dim=0)) if cfg else (lambda v: v)
        out = teacher_stub("v")(rep(z), rep(tt), y_in).float().contiguous()
        _hip.consist_mid(z, out, coef, 0, cfg, True, zs, dz, xh, B, C, HW)
        assert torch.equal(zs, xh) and torch.equal(cd.last_target, xh)
        assert float((dz.double() - (xh.double() - z.double())).abs().max()) <= 2.0 ** -22 * float(xh.abs().max() + z.abs().max())
        gd = vd.GaussianDiffusion(schedule(vd), N, "v", "fixed_large", "constant", "mse", w_guide=w, p_uncond=0.0)
        last = gd.p_sample_step(teacher_stub("v"), z, torch.zeros(B, device=DEV, dtype=torch.long), yd, clip_denoised=True, use_ddim=True)
        assert float((last - xh).abs().max()) <= 2.0 ** -21 * (1.0 + 2 * w)


def test_entry_points_refuse_bad_arguments(vd):
    from v_diffusion import _hip
    z = torch.zeros((2, 3, 4, 4), device=DEV)
    coef = torch.zeros((2, 24), device=DEV)
    v = torch.zeros(2, device=DEV)
    with pytest.raises(_hip.HipError, match="null"):
        _hip.consist_mid(z, None, coef, 0, False, False, z.clone(), z.clone(), None, 2, 3, 16)
    with pytest.raises(_hip.HipError, match="empty"):
        _hip.consist_pair(z, z, coef, z.clone(), z.clone(), z.clone(), 0, 3, 16)
    with pytest.raises(_hip.HipError, match="model_out_type"):
        _hip.consist_loss_fwd(z, z, z, z, z, coef, 4, 0, 1.0, v, z.clone(), v.clone(), None, 2, 3, 16)
    with pytest.raises(_hip.HipError, match="metric"):
        _hip.consist_loss_fwd(z, z, z, z, z, coef, 0, 2, 1.0, v, z.clone(), v.clone(), None, 2, 3, 16)
    with pytest.raises(_hip.HipError, match="metric"):
        _hip.consist_loss_fwd(z, z, z, z, z, coef, 0, 1, 0.0, v, z.clone(), v.clone(), None, 2, 3, 16)
    with pytest.raises(_hip.HipError, match="null"):
        _hip.consist_loss_bwd(z, coef, None, v, 0, z.clone(), 2, 3, 16)
    with pytest.raises(_hip.HipError, match="decay"):
        _hip.ema_track_batched(torch.zeros((1, 8), dtype=torch.int64, device=DEV), 1, 1, 1.5)


def test_wrong_channel_counts_are_refused(vd):
    shp = SHAPES["75"]
    x0, noise, y, _ = data(shp, seed=75)
    xd, nd, yd = x0.to(DEV), noise.to(DEV), y.to(DEV)
    t = torch.full((shp[0],), 0.5, dtype=torch.float64, device=DEV)
    wide = lambda x, tt, yy: torch.cat([x, x], dim=1)                # noqa: E731
    wide.training = False
    with pytest.raises(RuntimeError, match="teacher's output"):
        make_cd(vd, 4, "v", "constant", "l2", wide, "v").train_loss(student_stub("v"), xd, t, yd, nd)
    with pytest.raises(RuntimeError, match="target network's output"):
        make_cd(vd, 4, "v", "constant", "l2", target=wide).train_loss(student_stub("v"), xd, t, yd, nd)
    with pytest.raises(RuntimeError, match="student's output"):
        make_cd(vd, 4, "v", "constant", "l2").train_loss(wide, xd, t, yd, nd)
    hot = teacher_stub("v")
    hot.training = True
    with pytest.raises(RuntimeError, match="eval mode"):
        make_cd(vd, 4, "v", "constant", "l2", hot, "v").train_loss(student_stub("v"), xd, t, yd, nd)


def _tiny(vd, train, seed=0):
    from oracle.cases import TINY, make_weights
    case = TINY["tinyA"]
    cfg = dict(case["cfg"], drop_rate=0.0)
    model = vd.UNet(**cfg)
    model.load_state_dict(make_weights(case["cfg"], seed=seed))
    model.to(DEV)
    return (model.train() if train else model.eval()), case


def _tiny_batch(case, B=4, seed=3):
    from oracle.cases import make_inputs
    x0, _, y = make_inputs(case["cfg"], B, case["R"], case["label"], seed=seed)
    return x0.clamp(-1, 1).to(DEV), y.clamp(min=1).to(DEV)


def test_update_target(vd):
    """one launch over every parameter: decay 0 copies bit for bit, decay 1 changes nothing, decay 0.9 is the fp32 torch expression
    e + (1 - d) * (p - e) bit for bit; when a FusedAdamW flat store has re-pointed the student's storages the cached table is rebuilt"""
    from v_diffusion.trainer import HotPathTrainer
    student, case = _tiny(vd, train=True)
    other, _ = _tiny(vd, train=True, seed=1)
    cd = make_cd(vd, 4, "v", "snr_trunc", "huber", target=None)
    cd.target_fn = cd.make_target(other)
    tgt = cd.target_fn
    assert not tgt.training and any(not torch.equal(e, p) for e, p in zip(tgt.parameters(), student.parameters()))
    start = [e.detach().clone() for e in tgt.parameters()]
    cd.update_target(student, 1.0)
    assert all(torch.equal(e, e0) for e, e0 in zip(tgt.parameters(), start))
    d = 0.9
    want = [e + (1 - d) * (p.detach() - e) for e, p in zip(start, student.parameters())]
    cd.update_target(student, d)
    assert all(torch.equal(e, w_) for e, w_ in zip(tgt.parameters(), want))
    assert any(not torch.equal(e, e0) for e, e0 in zip(tgt.parameters(), start))
    table0 = cd._ema_tables[(id(tgt), id(student))][3]
    cd.update_target(student, 0.0)
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(tgt.parameters(), student.parameters()))
    assert cd._ema_tables[(id(tgt), id(student))][3] is table0                           # built once per pair
    # a trainer moves the student's parameters into its flat store: every data pointer changes
    before = [p.data_ptr() for p in student.parameters()]
    trainer = HotPathTrainer(student, cd, lr=1e-2, warmup=0, use_ema=False, timesteps=4)
    x0, y = _tiny_batch(case)
    trainer.step(x0, y)
    assert any(a != p.data_ptr() for a, p in zip(before, student.parameters()))
    assert any(not torch.equal(e, p) for e, p in zip(tgt.parameters(), student.parameters()))   # the step moved the student
    start = [e.detach().clone() for e in tgt.parameters()]
    d = 0.5
    want = [e + (1 - d) * (p.detach() - e) for e, p in zip(start, student.parameters())]
    cd.update_target(student, d)
    assert cd._ema_tables[(id(tgt), id(student))][3] is not table0
    assert all(torch.equal(e, w_) for e, w_ in zip(tgt.parameters(), want))
    ddp_like = torch.nn.Sequential()
    ddp_like.module = student
    cd.update_target(ddp_like, 0.0)                                                       # unwrapped as next_stage unwraps
    assert all(torch.equal(e, p) for e, p in zip(tgt.parameters(), student.parameters()))


def test_student_as_its_own_target(vd):
    """target_fn=None runs the student itself, without gradients and in eval mode for that one forward: with drop_rate = 0 loss and
    parameter gradients equal, bit for bit, those of a separate detached copy; the module is in training mode afterwards, also when the
    target forward raises"""
    model, case = _tiny(vd, train=True)
    x0, y = _tiny_batch(case)
    t = (torch.tensor([1, 2, 3, 4], dtype=torch.float64) / 4).to(DEV)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    runs = []
    for own in (True, False):
        cd = make_cd(vd, 4, "v", "snr_trunc", "huber", target=None)
        if not own:
            cd.target_fn = cd.make_target(model)
        model.zero_grad(set_to_none=True)
        loss = cd.train_loss(model, x0, t, y, noise)
        loss.mean().backward()
        assert model.training
        runs.append((loss.detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and bool(torch.isfinite(runs[0][0]).all())
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert any(float(g.abs().max()) > 0 for g in runs[0][1])

    class Flaky(torch.nn.Module):
        def forward(self, x, tt, yy):
            if not self.training:
                raise RuntimeError("boom")
            return x

    flaky = Flaky().train()
    with pytest.raises(RuntimeError, match="boom"):
        make_cd(vd, 4, "v", "snr_trunc", "huber", target=None).train_loss(flaky, x0, t, y, noise)
    assert flaky.training


@pytest.mark.parametrize("distil,own", ((True, False), (False, False), (False, True)),
                         ids=("distillation", "training", "training-student-as-target"))
def test_three_trainer_steps_through_the_real_network(vd, distil, own):
    """a detached-copy teacher and target (distillation), a separate target moved by update_target (training), and the student as its
    own target (training, target_fn=None: two forwards of one module per step, the first without gradients)"""
    from v_diffusion.trainer import HotPathTrainer
    student, case = _tiny(vd, train=True)
    teacher = student.detached_copy().eval().requires_grad_(False) if distil else None
    frozen = None if teacher is None else [p.clone() for p in teacher.parameters()]
    cd = make_cd(vd, 4, "v", "snr_trunc", "huber", teacher, "v", 1.0 if distil else 0.0, target=None)
    if not own:
        cd.target_fn = cd.make_target(student)
    trainer = HotPathTrainer(student, cd, lr=1e-3, warmup=0, use_ema=False, timesteps=4)
    x0, y = _tiny_batch(case)
    losses = []
    for _ in range(3):
        losses.append(float(trainer.step(x0, y)))
        if not own:
            cd.update_target(student, 0.5)
        assert student.training
    assert all(v == v and abs(v) != float("inf") and v > 0 for v in losses), losses
    assert len(set(losses)) == 3, losses
    if frozen is not None:
        assert all(torch.equal(a, b) for a, b in zip(frozen, teacher.parameters())) and all(p.grad is None for p in teacher.parameters())


# ---- the sampler
def _sampler(vd, T, s, w):
    return vd.GaussianDiffusion(schedule(vd), T, s, "fixed_large", "constant", "mse", w_guide=w, p_uncond=0.0)


class Counting:
    training = False

    def __init__(self, stub):
        self.stub, self.times = stub, []

    def __call__(self, x, t, y):
        self.times.append(t.clone())
        return self.stub(x, t, y)


@pytest.mark.parametrize("s", ("v", "both"))
@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_sampler_is_a_loop_of_sample_step_on_the_replayed_stream(vd, shape, guided, s):
    """the draw-order contract: x_T first, then one image-shaped draw per non-final step, from one seeded generator; each step is the
    network call and one vd_sample_step launch with the row of consistency_sample_coefs, the last with last_step = 1"""
    from v_diffusion import _hip
    shp = SHAPES[shape]
    B, C, HW = shp[0], shp[1], shp[2] * shp[3]
    T, idx, seed = 1024, [1024, 700, 300, 1], 5
    w = W_GUIDE if guided else 0.0
    gd = _sampler(vd, T, s, w)
    net = Counting(student_stub(s))
    y = torch.arange(1, B + 1, dtype=torch.float32)
    for clip in (True, False):
        net.times.clear()
        got = gd.p_sample_consistency(net, shp, label=y, device=DEV, seed=seed, steps=idx, clip_denoised=clip)
        assert not got.is_cuda and len(net.times) == len(idx)
        assert [float(t_[0]) for t_ in net.times] == [i / T for i in idx]
        table, _ = vd.consistency_sample_coefs(gd.logsnr_fn, idx, T, s, w)
        g = torch.Generator(DEV).manual_seed(seed)
        x = torch.randn(shp, device=DEV, generator=g)
        yd = y.to(DEV)
        if guided:
            yd = yd.repeat_interleave(2).clone()
            yd[1::2] = 0
        for j, i in enumerate(idx):
            rows = B * (2 if guided else 1)
            x_in = x.repeat_interleave(2, dim=0) if guided else x
            out = student_stub(s)(x_in, torch.full((rows,), i / T, dtype=torch.float64, device=DEV), yd).float().contiguous()
            last = j == len(idx) - 1
            eps = None if last else torch.randn(shp, device=DEV, generator=g)
            xn = torch.empty_like(x)
            _hip.sample_step(x, out, eps, table[j].tolist(), _hip.OUT_TYPES[s], guided, last, clip, xn, None, B, C, HW)
            x = xn
        assert torch.equal(got, x.cpu())
        assert torch.equal(got, gd.p_sample_consistency(net, shp, label=y, device=DEV, seed=seed, steps=idx, clip_denoised=clip))


@pytest.mark.parametrize("s", ("v", "both"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_sampler_against_fp64(vd, shape, s):
    """guided and plain, clipped and not, 1 to 4 steps: the sampler may be at most 2x as far from the fp64 restatement as the fp32
    torch composition of the same arithmetic from the same rows (per run: plus 4 ulp of the row's scale)"""
    shp = SHAPES[shape]
    B, C = shp[:2]
    T, seed = 1024, 7
    y = torch.arange(1, B + 1, dtype=torch.float32)
    fn = schedule(vd)
    kmax = cmax = 0.0
    for guided in (False, True):
        w = W_GUIDE if guided else 0.0
        gd = _sampler(vd, T, s, w)
        for idx in ([1024], [1024, 512], [1024, 700, 300, 1]):
            for clip in (True, False):
                got = gd.p_sample_consistency(student_stub(s), shp, label=y, device=DEV, seed=seed, steps=idx, clip_denoised=clip)
                g = torch.Generator(DEV).manual_seed(seed)
                x_T = torch.randn(shp, device=DEV, generator=g)
                draws = [torch.randn(shp, device=DEV, generator=g) for _ in idx[1:]]
                ls = [float(fn(torch.tensor([i / T], dtype=torch.float64)).float()) for i in idx]
                ref = R.sample(student_stub(s), x_T.cpu().double(), [d.cpu().double() for d in draws], [i / T for i in idx], ls,
                               y.double(), s, w, clip)
                # composition: fp32 tensor ops from the table's rows
                table, _ = vd.consistency_sample_coefs(fn, idx, T, s, w)
                x, yd = x_T, y.to(DEV)
                for j, i in enumerate(idx):
                    k = table[j].tolist()
                    tt = torch.full((B,), i / T, dtype=torch.float64, device=DEV)

                    def pred(lab):
                        o = student_stub(s)(x, tt, lab)
                        p = k[0] * x + k[1] * o[:, :C] + (k[2] * o[:, C:] if s == "both" else 0.0)
                        return p.clamp(-1.0, 1.0) if clip else p
                    p = pred(yd)
                    if guided:
                        p = p + w * (p - pred(torch.zeros_like(yd)))
                    x = p if j == len(idx) - 1 else k[4] * p + k[5] * draws[j]
                ek, ec = row_err(got, ref), row_err(x, ref)
                assert ek <= 2.0 * ec + FLOOR, f"steps={idx} clip={clip} guided={guided}: sampler {ek:.3e}, composition {ec:.3e}"
                kmax, cmax = max(kmax, ek), max(cmax, ec)
    print(f"[consistency sampler {shape} {s}] sampler {kmax:.3e}  composition {cmax:.3e}")
    assert kmax <= 2.0 * cmax


def test_one_step_is_one_network_call_and_one_draw(vd):
    shp = SHAPES["75"]
    T = 8
    gd = _sampler(vd, T, "v", 0.0)
    net = Counting(student_stub("v"))
    torch.cuda.manual_seed(11)
    got = gd.p_sample_consistency(net, shp, device=DEV, steps=1)          # seed=None: the device's default generator
    after = torch.randn(4, device=DEV)
    assert len(net.times) == 1 and float(net.times[0][0]) == 1.0
    torch.cuda.manual_seed(11)
    x_T = torch.randn(shp, device=DEV)
    assert torch.equal(after, torch.randn(4, device=DEV))                 # nothing was drawn after the initial state
    # and the result is the clipped x0 prediction at t = 1
    a0, b0x = vd.consistency_sample_coefs(gd.logsnr_fn, 1, T, "v")[0][0, :2].tolist()
    tt = torch.ones(shp[0], dtype=torch.float64, device=DEV)
    want = (a0 * x_T + b0x * student_stub("v")(x_T, tt, None)).clamp(-1, 1)
    assert float((got - want.cpu()).abs().max()) <= 2.0 ** -22
    # a given initial state is used as it is, and the int and list forms agree
    a = gd.p_sample_consistency(net, shp, noise=x_T, device=DEV, steps=1)
    assert torch.equal(a, got)
    b = gd.p_sample_consistency(net, shp, device=DEV, seed=3, steps=2)
    c = gd.p_sample_consistency(net, shp, device=DEV, seed=3, steps=[8, 4])
    assert torch.equal(b, c) and not torch.equal(b, gd.p_sample_consistency(net, shp, device=DEV, seed=3, steps=[8, 5]))


def test_distillation_object_samples_with_it(vd):
    shp = SHAPES["75"]
    dd = vd.DistillationDiffusion(teacher_stub("v"), 4, logsnr_fn=schedule(vd), model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="constant")
    cd = make_cd(vd, 4, "v", "constant", "huber")
    a = dd.p_sample_consistency(student_stub("v"), shp, device=DEV, seed=2, steps=2)
    b = cd.p_sample_consistency(student_stub("v"), shp, device=DEV, seed=2, steps=2)
    assert a.shape == shp and bool(torch.isfinite(a).all()) and torch.equal(a, b)
