"""The DPM-Solver++(2M) sampler on the GPU (v_diffusion/solver.py over vd_solver_step) against the float64 restatement of
tests/solver_ref.py.  Networks of the kernel and chain tests are pointwise stand-ins, a(t) x + b(t) tanh(x) + g y, the same function
in fp64 on the CPU and in fp32 on the GPU.  The yardstick for the kernel's error is the same arithmetic, in the order the header
states, as plain fp32 torch ops on the GPU from the same table: kernel and composition differ in FMA contraction only, so the kernel
may be at most 2x as far from fp64, plus 4 ulp of the row's scale (both start from the same fp32 inputs and table and end in one fp32
rounding, each worth up to half an ulp that the comparison cannot see).  Needs an MI355X."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as R                                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {"75": (3, 3, 5, 5), "972": (2, 3, 18, 18)}    # C*HW = 75: odd, below one block, scalar; 972: above 256, 4 | 972, no multiple of 256, wide
MOTS = ("v", "eps", "x0", "both")
W_GUIDE = 1.5
FLOOR = 4 * 2.0 ** -24
GUARD, SENTINEL = 64, -12345.0


@pytest.fixture(scope="module")
def vd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import v_diffusion
    from v_diffusion import _hip
    _hip.lib()
    return v_diffusion


class Stub:
    """pointwise stand-in network"""

    training = False

    def __init__(self, a=(0.3, -0.5), b=(0.4, 0.3), g=0.07, both=False):
        self.a, self.b, self.g, self.both = a, b, g, both

    def __call__(self, x, t, y):
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        return torch.cat([out, 0.5 * out - 0.25 * x], dim=1) if self.both else out


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float()


def guarded(shape, offset=0):
    """a contiguous tensor of ``shape`` starting ``offset`` floats into a 16-byte aligned sentinel-filled buffer with GUARD floats
    behind it, and the check that the band was left alone"""
    n = int(torch.Size(shape).numel())
    buf = torch.full((offset + n + GUARD,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + n].view(shape), lambda: bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


def placed(t, offset=0):
    v, ok = guarded(t.shape, offset)
    v.copy_(t)
    return v, ok


@functools.lru_cache(maxsize=None)
def cosine_table(steps, mot, w):
    """computed once and shared (the tests only read it)"""
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    return (fn,) + tuple(vd.solver_coefs(fn, steps, order=2, spacing="time", model_out_type=mot, w_guide=w))


def step_inputs(vd, shape, mot, cfg, steps, row, seed):
    """table row ``row`` of the cosine +-20 schedule with ``steps`` steps; x_t at the row's log-SNR, a stand-in network output of
    n*(1+cfg) interleaved rows and C (2C) channels, and the previous prediction (zero on the first executed row)"""
    fn, table, t_net = cosine_table(steps, mot, W_GUIDE if cfg else 0.0)
    B, C = shape[:2]
    a, s = R.alpha_sigma(fn(t_net[row:row + 1].clone()).float())
    xt = (float(a) * rnd(shape, seed + 1).clamp(-1, 1).double() + float(s) * rnd(shape, seed + 2).double()).float()
    out = rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), seed + 3, 0.8)
    hist = torch.zeros(shape) if row == steps - 1 else rnd(shape, seed + 4, 0.7)
    return table[row], xt, out, hist


def run_kernel(H, k, xt, out, hist, mot, cfg, clip, alias=False, k_dev=False, offset=0):
    """(xn, new hist, xdup, guard bands intact) of one launch on device copies of the inputs placed ``offset`` floats off alignment"""
    B, C = xt.shape[:2]
    HW = xt[0, 0].numel()
    (xd, ok_x), (od, _), (hd, ok_h) = placed(xt, offset), placed(out, offset), placed(hist, offset)
    xn, ok_n = (xd, ok_x) if alias else guarded(xt.shape, offset)
    xdup, ok_d = guarded((2 * B,) + tuple(xt.shape[1:]), offset) if cfg else (None, lambda: True)
    kd = k.to(DEV).contiguous() if k_dev else None
    H.solver_step(xd, od, hd, None if k_dev else k.tolist(), H.OUT_TYPES[mot], cfg, clip, xn, xdup, B, C, HW, k_dev=kd)
    torch.cuda.synchronize()
    assert torch.equal(od.cpu(), out) and (alias or torch.equal(xd.cpu(), xt))           # inputs left alone
    return xn.clone(), hd.clone(), None if xdup is None else xdup.clone(), ok_n() and ok_h() and ok_d()


def fp64_step(k, xt, out, hist, mot, cfg, clip):
    oc, ou = (out[0::2], out[1::2]) if cfg else (out, out)
    net = lambda x, t, lab: (oc if bool(lab.any()) else ou).double()
    g = R.guided_x0(net, xt.double(), None, torch.ones(xt.shape[0]), k.double(), mot == "both", cfg, clip)
    return R.step(xt.double(), g, hist.double(), k.double()), g


def composition(k, xt, out, hist, mot, cfg, clip):
    """the kernel's arithmetic in its stated order as fp32 tensor ops on the GPU"""
    a0, b0x, b0e, c1, c2, c2r, w, _ = k.tolist()
    xt, out, hist = xt.to(DEV), out.to(DEV), hist.to(DEV)
    C = xt.shape[1]

    def pred(o):
        p = a0 * xt + b0x * o[:, :C]
        if mot == "both":
            p = p + b0e * o[:, C:]
        return p.clamp(-1.0, 1.0) if clip else p
    if cfg:
        xc, xu = pred(out[0::2]), pred(out[1::2])
        g = xc + w * (xc - xu)
    else:
        g = pred(out)
    return c1 * xt + c2 * g + c2r * (g - hist), g


def row_err(got, ref):
    """max over rows of the row's max error relative to the row's own scale"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.detach().double().reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1).clamp(min=1e-300)
    return float(((got - ref).abs().amax(dim=1) / scale).max())


@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_kernel_against_fp64(vd, shape, mot, cfg, clip):
    """xn, the new hist and xdup on a first row (c2rho = 0, zero hist), an interior row and row 0, at 8 steps and at 1024 (weights near 1)"""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    worst = {"xn": (0.0, 0.0), "hist": (0.0, 0.0)}
    for steps, mid in ((8, 3), (1024, 300)):
        for row in (steps - 1, mid, 0):
            k, xt, out, hist = step_inputs(vd, shp, mot, cfg, steps, row, seed=17 + row)
            xn, hn, xdup, intact = run_kernel(H, k, xt, out, hist, mot, cfg, clip)
            ref = fp64_step(k, xt, out, hist, mot, cfg, clip)
            cmp = composition(k, xt, out, hist, mot, cfg, clip)
            assert intact, "guard band written"
            if row == 0:
                assert torch.equal(xn, hn)                                  # (0, 1, 0): the guided x0 prediction itself
            for q, g_, r_, c_ in zip(("xn", "hist"), (xn, hn), ref, cmp):
                ek, ec = row_err(g_, r_), row_err(c_, r_)
                worst[q] = max(worst[q], (ek, ec))
                assert ek <= 2.0 * ec + FLOOR, f"{q} steps={steps} row={row}: kernel {ek:.3e}, composition {ec:.3e}"
            if cfg:
                assert torch.equal(xdup[0::2], xn) and torch.equal(xdup[1::2], xn)
    print(f"[solver step {shape} {mot} {'guided' if cfg else 'plain'} {'clip' if clip else 'noclip'}] "
          + "  ".join(f"{q}: kernel {v[0]:.3e} composition {v[1]:.3e}" for q, v in worst.items()))


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_aliasing_forms_alignment_and_guard_bands(vd, shape, mot, cfg):
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    k, xt, out, hist = step_inputs(vd, shp, mot, cfg, 8, 3, seed=5)
    base = run_kernel(H, k, xt, out, hist, mot, cfg, True)
    assert base[3], "guard band written"
    for what, kw in (("xn aliasing xt", dict(alias=True)), ("k_dev", dict(k_dev=True)), ("bases one float off alignment", dict(offset=1)),
                     ("aliased, k_dev, off alignment", dict(alias=True, k_dev=True, offset=3))):
        got = run_kernel(H, k, xt, out, hist, mot, cfg, True, **kw)
        assert got[3], f"{what}: guard band written"
        for a, b in zip(base[:3], got[:3]):
            assert (a is None and b is None) or torch.equal(a, b), what


def test_entry_point_refuses_bad_arguments(vd):
    from v_diffusion import _hip as H
    z = torch.zeros((2, 3, 4, 4), device=DEV)
    k = [0.0] * 8
    with pytest.raises(H.HipError, match="either"):
        H.solver_step(z, z.clone(), z.clone(), k, 0, False, False, z.clone(), None, 2, 3, 16, k_dev=torch.zeros(8, device=DEV))
    with pytest.raises(H.HipError, match="null"):
        H.solver_step(z, z.clone(), None, k, 0, False, False, z.clone(), None, 2, 3, 16)
    with pytest.raises(H.HipError, match="model_out_type"):
        H.solver_step(z, z.clone(), z.clone(), k, 4, False, False, z.clone(), None, 2, 3, 16)
    with pytest.raises(H.HipError, match="empty"):
        H.solver_step(z, z.clone(), z.clone(), k, 0, False, False, z.clone(), None, 0, 3, 16)
    with pytest.raises(H.HipError, match="of its own"):
        H.solver_step(z, z.clone(), z, k, 0, False, False, z.clone(), None, 2, 3, 16)


def test_order_one_against_the_existing_ddim_sampler(vd):
    """p_sample_solver(order=1) and p_sample(use_ddim=True) evaluate the same formula from the same numbers in different groupings
    (the existing kernel guides the two means, this one the two predictions): each is held to the fp64 chain, not to the other"""
    shp, T, w = SHAPES["972"], 8, 1.0
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    gd = vd.GaussianDiffusion(fn, T, "v", "fixed_large", "snr_trunc", "mse", w_guide=w, p_uncond=0.0)
    noise, y = rnd(shp, 29), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    new = gd.p_sample_solver(Stub(), shp, noise=noise, label=y, device=DEV, order=1, spacing="time")
    old = gd.p_sample(Stub(), shp, noise=noise, label=y, device=DEV, use_ddim=True)
    table, t_net = vd.solver_coefs(fn, T, order=1, spacing="time", model_out_type="v", w_guide=w)
    ref = R.chain(Stub(), noise, table, t_net, y.double(), cfg=True, clip=True)
    scale = float(ref.abs().max())
    en, eo = float((new.double() - ref).abs().max()), float((old.double() - ref).abs().max())
    print(f"[solver order 1 vs DDIM, T={T}] p_sample_solver {en:.3e}  p_sample {eo:.3e}  (scale {scale:.3e})")
    assert new.shape == shp and new.device.type == "cpu"
    assert en <= 2.0 * eo + FLOOR * scale, (en, eo)
    # order 2 on the same chain: a different trajectory, again the fp64 chain's to the same bound
    new2 = gd.p_sample_solver(Stub(), shp, noise=noise, label=y, device=DEV, order=2)
    table2, _ = vd.solver_coefs(fn, T, order=2, spacing="time", model_out_type="v", w_guide=w)
    ref2 = R.chain(Stub(), noise, table2, t_net, y.double(), cfg=True, clip=True)
    e2 = float((new2.double() - ref2).abs().max())
    print(f"[solver order 2, T={T}] p_sample_solver {e2:.3e}  (differs from order 1 by {float((new2 - new).abs().max()):.3e})")
    assert not torch.equal(new2, new)
    assert e2 <= 2.0 * eo + FLOOR * float(ref2.abs().max()), (e2, eo)


def test_order_of_convergence_through_the_kernel(vd):
    """the Gaussian problem of test_solver_cpu.py through p_sample_solver: x_T = z sqrt(alpha_1^2 s^2 + sigma_1^2), the stub's factor in
    fp64 from logsnr_fn(t) and cast to fp32, no clip.  The chain ends on the x0 prediction at tau_1, factor(tau_1) * x(tau_1): dividing
    by factor(tau_1) * z gives the state at tau_1 per unit z, which the three conditions are stated for."""
    shp = (2, 3, 5, 5)
    z = rnd(shp, 43)
    z = torch.where(z.abs() < 0.05, torch.full_like(z, 0.05), z)                # the error is measured relative to z
    fn = vd.get_logsnr_schedule("cosine", -6.0, 6.0)
    calls = []

    def run(net, m1, table, t_net, order):
        T = len(table)
        gd = vd.GaussianDiffusion(fn, T, "x0", "fixed_large", "snr_trunc", "mse", w_guide=0.0, p_uncond=0.0)
        factor = lambda t: net(torch.ones((t.numel(), 1, 1, 1), dtype=torch.float64), t.cpu(), None)

        def dev_net(x, t, y):
            calls.append(float(t[0]))
            return factor(t).float().to(x.device) * x
        out = gd.p_sample_solver(dev_net, shp, noise=(z.double() * m1).float(), device=DEV, order=order, spacing="logsnr",
                                 clip_denoised=False)
        assert calls[-T:] == list(reversed(t_net.tolist()))                     # one network call per step, at the grid times
        return out.double() / (factor(t_net[0:1]) * z.double())

    R.check_convergence(R.convergence_errors(fn, vd.solver_coefs, 1, run), R.convergence_errors(fn, vd.solver_coefs, 2, run))


def _tiny(vd):
    from oracle.cases import TINY, make_weights
    case = TINY["tinyA"]                                          # attention, class labels
    model = vd.UNet(**case["cfg"])
    model.load_state_dict(make_weights(case["cfg"]), strict=True)
    return model.to(DEV).eval(), case


def test_real_network_eager_graph_and_distillation_object(vd):
    model, case = _tiny(vd)
    B, R_, T = 2, case["R"], 4
    shp = (B, 3, R_, R_)
    y = torch.tensor([1.0, 4.0])
    gd = vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0)
    a = gd.p_sample_solver(model, shp, label=y, seed=5)
    b = gd.p_sample_solver(model, shp, label=y, seed=5, use_graph=False)
    assert a.shape == shp and a.device.type == "cpu" and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    # only x_T is drawn, and it is p_sample's: the first draw of the seeded generator
    x_T = torch.randn(shp, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    assert torch.equal(a, gd.p_sample_solver(model, shp, noise=x_T, label=y))
    c = gd.p_sample_solver(model, shp, label=y, seed=5, use_graph=True)
    d = gd.p_sample_solver(model, shp, label=y, seed=5, use_graph=True)            # cached graph
    assert torch.equal(a, c) and torch.equal(a, d), (a - c).abs().max()
    assert len(gd._solver_graphs) == 1 and "_graphs" not in gd.__dict__            # a cache of its own
    entry = next(iter(gd._solver_graphs.values()))
    assert entry[2] is not None                                                    # the entry pins the forward's ConvPacks
    # other steps / order / spacing are data of the same graph
    e = gd.p_sample_solver(model, shp, label=y, seed=5, steps=3, order=1, spacing="logsnr", use_graph=True)
    assert torch.equal(e, gd.p_sample_solver(model, shp, label=y, seed=5, steps=3, order=1, spacing="logsnr")) and len(gd._solver_graphs) == 1
    assert not torch.equal(a, gd.p_sample_solver(model, shp, label=y, seed=5, order=1))
    dd = vd.DistillationDiffusion(model, T, logsnr_fn=gd.logsnr_fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="snr_trunc")
    s = dd.p_sample_solver(model, shp, label=y, seed=5)
    assert s.shape == shp and bool(torch.isfinite(s).all())
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_solver(model, shp, label=y, seed=5, device="cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_solver(vd.UNet(**case["cfg"]).eval(), shp, label=y, seed=5)    # parameters on the CPU
