"""The UniPC sampler on the GPU (v_diffusion/unipc.py over vd_unipc_step) against the float64 restatement of tests/unipc_ref.py.  The
networks of the kernel and chain tests are pointwise stand-ins (``unipc_ref.Stub``), the same function in fp64 on the CPU and in fp32 on
the GPU.  The yardstick for the kernel's error is the one of tests/test_solver_gpu.py: the same arithmetic, in the order the header
states, as plain fp32 torch ops on the GPU from the same table.  Kernel and composition differ in FMA contraction only, so the kernel
may be at most 2x as far from fp64, plus 4 ulp of the row's scale (both start from the same fp32 inputs and table and end in one fp32
rounding, each worth up to half an ulp that the comparison cannot see).  Needs an MI355X."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unipc_ref as U                                             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {"75": (3, 3, 5, 5), "972": (2, 3, 18, 18)}    # C*HW = 75: odd, below one block, scalar; 972: above 256, 4 | 972, no multiple of 256, wide
MOTS = ("v", "eps", "x0", "both")
W_GUIDE = 1.5
FLOOR = 4 * 2.0 ** -24
GUARD, SENTINEL = 64, -12345.0
STEPS, MID = 8, 3                                       # row 3 of 8: the fifth node, order 3 on both sides, with the corrector


@pytest.fixture(scope="module")
def vd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import v_diffusion
    from v_diffusion import _hip
    _hip.lib()
    return v_diffusion


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
def cosine_table(mot, w):
    """computed once and shared (the tests only read it)"""
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    return (fn,) + tuple(vd.unipc_coefs(fn, STEPS, order=3, variant="bh2", corrector=True, spacing="time", model_out_type=mot, w_guide=w))


def step_inputs(shape, mot, cfg, row, seed):
    """table row ``row``; x_t at the row's log-SNR, a stand-in network output of n*(1+cfg) interleaved rows and C (2C) channels, and
    the three previous predictions (zero on the first executed row)"""
    fn, table, t_net = cosine_table(mot, W_GUIDE if cfg else 0.0)
    B, C = shape[:2]
    a, s = U.alpha_sigma(fn(t_net[row:row + 1].clone()).float())
    xt = (float(a) * rnd(shape, seed + 1).clamp(-1, 1).double() + float(s) * rnd(shape, seed + 2).double()).float()
    out = rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), seed + 3, 0.8)
    hs = [torch.zeros(shape) if row == STEPS - 1 else rnd(shape, seed + 4 + j, 0.7) for j in range(3)]
    return table[row], xt, out, hs


def run_kernel(H, k, xt, out, hs, mot, cfg, clip, alias=False, k_dev=False, offset=0, want_xc=True):
    """(xn, xc, h0, h1, h2, xdup) of one launch on device copies of the inputs placed ``offset`` floats off alignment, and whether
    every guard band is intact"""
    B, C = xt.shape[:2]
    HW = xt[0, 0].numel()
    (xd, ok_x), (od, ok_o) = placed(xt, offset), placed(out, offset)
    hd = [placed(h, offset) for h in hs]
    xn, ok_n = (xd, ok_x) if alias else guarded(xt.shape, offset)
    xc, ok_c = guarded(xt.shape, offset) if want_xc else (None, lambda: True)
    xdup, ok_d = guarded((2 * B,) + tuple(xt.shape[1:]), offset) if cfg else (None, lambda: True)
    kd = k.to(DEV).contiguous() if k_dev else None
    H.unipc_step(xd, od, hd[0][0], hd[1][0], hd[2][0], None if k_dev else k.tolist(), H.OUT_TYPES[mot], cfg, clip, xn, xdup, xc, B, C, HW,
                 k_dev=kd)
    torch.cuda.synchronize()
    assert torch.equal(od.cpu(), out) and (alias or torch.equal(xd.cpu(), xt))           # inputs left alone
    intact = ok_x() and ok_o() and ok_n() and ok_c() and ok_d() and all(ok() for _, ok in hd)
    clone = lambda t: None if t is None else t.clone()
    return [clone(t) for t in (xn, xc, hd[0][0], hd[1][0], hd[2][0], xdup)], intact


def split(out, cfg):
    return (out[0::2], out[1::2]) if cfg else (out, None)


def fp64_node(k, xt, out, hs, mot, cfg, clip):
    oc, ou = split(out.double(), cfg)
    return U.node(k.double().tolist(), xt.double(), oc, ou, *[h.double() for h in hs], both=mot == "both", cfg=cfg, clip=clip)


def composition(k, xt, out, hs, mot, cfg, clip):
    """the kernel's arithmetic in its stated order as fp32 tensor ops on the GPU"""
    oc, ou = split(out.to(DEV), cfg)
    return U.node(k.double().tolist(), xt.to(DEV), oc, ou, *[h.to(DEV) for h in hs], both=mot == "both", cfg=cfg, clip=clip)


def row_err(got, ref):
    """max over rows of the row's max error relative to the row's own scale"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.detach().cpu().double().reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1).clamp(min=1e-300)
    return float(((got - ref).abs().amax(dim=1) / scale).max())


@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_kernel_against_fp64(vd, shape, mot, cfg, clip):
    """xn, xc_out, the new h0 (by the bound) and h1, h2, xdup (bitwise) on the first row (zero history, e = 0), a middle row at order 3
    with the corrector, and row 0; then the middle row again with xn aliasing xt, device coefficients, and every base 4 bytes off
    alignment (the scalar form), each bit for bit the plain launch"""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    worst = {"xn": (0.0, 0.0), "xc": (0.0, 0.0), "h0": (0.0, 0.0)}
    for row in (STEPS - 1, MID, 0):
        k, xt, out, hs = step_inputs(shp, mot, cfg, row, seed=17 + row)
        ks = k.tolist()
        if row == STEPS - 1:
            assert ks[6:] == [0.0] * 10                           # order 1 leaves, nothing arrived
        if row == MID:
            assert all(v != 0.0 for v in ks[4:11])
        if row == 0:
            assert ks[4:8] == [0.0, 1.0, 0.0, 0.0] and all(v != 0.0 for v in ks[8:11])
        (xn, xc, h0, h1, h2, xdup), intact = run_kernel(H, k, xt, out, hs, mot, cfg, clip)
        ref = fp64_node(k, xt, out, hs, mot, cfg, clip)
        cmp = composition(k, xt, out, hs, mot, cfg, clip)
        assert intact, "guard band written"
        assert torch.equal(h1.cpu(), hs[0]) and torch.equal(h2.cpu(), hs[1])
        if row == STEPS - 1:
            assert torch.equal(xc.cpu(), xt)                      # e = 0: the corrected state is the state
        if row == 0:
            assert torch.equal(xn, h0)                            # (0, 1, 0, 0): the guided x0 prediction itself
        for q, g_, r_, c_ in zip(("xn", "xc", "h0"), (xn, xc, h0), ref, cmp):
            ek, ec = row_err(g_, r_), row_err(c_, r_)
            worst[q] = max(worst[q], (ek, ec))
            assert ek <= 2.0 * ec + FLOOR, f"{q} row={row}: kernel {ek:.3e}, composition {ec:.3e}"
        if cfg:
            assert torch.equal(xdup[0::2], xn) and torch.equal(xdup[1::2], xn)
        if row != MID:
            continue
        base = (xn, xc, h0, h1, h2, xdup)
        for what, kw in (("xn aliasing xt", dict(alias=True)), ("k_dev", dict(k_dev=True)), ("bases one float off alignment", dict(offset=1)),
                         ("aliased, k_dev, off alignment, no xc_out", dict(alias=True, k_dev=True, offset=3, want_xc=False))):
            got, intact = run_kernel(H, k, xt, out, hs, mot, cfg, clip, **kw)
            assert intact, f"{what}: guard band written"
            for a, b in zip(base, got):
                assert b is None or torch.equal(a, b), what
    print(f"[unipc node {shape} {mot} {'guided' if cfg else 'plain'} {'clip' if clip else 'noclip'}] "
          + "  ".join(f"{q}: kernel {v[0]:.3e} composition {v[1]:.3e}" for q, v in worst.items()))


@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_history_shifts_by_one(vd, shape):
    """after one launch h2 = the old h1, h1 = the old h0 and h0 = g -- the same bits the launch used for xn, read off row 0, whose xn is g"""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    for cfg in (False, True):
        k, xt, out, hs = step_inputs(shp, "v", cfg, 0, seed=71)
        (xn, _, h0, h1, h2, _), intact = run_kernel(H, k, xt, out, hs, "v", cfg, True)
        assert intact
        assert torch.equal(h2.cpu(), hs[1]) and torch.equal(h1.cpu(), hs[0]) and torch.equal(h0, xn)
        assert not torch.equal(h0.cpu(), hs[0])
        # a second launch on the shifted buffers moves them once more
        (_, _, g0, g1, g2, _), _ = run_kernel(H, k, xt, out, [h0.cpu(), h1.cpu(), h2.cpu()], "v", cfg, True)
        assert torch.equal(g2, h1) and torch.equal(g1, h0) and torch.equal(g0, h0)        # same inputs: the same g


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
def test_reduces_to_the_solver_step(vd, mot, cfg):
    """a row with e = 0, p2 = 0 and p1 = -c2rho against vd_solver_step on the same inputs: the two updates differ by where one sign
    sits (p1*(h0 - g) against c2rho*(g - h0)), so xn agrees within 1 ulp of the row's scale and the stored prediction bit for bit"""
    from v_diffusion import _hip as H
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    table, _ = vd.solver_coefs(fn, STEPS, order=2, spacing="time", model_out_type=mot, w_guide=W_GUIDE if cfg else 0.0)
    a0, b0x, b0e, c1, c2, c2rho, w, _ = k8 = table[MID].tolist()
    assert c2rho != 0.0
    k16 = torch.tensor([a0, b0x, b0e, w, c1, c2, -c2rho, 0.0] + [0.0] * 8)
    for shape, shp in SHAPES.items():
        _, xt, out, hs = step_inputs(shp, mot, cfg, MID, seed=5)
        (xn, xc, h0, _, _, xdup), intact = run_kernel(H, k16, xt, out, hs, mot, cfg, True)
        B, C = shp[:2]
        xd, od, hd = xt.to(DEV), out.to(DEV), hs[0].to(DEV)
        xs = torch.empty_like(xd)
        H.solver_step(xd, od, hd, k8, H.OUT_TYPES[mot], cfg, True, xs, None, B, C, shp[2] * shp[3])
        torch.cuda.synchronize()
        err = row_err(xn, xs)
        print(f"[unipc as solver step {shape} {mot} {'guided' if cfg else 'plain'}] {err:.3e}")
        assert intact and err <= 2.0 ** -23, err
        assert torch.equal(h0, hd) and torch.equal(xc.cpu(), xt)


def chain_case(vd, shp, T, cfg, order, variant, mot="v", clip=True):
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    w = 1.0 if cfg else 0.0
    gd = vd.GaussianDiffusion(fn, T, mot, "fixed_large", "snr_trunc", "mse", w_guide=w, p_uncond=0.0)
    y = torch.arange(1, shp[0] + 1, dtype=torch.float32) if cfg else None
    return fn, gd, w, y


def test_whole_chain(vd):
    """p_sample_unipc with the stand-in network, T = 6, guided and plain, orders 1-3, both variants, against the fp64 chains: the
    published form (which the table is off by its fp32 rounding) and the same table in fp64 (which the sampler is off by its own rounding
    only).  The fp32 composition of the same chain is measured against each in the same way; the sampler may be 2x as far plus the floor."""
    shp, T = SHAPES["972"], 6
    noise = rnd(shp, 29)
    net = U.Stub()
    for cfg in (False, True):
        for order in (1, 2, 3):
            for variant in ("bh1", "bh2"):
                fn, gd, w, y = chain_case(vd, shp, T, cfg, order, variant)
                got = gd.p_sample_unipc(net, shp, noise=noise, label=y, device=DEV, order=order, variant=variant)
                assert got.shape == shp and got.device.type == "cpu"
                table, t_net = vd.unipc_coefs(fn, T, order=order, variant=variant, model_out_type="v", w_guide=w)
                y64 = None if y is None else y.double()
                pub = U.chain(net, noise, fn, [0.0] + t_net.tolist(), order, variant, True, y=y64, out_type="v", w=w, cfg=cfg, clip=True)
                tab = U.table_chain(net, noise, table, t_net, y64, cfg=cfg, clip=True)[0]
                cmp = U.table_chain(net, noise.to(DEV), table, t_net, y, cfg=cfg, clip=True, dtype=torch.float32)[0].cpu()
                for name, ref in (("published form", pub), ("table in fp64", tab)):
                    scale = float(ref.abs().max())
                    ek, ec = float((got.double() - ref).abs().max()), float((cmp.double() - ref).abs().max())
                    print(f"[unipc chain T={T} {'guided' if cfg else 'plain'} order {order} {variant} vs {name}] sampler {ek:.3e} "
                          f"composition {ec:.3e} (scale {scale:.3e})")
                    assert ek <= 2.0 * ec + FLOOR * scale, (name, ek, ec)
                assert torch.equal(got, gd.p_sample_unipc(net, shp, noise=noise, label=y, device=DEV, order=order, variant=variant))
    # without the corrector, and other orders, are other trajectories
    fn, gd, w, y = chain_case(vd, shp, T, True, 3, "bh2")
    runs = [gd.p_sample_unipc(net, shp, noise=noise, label=y, device=DEV, **kw)
            for kw in (dict(), dict(corrector=False), dict(order=2), dict(variant="bh1"), dict(spacing="logsnr"))]
    for i in range(len(runs)):
        for j in range(i):
            assert not torch.equal(runs[i], runs[j]), (i, j)
    # bh2, order 2, no corrector is p_sample_solver(order=2) up to the sign placement of one fused multiply-add per step
    old = gd.p_sample_solver(net, shp, noise=noise, label=y, device=DEV, order=2)
    new = gd.p_sample_unipc(net, shp, noise=noise, label=y, device=DEV, order=2, corrector=False)
    assert float((old - new).abs().max()) <= 1e-5 * float(old.abs().max())


def _tiny(vd):
    from oracle.cases import TINY, make_weights
    case = TINY["tinyA"]                                          # attention, class labels
    model = vd.UNet(**case["cfg"])
    model.load_state_dict(make_weights(case["cfg"]), strict=True)
    return model.to(DEV).eval(), case


def test_real_network_graph_equals_eager_and_seeds_repeat(vd):
    model, case = _tiny(vd)
    B, R_, T = 2, case["R"], 4
    shp = (B, 3, R_, R_)
    y = torch.tensor([1.0, 4.0])
    gd = vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0)
    a = gd.p_sample_unipc(model, shp, label=y, seed=5)
    b = gd.p_sample_unipc(model, shp, label=y, seed=5)
    assert a.shape == shp and a.device.type == "cpu" and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    x_T = torch.randn(shp, device=DEV, generator=torch.Generator(DEV).manual_seed(5))          # only x_T is drawn, and it is p_sample's
    assert torch.equal(a, gd.p_sample_unipc(model, shp, noise=x_T, label=y))
    c = gd.p_sample_unipc(model, shp, label=y, seed=5, use_graph=True)
    d = gd.p_sample_unipc(model, shp, label=y, seed=5, use_graph=True)                         # cached graph
    assert torch.equal(a, c) and torch.equal(a, d), (a - c).abs().max()
    assert len(gd._unipc_graphs) == 1 and "_graphs" not in gd.__dict__ and "_solver_graphs" not in gd.__dict__
    # other steps / order / variant / corrector / spacing are data of the same graph
    kw = dict(steps=3, order=2, variant="bh1", corrector=False, spacing="logsnr")
    e = gd.p_sample_unipc(model, shp, label=y, seed=5, use_graph=True, **kw)
    assert torch.equal(e, gd.p_sample_unipc(model, shp, label=y, seed=5, **kw)) and len(gd._unipc_graphs) == 1
    assert not torch.equal(a, e)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_unipc(model, shp, label=y, seed=5, device="cpu")


def test_convergence_through_the_kernel(vd):
    """the Gaussian problem of tests/unipc_ref.py (s = 2, cosine on [-6, 6], log-SNR-uniform grid) through vd_unipc_step: the exact
    x0-network's factor in fp64 from logsnr_fn(t), cast to fp32 and applied on the GPU, the state corrected at node 1 read from xc_out,
    e(T) = max |x(tau_1) / (z exact(tau_1)) - 1|.  fp64 figures of the same chains: unipc_ref.TABLE; each condition is met there with
    margin (e.g. corrector order 2, bh2: 4.000e-3 / 5.325e-4 = 7.5 >= 5).  No condition at T = 64: 4.7e-7 is at fp32 rounding."""
    from v_diffusion import _hip as H
    shp = (2, 3, 5, 5)
    B, C, HW = 2, 3, 25
    z = rnd(shp, 43)
    z = torch.where(z.abs() < 0.05, torch.full_like(z, 0.05), z)                # the error is measured relative to z
    fn = vd.get_logsnr_schedule("cosine", -6.0, 6.0)
    scale, net = U.gaussian_problem(fn)
    factor = lambda t: float(net(torch.ones((1, 1, 1, 1), dtype=torch.float64), torch.tensor([t], dtype=torch.float64), None))

    def err(T, order, variant, corrector):
        table, t_net = vd.unipc_coefs(fn, T, order=order, variant=variant, corrector=corrector, spacing="logsnr", model_out_type="x0")
        x = (z.double() * scale(1.0)[2]).float().to(DEV)
        h0, h1, h2, xc = (torch.zeros_like(x) for _ in range(4))
        for i in reversed(range(T)):
            out = torch.tensor(factor(float(t_net[i])), dtype=torch.float32) * x
            H.unipc_step(x, out, h0, h1, h2, table[i].tolist(), H.OUT_TYPES["x0"], False, False, x, None, xc, B, C, HW)
        return float((xc.cpu().double() / (z.double() * scale(float(t_net[0]))[2]) - 1.0).abs().max())

    for variant in ("bh1", "bh2"):
        e = {(c, o, T): err(T, o, variant, c) for c, o in ((True, 1), (True, 2), (True, 3), (False, 2), (False, 3)) for T in (16, 32)}
        for (c, o) in ((True, 1), (True, 2), (True, 3), (False, 2), (False, 3)):
            print(f"[unipc convergence {variant} corrector={c} order {o}] e(16) {e[c, o, 16]:.3e}  e(32) {e[c, o, 32]:.3e}  "
                  f"(fp64: {U.TABLE[variant, c, o][1]:.3e} {U.TABLE[variant, c, o][2]:.3e})")
        assert e[True, 2, 16] / e[True, 2, 32] >= 5, variant
        assert e[True, 1, 16] / e[True, 1, 32] >= 3, variant
        assert e[True, 2, 32] <= e[False, 2, 32] / 3, variant
        assert e[True, 3, 32] <= e[True, 2, 32] / 8, variant
        assert e[False, 3, 32] <= e[False, 2, 32] / 8, variant


def test_distillation_object_runs_the_sampler(vd):
    model, case = _tiny(vd)
    shp, T = (2, 3, case["R"], case["R"]), 4
    y = torch.tensor([1.0, 4.0])
    dd = vd.DistillationDiffusion(model, T, logsnr_fn=vd.get_logsnr_schedule("cosine", -20.0, 20.0), model_out_type="v",
                                  model_var_type="fixed_large", reweight_type="snr_trunc")
    s = dd.p_sample_unipc(model, shp, label=y, seed=5)
    assert s.shape == shp and s.device.type == "cpu" and bool(torch.isfinite(s).all())
    assert torch.equal(s, dd.p_sample_unipc(model, shp, label=y, seed=5))
    assert not torch.equal(s, dd.p_sample_unipc(model, shp, label=y, seed=5, order=1, corrector=False))


def test_refusals_come_before_any_launch(vd):
    from v_diffusion import _hip as H
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)

    def net(x, t, y):
        raise AssertionError("the network was called")
    mk = lambda **kw: vd.GaussianDiffusion(fn, 4, "v", kw.pop("model_var_type", "fixed_large"), "snr_trunc", "mse", w_guide=0.0, p_uncond=0.0, **kw)
    shp = (2, 3, 4, 4)
    with pytest.raises(NotImplementedError, match="learned"):
        mk(model_var_type="learned").p_sample_unipc(net, shp, device=DEV)
    with pytest.raises(NotImplementedError, match="x0eps_coef"):
        mk(x0eps_coef=True).p_sample_unipc(net, shp, device=DEV)
    with pytest.raises(NotImplementedError, match="dynamic"):
        mk().p_sample_unipc(net, shp, device=DEV, clip_denoised="dynamic")
    with pytest.raises(ValueError, match="order"):
        mk().p_sample_unipc(net, shp, device=DEV, order=4)
    with pytest.raises(ValueError, match="variant"):
        mk().p_sample_unipc(net, shp, device=DEV, variant="vary_coeff")
    # the entry point's own refusals
    z = torch.zeros(shp, device=DEV)
    k = [0.0] * 16
    new = lambda: torch.zeros(shp, device=DEV)
    with pytest.raises(H.HipError, match="either"):
        H.unipc_step(z, new(), new(), new(), new(), k, 0, False, False, new(), None, None, 2, 3, 16, k_dev=torch.zeros(16, device=DEV))
    with pytest.raises(H.HipError, match="either"):
        H.unipc_step(z, new(), new(), new(), new(), None, 0, False, False, new(), None, None, 2, 3, 16)
    with pytest.raises(H.HipError, match="null"):
        H.unipc_step(z, new(), new(), None, new(), k, 0, False, False, new(), None, None, 2, 3, 16)
    with pytest.raises(H.HipError, match="model_out_type"):
        H.unipc_step(z, new(), new(), new(), new(), k, 4, False, False, new(), None, None, 2, 3, 16)
    with pytest.raises(H.HipError, match="empty"):
        H.unipc_step(z, new(), new(), new(), new(), k, 0, False, False, new(), None, None, 0, 3, 16)
    with pytest.raises(H.HipError, match="cfg"):
        H.unipc_step(z, new(), new(), new(), new(), k, 0, False, False, new(), torch.zeros((4, 3, 4, 4), device=DEV), None, 2, 3, 16)
    h = new()
    for hs in ((z, new(), new()), (h, h, new()), (new(), h, h), (h, new(), h)):
        with pytest.raises(H.HipError, match="of its own"):
            H.unipc_step(z, new(), *hs, k, 0, False, False, new(), None, None, 2, 3, 16)
    with pytest.raises(H.HipError, match="of its own"):
        H.unipc_step(z, new(), new(), new(), h, k, 0, False, False, h, None, None, 2, 3, 16)            # a history image as xn
    with pytest.raises(H.HipError, match="of its own"):
        H.unipc_step(z, new(), new(), new(), new(), k, 0, False, False, h, None, h, 2, 3, 16)            # xc_out as xn
    assert float(z.abs().max()) == 0.0
