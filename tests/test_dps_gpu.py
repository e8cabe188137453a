"""Diffusion Posterior Sampling on the GPU: the input-gradient-only backward pass of the UNet (``UNet.forward_vjp``, the frozen-network
autograd node), the two kernels vd_dps_residual / vd_dps_step against the float64 restatement of tests/dps_ref.py, and the chains of
``GaussianDiffusion.p_sample_dps``.

The input-only pass is held to the FULL backward pass bit for bit and to the reference's dx in tests/golden/unet_<name>.npz.  The yardstick
of a kernel's error is the rule of tests/test_inpaint_gpu.py: the same arithmetic as plain fp32 torch ops on the GPU from the same
coefficients (dps_ref's functions on fp32 GPU tensors) -- the kernel may be at most 2x as far from fp64, plus 4 ulp of the row's scale.
Inputs of the clipped cases are kept 1e-3 away from the clip's two corners, where the pass mask of fp32 and fp64 arithmetic may
legitimately differ.  The exact properties compare the new kernels with the existing step kernel or with themselves.  Networks of the kernel
and stand-in chain tests are the pointwise a(t) x + b(t) tanh(x) + g y of the other sampler tests.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dps_ref as R                                               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MOTS = ("v", "eps", "x0", "both")
W_GUIDE = 1.5
FLOOR = 4 * 2.0 ** -24
GUARD, SENTINEL = 64, -12345.0
NAN, INF = float("nan"), float("inf")
# (shape, operator, par): C*HW = 75 odd and scalar; 100 = 4*25, a wide access would straddle the channels of a one-channel mask; 972 wide;
# a non-square image; one block per channel; both channel counts of the grey operator
CASES = {"mask75": ((3, 3, 5, 5), "mask", 3), "mask100one": ((2, 4, 5, 5), "mask", 1), "mask100C": ((2, 4, 5, 5), "mask", 4),
         "mask972": ((2, 3, 18, 18), "mask", 1), "down2": ((2, 3, 6, 10), "down", 2), "down4": ((2, 3, 8, 8), "down", 4),
         "down8": ((1, 3, 8, 8), "down", 8), "gray3": ((2, 3, 6, 6), "gray", None), "gray4": ((2, 4, 5, 5), "gray", None)}
ROWS = ((8, 7, False), (8, 3, True), (8, 0, False), (1024, 300, False))      # (T, the index the step lands on, DDIM)


@pytest.fixture(scope="module")
def vd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import v_diffusion
    from v_diffusion import _hip
    _hip.lib()
    return v_diffusion


class Stub:
    """pointwise stand-in network; ``calls`` (optional list) receives the time of every call"""

    training = False

    def __init__(self, a=(0.3, -0.5), b=(0.4, 0.3), g=0.07, both=False, calls=None):
        self.a, self.b, self.g, self.both, self.calls = a, b, g, both, calls

    def __call__(self, x, t, y):
        if self.calls is not None:
            self.calls.append(float(t[0]))
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        return torch.cat([out, 0.5 * out - 0.25 * x], dim=1) if self.both else out


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float()


def guarded(shape, offset=0):
    """a contiguous tensor of ``shape`` starting ``offset`` floats into a 16-byte aligned sentinel-filled buffer with GUARD floats behind
    it, and the check that the bands were left alone"""
    n = int(torch.Size(shape).numel())
    buf = torch.full((offset + n + GUARD,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + n].view(shape), lambda: bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


def placed(t, offset=0):
    v, ok = guarded(t.shape, offset)
    v.copy_(t)
    return v, ok


def cosine(lim=20.0):
    import v_diffusion as vd
    return vd.get_logsnr_schedule("cosine", -lim, lim)


def make_gd(vd, T, mot="v", w=0.0):
    return vd.GaussianDiffusion(cosine(), T, mot, "fixed_large", "snr_trunc", "mse", w_guide=w, p_uncond=0.0)


@functools.lru_cache(maxsize=None)
def step_row(T, i, mot, w, ddim, clip=True):
    """the 8 fp32 weights, as python floats, of the reverse step that lands on grid index i of the T-step cosine +-20 schedule"""
    import v_diffusion as vd
    k8, _ = make_gd(vd, T, mot, w)._step_coefs(i, ddim, clip)
    return tuple(torch.tensor(list(k8), dtype=torch.float64).float().tolist())


@functools.lru_cache(maxsize=None)
def case_inputs(case, mot, cfg, clip, T, i, ddim, seed):
    """CPU fp32 inputs of one step, computed once and shared (the tests only read): x_t at the log-SNR the step leaves, a network output of
    n*(1+cfg) interleaved rows, the posterior noise, a mask (exact 0, exact 1 and values between), a noisy measurement of a clean image, and
    a stand-in for the network's input gradient.  With clip, elements whose prediction lies within 1e-3 of -1 or 1 are moved off."""
    shape, op, par = CASES[case]
    B, C = shape[:2]
    k = step_row(T, i, mot, W_GUIDE if cfg else 0.0, ddim, clip)
    a, s = R.IR.alpha_sigma(cosine()(torch.tensor([(i + 1) / T], dtype=torch.float64)).float())
    clean = rnd(shape, seed + 1, 0.6).clamp(-1, 1)
    xt = (float(a) * clean.double() + float(s) * rnd(shape, seed + 2).double()).float()
    out = rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), seed + 3, 0.8)
    mask = None
    if op == "mask":
        g = torch.Generator().manual_seed(seed + 7)
        pick, frac = torch.rand((B, par) + shape[2:], generator=g), torch.rand((B, par) + shape[2:], generator=g) * 0.98 + 0.01
        mask = torch.where(pick < 1 / 3, torch.zeros_like(frac), torch.where(pick < 2 / 3, torch.ones_like(frac), frac))
    if clip:
        for _ in range(20):
            near = torch.zeros(shape, dtype=torch.bool)
            for rows in ((out[0::2], out[1::2]) if cfg else (out,)):
                p = R.branch(k, xt.double(), rows.double(), mot == "both", False)[0]
                near |= ((p.abs() - 1.0).abs() < 1e-3)
            if not bool(near.any()):
                break
            xt = torch.where(near, xt * 1.01 + 0.003, xt)
            step = near.repeat_interleave(1 + cfg, dim=0)
            out[:, :C] = torch.where(step, out[:, :C] * 0.99 - 0.002, out[:, :C])
        assert not bool(near.any()), "could not move the inputs off the clip's corners"
    meas = (R.apply_A(op, clean.double(), par, None if mask is None else mask.double()) + 0.05 * rnd(R.measurement_shape(op, shape, par),
                                                                                                  seed + 4).double()).float()
    return xt, out, rnd(shape, seed + 5), mask, meas, rnd((B * (1 + cfg),) + shape[1:], seed + 6, 0.3)


def run_residual(H, k, xt, out, meas, mask, op, par, mot, cfg, clip, want_x0=True, offset=0):
    """(dout, dxt, sumsq, x0hat, guard bands intact) of one launch on device copies placed ``offset`` floats off alignment"""
    B, C, Hh, Ww = xt.shape
    (xd, ok1), (od, ok2), (md, ok3) = (placed(t, offset) for t in (xt, out, meas))
    kd = None if mask is None else placed(mask, offset)[0]
    dout, ok4 = guarded(out.shape, offset)
    dxt, ok5 = guarded(xt.shape, offset)
    ss, ok6 = guarded((B,), offset)
    x0, ok7 = guarded(xt.shape, offset) if want_x0 else (None, lambda: True)
    H.dps_residual(xd, od, md, kd, list(k), H.OUT_TYPES[mot], cfg, clip, H.DPS_OPS[op], par or 0, dout, dxt, ss, x0, B, C, Hh, Ww)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), xt) and torch.equal(od.cpu(), out) and torch.equal(md.cpu(), meas)            # inputs left alone
    intact = all(f() for f in (ok1, ok2, ok3, ok4, ok5, ok6, ok7))
    return dout.clone(), dxt.clone(), ss.clone(), None if x0 is None else x0.clone(), intact


def run_step(H, k, xt, out, noise, dxin, dxt, sumsq, zeta, mot, cfg, last, clip, alias=False, offset=0):
    """(xn, xdup, guard bands intact) of one vd_dps_step launch"""
    B, C = xt.shape[:2]
    HW = xt[0, 0].numel()
    (xd, ok_x), (od, _), (dd, _), (dz, _), (sd, _) = (placed(t.cpu(), offset) for t in (xt, out, dxin, dxt, sumsq))
    nd = None if noise is None else placed(noise, offset)[0]
    xn, ok_n = (xd, ok_x) if alias else guarded(xt.shape, offset)
    xdup, ok_d = guarded((2 * B,) + tuple(xt.shape[1:]), offset) if cfg else (None, lambda: True)
    H.dps_step(xd, od, nd, dd, dz, sd, list(k), zeta, H.OUT_TYPES[mot], cfg, last, clip, xn, xdup, B, C, HW)
    torch.cuda.synchronize()
    assert alias or torch.equal(xd.cpu(), xt.cpu()) or bool(torch.isnan(xt).any())
    return xn.clone(), None if xdup is None else xdup.clone(), ok_n() and ok_x() and ok_d()


def run_sample_step(H, k, xt, out, noise, mot, cfg, last, clip):
    B, C = xt.shape[:2]
    xn = torch.empty(xt.shape, device=DEV)
    xdup = torch.empty((2 * B,) + tuple(xt.shape[1:]), device=DEV) if cfg else None
    H.sample_step(xt.to(DEV), out.to(DEV), None if noise is None else noise.to(DEV), list(k), H.OUT_TYPES[mot], cfg, last, clip, xn, xdup,
                  B, C, xt[0, 0].numel())
    torch.cuda.synchronize()
    return xn, xdup


def row_err(got, ref):
    """max over rows of the row's max error relative to the row's own scale"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.detach().cpu().double().reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1).clamp(min=1e-300)
    return float(((got - ref).abs().amax(dim=1) / scale).max())


def held(name, got, cmp, ref, what):
    ek, ec = row_err(got, ref), row_err(cmp, ref)
    print(f"[{what}] {name}: kernel {ek:.3e} composition {ec:.3e}")
    assert ek <= 2.0 * ec + FLOOR, f"{what} {name}: kernel {ek:.3e}, composition {ec:.3e}"


# ------------------------------------------------------------------------------------------------ 1. the input-only backward pass
def _build(vd, cfg, train=True):
    from oracle.cases import make_weights
    m = vd.UNet(**cfg)
    m.load_state_dict(make_weights(cfg), strict=True)
    return m.to(DEV).train(train)                              # (drop_rate = 0 in the tiny configs: train == eval numerics)


@pytest.mark.parametrize("name", ["tinyA", "tinyB", "tinyC"])
def test_input_only_dx_is_the_full_pass_s(vd, golden_dir, monkeypatch, name):
    from oracle import detrand
    from oracle.cases import TINY, make_inputs
    from v_diffusion import _hip as H
    case = TINY[name]
    cfg, B, R_, label = case["cfg"], case["B"], case["R"], case["label"]
    g = np.load(os.path.join(golden_dir, f"unet_{name}.npz"), allow_pickle=False)
    model = _build(vd, cfg)
    x, t, y = (None if v is None else v.to(DEV) for v in make_inputs(cfg, B, R_, label))
    gout = detrand.normal("gout", (B, cfg["out_channels"], R_, R_), 1).to(DEV)
    # the existing full path
    xd = x.clone().requires_grad_(True)
    out_full = model(xd, t, y)
    (out_full * gout).sum().backward()
    dx_full = xd.grad.clone()
    assert all(p.grad is not None for p in model.parameters())
    model.zero_grad(set_to_none=True)
    pool = {k: v.data_ptr() for k, v in model._grad_pool.items()}
    # forward_vjp: no autograd
    out, vjp = model.forward_vjp(x, t, y)
    dx = vjp(gout)
    assert torch.equal(out, out_full.detach()) and not out.requires_grad
    assert dx.dtype == torch.float32 and dx.is_cuda and tuple(dx.shape) == tuple(x.shape)
    assert torch.equal(dx, dx_full), f"input-only dx differs from the full pass by {float((dx - dx_full).abs().max()):.3e}"
    np.testing.assert_allclose(dx.cpu().numpy(), g["dx"], atol=2e-5, rtol=1e-4)
    assert all(p.grad is None for p in model.parameters())
    assert {k: v.data_ptr() for k, v in model._grad_pool.items()} == pool and model._flat_grad_views is None
    with pytest.raises(RuntimeError, match="called twice"):
        vjp(gout)
    with pytest.raises(ValueError, match="shape"):
        model.forward_vjp(x, t, y)[1](gout[:1])
    with torch.inference_mode():
        out_i, vjp_i = model.forward_vjp(x, t, y)
        assert torch.equal(vjp_i(gout), dx_full) and torch.equal(out_i, out)
    with torch.no_grad():
        assert torch.equal(model.forward_vjp(x, t, y)[1](gout), dx_full)
    # a frozen network under autograd: one node, none of the weight-gradient work
    counts = {"conv3x3_wgrad": 0, "gemm_grouped_wgrad": 0, "gn_param_sums_batched": 0}
    for fn in counts:
        def counted(*a, _fn=fn, _real=getattr(H, fn), **kw):
            counts[_fn] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(H, fn, counted)
    model.requires_grad_(False)
    xf = x.clone().requires_grad_(True)
    of = model(xf, t, y)
    assert of.grad_fn is not None and "UNetInputFn" in type(of.grad_fn).__name__
    (dxf,) = torch.autograd.grad(of, xf, gout)
    assert torch.equal(dxf, dx_full) and torch.equal(of.detach(), out)
    assert counts == dict.fromkeys(counts, 0), counts
    assert all(p.grad is None for p in model.parameters())
    # ... and unfrozen it routes as before
    model.requires_grad_(True)
    xu = x.clone().requires_grad_(True)
    (model(xu, t, y) * gout).sum().backward()
    assert all(p.grad is not None for p in model.parameters()) and torch.equal(xu.grad, dx_full)
    assert counts["gn_param_sums_batched"] == 1 and counts["conv3x3_wgrad"] + counts["gemm_grouped_wgrad"] > 0


def test_forward_vjp_without_labels_empty_batches_and_cpu_tensors(vd):
    from oracle.cases import TINY, make_inputs
    case = TINY["tinyA"]
    cfg, R_ = case["cfg"], case["R"]
    model = _build(vd, cfg, train=False)
    x, t, _ = (v.to(DEV) for v in make_inputs(cfg, 2, R_, case["label"]))
    gout = rnd((2, 3, R_, R_), 3).to(DEV)
    xd = x.clone().requires_grad_(True)
    (model(xd, t, None) * gout).sum().backward()                  # class-conditional network called without labels
    model.zero_grad(set_to_none=True)
    out, vjp = model.forward_vjp(x, t)
    assert torch.equal(vjp(gout), xd.grad) and bool(torch.isfinite(out).all())
    o0, v0 = model.forward_vjp(x[:0], t[:0])
    assert tuple(o0.shape) == (0, 3, R_, R_) and tuple(v0(gout[:0]).shape) == (0, 3, R_, R_)
    with pytest.raises(RuntimeError, match="called twice"):
        v0(gout[:0])
    with pytest.raises(RuntimeError, match="MI355X"):
        model.forward_vjp(x.cpu(), t.cpu())


# ------------------------------------------------------------------------------------------------ 2. the kernels against fp64
@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("case", CASES, ids=list(CASES))
def test_kernels_against_fp64(vd, case, mot, cfg, clip):
    """both launches on the first, an interior and the last row of the 8-step table and a row of the 1024-step table (weights near 1), DDPM
    and DDIM coefficients, last_step on and off"""
    from v_diffusion import _hip as H
    shape, op, par = CASES[case]
    both = mot == "both"
    d, g = (lambda t: None if t is None else t.double()), (lambda t: None if t is None else t.to(DEV))
    for T, i, ddim in ROWS:
        k = step_row(T, i, mot, W_GUIDE if cfg else 0.0, ddim, clip)
        xt, out, noise, mask, meas, dxin = case_inputs(case, mot, cfg, clip, T, i, ddim, 17 + i)
        what = f"{case} {mot} {'guided' if cfg else 'plain'} {'clip' if clip else 'noclip'} T={T} i={i}"
        dout, dxt, ss, x0, intact = run_residual(H, k, xt, out, meas, mask, op, par, mot, cfg, clip)
        assert intact, "guard band written"
        ref = R.residual(k, d(xt), d(out), d(meas), op, par, d(mask), both, cfg, clip)
        cmp = R.residual(k, g(xt), g(out), g(meas), op, par, g(mask), both, cfg, clip)
        for name, got in (("dout", dout), ("dxt", dxt), ("sumsq", ss), ("x0hat", x0)):
            held(name, got, cmp[name], ref[name], what)
        zeta = 0.7
        for last in (False, True):
            xn, xdup, intact = run_step(H, k, xt, out, noise, dxin, dxt, ss, zeta, mot, cfg, last, clip)
            assert intact, "guard band written"
            rs = R.step(k, d(xt), d(out), d(noise), d(dxin), dxt.cpu().double(), ss.cpu().double(), zeta, both, cfg, last, clip)
            cs = R.step(k, g(xt), g(out), g(noise), g(dxin), dxt, ss, zeta, both, cfg, last, clip)
            held(f"xn last={int(last)}", xn, cs, rs, what)
            if cfg:
                assert torch.equal(xdup[0::2], xn) and torch.equal(xdup[1::2], xn)


# ------------------------------------------------------------------------------------------------ 3. exact properties
PROP_CASES = ("mask75", "mask972", "mask100one", "down2", "gray4")


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("case", PROP_CASES)
def test_exact_properties(vd, case, mot, cfg):
    from v_diffusion import _hip as H
    shape, op, par = CASES[case]
    B = shape[0]
    T, i = 8, 3
    k = step_row(T, i, mot, W_GUIDE if cfg else 0.0, False)
    xt, out, noise, mask, meas, dxin = case_inputs(case, mot, cfg, True, T, i, False, 5)
    dout, dxt, ss, x0, intact = run_residual(H, k, xt, out, meas, mask, op, par, mot, cfg, True)
    assert intact and bool(torch.isfinite(ss).all()) and bool((ss > 0).all())
    # the same call gives the same bits; x0hat is optional and changes nothing; so does the placement of the buffers
    for kw in (dict(), dict(want_x0=False), dict(offset=1), dict(offset=3)):
        d2, z2, s2, x2, ok = run_residual(H, k, xt, out, meas, mask, op, par, mot, cfg, True, **kw)
        assert ok and torch.equal(d2, dout) and torch.equal(z2, dxt) and torch.equal(s2, ss), kw
        assert (x2 is None) == (kw.get("want_x0") is False) and (x2 is None or torch.equal(x2, x0))
    for last in (False, True):
        for nz in (noise, None) if (last or i == 0) else (noise,):
            kk = list(k)
            if nz is None:
                kk[5] = 0.0
            base, bdup = run_sample_step(H, kk, xt, out, nz, mot, cfg, last, True)
            # zeta = 0: vd_sample_step's bits, whatever the gradient buffers hold
            junk = torch.full_like(dxin, NAN)
            xn, xdup, ok = run_step(H, kk, xt, out, nz, junk, torch.full_like(dxt, NAN), ss, 0.0, mot, cfg, last, True)
            assert ok and torch.equal(xn, base) and (not cfg or torch.equal(xdup, bdup))
            # the step proper: aliasing, alignment (wide and scalar forms), the duplicate
            xn, xdup, ok = run_step(H, kk, xt, out, nz, dxin, dxt, ss, 0.7, mot, cfg, last, True)
            assert ok and not torch.equal(xn, base) and bool(torch.isfinite(xn).all())
            for kw in (dict(alias=True), dict(offset=1), dict(offset=2, alias=True)):
                x2, d2, ok = run_step(H, kk, xt, out, nz, dxin, dxt, ss, 0.7, mot, cfg, last, True, **kw)
                assert ok and torch.equal(x2, xn) and (not cfg or torch.equal(d2, xdup)), kw
            if B < 2:
                continue
            # a row with sumsq = 0 is vd_sample_step's row and reads nothing of its gradient; the other rows do not notice
            s0 = ss.clone()
            s0[0] = 0.0
            clean, _, _ = run_step(H, kk, xt, out, nz, dxin, dxt, s0, 0.7, mot, cfg, last, True)
            din, dz = dxin.clone(), dxt.clone()
            din[: 1 + cfg], dz[0] = NAN, NAN
            x3, _, ok = run_step(H, kk, xt, out, nz, din, dz, s0, 0.7, mot, cfg, last, True)
            assert ok and torch.equal(x3[0], base[0]) and torch.equal(x3, clean) and torch.equal(x3[1:], xn[1:])
            # a sumsq that is not finite: that row NaN, the others unchanged
            for badv in (INF, NAN, -1.0):
                s1 = ss.clone()
                s1[B - 1] = badv
                x4, _, ok = run_step(H, kk, xt, out, nz, dxin, dxt, s1, 0.7, mot, cfg, last, True)
                assert ok and bool(torch.isnan(x4[B - 1]).all()) and torch.equal(x4[: B - 1], xn[: B - 1]), badv


def test_an_unmeasured_sample_has_no_residual(vd):
    """an all-zero mask row with the measurement A x = 0: sumsq is exactly 0, the cotangents are zeros, and the step leaves that row to
    vd_sample_step with NaN planted in its gradient"""
    from v_diffusion import _hip as H
    case, mot, cfg = "mask972", "v", True
    shape, op, par = CASES[case]
    k = step_row(8, 3, mot, W_GUIDE, False)
    xt, out, noise, mask, meas, dxin = case_inputs(case, mot, cfg, True, 8, 3, False, 5)
    mask, meas = mask.clone(), meas.clone()
    mask[0], meas[0] = 0.0, 0.0
    dout, dxt, ss, _, ok = run_residual(H, k, xt, out, meas, mask, op, par, mot, cfg, True)
    assert ok and float(ss[0]) == 0.0 and float(ss[1]) > 0 and not bool(dout[:2].any()) and not bool(dxt[0].any())
    base, _ = run_sample_step(H, k, xt, out, noise, mot, cfg, False, True)
    ref, _, _ = run_step(H, k, xt, out, noise, dxin, dxt, ss, 0.7, mot, cfg, False, True)
    din, dz = dxin.clone(), dxt.clone()
    din[:2], dz[0] = NAN, NAN
    xn, _, ok = run_step(H, k, xt, out, noise, din, dz, ss, 0.7, mot, cfg, False, True)
    assert ok and torch.equal(xn[0], base[0]) and torch.equal(xn[1], ref[1]) and not torch.equal(xn[1], base[1])


def test_wrappers_refuse_bad_arguments(vd):
    from v_diffusion import _hip as H
    z = lambda *s: torch.zeros(s, device=DEV)
    k = [0.8, -0.6, 0.0, 0.3, 0.7, 0.1, 0.0, 0.0]
    res = lambda **kw: H.dps_residual(*{**dict(xt=z(1, 3, 4, 4), out=z(1, 3, 4, 4), meas=z(1, 3, 4, 4), mask=z(1, 1, 4, 4), k=k, mot=0, cfg=0,
                                               clip=1, op=0, par=1, dout=z(1, 3, 4, 4), dxt=z(1, 3, 4, 4), ss=z(1), x0=None, n=1, C=3, H=4,
                                               W=4), **kw}.values())
    res()
    for kw, msg in ((dict(op=3), "bad op"), (dict(mot=5), "model_out_type"), (dict(mask=None), "null"), (dict(ss=None), "null"),
                    (dict(par=2), "channels"), (dict(op=1, par=3), "down-sampling"), (dict(op=1, par=8), "down-sampling"),
                    (dict(n=0), "empty"), (dict(W=0), "empty")):
        with pytest.raises(H.HipError, match=msg):
            res(**kw)
    with pytest.raises(H.HipError, match="CPU tensor"):
        res(xt=torch.zeros(1, 3, 4, 4))
    stp = lambda **kw: H.dps_step(*{**dict(xt=z(1, 3, 4, 4), out=z(1, 3, 4, 4), noise=z(1, 3, 4, 4), dxin=z(1, 3, 4, 4), dxt=z(1, 3, 4, 4),
                                           ss=z(1), k=k, zeta=0.5, mot=0, cfg=0, last=0, clip=1, xn=z(1, 3, 4, 4), xdup=None, n=1, C=3,
                                           HW=16), **kw}.values())
    stp()
    for kw, msg in ((dict(mot=-1), "model_out_type"), (dict(dxin=None), "null"), (dict(ss=None), "null"), (dict(noise=None), "noise"),
                    (dict(n=0), "empty"), (dict(HW=0), "empty")):
        with pytest.raises(H.HipError, match=msg):
            stp(**kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. chains
def replay(seed, shape, count):
    """the sampler's draws: ``count`` tensors of the image shape from one generator on the GPU, in order"""
    g = torch.Generator(DEV).manual_seed(seed)
    return [torch.randn(shape, device=DEV, generator=g) for _ in range(count)]


def operator_of(op, par, mask):
    return {"mask": ("mask", mask), "down": ("down", par), "gray": ("gray",)}[op]


@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("op,par", (("mask", 1), ("down", 2), ("gray", None)))
def test_stand_in_chain_against_fp64(vd, op, par, guided):
    """T = 6 through the autograd route (the stand-in is no UNet), seeded: the sampler against the fp64 chain over the replayed draws, by
    the error of the same chain as fp32 torch ops"""
    T, shape, seed, zeta = 6, (2, 3, 8, 8), 29, 0.4
    gd = make_gd(vd, T, "v", 1.0 if guided else 0.0)
    y = torch.arange(1, shape[0] + 1, dtype=torch.float32) if guided else None
    mask = None
    if op == "mask":
        mask = torch.zeros((1, 1) + shape[2:])
        mask[..., : shape[3] // 2] = 1.0
        mask[..., shape[3] // 2] = 0.5
    clean = rnd(shape, 31, 0.6).clamp(-1, 1)
    meas = (vd.dps_measure(clean, operator_of(op, par, mask)) + 0.05 * rnd(R.measurement_shape(op, shape, par), 33)).to(DEV)
    calls = []
    got = gd.p_sample_dps(Stub(calls=calls), meas, operator_of(op, par, mask), shape, label=y, seed=seed, zeta=zeta)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape and not got.requires_grad
    assert calls == [(i + 1) / T for i in reversed(range(T))]                      # one network call per step
    draws = replay(seed, shape, T + 1)
    row = lambda i: gd._step_coefs(i, False, True)
    c = lambda t: None if t is None else t.detach().cpu().double()
    g = lambda t: None if t is None else t.to(DEV)
    ref = R.chain(Stub(), c(draws[0]), c(meas), op, row, [c(n) for n in draws[1:]], [zeta] * T, par, c(mask), c(y), cfg=guided)
    cmp = R.chain(Stub(), draws[0], meas, op, row, draws[1:], [zeta] * T, par, g(mask), g(y), cfg=guided)
    scale = float(ref.abs().max())
    es, ec = float((got.cpu().double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    print(f"[dps chain {op} {'guided' if guided else 'plain'} T={T}] sampler {es:.3e}  composition {ec:.3e}  (scale {scale:.3e})")
    assert es <= 2.0 * ec + FLOOR * scale, (es, ec)
    assert torch.equal(got, gd.p_sample_dps(Stub(), meas, operator_of(op, par, mask), shape, label=y, seed=seed, zeta=[zeta] * T))
    plain = gd.p_sample_dps(Stub(), meas, operator_of(op, par, mask), shape, label=y, seed=seed, zeta=0.0)
    A = lambda x: R.apply_A(op, x.double(), par, None if mask is None else g(mask).double())
    assert float((meas.double() - A(got)).norm()) < float((meas.double() - A(plain)).norm())     # it does move towards the measurement


def _tiny(vd, name):
    from oracle.cases import TINY
    return _build(vd, TINY[name]["cfg"], train=False), TINY[name]


@pytest.mark.parametrize("name", ("tinyC", "tinyA"))
def test_forward_vjp_chain_is_the_autograd_chain(vd, name):
    """T = 3 on a real network: the chain through ``forward_vjp`` against the same chain with the UNet hidden behind a plain callable of a
    frozen copy (``torch.autograd.grad`` through the frozen-network node), bit for bit.  tinyC: B = 2, 8x8, down-sampling by 2,
    unconditional; tinyA: guided, a mask."""
    model, case = _tiny(vd, name)
    T, R_ = 3, case["R"]
    shape = (2, 3, R_, R_)
    if name == "tinyC":
        gd, y, op = make_gd(vd, T, "v", 0.0), None, ("down", 2)
    else:
        mask = torch.zeros((1, 1, R_, R_), device=DEV)
        mask[..., R_ // 2:, :] = 1.0
        gd, y, op = make_gd(vd, T, "v", 1.0), torch.tensor([1.0, 4.0]), ("mask", mask)
    meas = vd.dps_measure(rnd(shape, 53, 0.6).clamp(-1, 1).to(DEV), op)
    frozen = model.detached_copy().requires_grad_(False).eval()
    hidden = lambda x, t, yy: frozen(x, t, yy)
    a = gd.p_sample_dps(model, meas, op, shape, label=y, seed=5, zeta=0.5)
    b = gd.p_sample_dps(hidden, meas, op, shape, label=y, seed=5, zeta=0.5, device=DEV)
    assert a.is_cuda and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert all(p.grad is None for p in model.parameters()) and all(p.grad is None for p in frozen.parameters())
    assert not torch.equal(a, gd.p_sample_dps(model, meas, op, shape, label=y, seed=5, zeta=0.0))
    wrapped = type("Wrap", (), {"module": model, "__call__": lambda self, *args: model(*args)})()
    assert torch.equal(gd.p_sample_dps(wrapped, meas, op, shape, label=y, seed=5, zeta=0.5), a)      # unwrapped through .module


@pytest.mark.parametrize("ddim", (False, True), ids=("ddpm", "ddim"))
def test_zeta_zero_is_p_sample(vd, ddim):
    model, case = _tiny(vd, "tinyA")
    T, R_ = 4, case["R"]
    shape, y = (2, 3, R_, R_), torch.tensor([1.0, 4.0])
    gd = make_gd(vd, T, "v", 1.0)
    meas = torch.zeros((2, 1, R_, R_), device=DEV)
    got = gd.p_sample_dps(model, meas, ("gray",), shape, label=y, seed=7, zeta=0.0, use_ddim=ddim)
    want = gd.p_sample(model, shape, label=y, seed=7, use_ddim=ddim)
    assert got.is_cuda and torch.equal(got.cpu(), want)
    dd = vd.DistillationDiffusion(model, T, logsnr_fn=gd.logsnr_fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="snr_trunc")
    s = dd.p_sample_dps(model, meas, ("gray",), shape, label=y, seed=7, zeta=0.3)
    assert tuple(s.shape) == shape and bool(torch.isfinite(s).all())


def test_draw_order(vd, monkeypatch):
    """one generator, seeded on the device; the initial state, then one image-shaped draw per step and nothing else"""
    import v_diffusion.restore as restore          # (the chain is opened, and every draw made, there)
    T, shape, seed = 5, (2, 3, 8, 8), 13
    gd = make_gd(vd, T)
    seen = []
    real = torch.randn

    class Recording:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def randn(*a, **kw):
            t = real(*a, **kw)
            seen.append((kw.get("generator"), t.clone()))
            return t
    monkeypatch.setattr(restore, "torch", Recording())
    meas = torch.zeros((2, 1, 8, 8), device=DEV)
    gd.p_sample_dps(Stub(), meas, ("gray",), shape, seed=seed, zeta=0.3)
    monkeypatch.undo()
    want = replay(seed, shape, T + 1)
    assert len(seen) == T + 1 and len({id(g) for g, _ in seen}) == 1 and seen[0][0] is not None and seen[0][0].device.type == "cuda"
    assert all(tuple(t.shape) == shape and torch.equal(t, w) for (_, t), w in zip(seen, want))


def test_gpu_refusals(vd):
    model, case = _tiny(vd, "tinyA")
    R_ = case["R"]
    shape = (2, 3, R_, R_)
    gd = make_gd(vd, 2)
    meas = torch.zeros((2, 1, R_, R_), device=DEV)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_dps(model, meas, ("gray",), shape, device="cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_dps(model, meas.cpu(), ("gray",), shape)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_dps(vd.UNet(**case["cfg"]).eval(), meas, ("gray",), shape)               # parameters on the CPU
    with pytest.raises(ValueError, match="measurement"):
        gd.p_sample_dps(model, meas, ("down", 2), shape)
    with pytest.raises(ValueError, match="finite"):
        gd.p_sample_dps(model, meas, ("gray",), shape, zeta=-1.0)
    with pytest.raises(RuntimeError, match="input gradient"):
        gd.p_sample_dps(lambda x, t, y: torch.zeros_like(x), meas, ("gray",), shape, device=DEV)
    x = gd.p_sample_dps(model, meas, ("gray",), shape, seed=1, zeta=0.5)                       # and after the refusals it runs
    assert bool(torch.isfinite(x).all())
