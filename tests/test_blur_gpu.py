"""The blur operator of Diffusion Posterior Sampling on the GPU: the residual launch vdx_dps_residual_blur and the operator launch
vdx_blur_planes (include/vdiff_blur.h, csrc/diffusion.hip) against the float64 restatement of tests/blur_ref.py, their exact properties,
and the chains of ``GaussianDiffusion.p_sample_dps(..., operator=("blur", kernel))``.

The helpers are those of tests/test_dps_gpu.py (guard bands, ``held``, ``step_row``, ``Stub``) and so is the yardstick: the same arithmetic
as plain fp32 torch ops on the GPU from the same coefficients (blur_ref's functions on fp32 GPU tensors: a sum of shifted slices, no
library convolution) -- the kernel may be at most 2x as far from fp64, plus 4 ulp of the row's scale; no element is left out.  Inputs of
the clipped cases are kept 1e-3 away from the clip's two corners.  Shapes are the smallest that can go wrong: an odd plane smaller than a
wavefront under asymmetric taps (a flipped kernel shows), radii of H - 1 and W - 1 (every fold, three preimages per axis), a plane of 272
elements with C = 1 and B = 3, the 32 x 32 Gaussian of the experiments, and both maxima at once.  Needs an MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blur_ref as BR                                             # noqa: E402
import dps_ref as R                                               # noqa: E402
import test_dps_gpu as D                                          # noqa: E402  (the helpers: imported, not copied)
from test_dps_gpu import vd                                       # noqa: E402,F401  (the module fixture)

pytestmark = pytest.mark.gpu
DEV = D.DEV
W_GUIDE = D.W_GUIDE
# name -> (image shape, taps): fp32 taps, made once
CASES = {"odd": ((2, 3, 5, 7), (3, 5)), "fold": ((1, 2, 3, 4), (5, 7)), "trip2": ((3, 1, 17, 16), (3, 3)), "gauss": ((2, 3, 32, 32), None),
         "max": ((1, 3, 64, 64), (33, 33))}
SMALL = ("odd", "fold", "trip2", "gauss")
ROWS = ((8, 3, True), (1024, 300, False))                          # (T, the index the step lands on, DDIM)


@functools.lru_cache(maxsize=None)
def taps_of(case):
    """random taps of both signs with an absolute sum near 1 (asymmetric in both directions), or the Gaussian of the DPS experiments"""
    import v_diffusion
    ks = CASES[case][1]
    if ks is None:
        return v_diffusion.gaussian_kernel(9, 1.5)
    t = D.rnd(ks, 101 + ks[0] * ks[1])
    return (t.double() / t.double().abs().sum()).float()


@functools.lru_cache(maxsize=None)
def inputs(case, mot, cfg, clip, T, i, ddim, seed):
    """CPU fp32 inputs of one step, computed once and shared (the tests only read), made as tests/test_dps_gpu.py's case_inputs makes
    them: x_t at the log-SNR the step leaves, a network output of n*(1+cfg) interleaved rows, a noisy measurement of a clean image.
    With clip, elements whose prediction lies within 1e-3 of -1 or 1 are moved off."""
    shape = CASES[case][0]
    B, C = shape[:2]
    k = D.step_row(T, i, mot, W_GUIDE if cfg else 0.0, ddim, clip)
    a, s = R.IR.alpha_sigma(D.cosine()(torch.tensor([(i + 1) / T], dtype=torch.float64)).float())
    clean = D.rnd(shape, seed + 1, 0.6).clamp(-1, 1)
    xt = (float(a) * clean.double() + float(s) * D.rnd(shape, seed + 2).double()).float()
    out = D.rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), seed + 3, 0.8)
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
    meas = (BR.apply_A(clean.double(), taps_of(case)) + 0.05 * D.rnd(shape, seed + 4).double()).float()
    return xt, out, meas


@functools.lru_cache(maxsize=None)
def reference(case, mot, cfg, clip, T, i, ddim, seed):
    """the fp64 outputs of the launch on ``inputs``: computed once, shared, left unchanged"""
    xt, out, meas = inputs(case, mot, cfg, clip, T, i, ddim, seed)
    k = D.step_row(T, i, mot, W_GUIDE if cfg else 0.0, ddim, clip)
    return BR.residual(k, xt.double(), out.double(), meas.double(), taps_of(case), mot == "both", cfg, clip)


def run_blur(H, k, xt, out, meas, taps, mot, cfg, clip, want_x0=True, offset=0):
    """(dout, dxt, sumsq, x0hat, guard bands intact) of one launch on device copies placed ``offset`` floats off alignment"""
    B, C, Hh, Ww = xt.shape
    (xd, ok1), (od, ok2), (md, ok3), (td, ok0) = (D.placed(t, offset) for t in (xt, out, meas, taps))
    dout, ok4 = D.guarded(out.shape, offset)
    dxt, ok5 = D.guarded(xt.shape, offset)
    ss, ok6 = D.guarded((B,), offset)
    x0, ok7 = D.guarded(xt.shape, offset) if want_x0 else (None, lambda: True)
    H.dps_residual_blur(xd, od, md, td, list(k), H.OUT_TYPES[mot], cfg, clip, dout, dxt, ss, x0, B, C, Hh, Ww)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), xt) and torch.equal(od.cpu(), out) and torch.equal(md.cpu(), meas) and torch.equal(td.cpu(), taps)
    intact = all(f() for f in (ok0, ok1, ok2, ok3, ok4, ok5, ok6, ok7))
    return dout.clone(), dxt.clone(), ss.clone(), None if x0 is None else x0.clone(), intact


def against_fp64(H, case, mot, cfg, clip):
    g = lambda t: t.to(DEV)
    taps = taps_of(case)
    for T, i, ddim in ROWS:
        k = D.step_row(T, i, mot, W_GUIDE if cfg else 0.0, ddim, clip)
        xt, out, meas = inputs(case, mot, cfg, clip, T, i, ddim, 17 + i)
        what = f"blur {case} {mot} {'guided' if cfg else 'plain'} {'clip' if clip else 'noclip'} T={T} i={i}"
        dout, dxt, ss, x0, intact = run_blur(H, k, xt, out, meas, taps, mot, cfg, clip)
        assert intact, "guard band written"
        ref = reference(case, mot, cfg, clip, T, i, ddim, 17 + i)
        cmp = BR.residual(k, g(xt), g(out), g(meas), taps, mot == "both", cfg, clip)
        for name, got in (("dout", dout), ("dxt", dxt), ("sumsq", ss), ("x0hat", x0)):
            D.held(name, got, cmp[name], ref[name], what)


# ------------------------------------------------------------------------------------------------ 1. the launches against fp64
@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("case", SMALL)
def test_residual_launch_against_fp64(vd, case, mot, cfg, clip):
    from v_diffusion import _hip as H
    against_fp64(H, case, mot, cfg, clip)


def test_residual_launch_against_fp64_at_both_maxima(vd):
    """64 x 64 planes (the bound) under 33 x 33 taps (the bound): one combination, the widest -- "both", guided, clipped"""
    from v_diffusion import _hip as H
    against_fp64(H, "max", "both", True, True)


@pytest.mark.parametrize("case", list(CASES))
def test_operator_and_adjoint_against_fp64(vd, case):
    """vdx_blur_planes in both directions, through ``v_diffusion.blur``; then <A x, r> = <x, A^T r> through the DEVICE results, the dots
    taken in fp64 on the host.  Each device output is one fp32 rounding of an fp64 sum, so the two dots differ by at most
    2^-24 (sum |A x| |r| + sum |x| |A^T r|); the fp64 chains' own rounding (K^2 2^-53 of the same sums) is the 1e-12 beside it."""
    shape, taps = CASES[case][0], taps_of(case)
    x, r = D.rnd(shape, 41), D.rnd(shape, 43)
    got = {}
    for adjoint, src, f in ((False, x, BR.apply_A), (True, r, BR.apply_At)):
        xd, ok_in = D.placed(src)
        y = vd.blur(xd, taps, adjoint=adjoint)
        torch.cuda.synchronize()
        assert ok_in() and torch.equal(xd.cpu(), src) and y.dtype == torch.float32 and tuple(y.shape) == shape and y.data_ptr() != xd.data_ptr()
        D.held("A^T x" if adjoint else "A x", y, f(src.to(DEV), taps), f(src.double(), taps), f"blur planes {case}")
        assert torch.equal(y, vd.blur(xd, taps.to(DEV).double(), adjoint=adjoint))        # the same bits; the kernel's device and dtype are free
        got[adjoint] = y.cpu().double()
    Ax, Atr, x, r = got[False], got[True], x.double(), r.double()
    lhs, rhs = float((Ax * r).sum()), float((x * Atr).sum())
    bound = (2.0 ** -24 + 1e-12) * float((Ax.abs() * r.abs()).sum() + (x.abs() * Atr.abs()).sum())
    print(f"[blur adjoint identity {case}] <Ax, r> {lhs:.9e}  <x, A^T r> {rhs:.9e}  difference {abs(lhs - rhs):.3e}  bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


# ------------------------------------------------------------------------------------------------ 2. exact properties
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("case", SMALL)
def test_exact_properties(vd, case, mot, cfg):
    from v_diffusion import _hip as H
    B = CASES[case][0][0]
    T, i = 8, 3
    taps = taps_of(case)
    k = D.step_row(T, i, mot, W_GUIDE if cfg else 0.0, False)
    xt, out, meas = inputs(case, mot, cfg, True, T, i, False, 5)
    dout, dxt, ss, x0, intact = run_blur(H, k, xt, out, meas, taps, mot, cfg, True)
    assert intact and bool(torch.isfinite(ss).all()) and bool((ss > 0).all()) and bool(torch.isfinite(dout).all())
    assert not bool((dout == D.SENTINEL).any()) and not bool((dxt == D.SENTINEL).any()) and not bool((x0 == D.SENTINEL).any())
    # the same call gives the same bits; x0hat is optional and changes nothing; so does the placement of the buffers
    for kw in (dict(), dict(want_x0=False), dict(offset=1), dict(offset=3)):
        d2, z2, s2, x2, ok = run_blur(H, k, xt, out, meas, taps, mot, cfg, True, **kw)
        assert ok and torch.equal(d2, dout) and torch.equal(z2, dxt) and torch.equal(s2, ss), kw
        assert (x2 is None) == (kw.get("want_x0") is False) and (x2 is None or torch.equal(x2, x0))
    # a sample's results do not depend on the other samples
    rows = 1 + cfg
    for b in range(B if B > 1 else 0):
        d1, z1, s1, x1, ok = run_blur(H, k, xt[b:b + 1], out[b * rows:(b + 1) * rows], meas[b:b + 1], taps, mot, cfg, True)
        assert ok and torch.equal(d1, dout[b * rows:(b + 1) * rows]) and torch.equal(z1[0], dxt[b]) and torch.equal(s1[0], ss[b])
        assert torch.equal(x1[0], x0[b])


IDENTITIES = {"one": ([[1.0]], 1.0), "half": ([[0.5]], 0.5), "centre": ([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], 1.0)}


@pytest.mark.parametrize("mot,cfg", (("v", False), ("both", True)), ids=("v-plain", "both-guided"))
@pytest.mark.parametrize("case", ("odd", "trip2"))
@pytest.mark.parametrize("ident", list(IDENTITIES))
def test_a_one_tap_kernel_is_the_uniform_mask(vd, ident, case, mot, cfg):
    """taps [[1]], [[0.5]] and a 3 x 3 with a lone 1 at its centre: dout, dxt and x0hat are vd_dps_residual's with a uniform one-channel
    mask of that value, bit for bit; sumsq within one fp32 ulp (the per-thread order of the fp64 sum differs)"""
    from v_diffusion import _hip as H
    shape = CASES[case][0]
    taps, value = torch.tensor(IDENTITIES[ident][0]), IDENTITIES[ident][1]
    k = D.step_row(8, 3, mot, W_GUIDE if cfg else 0.0, False)
    xt, out, meas = inputs(case, mot, cfg, True, 8, 3, False, 5)
    mask = torch.full((shape[0], 1) + shape[2:], value)
    want = D.run_residual(H, k, xt, out, meas, mask, "mask", 1, mot, cfg, True)
    got = run_blur(H, k, xt, out, meas, taps, mot, cfg, True)
    assert want[4] and got[4]
    for name, a, b in zip(("dout", "dxt", "sumsq", "x0hat"), got, want):
        if name == "sumsq":
            ulp = np.spacing(np.maximum(a.cpu().numpy(), b.cpu().numpy()))
            assert bool((np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64)) <= ulp).all()), (a, b)
        else:
            assert torch.equal(a, b), name


def test_a_refused_call_writes_nothing(vd):
    from v_diffusion import _hip as H
    k = [0.8, -0.6, 0.0, 0.3, 0.7, 0.1, 0.0, 0.0]
    z = lambda *s: torch.zeros(s, device=DEV)
    s = lambda *sh: torch.full(sh, D.SENTINEL, device=DEV)
    for taps, hw, msg in ((z(2, 3), (4, 4), "odd"), (z(3, 35), (40, 40), "odd"), (z(9, 3), (4, 4), "do not fit"), (z(1, 1), (64, 65), "over the bound")):
        shape = (1, 3) + hw
        dout, dxt, ss, x0 = s(*shape), s(*shape), s(1), s(*shape)
        with pytest.raises(H.HipError, match=msg):
            H.dps_residual_blur(z(*shape), z(*shape), z(*shape), taps, k, 0, 0, 1, dout, dxt, ss, x0, 1, 3, *hw)
        y = s(*shape)
        with pytest.raises(H.HipError, match=msg):
            H.blur_planes(z(*shape), taps, False, y, 3, *hw)
        torch.cuda.synchronize()
        assert all(bool((t == D.SENTINEL).all()) for t in (dout, dxt, ss, x0, y)), msg
    shape = (1, 3, 4, 4)
    dout = s(*shape)
    for kw, msg in ((dict(mot=5), "model_out_type"), (dict(meas=None), "null"), (dict(n=0), "empty")):
        a = {**dict(xt=z(*shape), out=z(*shape), meas=z(*shape), taps=z(3, 3), k=k, mot=0, cfg=0, clip=1, dout=dout, dxt=s(*shape), ss=s(1),
                    x0=None, n=1, C=3, H=4, W=4), **kw}
        with pytest.raises(H.HipError, match=msg):
            H.dps_residual_blur(*a.values())
    with pytest.raises(H.HipError, match="CPU tensor"):
        H.dps_residual_blur(torch.zeros(shape), z(*shape), z(*shape), z(3, 3), k, 0, 0, 1, dout, s(*shape), s(1), None, 1, 3, 4, 4)
    with pytest.raises(H.HipError, match="over the bound"):
        vd.blur(z(1, 1, 64, 65), torch.ones(1, 1))
    torch.cuda.synchronize()
    assert bool((dout == D.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 3. chains
@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
def test_stand_in_chain_against_fp64(vd, guided):
    """T = 6 through the autograd route (the stand-in is no UNet), seeded: the sampler against the fp64 chain over the replayed draws, by
    the error of the same chain as fp32 torch ops"""
    T, shape, seed, zeta = 6, (2, 3, 8, 8), 29, 0.4
    gd = D.make_gd(vd, T, "v", 1.0 if guided else 0.0)
    y = torch.arange(1, shape[0] + 1, dtype=torch.float32) if guided else None
    taps = taps_of("odd")
    clean = D.rnd(shape, 31, 0.6).clamp(-1, 1)
    meas = (vd.dps_measure(clean, ("blur", taps)) + 0.05 * D.rnd(shape, 33)).to(DEV)
    calls = []
    got = gd.p_sample_dps(D.Stub(calls=calls), meas, ("blur", taps), shape, label=y, seed=seed, zeta=zeta)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape and not got.requires_grad
    assert calls == [(i + 1) / T for i in reversed(range(T))]                      # one network call per step
    draws = D.replay(seed, shape, T + 1)
    row = lambda i: gd._step_coefs(i, False, True)
    c = lambda t: None if t is None else t.detach().cpu().double()
    g = lambda t: None if t is None else t.to(DEV)
    ref = BR.chain(D.Stub(), c(draws[0]), c(meas), taps, row, [c(n) for n in draws[1:]], [zeta] * T, c(y), cfg=guided)
    cmp = BR.chain(D.Stub(), draws[0], meas, taps, row, draws[1:], [zeta] * T, g(y), cfg=guided)
    scale = float(ref.abs().max())
    es, ec = float((got.cpu().double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    print(f"[dps blur chain {'guided' if guided else 'plain'} T={T}] sampler {es:.3e}  composition {ec:.3e}  (scale {scale:.3e})")
    assert es <= 2.0 * ec + D.FLOOR * scale, (es, ec)
    assert torch.equal(got, gd.p_sample_dps(D.Stub(), meas, ("blur", taps.to(DEV).double()), shape, label=y, seed=seed, zeta=[zeta] * T))
    assert not torch.equal(got, gd.p_sample_dps(D.Stub(), meas, ("blur", taps), shape, label=y, seed=seed, zeta=0.0))


@pytest.mark.parametrize("ddim", (False, True), ids=("ddpm", "ddim"))
def test_zeta_zero_is_p_sample(vd, ddim):
    model, case = D._tiny(vd, "tinyA")
    T, R_ = 4, case["R"]
    shape, y = (2, 3, R_, R_), torch.tensor([1.0, 4.0])
    gd = D.make_gd(vd, T, "v", 1.0)
    meas, op = torch.zeros(shape, device=DEV), ("blur", taps_of("odd"))
    got = gd.p_sample_dps(model, meas, op, shape, label=y, seed=7, zeta=0.0, use_ddim=ddim)
    want = gd.p_sample(model, shape, label=y, seed=7, use_ddim=ddim)
    assert got.is_cuda and torch.equal(got.cpu(), want)
    dd = vd.DistillationDiffusion(model, T, logsnr_fn=gd.logsnr_fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="snr_trunc")
    s = dd.p_sample_dps(model, meas, op, shape, label=y, seed=7, zeta=0.3)
    assert tuple(s.shape) == shape and bool(torch.isfinite(s).all())


@pytest.mark.parametrize("name", ("tinyC", "tinyA"))
def test_forward_vjp_chain_is_the_autograd_chain(vd, name):
    """T = 3 on a real network: the blur chain through ``forward_vjp`` against the same chain with the UNet hidden behind a plain callable
    of a frozen copy (``torch.autograd.grad`` through the frozen-network node), bit for bit.  tinyC unconditional, tinyA guided."""
    model, case = D._tiny(vd, name)
    T, R_ = 3, case["R"]
    shape = (2, 3, R_, R_)
    gd, y = (D.make_gd(vd, T, "v", 0.0), None) if name == "tinyC" else (D.make_gd(vd, T, "v", 1.0), torch.tensor([1.0, 4.0]))
    op = ("blur", taps_of("odd"))
    meas = vd.dps_measure(D.rnd(shape, 53, 0.6).clamp(-1, 1).to(DEV), op)
    frozen = model.detached_copy().requires_grad_(False).eval()
    hidden = lambda x, t, yy: frozen(x, t, yy)
    a = gd.p_sample_dps(model, meas, op, shape, label=y, seed=5, zeta=0.5)
    b = gd.p_sample_dps(hidden, meas, op, shape, label=y, seed=5, zeta=0.5, device=DEV)
    assert a.is_cuda and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert all(p.grad is None for p in model.parameters()) and all(p.grad is None for p in frozen.parameters())
    assert not torch.equal(a, gd.p_sample_dps(model, meas, op, shape, label=y, seed=5, zeta=0.0))
