"""Dynamic thresholding in the DPM-Solver++ sampler on the GPU: the exact per-row order statistic (vd_abs_kth_rows) bit for bit against
numpy.partition, the fused step (vd_solver_step_dyn) against the float64 restatement of tests/threshold_ref.py, and the chains of
``p_sample_solver(clip_denoised="dynamic")``.  The harness is that of tests/test_solver_gpu.py: pointwise stand-in networks, the same
function in fp64 on the CPU and in fp32 on the GPU, and as the yardstick of the kernel's error the same arithmetic, in the order the
header states, as plain fp32 torch ops on the GPU (``torch.kthvalue`` for the order statistic): the kernel may be at most 2x as far
from fp64 as that composition, plus 4 ulp of the row's scale.  The order statistic is 1-Lipschitz in the sup norm and
clamp(g, -s, s)/s is Lipschitz in (g, s) for s >= 1, so thresholding needs no looser rule.  Needs an MI355X."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as R                                            # noqa: E402
import threshold_ref as T                                         # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {"75": (3, 3, 5, 5), "972": (3, 3, 18, 18)}    # C*HW = 75: odd, scalar accesses; 972: 4 | 972, dwordx4, 243 of the workgroup's 1024 threads
MOTS = ("v", "eps", "x0", "both")
W_GUIDE = 1.5
Q = 0.995
FLOOR = 4 * 2.0 ** -24
GUARD, SENTINEL = 64, -12345.0
INF = math.inf
# row lengths of the selection test.  The kernel has one path; what changes with N is the access width (4 | N and an aligned base:
# dwordx4) and the trips of the workgroup's 1024 threads per pass: 1025 is the first scalar row with a second trip, 4096 the last
# dwordx4 row with one, 4100 the first with two; 12288 = 3 x 64 x 64 takes three.
ROW_SIZES = (1, 2, 75, 192, 255, 256, 257, 972, 1025, 4096, 4100, 12288)
NAN_COUNT = 3


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

    def __init__(self, a=(0.3, -0.5), b=(0.4, 0.3), g=0.07):
        self.a, self.b, self.g = a, b, g

    def __call__(self, x, t, y):
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        return out


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. the selection
@functools.lru_cache(maxsize=None)
def selection_rows(N):
    """(5, N) fp32, one family per row, and the number of NaNs in the last one; computed once per N and only read"""
    rng = np.random.default_rng(1000 + N)
    x = np.empty((5, N), dtype=np.float32)
    x[0] = rng.standard_normal(N).astype(np.float32) * 2.0
    x[1] = np.round(rng.standard_normal(N) * 8.0) / 8.0                                  # multiples of 1/8: massive ties
    x[2] = -0.75                                                                          # all equal
    special = np.array([0.0, -0.0, 1e-45, -1e-40, 1.1754942e-38, 3e38, -3e38, np.inf, 1.0, -2.5, 5e-39, -np.inf], dtype=np.float32)
    x[3] = special[rng.permutation(N) % len(special)]
    x[4] = rng.standard_normal(N).astype(np.float32)
    nans = min(NAN_COUNT, N - 1)
    x[4, rng.permutation(N)[:nans]] = np.nan
    x.setflags(write=False)
    return x, nans


@pytest.mark.parametrize("N", ROW_SIZES)
def test_selection_is_numpys_partition_bit_for_bit(vd, N):
    from v_diffusion import _hip as H
    x, nans = selection_rows(N)
    ax = np.abs(x)
    assert np.array_equal(bits(ax), bits(x) & 0x7FFFFFFF)                                 # numpy's abs clears the sign bit and nothing else
    for offset in (0, 1):                                                                 # 1: bases one float off 16-byte alignment
        xd, ok_x = placed(torch.from_numpy(x.copy()), offset)
        for r in sorted({0, N // 2, T.rank(N, Q), N - 1}):
            kth, ok_k = guarded((5,), offset)
            H.abs_kth_rows(xd, 5, N, r, kth)
            torch.cuda.synchronize()
            got = kth.cpu().numpy()
            want = np.partition(ax, r, axis=1)[:, r]
            assert ok_k() and ok_x(), "guard band written"
            assert np.array_equal(bits(got), bits(want)), (N, r, offset, got, want)
            assert bool(np.isnan(got[4])) == (r >= N - nans)                              # NaNs sort above +Inf, and only there
            assert not np.isnan(got[:4]).any()
        assert np.array_equal(bits(xd.cpu().numpy()), bits(x))                            # the input is left alone


def test_selection_refuses_bad_arguments(vd):
    from v_diffusion import _hip as H
    x, k = torch.zeros((2, 8), device=DEV), torch.zeros((2,), device=DEV)
    with pytest.raises(H.HipError, match="null"):
        H.abs_kth_rows(None, 2, 8, 0, k)
    with pytest.raises(H.HipError, match="empty"):
        H.abs_kth_rows(x, 0, 8, 0, k)
    with pytest.raises(H.HipError, match="empty"):
        H.abs_kth_rows(x, 2, 0, 0, k)
    for r in (-1, 8):
        with pytest.raises(H.HipError, match="rank"):
            H.abs_kth_rows(x, 2, 8, r, k)
    with pytest.raises(H.HipError, match="at most"):
        H.abs_kth_rows(x, 2, 2 ** 31, 0, k)


# --------------------------------------------------------------------------------------------------------------- 2. the fused step
@functools.lru_cache(maxsize=None)
def cosine_table(steps, mot, w):
    """computed once and shared (the tests only read it)"""
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    return (fn,) + tuple(vd.solver_coefs(fn, steps, order=2, spacing="time", model_out_type=mot, w_guide=w))


def step_inputs(shape, mot, cfg, steps, row, seed):
    """table row ``row`` of the cosine +-20 schedule with ``steps`` steps; x_t at the row's log-SNR, a stand-in network output of
    n*(1+cfg) interleaved rows and C (2C) channels, and the previous prediction (zero on the first executed row).  Sample 0's x_t and
    output rows are scaled by 0.05: its predictions stay inside the data range, where the threshold is the static one."""
    fn, table, t_net = cosine_table(steps, mot, W_GUIDE if cfg else 0.0)
    B, C = shape[:2]
    a, s = R.alpha_sigma(fn(t_net[row:row + 1].clone()).float())
    xt = (float(a) * rnd(shape, seed + 1).clamp(-1, 1).double() + float(s) * rnd(shape, seed + 2).double()).float()
    out = rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), seed + 3, 0.8)
    hist = torch.zeros(shape) if row == steps - 1 else rnd(shape, seed + 4, 0.7)
    xt[0] *= 0.05
    out[:1 + cfg] *= 0.05
    return table[row], xt, out, hist


def run_kernel(H, k, xt, out, hist, mot, cfg, r, s_max=INF, alias=False, k_dev=False, offset=0):
    """(xn, new hist, s, xdup, guard bands intact) of one launch on device copies of the inputs placed ``offset`` floats off alignment"""
    B, C = xt.shape[:2]
    HW = xt[0, 0].numel()
    (xd, ok_x), (od, _), (hd, ok_h) = placed(xt, offset), placed(out, offset), placed(hist, offset)
    xn, ok_n = (xd, ok_x) if alias else guarded(xt.shape, offset)
    xdup, ok_d = guarded((2 * B,) + tuple(xt.shape[1:]), offset) if cfg else (None, lambda: True)
    sd, ok_s = guarded((B,), offset)
    kd = k.to(DEV).contiguous() if k_dev else None
    H.solver_step_dyn(xd, od, hd, None if k_dev else k.tolist(), H.OUT_TYPES[mot], cfg, r, s_max, sd, xn, xdup, B, C, HW, k_dev=kd)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))      # as bits: a test may plant a NaN
    assert same(od, out) and (alias or same(xd, xt))                                     # inputs left alone
    return xn.clone(), hd.clone(), sd.clone(), None if xdup is None else xdup.clone(), ok_n() and ok_h() and ok_d() and ok_s()


def composition(k, xt, out, hist, mot, cfg, r, s_max=INF):
    """the kernel's arithmetic in its stated order as fp32 tensor ops on the GPU: (xn, g', s, g)"""
    a0, b0x, b0e, c1, c2, c2r, w, _ = k.tolist()
    xt, out, hist = xt.to(DEV), out.to(DEV), hist.to(DEV)
    B, C = xt.shape[:2]

    def pred(o):
        p = a0 * xt + b0x * o[:, :C]
        return p + b0e * o[:, C:] if mot == "both" else p
    if cfg:
        xc, xu = pred(out[0::2]), pred(out[1::2])
        g = xc + w * (xc - xu)
    else:
        g = pred(out)
    s = torch.kthvalue(g.abs().reshape(B, -1), r + 1, dim=1).values.clamp(min=1.0).clamp(max=s_max)
    sb = s.reshape(B, 1, 1, 1)
    gp = torch.maximum(torch.minimum(g, sb), -sb) / sb
    return c1 * xt + c2 * gp + c2r * (gp - hist), gp, s, g


def row_err(got, ref):
    """max over rows of the row's max error relative to the row's own scale"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.detach().double().reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1).clamp(min=1e-300)
    return float(((got - ref).abs().amax(dim=1) / scale).max())


def held_to_fp64(what, got, ref, cmp):
    worst = []
    for q, g_, r_, c_ in zip(("xn", "hist", "s"), got, ref, cmp):
        ek, ec = row_err(g_, r_), row_err(c_, r_)
        worst.append((q, ek, ec))
        print(f"[dyn step {what}] {q}: kernel {ek:.3e} composition {ec:.3e}")
    for q, ek, ec in worst:
        assert ek <= 2.0 * ec + FLOOR, f"{what} {q}: kernel {ek:.3e}, composition {ec:.3e}"


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_kernel_against_fp64(vd, shape, mot, cfg):
    """xn, the new hist and s on a first row (c2rho = 0, zero hist), an interior row and row 0, at 8 steps and at 1024 (weights near 1),
    q = 0.995, no cap; and the invariants of the kernel's own output.  The regime of every sample (s_raw below or above 1) is read off
    the fp64 restatement, and both must occur in every launch but the eps network's first executed row, where 1/alpha ~ e^10 puts
    even the scaled-down sample 0 above 1."""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    N = shp[1] * shp[2] * shp[3]
    r = T.rank(N, Q)
    for steps, mid in ((8, 3), (1024, 300)):
        for row in (steps - 1, mid, 0):
            k, xt, out, hist = step_inputs(shp, mot, cfg, steps, row, seed=17 + row)
            what = f"{shape} {mot} {'guided' if cfg else 'plain'} steps={steps} row={row}"
            xn, hn, s, xdup, intact = run_kernel(H, k, xt, out, hist, mot, cfg, r)
            assert intact, "guard band written"
            ref_xn, ref_g, ref_s = T.step_dyn(k, xt, out, hist, mot == "both", cfg, r)
            oc, ou = (out[0::2], out[1::2]) if cfg else (out, out)
            net = lambda x_, t_, lab: (oc if bool(lab.any()) else ou).double()
            g_ref = R.guided_x0(net, xt.double(), None, torch.ones(shp[0]), k.double(), mot == "both", cfg, clip=False)
            raw = T.s_raw(g_ref, r)
            print(f"[dyn step {what}] reference s_raw {[round(float(v), 4) for v in raw]}")
            above = raw > 1.0
            assert bool(above.any()), what
            if not (mot == "eps" and row == steps - 1):
                assert not bool(above[0]), what                                          # the scaled-down sample: s = 1, the static clamp
                assert bool(above[1:].any()), what
            cxn, cg, cs, _ = composition(k, xt, out, hist, mot, cfg, r)
            held_to_fp64(what, (xn, hn, s), (ref_xn, ref_g, ref_s), (cxn, cg, cs))
            # ---- invariants of the kernel's own output
            hb = hn.cpu().reshape(shp[0], -1)
            assert bool((hb.abs() <= 1.0).all()) and bool((s >= 1.0).all()), what
            if row == 0:                                                                 # (0, 1, 0): the thresholded prediction itself
                assert torch.equal(xn, hn) and bool((xn.abs() <= 1.0).all()), what
            for b in range(shp[0]):
                if bool(above[b]):                                                       # the element that holds s_raw maps to exactly +-1
                    ones = int((hb[b].abs() == 1.0).sum())
                    ties = int((g_ref[b].float().abs() == raw[b].float()).sum())
                    assert 1 <= ones <= N - 1 - r + max(ties, 1), (what, b, ones, ties)
            if cfg:
                assert torch.equal(xdup[0::2], xn) and torch.equal(xdup[1::2], xn)


@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_cap_and_lower_quantiles_against_fp64(vd, shape, mot):
    """the same rule with s_max = 1.25 (the cap binds for samples 1 and 2) and at q = 0.5 and q = 1 (a pure rescale), guided, interior row"""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    N = shp[1] * shp[2] * shp[3]
    k, xt, out, hist = step_inputs(shp, mot, True, 8, 3, seed=11)
    for q, s_max in ((Q, 1.25), (0.5, INF), (1.0, INF)):
        r = T.rank(N, q)
        xn, hn, s, xdup, intact = run_kernel(H, k, xt, out, hist, mot, True, r, s_max)
        ref = T.step_dyn(k, xt, out, hist, mot == "both", True, r, s_max)
        cmp = composition(k, xt, out, hist, mot, True, r, s_max)
        assert intact, "guard band written"
        held_to_fp64(f"{shape} {mot} q={q} s_max={s_max}", (xn, hn, s), ref, cmp[:3])
        assert bool((s <= s_max).all()) and bool((hn.abs() <= 1.0).all())
        if s_max < INF:
            assert bool((ref[2][1:] == s_max).all()) and bool((s[1:].cpu() == s_max).all())
        if q == 1.0:                                                                     # nothing is clamped: exactly one +-1 per rescaled sample
            hb = hn.cpu().reshape(shp[0], -1)
            assert [int((hb[b].abs() == 1.0).sum()) for b in (1, 2)] == [1, 1]


@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_cap_one_without_guidance_is_the_static_clip_bit_for_bit(vd, shape, mot):
    """s_max = 1 forces s = 1: clamp to +-1, division by 1 -- vd_solver_step(clip = 1), whose guided prediction without cfg is the
    clipped branch itself"""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    N = shp[1] * shp[2] * shp[3]
    B, C, HW = shp[0], shp[1], shp[2] * shp[3]
    for steps, row in ((8, 7), (8, 3), (8, 0), (1024, 300)):
        k, xt, out, hist = step_inputs(shp, mot, False, steps, row, seed=23 + row)
        xn, hn, s, _, intact = run_kernel(H, k, xt, out, hist, mot, False, T.rank(N, Q), 1.0)
        xd, od, hd = xt.to(DEV), out.to(DEV), hist.to(DEV)
        sx = torch.empty_like(xd)
        H.solver_step(xd, od, hd, k.tolist(), H.OUT_TYPES[mot], False, True, sx, None, B, C, HW)
        assert intact and bool((s == 1.0).all())
        assert torch.equal(xn, sx) and torch.equal(hn, hd), (steps, row, float((xn - sx).abs().max()), float((hn - hd).abs().max()))


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_aliasing_forms_alignment_and_guard_bands(vd, shape, mot, cfg):
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    r = T.rank(shp[1] * shp[2] * shp[3], Q)
    k, xt, out, hist = step_inputs(shp, mot, cfg, 8, 3, seed=5)
    base = run_kernel(H, k, xt, out, hist, mot, cfg, r)
    assert base[4], "guard band written"
    for what, kw in (("xn aliasing xt", dict(alias=True)), ("k_dev", dict(k_dev=True)), ("bases one float off alignment", dict(offset=1)),
                     ("aliased, k_dev, off alignment", dict(alias=True, k_dev=True, offset=3))):
        got = run_kernel(H, k, xt, out, hist, mot, cfg, r, **kw)
        assert got[4], f"{what}: guard band written"
        for a, b in zip(base[:4], got[:4]):
            assert (a is None and b is None) or torch.equal(a, b), what
    # s_out is optional
    xd, od, hd = xt.to(DEV), out.to(DEV), hist.to(DEV)
    xn = torch.empty_like(xd)
    H.solver_step_dyn(xd, od, hd, k.tolist(), H.OUT_TYPES[mot], cfg, r, INF, None, xn, None, shp[0], shp[1], shp[2] * shp[3])
    assert torch.equal(xn, base[0]) and torch.equal(hd, base[1])


def test_a_nan_or_infinite_threshold_stays_in_its_sample(vd):
    """q = 1 with one NaN (one +Inf) in sample 1's network output: s is NaN (Inf) there and the sample's outputs are NaN (0 or NaN);
    samples 0 and 2 are what they are without it"""
    from v_diffusion import _hip as H
    shp = SHAPES["972"]
    N = 972
    k, xt, out, hist = step_inputs(shp, "v", False, 8, 3, seed=31)
    clean = run_kernel(H, k, xt, out, hist, "v", False, N - 1)
    for bad in (float("nan"), INF):
        o2 = out.clone()
        o2[1, 2, 7, 5] = bad
        xn, hn, s, _, intact = run_kernel(H, k, xt, o2, hist, "v", False, N - 1)
        assert intact
        for b in (0, 2):
            assert torch.equal(xn[b], clean[0][b]) and torch.equal(hn[b], clean[1][b]) and torch.equal(s[b], clean[2][b])
        if bad != bad:
            assert bool(torch.isnan(s[1])) and bool(torch.isnan(hn[1]).all()) and bool(torch.isnan(xn[1]).all())
        else:
            h1 = hn[1].cpu().reshape(-1)
            assert float(s[1]) == INF and int(torch.isnan(h1).sum()) == 1 and bool((h1[~torch.isnan(h1)] == 0.0).all())
    # below the top rank the NaN is one element among the others: s is a number and only that element is NaN
    o2 = out.clone()
    o2[1, 2, 7, 5] = float("nan")
    xn, hn, s, _, _ = run_kernel(H, k, xt, o2, hist, "v", False, N - 2)
    assert bool(torch.isfinite(s).all()) and int(torch.isnan(hn).sum()) == 1 and int(torch.isnan(xn).sum()) == 1


def test_entry_point_refuses_bad_arguments(vd):
    from v_diffusion import _hip as H
    z = torch.zeros((2, 3, 4, 4), device=DEV)
    k = [0.0] * 8
    call = lambda *a, **kw: H.solver_step_dyn(*a, **kw)
    with pytest.raises(H.HipError, match="either"):
        call(z, z.clone(), z.clone(), k, 0, False, 47, INF, None, z.clone(), None, 2, 3, 16, k_dev=torch.zeros(8, device=DEV))
    with pytest.raises(H.HipError, match="either"):
        call(z, z.clone(), z.clone(), None, 0, False, 47, INF, None, z.clone(), None, 2, 3, 16)
    with pytest.raises(H.HipError, match="null"):
        call(z, z.clone(), None, k, 0, False, 47, INF, None, z.clone(), None, 2, 3, 16)
    with pytest.raises(H.HipError, match="model_out_type"):
        call(z, z.clone(), z.clone(), k, 4, False, 47, INF, None, z.clone(), None, 2, 3, 16)
    with pytest.raises(H.HipError, match="empty"):
        call(z, z.clone(), z.clone(), k, 0, False, 47, INF, None, z.clone(), None, 0, 3, 16)
    with pytest.raises(H.HipError, match="of its own"):
        call(z, z.clone(), z, k, 0, False, 47, INF, None, z.clone(), None, 2, 3, 16)
    with pytest.raises(H.HipError, match="of its own"):
        call(z, z.clone(), (h := z.clone()), k, 0, False, 47, INF, None, h, None, 2, 3, 16)
    with pytest.raises(H.HipError, match="guided"):
        call(z, z.clone(), z.clone(), k, 0, False, 47, INF, None, z.clone(), torch.zeros((4, 3, 4, 4), device=DEV), 2, 3, 16)
    for s_max in (0.999, 0.0, float("nan")):
        with pytest.raises(H.HipError, match="s_max"):
            call(z, z.clone(), z.clone(), k, 0, False, 47, s_max, None, z.clone(), None, 2, 3, 16)
    for r in (-1, 48):
        with pytest.raises(H.HipError, match="rank"):
            call(z, z.clone(), z.clone(), k, 0, False, r, INF, None, z.clone(), None, 2, 3, 16)


# -------------------------------------------------------------------------------------------------------------------- 3. the chains
@pytest.mark.parametrize("order", (1, 2))
def test_dynamic_chain_against_fp64(vd, order):
    """p_sample_solver(clip_denoised="dynamic"), guided, T = 8, held to threshold_ref.chain_dyn; the allowance is the error of the static
    chain of the same call against solver_ref.chain, as in the solver's own chain test"""
    shp, steps = SHAPES["972"], 8
    N = shp[1] * shp[2] * shp[3]
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    gd = vd.GaussianDiffusion(fn, steps, "v", "fixed_large", "snr_trunc", "mse", w_guide=W_GUIDE, p_uncond=0.0)
    noise, y = rnd(shp, 29), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    dyn = gd.p_sample_solver(Stub(), shp, noise=noise, label=y, device=DEV, order=order, clip_denoised="dynamic")
    sta = gd.p_sample_solver(Stub(), shp, noise=noise, label=y, device=DEV, order=order, clip_denoised=True)
    table, t_net = vd.solver_coefs(fn, steps, order=order, spacing="time", model_out_type="v", w_guide=W_GUIDE)
    ref_d = T.chain_dyn(Stub(), noise, table, t_net, T.rank(N, Q), y=y.double(), cfg=True)
    ref_s = R.chain(Stub(), noise, table, t_net, y.double(), cfg=True, clip=True)
    ed, es = float((dyn.double() - ref_d).abs().max()), float((sta.double() - ref_s).abs().max())
    print(f"[dyn chain order {order}, T={steps}] dynamic {ed:.3e}  static {es:.3e}  (scales {float(ref_d.abs().max()):.3e} {float(ref_s.abs().max()):.3e})"
          f"  dynamic - static {float((dyn - sta).abs().max()):.3e}")
    assert dyn.shape == shp and dyn.device.type == "cpu" and bool((dyn.abs() <= 1.0).all())
    assert not torch.equal(dyn, sta)
    assert ed <= 2.0 * es + FLOOR * float(ref_d.abs().max()), (ed, es)
    # another quantile and a cap are other chains, each the restatement's
    capped = gd.p_sample_solver(Stub(), shp, noise=noise, label=y, device=DEV, order=order, clip_denoised="dynamic", dynamic_quantile=0.9,
                                dynamic_max=1.5)
    ref_c = T.chain_dyn(Stub(), noise, table, t_net, T.rank(N, 0.9), 1.5, y=y.double(), cfg=True)
    ec = float((capped.double() - ref_c).abs().max())
    print(f"[dyn chain order {order}, T={steps}] q=0.9 cap 1.5: {ec:.3e}")
    assert not torch.equal(capped, dyn) and ec <= 2.0 * es + FLOOR * float(ref_c.abs().max()), (ec, es)


def test_static_modes_did_not_move(vd):
    """clip_denoised=True / False through the method equal the module-level function called positionally with the arguments it had
    before the dynamic mode existed"""
    from v_diffusion import solver
    shp = SHAPES["972"]
    gd = vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), 8, "v", "fixed_large", "snr_trunc", "mse", w_guide=W_GUIDE,
                              p_uncond=0.0)
    noise, y = rnd(shp, 29), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    for clip in (True, False):
        new = gd.p_sample_solver(Stub(), shp, noise=noise, label=y, device=DEV, clip_denoised=clip)
        old = solver.p_sample_solver(gd, Stub(), shp, noise, y, DEV, None, None, 2, "time", clip, False).cpu()
        assert torch.equal(new, old)


def _tiny(vd):
    from oracle.cases import TINY, make_weights
    case = TINY["tinyA"]                                          # attention, class labels
    model = vd.UNet(**case["cfg"])
    model.load_state_dict(make_weights(case["cfg"]), strict=True)
    return model.to(DEV).eval(), case


def test_real_network_eager_and_graph(vd):
    model, case = _tiny(vd)
    B, R_, steps = 2, case["R"], 4
    shp = (B, 3, R_, R_)
    y = torch.tensor([1.0, 4.0])
    gd = vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), steps, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0)
    kw = dict(label=y, seed=5, clip_denoised="dynamic")
    a = gd.p_sample_solver(model, shp, **kw)
    assert a.shape == shp and a.device.type == "cpu" and bool(torch.isfinite(a).all()) and bool((a.abs() <= 1.0).all())
    c = gd.p_sample_solver(model, shp, use_graph=True, **kw)
    d = gd.p_sample_solver(model, shp, use_graph=True, **kw)                       # cached graph
    assert torch.equal(a, c) and torch.equal(a, d), (a - c).abs().max()
    assert len(gd._solver_graphs) == 1
    # the rank and the cap are launch arguments of the captured kernel: another quantile is another graph, not a wrong replay
    e = gd.p_sample_solver(model, shp, use_graph=True, dynamic_quantile=0.5, **kw)
    assert len(gd._solver_graphs) == 2
    assert torch.equal(e, gd.p_sample_solver(model, shp, dynamic_quantile=0.5, **kw)) and not torch.equal(e, a)
    f = gd.p_sample_solver(model, shp, use_graph=True, dynamic_max=1.0, **kw)
    assert len(gd._solver_graphs) == 3 and torch.equal(f, gd.p_sample_solver(model, shp, dynamic_max=1.0, **kw))
    # the static graph is a fourth entry and still the static chain
    g = gd.p_sample_solver(model, shp, label=y, seed=5, use_graph=True)
    assert len(gd._solver_graphs) == 4 and torch.equal(g, gd.p_sample_solver(model, shp, label=y, seed=5))
    assert torch.equal(c, gd.p_sample_solver(model, shp, use_graph=True, **kw))   # and the first entry replays as before
    dd = vd.DistillationDiffusion(model, steps, logsnr_fn=gd.logsnr_fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="snr_trunc")
    s = dd.p_sample_solver(model, shp, **kw)
    assert s.shape == shp and bool(torch.isfinite(s).all()) and bool((s.abs() <= 1.0).all())


@pytest.mark.parametrize("shape", ((3, 75), (2, 3, 18, 18), (4, 12288)), ids=("3x75", "2x3x18x18", "4x12288"))
def test_dynamic_threshold_function(vd, shape):
    x = rnd(shape, 71, 1.0)
    x[0] *= 0.2                                                                       # sample 0 stays inside the data range
    x[-1] *= 3.0
    B, N = shape[0], int(np.prod(shape[1:]))
    for q, cap in ((Q, None), (0.9, 2.0), (1.0, None)):
        got, s = vd.dynamic_threshold(x.to(DEV), q, cap)
        r = T.rank(N, q)
        raw = np.partition(np.abs(x.numpy().reshape(B, N)), r, axis=1)[:, r]
        want_s = np.minimum(np.maximum(raw, np.float32(1.0)), np.float32(INF if cap is None else cap))
        assert s.shape == (B,) and np.array_equal(bits(s.cpu().numpy()), bits(want_s))
        ref, ref_s = T.threshold(x.double(), r, INF if cap is None else cap)
        assert got.shape == x.shape and got.dtype == torch.float32 and float(s[0]) == 1.0 and float(s[-1]) > 1.0
        assert torch.equal(ref_s.float(), s.cpu())
        assert float((got.cpu().double() - ref).abs().max()) <= 2.0 ** -24                # one rounding of a quotient of magnitude <= 1
    with pytest.raises(RuntimeError, match="MI355X"):
        vd.dynamic_threshold(x)
