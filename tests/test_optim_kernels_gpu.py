"""The optimizer tail (csrc/optim.hip: vd_sumsq, vd_adamw_ema, vd_adamw_ema_flagged) against tests/optim_ref.py at the constants the product
trains with: EMA decay 0.9999, betas (0.9, 0.999), a clipped and an unclipped step in turn, a range that sits steps out, 24 steps.

The rate tests isolate one constant each.  With m = v = 0 the new moments are (1 - beta) g and (1 - beta) g^2: what is off the fp64 value is
the rounding of the constant and of the products, a few u = 2^-24, and a constant formed as 1.f - fp32(beta) is seen directly.  The EMA
rate is read from the movement of the shadow: err = (e_got - e_0) - mv with mv the fp64 movement, s = sum(err mv) / sum(mv^2).  The
rounding of the stored shadow (up to u of |e| per element, independent of mv) is projected out at a rate of 1 / sqrt(n); what remains
in s is the relative error of the rate.  Its bound, 8 u rms(e) / ((1 - decay) rms(p - e_0) sqrt(n)) + 2 u, is about 13 standard deviations
of that projection (sqrt(K) times as many over K steps) plus the rounding of the constant itself.

Everywhere else the bound is test_kernels_gpu.close: 4 x the error of step32_torch (the same update through torch's own fp32 operators on
the CPU) plus 2 u of the buffer's largest element, and for m, v and the shadow the median of got / ref64 - 1 within 4 u: a systematic
factor shows in the median however small it is against the largest element.

All data comes from seeded CPU generators; the references of a case are computed once and shared.  Needs an MI355X."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R                                             # noqa: E402
from test_kernels_gpu import close                                # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
N = 65539                           # 2^16 + 3
KEYS = R.KEYS
PRODUCT = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, wd=0.01)


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


def randn(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).float()


def to_dev(state):
    return {k: state[k].clone().to(DEV) for k in KEYS}


def to_cpu(dstate):
    return {k: dstate[k].cpu() for k in KEYS}


def dev_step(H, d, g, *, lr, betas, eps, wd, max_norm, gnorm_sq, decay, k, rng=None, rng_mode=0, rng_k=None, flag=None, steps=None):
    """one launch on the device state d (in place).  gnorm_sq: a device tensor or None.  flag / steps given: vd_adamw_ema_flagged"""
    b1, b2 = betas
    args = (d["p"], g, d["m"], d["v"], d["ema"], gnorm_sq, max_norm, lr, b1, b2, eps, wd, 1 - b1 ** k, 1 - b2 ** k, decay)
    if flag is not None:
        H.adamw_ema_flagged(*args, rng[0], rng[1], flag, steps)
    elif rng is None or rng_mode == 0:
        H.adamw_ema(*args)
    else:
        r_bc = (1 - b1 ** rng_k, 1 - b2 ** rng_k) if rng_mode == 2 else (1.0, 1.0)
        H.adamw_ema(*args, r_lo=rng[0], r_hi=rng[1], r_mode=rng_mode, r_bc1=r_bc[0], r_bc2=r_bc[1])


def refs(state, g, **kw):
    return R.step64(state, g, **kw), R.step32_torch(state, g, **kw)


def compare(got, ref64, ref32, what, keep=None, keys=KEYS):
    """close() per buffer, over the elements `keep` (all by default); returns the worst error / tolerance"""
    worst = 0.0
    for key in keys:
        a, b, c = (t[key] if keep is None else t[key][keep] for t in (got, ref64, ref32))
        scale = max(b.abs().max().item(), 1e-30)
        nat = (c.double() - b).abs().max().item()
        err = close(a, b, ref32=c, slack=4.0, floor=2 * U, name=f"{what} {key}")
        ratio = err / (4.0 * nat + 2 * U * scale)
        print(f"[{what}] {key}: max err {err:.3e}, natural fp32 noise {nat:.3e}, scale {scale:.3e}, err / tol {ratio:.3f}")
        worst = max(worst, ratio)
    return worst


def rel_median(got, ref64):
    ok = ref64 != 0
    return float((got.double()[ok] / ref64[ok] - 1.0).median())


def rms(x):
    return float(x.double().pow(2).mean().sqrt())


def rate_error(e_got, e0, mv):
    """s = sum(err mv) / sum(mv^2), err = (e_got - e0) - mv: the relative error of the rate the shadow moved with"""
    mv = mv.double()
    err = (e_got.double() - e0.double()) - mv
    return float((err * mv).sum() / (mv * mv).sum())


def rate_bound(e_got, decay, p0, e0, K=1):
    n = e_got.numel()
    return 8 * U * rms(e_got) * math.sqrt(K) / ((1 - decay) * rms(p0.double() - e0.double()) * math.sqrt(n)) + 2 * U


# ------------------------------------------------------------------------------------------------ rate constants, one step, isolated
@functools.lru_cache(maxsize=None)
def _moment_case():
    zero = torch.zeros(N)
    return {"p": randn(N, 11), "m": zero, "v": zero, "ema": randn(N, 12)}, randn(N, 13, 0.1)


@pytest.mark.parametrize("b2", [0.999, 0.99, 0.95])
def test_second_moment_rate(H, b2):
    """v = (1 - b2) g^2 from v = 0: |v / v64 - 1| <= 4 u on every element with g != 0 -- the rounding of the constant and of two products
    (three roundings, 1.5 u; torch's fp32 form reaches 2.7 u on the CPU).  (1.f - fp32(b2)) is 218 u, 18 u and 5.7 u off."""
    state, g = _moment_case()
    kw = dict(PRODUCT, betas=(0.9, b2), max_norm=1.0, gnorm_sq=None, decay=0.9999, k=1)
    d = to_dev(state)
    dev_step(H, d, g.to(DEV), **kw)
    v64 = R.step64(state, g, **kw)["v"]
    ok = g != 0
    worst = float((d["v"].cpu().double()[ok] / v64[ok] - 1).abs().max())
    print(f"[second moment b2={b2}] worst |v / v64 - 1| = {worst / U:.2f} u, median {rel_median(d['v'].cpu(), v64) / U:+.2f} u")
    assert worst <= 4 * U, f"b2 = {b2}: v is {worst / U:.1f} u off (1 - b2) g^2"


@pytest.mark.parametrize("b1", [0.9, 0.95, 0.5])
def test_first_moment_rate(H, b1):
    """m = (1 - b1) g from m = 0: |m / m64 - 1| <= 2 u (the constant and one product: 1 u; 1.2 u measured for the fp32 form on the CPU;
    (1.f - fp32(b1)) reaches 4.95 u at 0.9 and 0.95)"""
    state, g = _moment_case()
    kw = dict(PRODUCT, betas=(b1, 0.999), max_norm=1.0, gnorm_sq=None, decay=0.9999, k=1)
    d = to_dev(state)
    dev_step(H, d, g.to(DEV), **kw)
    m64 = R.step64(state, g, **kw)["m"]
    ok = g != 0
    worst = float((d["m"].cpu().double()[ok] / m64[ok] - 1).abs().max())
    print(f"[first moment b1={b1}] worst |m / m64 - 1| = {worst / U:.2f} u")
    assert worst <= 2 * U, f"b1 = {b1}: m is {worst / U:.1f} u off (1 - b1) g"


@pytest.mark.parametrize("decay", [0.9999, 0.999, 0.99, 0.9])
def test_ema_rate(H, decay):
    """lr = 0, wd = 0, g = 0: p stays, the shadow moves by (1 - decay) (p - e0).  |s| within the bound of the module docstring, for the
    kernel and -- so that the yardstick is checked where it is used -- for step32_torch."""
    p, e0, zero = randn(N, 21), randn(N, 22), torch.zeros(N)
    state = {"p": p, "m": zero, "v": zero, "ema": e0}
    kw = dict(lr=0.0, betas=(0.9, 0.999), eps=1e-8, wd=0.0, max_norm=1.0, gnorm_sq=None, decay=decay, k=1)
    d = to_dev(state)
    dev_step(H, d, zero.to(DEV), **kw)
    got = to_cpu(d)
    assert torch.equal(got["p"], p), "p moved with lr = 0, wd = 0, g = 0"
    mv = (1 - decay) * (p.double() - e0.double())
    s_dev = rate_error(got["ema"], e0, mv)
    s_t32 = rate_error(R.step32_torch(state, zero, **kw)["ema"], e0, mv)
    bound = rate_bound(got["ema"], decay, p, e0)
    print(f"[ema rate decay={decay}] s kernel {s_dev:+.3e}, s torch fp32 {s_t32:+.3e}, bound {bound:.3e}")
    assert abs(s_t32) <= bound, f"decay {decay}: the fp32 yardstick's own rate is {s_t32:.3e} off, bound {bound:.3e}"
    assert abs(s_dev) <= bound, f"decay {decay}: the shadow moved at a rate {s_dev:.3e} off 1 - decay, bound {bound:.3e}"
    close(got["ema"], R.step64(state, zero, **kw)["ema"], None, floor=2 * U, name="ema")


# ------------------------------------------------------------------------------------------------ multi-step drift at the product's constants
K_STEPS, DRIFT_RANGE, SIT_OUT, DRIFT_DECAY = 24, (777, 5001), (3, 4, 9), 0.9999
FLAG_CYCLE = (1.0, 2.0, 0.5)        # a rank sum of 2 and a fractional mean are both "set"


@functools.lru_cache(maxsize=None)
def _drift_inputs():
    """the start and one fresh gradient per step: scale 0.1 (norm about 25: clipped) and 0.002 (norm about 0.5: not clipped) in turn; on
    a step the range sits out its gradient is zero, as the engine leaves it"""
    state = {"p": randn(N, 31), "m": torch.zeros(N), "v": torch.zeros(N), "ema": randn(N, 32)}
    gs = []
    for s in range(1, K_STEPS + 1):
        g = randn(N, 40 + s, 0.1 if s % 2 else 0.002)
        if s in SIT_OUT:
            g[DRIFT_RANGE[0]:DRIFT_RANGE[1]] = 0
        gs.append(g)
    return state, tuple(gs)


@functools.lru_cache(maxsize=None)
def _drift_refs(norms):
    """(fp64, torch fp32) states after K_STEPS steps, both given the squared norms the device computed"""
    state, gs = _drift_inputs()
    s64, s32, rk = state, state, 0
    for s in range(1, K_STEPS + 1):
        mode = 1 if s in SIT_OUT else 2
        rk += mode == 2
        kw = dict(PRODUCT, max_norm=1.0, gnorm_sq=norms[s - 1], decay=DRIFT_DECAY, k=s, rng=DRIFT_RANGE, rng_mode=mode, rng_k=rk)
        s64, s32 = R.step64(s64, gs[s - 1], **kw), R.step32_torch(s32, gs[s - 1], **kw)
    return s64, s32


@pytest.mark.parametrize("flagged", [False, True], ids=["host_decided", "flagged"])
def test_multi_step_drift(H, flagged):
    """24 steps of the product's settings, the norm from vd_sumsq each step, the range [777, 5001) sitting out steps 3, 4 and 9 and running on
    its own count otherwise -- decided on the host (r_mode 1 / 2) or on the device from a flag of 0 / {1, 2, 0.5} and an int32 counter
    from 0.  p, m, v and the shadow against fp64: close() with the torch-fp32 run as yardstick, the median of got / ref64 - 1 of m, v
    and the shadow within 4 u, the rate of the shadow's 24-step movement within sqrt(24) x the one-step noise + 2 u.  Inside the range
    p, m, v keep their bits over every step sat out, and the device counter ends at the number of positive flags."""
    state, gs = _drift_inputs()
    lo, hi = DRIFT_RANGE
    d = to_dev(state)
    ss = torch.empty(1, device=DEV)
    flag = torch.zeros(1, device=DEV)
    steps = torch.zeros(1, dtype=torch.int32, device=DEV)
    norms, rk, nset = [], 0, 0
    for s in range(1, K_STEPS + 1):
        g = gs[s - 1].to(DEV)
        H.sumsq(g, ss)
        norms.append(float(ss))
        close(ss, R.sumsq64(gs[s - 1]).reshape(1), ref32=(gs[s - 1] * gs[s - 1]).sum().reshape(1), floor=1e-6, name=f"sumsq step {s}")
        out = s in SIT_OUT
        rk += not out
        kw = dict(PRODUCT, max_norm=1.0, gnorm_sq=ss, decay=DRIFT_DECAY, k=s, rng=DRIFT_RANGE)
        if out:
            before = {k: d[k][lo:hi].clone() for k in ("p", "m", "v")}
        if flagged:
            flag.fill_(0.0 if out else FLAG_CYCLE[nset % 3])
            nset += not out
            dev_step(H, d, g, flag=flag, steps=steps, **kw)
        else:
            dev_step(H, d, g, rng_mode=1 if out else 2, rng_k=rk, **kw)
        if out:
            for k in ("p", "m", "v"):
                assert torch.equal(d[k][lo:hi].view(torch.int32), before[k].view(torch.int32)), f"step {s}: {k}[{lo}:{hi}) changed"
    got = to_cpu(d)
    if flagged:
        assert int(steps[0]) == K_STEPS - len(SIT_OUT) == nset, int(steps[0])
    ref64, ref32 = _drift_refs(tuple(norms))
    what = "drift flagged" if flagged else "drift"
    for key in ("m", "v", "ema"):
        print(f"[{what}] {key}: median of got / ref64 - 1 = {rel_median(got[key], ref64[key]):+.3e} ({rel_median(got[key], ref64[key]) / U:+.2f} u), "
              f"torch fp32 {rel_median(ref32[key], ref64[key]) / U:+.2f} u")
    mv = ref64["ema"] - state["ema"].double()
    s_dev, s_t32 = rate_error(got["ema"], state["ema"], mv), rate_error(ref32["ema"], state["ema"], mv)
    bound = rate_bound(got["ema"], DRIFT_DECAY, state["p"], state["ema"], K=K_STEPS)
    print(f"[{what}] ema rate over {K_STEPS} steps: s kernel {s_dev:+.3e}, s torch fp32 {s_t32:+.3e}, bound {bound:.3e}")
    worst = compare(got, ref64, ref32, what)
    print(f"[{what}] worst err / tol {worst:.3f}")
    for key in ("m", "v", "ema"):
        med = rel_median(got[key], ref64[key])
        assert abs(med) <= 4 * U, f"{key}: median of got / ref64 - 1 is {med:.3e} = {med / U:.1f} u"
    assert abs(s_dev) <= bound, f"the shadow's {K_STEPS}-step movement is {s_dev:.3e} off in rate, bound {bound:.3e}"


# ------------------------------------------------------------------------------------------------ step counts, clip edges: one step, n = 4099
N1, RANGE1 = 4099, (5, 1001)


@functools.lru_cache(maxsize=None)
def _one_step_case():
    """a state in mid-run (m of the gradient's size, v above its square's floor) and a gradient with its exact squared norm in fp32"""
    state = {"p": randn(N1, 51), "m": randn(N1, 52, 0.05), "v": randn(N1, 53, 0.05) ** 2 + 1e-5, "ema": randn(N1, 54)}
    g = randn(N1, 55, 0.1)
    return state, g, torch.tensor([float(R.sumsq64(g))], dtype=torch.float32)


@pytest.mark.parametrize("flagged", [False, True], ids=["host_decided", "flagged"])
@pytest.mark.parametrize("k", [1, 2, 1000, 200000])
def test_step_counts(H, k, flagged):
    """bias corrections from 1 - beta^k at k = 1 (bc2 = 1e-3) to k = 200000 (both 1 to fp32), the range at counts 1, 7 and 100000: handed in
    (r_mode 2) or formed on the device from a counter at 0, 6 and 99999, which the call advances"""
    state, g, sq = _one_step_case()
    for rk in (1, 7, 100000):
        kw = dict(PRODUCT, max_norm=1.0, decay=0.9999, k=k, rng=RANGE1)
        d = to_dev(state)
        if flagged:
            steps = torch.tensor([rk - 1], dtype=torch.int32, device=DEV)
            dev_step(H, d, g.to(DEV), gnorm_sq=sq.to(DEV), flag=torch.ones(1, device=DEV), steps=steps, **kw)
            assert int(steps[0]) == rk
        else:
            dev_step(H, d, g.to(DEV), gnorm_sq=sq.to(DEV), rng_mode=2, rng_k=rk, **kw)
        ref64, ref32 = refs(state, g, gnorm_sq=float(sq), rng_mode=2, rng_k=rk, **kw)
        compare(to_cpu(d), ref64, ref32, f"k={k} range k={rk}{' flagged' if flagged else ''}")


def _sq_of_norm(norm):
    """the fp32 squared norm handed to the kernel, and the same number for the references"""
    sq = torch.tensor([norm * norm], dtype=torch.float32)
    return sq, float(sq)


@pytest.mark.parametrize("factor", [1 - 1e-3, 1.0, 1 + 1e-3])
def test_clip_just_below_at_and_just_above_the_norm(H, factor):
    """sqrt(gnorm_sq) = max_norm (1 - 1e-3), max_norm, max_norm (1 + 1e-3): min(max_norm / (norm + 1e-6), 1) on both sides of its switch"""
    state, g, _ = _one_step_case()
    max_norm = 0.75
    sq, sqf = _sq_of_norm(max_norm * factor)
    kw = dict(PRODUCT, max_norm=max_norm, decay=0.9999, k=3)
    d = to_dev(state)
    dev_step(H, d, g.to(DEV), gnorm_sq=sq.to(DEV), **kw)
    ref64, ref32 = refs(state, g, gnorm_sq=sqf, **kw)
    compare(to_cpu(d), ref64, ref32, f"clip at {factor} max_norm")


def test_zero_gradient_with_norm_zero(H):
    """g = 0, norm 0: the clip factor is min(max_norm / 1e-6, 1) = 1, m and v decay by their betas, p by 1 - lr wd and the step of the
    decayed moments"""
    state, _, _ = _one_step_case()
    g = torch.zeros(N1)
    kw = dict(PRODUCT, max_norm=1.0, decay=0.9999, k=3)
    d = to_dev(state)
    dev_step(H, d, g.to(DEV), gnorm_sq=torch.zeros(1, device=DEV), **kw)
    got = to_cpu(d)
    ref64, ref32 = refs(state, g, gnorm_sq=0.0, **kw)
    compare(got, ref64, ref32, "zero gradient")
    for key, beta in (("m", 0.9), ("v", 0.999)):                     # one rounded constant, one product
        rel = (got[key].double() / (beta * state[key].double()) - 1).abs().max().item()
        assert rel <= 1.5 * U, (key, rel / U)


@pytest.mark.parametrize("case", ["max_norm_0", "no_norm"])
def test_no_clip_without_a_norm_or_a_bound(H, case):
    """max_norm = 0 with a norm given, and no norm with max_norm = 1: the gradient (norm about 6.4) is used as it is"""
    state, g, sq = _one_step_case()
    max_norm, sq_dev, sqf = (0.0, sq.to(DEV), float(sq)) if case == "max_norm_0" else (1.0, None, None)
    kw = dict(PRODUCT, max_norm=max_norm, decay=0.9999, k=3)
    d = to_dev(state)
    dev_step(H, d, g.to(DEV), gnorm_sq=sq_dev, **kw)
    got = to_cpu(d)
    ref64, ref32 = refs(state, g, gnorm_sq=sqf, **kw)
    compare(got, ref64, ref32, case)
    clipped = R.step64(state, g, gnorm_sq=float(sq), **dict(kw, max_norm=1.0))
    assert (clipped["m"] - ref64["m"]).abs().max() > 100 * 2 * U * ref64["m"].abs().max()      # (the case can tell the two apart)


def test_infinite_gradient_element(H):
    """one +inf element, norm +inf: clip = 0, that element's gradient is inf * 0 = NaN and every other one 0 -- the pattern
    clip_grad_norm_ + torch.optim.AdamW leave in fp32 on the CPU: p, m, v (and the shadow) NaN at the element, everything else updated
    with g = 0 inside the bounds"""
    state, g, _ = _one_step_case()
    g = g.clone()
    bad = 1234
    g[bad] = float("inf")
    kw = dict(PRODUCT, max_norm=1.0, decay=0.9999, k=1)
    d = to_dev({**state, "m": torch.zeros(N1), "v": torch.zeros(N1)})
    start = {**state, "m": torch.zeros(N1), "v": torch.zeros(N1)}
    dev_step(H, d, g.to(DEV), gnorm_sq=torch.full((1,), float("inf"), device=DEV), **kw)
    got = to_cpu(d)
    # torch's own pattern
    par = torch.nn.Parameter(state["p"].clone())
    par.grad = g.clone()
    opt = torch.optim.AdamW([par], lr=kw["lr"], betas=kw["betas"], eps=kw["eps"], weight_decay=kw["wd"])
    torch.nn.utils.clip_grad_norm_([par], 1.0)
    opt.step()
    st = opt.state_dict()["state"][0]
    want_nan = torch.zeros(N1, dtype=torch.bool)
    want_nan[bad] = True
    for key, t in (("p", par.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
        assert torch.equal(torch.isnan(t), want_nan), f"torch {key}"
        assert torch.equal(torch.isnan(got[key]), want_nan), f"{key}: NaN pattern differs from torch's"
        assert not torch.isinf(got[key]).any(), key
    assert torch.equal(torch.isnan(got["ema"]), want_nan)
    ref64, ref32 = refs(start, g, gnorm_sq=float("inf"), **kw)
    assert all(torch.equal(torch.isnan(ref64[key]), want_nan) for key in KEYS)
    compare(got, ref64, ref32, "inf gradient, the other elements", keep=~want_nan)
    zero_g = R.step64(start, torch.zeros(N1), gnorm_sq=None, **kw)
    for key in KEYS:
        assert torch.equal(zero_g[key][~want_nan], ref64[key][~want_nan]), key


# ------------------------------------------------------------------------------------------------ vd_sumsq
# sumsq_partial_kernel: 1024 blocks x 256 threads x one float4 = 2^20 elements per trip of the grid-stride loop, then a tail of n % 4
SUMSQ_SIZES = [1, 2, 3, 4, 5, 7, 255, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 5, 2 ** 21 + 3]


def _sumsq_check(H, g, name):
    out = torch.full((1,), float("nan"), device=DEV)
    H.sumsq(g.to(DEV), out)
    close(out, R.sumsq64(g).reshape(1), ref32=(g * g).sum().reshape(1), floor=1e-6, name=name)
    return float(out)


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_sizes(H, n):
    """N(0, 1); ones, where every partial sum is an integer below 2^24 and the result is n exactly; magnitudes of 1e15, whose squares
    (1e30) and their sum (below 1e38) are still finite"""
    _sumsq_check(H, randn(n, 60), f"sumsq randn n={n}")
    assert _sumsq_check(H, torch.ones(n), f"sumsq ones n={n}") == float(n)
    big = randn(n, 61).sign() * (1e15 * (1 + 0.5 * torch.rand(n, generator=torch.Generator().manual_seed(62))))
    got = _sumsq_check(H, big, f"sumsq 1e15 n={n}")
    assert math.isfinite(got)


def test_sumsq_keeps_small_terms(H):
    """magnitudes from 1e-3 to 1e3, log-uniform: squares over twelve decades in one sum"""
    n = 2 ** 20 + 5
    gen = torch.Generator().manual_seed(63)
    g = (10.0 ** (6 * torch.rand(n, generator=gen, dtype=torch.float64) - 3)).float() * randn(n, 64).sign()
    _sumsq_check(H, g, "sumsq 1e-3..1e3")


def test_sumsq_of_a_view_and_alignment(H):
    """a 16-byte aligned view into a larger buffer: the sum of the view only; a view one float off is refused before any launch"""
    n = 2 ** 20 + 5
    g = randn(n, 65)
    buf = torch.full((n + 16,), 1e3, device=DEV)
    view = buf[4:4 + n]
    view.copy_(g)
    out = torch.full((1,), float("nan"), device=DEV)
    H.sumsq(view, out)
    close(out, R.sumsq64(g).reshape(1), ref32=(g * g).sum().reshape(1), floor=1e-6, name="sumsq view")
    with pytest.raises(H.HipError):
        H.sumsq(buf[1:1 + n], out)
