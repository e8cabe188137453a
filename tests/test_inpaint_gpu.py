"""The RePaint inpainting sampler on the GPU (v_diffusion/inpaint.py over vd_inpaint_step and vd_forward_jump) against the float64
restatement of tests/inpaint_ref.py.  Networks of the kernel and chain tests are pointwise stand-ins, a(t) x + b(t) tanh(x) + g y, the
same function in fp64 on the CPU and in fp32 on the GPU.  The yardstick for a kernel's error is the same arithmetic, in the order the
header states, as plain fp32 torch ops on the GPU from the same coefficients (inpaint_ref's functions on fp32 GPU tensors): kernel and
composition differ in FMA contraction only, so the kernel may be at most 2x as far from fp64, plus 4 ulp of the row's scale (both start
from the same fp32 inputs and end in one fp32 rounding, each worth up to half an ulp that the comparison cannot see).  The exact
properties compare the new kernel with itself, so none of them depends on contraction.  Needs an MI355X."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref as R                                           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
# C*HW = 75: odd, below one block, scalar; 972 = 3*324: above 256, wide, HW % 4 == 0; 100: 4 | C*HW but HW = 25, so a wide access would
# straddle two channels of a one-channel mask (scalar for mask_c = 1, wide for mask_c = C)
SHAPES = {"75": (3, 3, 5, 5), "972": (2, 3, 18, 18), "100": (2, 4, 5, 5)}
MOTS = ("v", "eps", "x0", "both")
W_GUIDE = 1.5
FLOOR = 4 * 2.0 ** -24
GUARD, SENTINEL = 64, -12345.0
NAN = float("nan")


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
            assert bool((t == t[0]).all())
            self.calls.append(float(t[0]))
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        return torch.cat([out, 0.5 * out - 0.25 * x], dim=1) if self.both else out


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float()


def mixed_mask(shape, seed):
    """a random mix of exact 0, exact 1 and values strictly between"""
    g = torch.Generator().manual_seed(seed)
    pick = torch.rand(shape, generator=g)
    frac = torch.rand(shape, generator=g) * 0.98 + 0.01
    return torch.where(pick < 1 / 3, torch.zeros(shape), torch.where(pick < 2 / 3, torch.ones(shape), frac))


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


def cosine(lim=20.0):
    import v_diffusion as vd
    return vd.get_logsnr_schedule("cosine", -lim, lim)


@functools.lru_cache(maxsize=None)
def step_row(T, i, mot, w, ddim, clip=True):
    """(the 10 fp32 weights, as python floats, of the reverse step that lands on grid index i of the T-step cosine +-20 schedule, the
    network time): ``_step_coefs``'s eight and ``known_coefs``'s two.  Computed once and shared."""
    import v_diffusion as vd
    fn = cosine()
    gd = vd.GaussianDiffusion(fn, T, mot, "fixed_large", "snr_trunc", "mse", w_guide=w, p_uncond=0.0)
    k8, t_net = gd._step_coefs(i, ddim, clip)
    k = torch.tensor(list(k8) + list(vd.known_coefs(fn, T, i)), dtype=torch.float64).float()
    return tuple(k.tolist()), t_net


@functools.lru_cache(maxsize=None)
def step_inputs(shape, mot, cfg, mask_c, T, i, seed):
    """CPU fp32 inputs of the step that lands on index i: x_t at the log-SNR of index i + 1, a stand-in network output of n*(1+cfg)
    interleaved rows and C (2C) channels, both noises, a known image and a mixed mask.  Computed once and shared; the tests only read."""
    B, C = shape[:2]
    a, s = R.alpha_sigma(cosine()(torch.tensor([(i + 1) / T], dtype=torch.float64)).float())
    xt = (float(a) * rnd(shape, seed + 1).clamp(-1, 1).double() + float(s) * rnd(shape, seed + 2).double()).float()
    out = rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), seed + 3, 0.8)
    noise, knoise, known = rnd(shape, seed + 4), rnd(shape, seed + 5), rnd(shape, seed + 6, 0.6).clamp(-1, 1)
    mask = mixed_mask((B, mask_c) + tuple(shape[2:]), seed + 7)
    return xt, out, noise, known, mask, knoise


def run_kernel(H, k, xt, out, noise, known, mask, knoise, mot, cfg, last, clip, alias=False, k_dev=False, offset=0):
    """(xn, xdup, guard bands intact) of one launch on device copies of the inputs placed ``offset`` floats off alignment"""
    B, C = xt.shape[:2]
    HW = xt[0, 0].numel()
    (xd, ok_x), (od, _), (nd, _), (kd_, _), (md, _), (knd, _) = (placed(t, offset) for t in (xt, out, noise, known, mask, knoise))
    xn, ok_n = (xd, ok_x) if alias else guarded(xt.shape, offset)
    xdup, ok_d = guarded((2 * B,) + tuple(xt.shape[1:]), offset) if cfg else (None, lambda: True)
    kdev = torch.tensor(k, dtype=torch.float32, device=DEV) if k_dev else None
    H.inpaint_step(xd, od, nd, kd_, md, knd, None if k_dev else list(k), H.OUT_TYPES[mot], cfg, last, clip, mask.shape[1], xn, xdup,
                   B, C, HW, k_dev=kdev)
    torch.cuda.synchronize()
    for dev_t, host_t in ((od, out), (nd, noise), (kd_, known), (md, mask), (knd, knoise)):
        assert torch.equal(dev_t.cpu(), host_t.reshape(dev_t.shape)) or bool(torch.isnan(host_t).any())      # inputs left alone
    assert alias or torch.equal(xd.cpu(), xt) or bool(torch.isnan(xt).any())
    return xn.clone(), None if xdup is None else xdup.clone(), ok_n() and ok_x() and ok_d()


def fp64_step(k, xt, out, noise, known, mask, knoise, mot, cfg, last, clip):
    d = lambda t: t.double()
    return R.step(k, d(xt), d(out), d(noise), d(known), d(mask), d(knoise), mot == "both", cfg, last, clip)


def composition(k, xt, out, noise, known, mask, knoise, mot, cfg, last, clip):
    """the kernel's arithmetic in its stated order as fp32 tensor ops on the GPU"""
    g = lambda t: t.to(DEV)
    return R.step(k, g(xt), g(out), g(noise), g(known), g(mask), g(knoise), mot == "both", cfg, last, clip)


def row_err(got, ref):
    """max over rows of the row's max error relative to the row's own scale"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.detach().double().reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1).clamp(min=1e-300)
    return float(((got - ref).abs().amax(dim=1) / scale).max())


def lanes(mask, shape, value):
    """boolean image-shaped selection of the lanes whose mask equals ``value``"""
    return (mask == value).expand(shape)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("mask_c", ("one", "C"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_kernel_against_fp64(vd, shape, mask_c, mot, cfg, clip):
    """the first, an interior and the last row (last_step = 1, (ak, bk) = (1, 0)) of the 8-step and the 1024-step table (weights near
    1), DDPM and DDIM coefficients"""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    mc = 1 if mask_c == "one" else shp[1]
    worst = (0.0, 0.0)
    for T, mid in ((8, 3), (1024, 300)):
        for i in (T - 1, mid, 0):
            for ddim in (False, True):
                k, _ = step_row(T, i, mot, W_GUIDE if cfg else 0.0, ddim, clip)
                inp = step_inputs(shp, mot, cfg, mc, T, i, 17 + i)
                assert (k[8], k[9]) == ((1.0, 0.0) if i == 0 else vd.known_coefs(cosine(), T, i))
                xn, xdup, intact = run_kernel(H, k, *inp, mot, cfg, i == 0, clip)
                ref = fp64_step(k, *inp, mot, cfg, i == 0, clip)
                ek, ec = row_err(xn, ref), row_err(composition(k, *inp, mot, cfg, i == 0, clip), ref)
                worst = max(worst, (ek, ec))
                assert intact, "guard band written"
                assert ek <= 2.0 * ec + FLOOR, f"T={T} i={i} ddim={ddim}: kernel {ek:.3e}, composition {ec:.3e}"
                if cfg:
                    assert torch.equal(xdup[0::2], xn) and torch.equal(xdup[1::2], xn)
    print(f"[inpaint step {shape} mask_c={mask_c} {mot} {'guided' if cfg else 'plain'} {'clip' if clip else 'noclip'}] "
          f"kernel {worst[0]:.3e} composition {worst[1]:.3e}")


# ------------------------------------------------------------------------------------------------ 2. exact properties
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("mask_c", ("one", "C"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_the_ends_of_the_mask_select(vd, shape, mask_c, mot, cfg):
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    mc = 1 if mask_c == "one" else shp[1]
    T, i = 8, 3
    k, _ = step_row(T, i, mot, W_GUIDE if cfg else 0.0, False)
    xt, out, noise, known, mask, knoise = step_inputs(shp, mot, cfg, mc, T, i, 5)
    zero, one = lanes(mask, shp, 0.0), lanes(mask, shp, 1.0)
    assert bool(zero.any()) and bool(one.any()) and not bool((zero | one).all())
    base, _, intact = run_kernel(H, k, xt, out, noise, known, mask, knoise, mot, cfg, False, True)
    assert intact
    base = base.cpu()
    # (a) lanes with m == 0 are the all-zero-mask launch's
    allzero, _, _ = run_kernel(H, k, xt, out, noise, known, torch.zeros_like(mask), knoise, mot, cfg, False, True)
    assert torch.equal(base[zero], allzero.cpu()[zero])
    # (b) lanes with m == 1 do not see the unknown branch: NaN everywhere in it
    poisoned, _, _ = run_kernel(H, k, torch.full_like(xt, NAN), torch.full_like(out, NAN), torch.full_like(noise, NAN), known, mask, knoise,
                                mot, cfg, False, True)
    poisoned = poisoned.cpu()
    assert torch.equal(base[one], poisoned[one]) and bool(torch.isfinite(poisoned[one]).all())
    assert bool(torch.isnan(poisoned[~one]).all())
    # ... and lanes with m == 0 do not see the known branch
    pk, _, _ = run_kernel(H, k, xt, out, noise, torch.full_like(known, NAN), mask, torch.full_like(knoise, NAN), mot, cfg, False, True)
    assert torch.equal(base[zero], pk.cpu()[zero])
    # (c) with (ak, bk) = (1, 0) the m == 1 lanes are the known image, also on the last row
    k10 = k[:8] + (1.0, 0.0)
    kept, _, _ = run_kernel(H, k10, xt, out, noise, known, mask, knoise, mot, cfg, False, True)
    assert torch.equal(kept.cpu()[one], known[one])
    k0, _ = step_row(T, 0, mot, W_GUIDE if cfg else 0.0, False)
    last, _, _ = run_kernel(H, k0, xt, out, noise, known, mask, knoise, mot, cfg, True, True)
    assert torch.equal(last.cpu()[one], known[one])
    # (d) the all-zero-mask launch against vd_sample_step on the same inputs: each held to fp64, the new one by the existing one's error
    B, C = shp[:2]
    old = torch.empty(shp, device=DEV)
    H.sample_step(xt.to(DEV), out.to(DEV), noise.to(DEV), list(k[:8]), H.OUT_TYPES[mot], cfg, False, True, old, None, B, C, shp[2] * shp[3])
    ref = R.unknown(k, xt.double(), out.double(), noise.double(), mot == "both", cfg, False, True)
    en, eo = row_err(allzero, ref), row_err(old, ref)
    print(f"[inpaint zero mask vs vd_sample_step {shape} mask_c={mask_c} {mot} {'guided' if cfg else 'plain'}] new {en:.3e} old {eo:.3e} "
          f"bit-equal: {torch.equal(allzero, old)}")
    assert en <= 2.0 * eo + FLOOR, (en, eo)


# ------------------------------------------------------------------------------------------------ 3. forms
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("mask_c", ("one", "C"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_aliasing_forms_alignment_and_guard_bands(vd, shape, mask_c, mot, cfg):
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    mc = 1 if mask_c == "one" else shp[1]
    k, _ = step_row(8, 3, mot, W_GUIDE if cfg else 0.0, False)
    inp = step_inputs(shp, mot, cfg, mc, 8, 3, 5)
    base = run_kernel(H, k, *inp, mot, cfg, False, True)
    assert base[2], "guard band written"
    for what, kw in (("xn aliasing xt", dict(alias=True)), ("k_dev", dict(k_dev=True)), ("bases one float off alignment", dict(offset=1)),
                     ("bases three floats off alignment", dict(offset=3)), ("aliased, k_dev, off alignment", dict(alias=True, k_dev=True, offset=3))):
        got = run_kernel(H, k, *inp, mot, cfg, False, True, **kw)
        assert got[2], f"{what}: guard band written"
        for a, b in zip(base[:2], got[:2]):
            assert (a is None and b is None) or torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------ 4. vd_forward_jump
def run_jump(H, k, x, noise, dup, alias=False, k_dev=False, offset=0):
    B = x.shape[0]
    N = x[0].numel()
    (xd, ok_x), (nd, _) = placed(x, offset), placed(noise, offset)
    xn, ok_n = (xd, ok_x) if alias else guarded(x.shape, offset)
    xdup, ok_d = guarded((2 * B,) + tuple(x.shape[1:]), offset) if dup else (None, lambda: True)
    kdev = torch.tensor(k, dtype=torch.float32, device=DEV) if k_dev else None
    H.forward_jump(xd, nd, None if k_dev else list(k), xn, xdup, B, N, k_dev=kdev)
    torch.cuda.synchronize()
    assert torch.equal(nd.cpu(), noise) and (alias or torch.equal(xd.cpu(), x))
    return xn.clone(), None if xdup is None else xdup.clone(), ok_n() and ok_x() and ok_d()


@pytest.mark.parametrize("dup", (False, True), ids=("plain", "dup"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_forward_jump(vd, shape, dup):
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    x, noise = rnd(shp, 71, 0.7), rnd(shp, 72)
    for T, i, j in ((8, 2, 3), (8, 0, 8), (1024, 300, 1), (1024, 1, 10)):
        k = vd.jump_coefs(cosine(), T, i, j)
        xn, xdup, intact = run_jump(H, k, x, noise, dup)
        ref = R.jump(x.double(), noise.double(), *k)
        ek, ec = row_err(xn, ref), row_err(R.jump(x.to(DEV), noise.to(DEV), *k), ref)
        print(f"[forward jump {shape} T={T} {i}->{i + j}] kernel {ek:.3e} composition {ec:.3e}")
        assert intact, "guard band written"
        assert ek <= 2.0 * ec + FLOOR, (ek, ec)
        if dup:
            assert torch.equal(xdup[0::2], xn) and torch.equal(xdup[1::2], xn)
    k = vd.jump_coefs(cosine(), 8, 2, 3)
    base = run_jump(H, k, x, noise, dup)
    for what, kw in (("xn aliasing x", dict(alias=True)), ("k_dev", dict(k_dev=True)), ("bases one float off alignment", dict(offset=1)),
                     ("bases three floats off alignment", dict(offset=3)), ("aliased, k_dev, off alignment", dict(alias=True, k_dev=True, offset=3))):
        got = run_jump(H, k, x, noise, dup, **kw)
        assert got[2], f"{what}: guard band written"
        for a, b in zip(base[:2], got[:2]):
            assert (a is None and b is None) or torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_entry_points_refuse_bad_arguments(vd):
    from v_diffusion import _hip as H
    z = lambda: torch.zeros((2, 3, 4, 4), device=DEV)
    m1 = torch.zeros((2, 1, 4, 4), device=DEV)
    k = [0.0] * 10
    kd = torch.zeros(10, device=DEV)

    def call(xt=1, out=1, noise=1, known=1, mask=1, knoise=1, k10=k, mot=0, mask_c=1, xn=1, n=2, k_dev=None, cfg=False, xdup=None):
        t = lambda v: z() if isinstance(v, int) else v
        H.inpaint_step(t(xt), t(out), t(noise), t(known), m1 if isinstance(mask, int) else mask, t(knoise), k10, mot, cfg, False, False, mask_c,
                       t(xn), xdup, n, 3, 16, k_dev=k_dev)
    call()                                                      # the base call is accepted
    call(noise=None, knoise=None)                               # ... and so are null noises with zero scales
    with pytest.raises(H.HipError, match="either"):
        call(k_dev=kd)
    with pytest.raises(H.HipError, match="either"):
        call(k10=None)
    for name in ("xt", "out", "known", "mask", "xn"):
        with pytest.raises(H.HipError, match="null"):
            call(**{name: None})
    for mot in (-1, 4):
        with pytest.raises(H.HipError, match="model_out_type"):
            call(mot=mot)
    for mc in (0, 2, 4):
        with pytest.raises(H.HipError, match="mask_c"):
            call(mask_c=mc)
    for n in (0, -1):
        with pytest.raises(H.HipError, match="empty"):
            call(n=n)
    with pytest.raises(H.HipError, match="noise required"):
        call(noise=None, k10=[0.0] * 5 + [0.5] + [0.0] * 4)
    with pytest.raises(H.HipError, match="knoise required"):
        call(knoise=None, k10=[0.0] * 9 + [0.5])
    with pytest.raises(H.HipError, match="duplicated"):
        call(xdup=torch.zeros((4, 3, 4, 4), device=DEV))
    x = z()
    H.forward_jump(x, z(), [1.0, 0.0], z(), None, 2, 48)
    with pytest.raises(H.HipError, match="either"):
        H.forward_jump(x, z(), [1.0, 0.0], z(), None, 2, 48, k_dev=kd)
    with pytest.raises(H.HipError, match="either"):
        H.forward_jump(x, z(), None, z(), None, 2, 48)
    with pytest.raises(H.HipError, match="null"):
        H.forward_jump(x, None, [1.0, 0.0], z(), None, 2, 48)
    with pytest.raises(H.HipError, match="null"):
        H.forward_jump(x, z(), [1.0, 0.0], None, None, 2, 48)
    with pytest.raises(H.HipError, match="empty"):
        H.forward_jump(x, z(), [1.0, 0.0], z(), None, 0, 48)
    with pytest.raises(H.HipError, match="empty"):
        H.forward_jump(x, z(), [1.0, 0.0], z(), None, 2, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ chains
def replay(seed, shape, count):
    """the sampler's draws: ``count`` tensors of the image shape from one generator on the GPU, in order"""
    g = torch.Generator(DEV).manual_seed(seed)
    return [torch.randn(shape, device=DEV, generator=g) for _ in range(count)]


def draws_of(sched):
    """draws after the initial state: two per reverse step, one per jump"""
    return sum(2 if b < a else 1 for a, b in zip(sched, sched[1:]))


def chain_rows(vd, gd, use_ddim, clip=True):
    fn, T = gd.logsnr_fn, gd.sample_timesteps

    def step_row_(i):
        k8, t_net = gd._step_coefs(i, use_ddim, clip)
        return torch.tensor(list(k8) + list(vd.known_coefs(fn, T, i)), dtype=torch.float64).float().tolist(), t_net
    return step_row_, lambda i, j: vd.jump_coefs(fn, T, i, j)


def both_chains(vd, gd, sched, x0, known, mask, noises, y, use_ddim):
    """(the fp64 chain on the CPU, the same chain as fp32 torch ops on the GPU) from the state x0 (GPU fp32) over the replayed noises"""
    srow, jrow = chain_rows(vd, gd, use_ddim)
    c = lambda t: t.detach().cpu().double()
    ref = R.chain(Stub(), c(x0), c(known), c(mask), sched, srow, jrow, [c(n) for n in noises], None if y is None else y.double(),
                  cfg=y is not None, clip=True)
    g = lambda t: t.to(DEV, torch.float32)
    cmp = R.chain(Stub(), x0, g(known), g(mask), sched, srow, jrow, noises, None if y is None else y.to(DEV), cfg=y is not None, clip=True)
    return ref, cmp


def test_unmasked_ddim_chain_against_the_existing_sampler(vd):
    """mask = 0, DDIM, no resampling: the trajectory of p_sample(use_ddim=True) from the same x_T.  Each is held to the fp64 chain, the new
    one by the existing one's error (the rule of test_order_one_against_the_existing_ddim_sampler)."""
    shp, T, w = SHAPES["972"], 8, 1.0
    gd = vd.GaussianDiffusion(cosine(), T, "v", "fixed_large", "snr_trunc", "mse", w_guide=w, p_uncond=0.0)
    known, y = rnd(shp, 31, 0.6).clamp(-1, 1).to(DEV), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    mask = torch.zeros((1, 1) + shp[2:])
    sched = vd.resampling_schedule(T, 1, 1)
    draws = replay(11, shp, 1 + draws_of(sched))
    new = gd.p_sample_inpaint(Stub(), known, mask, label=y, seed=11, use_ddim=True, resamplings=1)
    old = gd.p_sample(Stub(), shp, noise=draws[0], label=y, device=DEV, use_ddim=True)
    ref, _ = both_chains(vd, gd, sched, draws[0], known, mask, draws[1:], y, True)
    scale = float(ref.abs().max())
    en, eo = float((new.double() - ref).abs().max()), float((old.double() - ref).abs().max())
    print(f"[inpaint mask=0 DDIM vs p_sample, T={T}] p_sample_inpaint {en:.3e}  p_sample {eo:.3e}  (scale {scale:.3e})")
    assert new.shape == shp and new.device.type == "cpu"
    assert en <= 2.0 * eo + FLOOR * scale, (en, eo)


def test_stochastic_masked_chain(vd):
    """T = 8, jumps of 2, 3 resamplings, DDPM, guided, half-image binary mask shared by the channels, seeded: the sampler against the
    fp64 chain over the replayed draws, by the error of the same chain as fp32 torch ops"""
    shp, T, j, r, seed = SHAPES["972"], 8, 2, 3, 23
    gd = vd.GaussianDiffusion(cosine(), T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0, p_uncond=0.0)
    known, y = rnd(shp, 37, 0.6).clamp(-1, 1).to(DEV), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    mask = torch.zeros((1, 1) + shp[2:])
    mask[..., : shp[3] // 2] = 1.0                                # keep the left half
    sched = vd.resampling_schedule(T, j, r)
    calls = []
    run = lambda s: gd.p_sample_inpaint(Stub(calls=calls), known, mask, label=y, seed=s, jump_length=j, resamplings=r)
    got = run(seed)
    assert calls == [(b + 1) / T for a, b in zip(sched, sched[1:]) if b < a]       # one call per reverse step, at the time it leaves
    assert len(calls) == T + (r - 1) * j * len(range(j, T - j + 1, j))
    draws = replay(seed, shp, 1 + draws_of(sched))
    ref, cmp = both_chains(vd, gd, sched, draws[0], known, mask, draws[1:], y, False)
    scale = float(ref.abs().max())
    es, ec = float((got.double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    print(f"[inpaint stochastic chain T={T} j={j} r={r}] sampler {es:.3e}  composition {ec:.3e}  (scale {scale:.3e})")
    assert got.shape == shp and got.device.type == "cpu"
    assert es <= 2.0 * ec + FLOOR * scale, (es, ec)
    keep = (mask == 1).expand(shp)
    assert torch.equal(got[keep], known.cpu()[keep])              # the known region is the known image, exactly
    assert torch.equal(got, run(seed))
    other = run(seed + 1)
    assert torch.equal(other[keep], known.cpu()[keep]) and not torch.equal(other[~keep], got[~keep])


def test_start_is_sdedit(vd):
    """start = 3 of T = 8 with an all-zero mask: x_3 = alpha_3 known + sigma_3 eps, three network calls, the fp64 chain from the replayed
    x_3"""
    shp, T, k, seed = SHAPES["972"], 8, 3, 41
    gd = vd.GaussianDiffusion(cosine(), T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0, p_uncond=0.0)
    known, y = rnd(shp, 43, 0.6).clamp(-1, 1).to(DEV), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    mask = torch.zeros((shp[0], shp[1]) + shp[2:])
    calls = []
    got = gd.p_sample_inpaint(Stub(calls=calls), known, mask, label=y, seed=seed, start=k)
    assert calls == [3 / T, 2 / T, 1 / T]
    sched = vd.resampling_schedule(k, 1, 1)
    draws = replay(seed, shp, 1 + draws_of(sched))
    ak, bk = vd.known_coefs(cosine(), T, k)
    x_ref = ak * known.cpu().double() + bk * draws[0].cpu().double()
    x_cmp = ak * known + bk * draws[0]
    srow, jrow = chain_rows(vd, gd, False)
    c = lambda t: t.detach().cpu().double()
    ref = R.chain(Stub(), x_ref, c(known), c(mask), sched, srow, jrow, [c(n) for n in draws[1:]], y.double(), cfg=True, clip=True)
    cmp = R.chain(Stub(), x_cmp, known, mask.to(DEV), sched, srow, jrow, draws[1:], y.to(DEV), cfg=True, clip=True)
    scale = float(ref.abs().max())
    es, ec = float((got.double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    print(f"[inpaint start={k} of T={T}] sampler {es:.3e}  composition {ec:.3e}  (scale {scale:.3e})")
    assert es <= 2.0 * ec + FLOOR * scale, (es, ec)
    for bad in (0, T + 1):
        with pytest.raises(ValueError, match="start"):
            gd.p_sample_inpaint(Stub(), known, mask, label=y, seed=seed, start=bad)


def _tiny(vd):
    from oracle.cases import TINY, make_weights
    case = TINY["tinyA"]                                          # attention, class labels
    model = vd.UNet(**case["cfg"])
    model.load_state_dict(make_weights(case["cfg"]), strict=True)
    return model.to(DEV).eval(), case


def test_real_network_and_distillation_object(vd):
    model, case = _tiny(vd)
    B, R_, T = 2, case["R"], 4
    shp = (B, 3, R_, R_)
    y = torch.tensor([1.0, 4.0])
    gd = vd.GaussianDiffusion(cosine(), T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0)
    known = rnd(shp, 53, 0.6).clamp(-1, 1).to(DEV)
    mask = torch.zeros((1, 1, R_, R_), dtype=torch.bool)
    mask[..., R_ // 2:, :] = True                                 # keep the lower half
    kw = dict(label=y, jump_length=1, resamplings=2)
    a = gd.p_sample_inpaint(model, known, mask, seed=5, **kw)
    keep = mask.expand(shp)
    assert a.shape == shp and a.device.type == "cpu" and bool(torch.isfinite(a).all())
    assert torch.equal(a[keep], known.cpu()[keep])
    assert torch.equal(a, gd.p_sample_inpaint(model, known, mask, seed=5, **kw))
    assert not torch.equal(a[~keep], gd.p_sample_inpaint(model, known, mask, seed=6, **kw)[~keep])
    dd = vd.DistillationDiffusion(model, T, logsnr_fn=gd.logsnr_fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="snr_trunc")
    s = dd.p_sample_inpaint(model, known, mask, seed=5, **kw)
    assert s.shape == shp and bool(torch.isfinite(s).all()) and torch.equal(s[keep], known.cpu()[keep])
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_inpaint(model, known, mask, seed=5, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_inpaint(vd.UNet(**case["cfg"]).eval(), known, mask, seed=5, **kw)     # parameters on the CPU
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_inpaint(model, known.cpu(), mask, seed=5, **kw)
