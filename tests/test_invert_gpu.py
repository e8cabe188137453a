"""Image inversion on the GPU (v_diffusion/invert.py over vd_noise_extract, vd_slerp_rows and the existing vd_sample_step /
vd_solver_step) against the float64 restatement of tests/invert_ref.py.  Networks of the kernel and chain tests are the pointwise
stand-in a(t) x + b(t) tanh(x) + g y, the same function in fp64 on the CPU and in fp32 on the GPU.  The yardstick for an error is the
project's: the same arithmetic, in the order the header states, as plain fp32 torch ops on the GPU from the same coefficients
(invert_ref's functions on fp32 GPU tensors); kernel and composition differ in FMA contraction only, so the kernel may be at most 2x as
far from fp64, plus 4 ulp of the row's scale.  The exact properties compare the new kernel with itself or with vd_inpaint_step's
known-region value, which is the same expression.  Needs an MI355X."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import invert_ref as R                                            # noqa: E402
import solver_ref as S                                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
# C*HW = 75: odd, below one block, scalar; 972 = 3*324: above 256, wide
SHAPES = {"75": (3, 3, 5, 5), "972": (2, 3, 18, 18)}
MOTS = ("v", "eps", "x0", "both")
W_GUIDE = 1.5
FLOOR = 4 * 2.0 ** -24
GUARD, SENTINEL = 64, -12345.0
NAN = float("nan")
F64 = torch.float64


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


def cosine(lim=20.0):
    import v_diffusion as vd
    return vd.get_logsnr_schedule("cosine", -lim, lim)


def _gd(T, mot="v", var="fixed_large", w=0.0, fn=None):
    import v_diffusion as vd
    return vd.GaussianDiffusion(fn or cosine(), T, mot, var, "snr_trunc", "mse", w_guide=w, p_uncond=0.0)


@functools.lru_cache(maxsize=None)
def step_row(T, i, mot, w, var, clip=True):
    """(the 10 fp32 weights of the DDPM step that lands on grid index i of the T-step cosine +-20 schedule, the network time); slot 5 of
    row 0 is 1.  Computed once and shared."""
    import v_diffusion as vd
    k, t_net = R.ddpm_row(vd, _gd(T, mot, var, w), i, clip)
    return tuple(k), t_net


@functools.lru_cache(maxsize=None)
def step_inputs(shape, mot, cfg, T, i, seed):
    """CPU fp32 inputs of the step that lands on index i: x_t at the log-SNR of index i + 1, a stand-in network output of n*(1+cfg)
    interleaved rows and C (2C) channels, the image and the draw.  Computed once and shared; the tests only read."""
    B, C = shape[:2]
    a, s = R.alpha_sigma(cosine()(torch.tensor([(i + 1) / T], dtype=torch.float64)).float())
    xt = (float(a) * rnd(shape, seed + 1).clamp(-1, 1).double() + float(s) * rnd(shape, seed + 2).double()).float()
    out = rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), seed + 3, 0.8)
    return xt, out, rnd(shape, seed + 6, 0.6).clamp(-1, 1), rnd(shape, seed + 5)


def run_kernel(H, k, xt, out, x0, eps, mot, cfg, last, clip, alias=False, k_dev=False, offset=0):
    """(xs, z, xdup, guard bands intact) of one launch on device copies of the inputs placed ``offset`` floats off alignment"""
    B, C = xt.shape[:2]
    HW = xt[0, 0].numel()
    (xd, ok_x), (od, _), (x0d, _) = (placed(t, offset) for t in (xt, out, x0))
    ed = None if eps is None else placed(eps, offset)[0]
    xs, ok_s = (xd, ok_x) if alias else guarded(xt.shape, offset)
    z, ok_z = guarded(xt.shape, offset)
    xdup, ok_d = guarded((2 * B,) + tuple(xt.shape[1:]), offset) if cfg else (None, lambda: True)
    kdev = torch.tensor(k, dtype=torch.float32, device=DEV) if k_dev else None
    H.noise_extract(xd, od, x0d, ed, None if k_dev else list(k), H.OUT_TYPES[mot], cfg, last, clip, xs, z, xdup, B, C, HW, k_dev=kdev)
    torch.cuda.synchronize()
    same = lambda d, h: torch.equal(d.cpu()[~torch.isnan(h)], h[~torch.isnan(h)]) and bool(torch.isnan(d.cpu()[torch.isnan(h)]).all())
    assert same(od, out) and same(x0d, x0) and (eps is None or same(ed, eps)) and (alias or same(xd, xt))        # inputs left alone
    return xs.clone(), z.clone(), None if xdup is None else xdup.clone(), ok_s() and ok_x() and ok_z() and ok_d()


def row_err(got, ref):
    """max over rows of the row's max error relative to the row's own scale"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.detach().cpu().double().reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1).clamp(min=1e-300)
    return float(((got - ref).abs().amax(dim=1) / scale).max())


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_kernel_against_fp64(vd, shape, mot, cfg, clip):
    """the first, an interior and the last row (last_step = 1, scale 1, (ak, bk) = (1, 0), no draw) of the 8-step and the 1024-step
    table, fixed_small and fixed_large; z and xs each by the 2x rule"""
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    worst = [0.0] * 4
    for T, mid in ((8, 3), (1024, 300)):
        for i in (T - 1, mid, 0):
            for var in ("fixed_small", "fixed_large"):
                k, _ = step_row(T, i, mot, W_GUIDE if cfg else 0.0, var, clip)
                xt, out, x0, eps = step_inputs(shp, mot, cfg, T, i, 17 + i)
                eps = None if i == 0 else eps
                assert (k[5], k[8], k[9]) == (1.0, 1.0, 0.0) if i == 0 else k[5] > 0
                xs, z, xdup, intact = run_kernel(H, k, xt, out, x0, eps, mot, cfg, i == 0, clip)
                d = lambda t: None if t is None else t.double()
                g = lambda t: None if t is None else t.to(DEV)
                xs_ref, z_ref = R.extract(k, d(xt), d(out), d(x0), d(eps), mot == "both", cfg, i == 0, clip)
                xs_cmp, z_cmp = R.extract(k, g(xt), g(out), g(x0), g(eps), mot == "both", cfg, i == 0, clip)
                e = (row_err(z, z_ref), row_err(z_cmp, z_ref), row_err(xs, xs_ref), row_err(xs_cmp, xs_ref))
                worst = [max(a, b) for a, b in zip(worst, e)]
                assert intact, "guard band written"
                assert e[0] <= 2.0 * e[1] + FLOOR, f"z, T={T} i={i} {var}: kernel {e[0]:.3e}, composition {e[1]:.3e}"
                assert e[2] <= 2.0 * e[3] + FLOOR, f"xs, T={T} i={i} {var}: kernel {e[2]:.3e}, composition {e[3]:.3e}"
                if cfg:
                    assert torch.equal(xdup[0::2], xs) and torch.equal(xdup[1::2], xs)
    print(f"[noise extract {shape} {mot} {'guided' if cfg else 'plain'} {'clip' if clip else 'noclip'}] worst z kernel {worst[0]:.3e} "
          f"composition {worst[1]:.3e}   xs kernel {worst[2]:.3e} composition {worst[3]:.3e}")


# ------------------------------------------------------------------------------------------------ 2. exact properties
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("shape", SHAPES, ids=list(SHAPES))
def test_exact_properties(vd, shape, mot, cfg):
    from v_diffusion import _hip as H
    shp = SHAPES[shape]
    B, C, HW = shp[0], shp[1], shp[2] * shp[3]
    T, i = 8, 3
    k, _ = step_row(T, i, mot, W_GUIDE if cfg else 0.0, "fixed_large")
    xt, out, x0, eps = step_inputs(shp, mot, cfg, T, i, 5)
    base = run_kernel(H, k, xt, out, x0, eps, mot, cfg, False, True)
    assert base[3], "guard band written"
    # (a) xs is vd_inpaint_step's known-region value: mask = 1 everywhere, the image as known, the draw as knoise
    xn = torch.empty(shp, device=DEV)
    H.inpaint_step(xt.to(DEV), out.to(DEV), rnd(shp, 9).to(DEV), x0.to(DEV), torch.ones((B, 1) + shp[2:], device=DEV), eps.to(DEV), list(k),
                   H.OUT_TYPES[mot], cfg, False, True, 1, xn, None, B, C, HW)
    assert torch.equal(base[0], xn)
    # (b) the duplicated rows
    if cfg:
        assert torch.equal(base[2][0::2], base[0]) and torch.equal(base[2][1::2], base[0])
    # (c) forms: aliasing, device coefficients, scalar access (bases off alignment) -- the same bits, guard bands intact
    for what, kw in (("xs aliasing xt", dict(alias=True)), ("k_dev", dict(k_dev=True)), ("bases one float off alignment", dict(offset=1)),
                     ("bases three floats off alignment", dict(offset=3)), ("aliased, k_dev, off alignment", dict(alias=True, k_dev=True, offset=1))):
        got = run_kernel(H, k, xt, out, x0, eps, mot, cfg, False, True, **kw)
        assert got[3], f"{what}: guard band written"
        for a, b in zip(base[:3], got[:3]):
            assert (a is None and b is None) or torch.equal(a, b), what
    # ... and on the last row (no draw)
    k0, _ = step_row(T, 0, mot, W_GUIDE if cfg else 0.0, "fixed_large")
    last = run_kernel(H, k0, xt, out, x0, None, mot, cfg, True, True)
    assert last[3] and torch.equal(last[0].cpu(), x0)              # (ak, bk) = (1, 0): the state the chain ends on is the image
    for kw in (dict(offset=1), dict(alias=True, k_dev=True)):
        got = run_kernel(H, k0, xt, out, x0, None, mot, cfg, True, True, **kw)
        assert got[3] and torch.equal(got[0], last[0]) and torch.equal(got[1], last[1])
    # (d) a NaN in one sample's network output stays in that sample's z and never reaches xs
    bad = out.clone()
    bad[(1 + cfg) * 1:(1 + cfg) * 2] = NAN                         # sample 1's rows (cond and uncond)
    xs, z, _, intact = run_kernel(H, k, xt, bad, x0, eps, mot, cfg, False, True)
    assert intact and torch.equal(xs, base[0])
    assert bool(torch.isnan(z[1]).all()) and torch.equal(z[0], base[1][0]) and torch.equal(z[2:], base[1][2:])
    xs, z, _, _ = run_kernel(H, k, torch.full_like(xt, NAN), out, x0, eps, mot, cfg, False, True)
    assert torch.equal(xs, base[0]) and bool(torch.isnan(z).all())


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_entry_points_refuse_bad_arguments(vd):
    from v_diffusion import _hip as H
    z = lambda: torch.zeros((2, 3, 4, 4), device=DEV)
    k = [0.0] * 5 + [0.5] + [0.0] * 4
    kd = torch.tensor(k, device=DEV)

    def call(xt=1, out=1, x0=1, eps=1, k10=k, mot=0, xs=1, zz=1, n=2, k_dev=None, cfg=False, xdup=None):
        t = lambda v: z() if isinstance(v, int) else v
        H.noise_extract(t(xt), t(out), t(x0), t(eps), k10, mot, cfg, False, False, t(xs), t(zz), xdup, n, 3, 16, k_dev=k_dev)
    call()                                                      # the base call is accepted
    call(eps=None)                                              # ... and so is a null draw with bk = 0
    call(k10=None, k_dev=kd)
    with pytest.raises(H.HipError, match="either"):
        call(k_dev=kd)
    with pytest.raises(H.HipError, match="either"):
        call(k10=None)
    for name in ("xt", "out", "x0", "xs", "zz"):
        with pytest.raises(H.HipError, match="null"):
            call(**{name: None})
    for mot in (-1, 4):
        with pytest.raises(H.HipError, match="model_out_type"):
            call(mot=mot)
    for n in (0, -1):
        with pytest.raises(H.HipError, match="empty"):
            call(n=n)
    for scale in (0.0, NAN, float("inf")):
        with pytest.raises(H.HipError, match="noise scale"):
            call(k10=[0.0] * 5 + [scale] + [0.0] * 4)
    with pytest.raises(H.HipError, match="eps required"):
        call(eps=None, k10=[0.0] * 5 + [0.5] + [0.0] * 3 + [0.5])
    with pytest.raises(H.HipError, match="duplicated"):
        call(xdup=torch.zeros((4, 3, 4, 4), device=DEV))
    same = z()
    with pytest.raises(H.HipError, match="buffer of its own"):
        call(xs=same, zz=same)
    a, b, o = z(), z() + 1.0, z()
    H.slerp_rows(a, b, 0.5, o, None, 2, 48)
    for out_ in (a, b):
        with pytest.raises(H.HipError, match="alias"):
            H.slerp_rows(a, b, 0.5, out_, None, 2, 48)
    with pytest.raises(H.HipError, match="either"):
        H.slerp_rows(a, b, 0.5, o, None, 2, 48, frac_dev=torch.zeros(2, device=DEV))
    with pytest.raises(H.HipError, match="either"):
        H.slerp_rows(a, b, None, o, None, 2, 48)
    for args in ((None, b, 0.5, o), (a, None, 0.5, o), (a, b, 0.5, None)):
        with pytest.raises(H.HipError, match="null"):
            H.slerp_rows(*args, None, 2, 48)
    for n, N in ((0, 48), (2, 0), (-1, 48)):
        with pytest.raises(H.HipError, match="empty"):
            H.slerp_rows(a, b, 0.5, o, None, n, N)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. chains with the stand-in
def replay_draws(seed, shape, count):
    """the sampler's draws: ``count`` tensors of the image shape from one generator on the GPU, in order"""
    g = torch.Generator(DEV).manual_seed(seed)
    return [torch.randn(shape, device=DEV, generator=g) for _ in range(count)]


@pytest.mark.parametrize("start", (None, 3), ids=("full", "start3"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
def test_invert_then_replay_returns_the_image(vd, mot, cfg, start):
    """T = 8: the reconstruction error of the samplers against that of the same two chains as fp32 torch ops over the replayed draws"""
    shp, T, seed = SHAPES["972"], 8, 29
    Tc = T if start is None else start
    gd = _gd(T, mot, "fixed_large", 1.0 if cfg else 0.0)
    x0 = rnd(shp, 31, 0.6).clamp(-1, 1).to(DEV)
    y = torch.arange(1, shp[0] + 1, dtype=torch.float32) if cfg else None
    calls = []
    x_start, maps = gd.p_invert_noise(R.Stub(both=mot == "both", calls=calls), x0, label=y, seed=seed, start=start)
    assert calls == [(i + 1) / T for i in reversed(range(Tc))]    # one call per step, at the time it leaves
    assert maps.shape == (Tc,) + shp and maps.dtype == torch.float32 and maps.is_cuda and x_start.shape == shp and x_start.is_cuda
    back = gd.p_sample_replay(R.Stub(both=mot == "both"), x_start, maps, label=y)
    assert back.shape == shp and back.device.type == "cpu"
    row = lambda i: R.ddpm_row(vd, gd, i)
    eps = replay_draws(seed, shp, Tc)
    yd = None if y is None else y.to(DEV)
    s_cmp, m_cmp = R.invert(R.Stub(both=mot == "both"), x0, row, Tc, eps, yd, mot == "both", cfg)
    b_cmp = R.replay(R.Stub(both=mot == "both"), s_cmp, row, m_cmp, yd, mot == "both", cfg)
    scale = float(x0.abs().max())
    es, ec = float((back - x0.cpu()).abs().max()), float((b_cmp - x0).abs().max())
    print(f"[invert -> replay T={T} start={start} {mot} {'guided' if cfg else 'plain'}] samplers {es:.3e}  composition {ec:.3e}  (scale {scale:.3e})")
    assert es <= 2.0 * ec + FLOOR * scale, (es, ec)
    if cfg:                                                       # another label is an edit; without the residual the prediction is left
        edit = gd.p_sample_replay(R.Stub(both=mot == "both"), x_start, maps, label=y + 3.0)
        assert float((edit - x0.cpu()).abs().max()) > 1e-3
    m0 = maps.clone()
    m0[0] = 0
    dropped = gd.p_sample_replay(R.Stub(both=mot == "both"), x_start, m0, label=y)
    assert float((dropped + maps[0].cpu() - back).abs().max()) <= FLOOR * scale


def test_draw_order(vd):
    """eps_Tc, eps_{Tc-1}, ..., eps_1 from one generator: the replayed stream gives the same x_start and the same first map, bit for bit"""
    from v_diffusion import _hip as H
    shp, T, seed = SHAPES["75"], 8, 7
    B, C, HW = shp[0], shp[1], shp[2] * shp[3]
    gd = _gd(T, "v", "fixed_small", 1.0)
    x0, y = rnd(shp, 33, 0.6).clamp(-1, 1).to(DEV), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    x_start, maps = gd.p_invert_noise(R.Stub(), x0, label=y, seed=seed)
    eps = replay_draws(seed, shp, T)
    mine = torch.empty_like(x0)
    H.forward_jump(x0, eps[0], vd.known_coefs(gd.logsnr_fn, T, T), mine, None, B, C * HW)
    assert torch.equal(mine, x_start)
    k, t_net = R.ddpm_row(vd, gd, T - 1)
    t = torch.full((B,), t_net, dtype=F64, device=DEV)
    out = R.I.net_out(R.Stub(), mine, t, y.to(DEV), True).contiguous()
    xs, z = torch.empty_like(x0), torch.empty_like(x0)
    H.noise_extract(mine, out, x0, eps[1], k, 0, True, False, True, xs, z, None, B, C, HW)
    assert torch.equal(z, maps[T - 1])
    assert torch.equal(x_start, gd.p_invert_noise(R.Stub(), x0, label=y, seed=seed)[0])
    assert not torch.equal(x_start, gd.p_invert_noise(R.Stub(), x0, label=y, seed=seed + 1)[0])


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
def test_replay_of_the_samplers_own_draws_is_p_sample(vd, cfg):
    """p_sample(seed, use_ddim=False) draws x_T and then one noise per step, T - 1 ... 0 (the last one with scale 0): fed as maps, with
    maps[0] = 0, the replay is that chain bit for bit"""
    shp, T, seed = SHAPES["972"], 8, 13
    gd = _gd(T, "v", "fixed_large", 1.0 if cfg else 0.0)
    y = torch.arange(1, shp[0] + 1, dtype=torch.float32) if cfg else None
    want = gd.p_sample(R.Stub(), shp, label=y, device=DEV, seed=seed, use_ddim=False)
    draws = replay_draws(seed, shp, 1 + T)
    maps = torch.stack(draws[1:][::-1])                           # maps[i] = the draw of the step landing on i
    maps[0] = 0
    got = gd.p_sample_replay(R.Stub(), draws[0], maps, label=y)
    assert torch.equal(got, want)


@pytest.mark.parametrize("order", (1, 2))
def test_encode_against_the_restatement(vd, order):
    """T = 8 on the cosine +-20 schedule, guided, the full latent and stop = 3; latent, composition and fp64 chain from the same table"""
    shp, T = SHAPES["972"], 8
    gd = _gd(T, "v", "fixed_large", 1.0)
    x0, y = rnd(shp, 41, 0.6).clamp(-1, 1).to(DEV), torch.arange(1, shp[0] + 1, dtype=torch.float32)
    table, t_net = vd.encode_coefs(gd.logsnr_fn, T, order=order, model_out_type="v", w_guide=1.0)
    for stop in (None, 3):
        calls = []
        lat = gd.p_encode(R.Stub(calls=calls), x0, label=y, order=order, stop=stop)
        n = T if stop is None else stop
        assert calls == [i / T for i in range(n)] and lat.shape == shp and lat.is_cuda
        ref = R.solver_chain(R.Stub(), x0.cpu().double(), table.double(), t_net, range(n), y.double(), cfg=True)
        cmp = R.solver_chain(R.Stub(), x0, table, t_net, range(n), y.to(DEV), cfg=True)
        scale = float(ref.abs().max())
        es, ec = float((lat.cpu().double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
        print(f"[encode T={T} order={order} stop={stop}] p_encode {es:.3e}  composition {ec:.3e}  (scale {scale:.3e})")
        assert es <= 2.0 * ec + FLOOR * scale, (es, ec)


@pytest.mark.parametrize("order", (1, 2))
def test_gaussian_round_trip(vd, order):
    """the exactly solvable problem of tests/test_invert_cpu.py at T = 16: p_encode then p_sample_solver (which ends on the x0 prediction)
    against the restatement of the same two chains in fp64, by the error of those chains as fp32 torch ops"""
    T, fn = 16, cosine(6.0)
    gd = _gd(T, "x0", "fixed_large", 0.0, fn)
    _, net = S.gaussian_problem(fn)
    shp = SHAPES["75"]
    x0 = rnd(shp, 47, 2.0).to(DEV)
    kw = dict(steps=T, order=order, spacing="logsnr", clip_denoised=False)
    lat = gd.p_encode(net, x0, **kw)
    got = gd.p_sample_solver(net, shp, noise=lat, device=DEV, **kw)
    up, t_up = vd.encode_coefs(fn, T, order=order, spacing="logsnr", model_out_type="x0")
    down, t_down = vd.solver_coefs(fn, T, order=order, spacing="logsnr", model_out_type="x0")

    def both_ways(x, cast):
        z = R.solver_chain(net, x, cast(up), t_up, range(T))
        return R.solver_chain(net, z, cast(down), t_down, reversed(range(T)))
    ref = both_ways(x0.cpu().double(), lambda t: t.double())
    cmp = both_ways(x0, lambda t: t)
    scale = float(ref.abs().max())
    es, ec = float((got.double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    trip = float((ref - x0.cpu().double()).abs().max() / x0.abs().max())
    print(f"[gaussian round trip T={T} order={order}] samplers {es:.3e}  composition {ec:.3e}  (scale {scale:.3e}; the fp64 round trip is "
          f"off the image by {trip:.3e})")
    assert es <= 2.0 * ec + FLOOR * scale, (es, ec)


# ------------------------------------------------------------------------------------------------ 5. vd_slerp_rows
def _ulp32(x):
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


# N = 75: one partial trip, scalar; 4097: five trips of the scalar form, the last with one thread; 4100: two trips of the wide form
@pytest.mark.parametrize("per_sample", (False, True), ids=("scalar_frac", "per_sample_frac"))
@pytest.mark.parametrize("shape", ((3, 3, 5, 5), (2, 4097), (2, 4100)), ids=("75", "4097", "4100"))
def test_slerp_against_fp64(vd, shape, per_sample):
    B = shape[0]
    a, b = rnd(shape, 61, 1.3), rnd(shape, 62, 0.8)
    frac = torch.tensor([0.3, 0.85, 0.5][:B]) if per_sample else 0.3
    f32 = frac.double() if per_sample else float(torch.tensor(0.3).float())
    ad, ok_a = placed(a)
    bd, ok_b = placed(b)
    out, w = vd.slerp(ad, bd, frac.to(DEV) if per_sample else frac, return_weights=True)
    again = vd.slerp(ad, bd, frac if per_sample else frac)
    torch.cuda.synchronize()
    assert ok_a() and ok_b() and torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b)
    assert out.shape == shape and out.is_cuda and w.shape == (B, 2) and torch.equal(out, again)        # two calls, the same bits
    ref, wa, wb = R.slerp(a.double(), b.double(), f32)
    cmp, _, _ = R.slerp(ad, bd, frac.to(DEV) if per_sample else frac)
    assert bool(((w[:, 0].cpu().double() - wa).abs() <= _ulp32(wa)).all()) and bool(((w[:, 1].cpu().double() - wb).abs() <= _ulp32(wb)).all()), \
        (w, wa, wb)
    ek, ec = row_err(out, ref), row_err(cmp, ref)
    print(f"[slerp {shape} {'per-sample' if per_sample else 'scalar'} frac] kernel {ek:.3e} composition {ec:.3e}")
    assert ek <= 2.0 * ec + FLOOR, (ek, ec)
    # written through the binding into a guarded buffer: nothing outside the rows
    from v_diffusion import _hip as H
    o2, ok_o = guarded(shape)
    H.slerp_rows(ad, bd, None if per_sample else 0.3, o2, None, B, a[0].numel(), frac_dev=frac.to(DEV) if per_sample else None)
    torch.cuda.synchronize()
    assert ok_o() and torch.equal(o2, out)


def test_slerp_branches(vd):
    """near-parallel rows (sin w < 1e-6) and a zero row take the linear weights; the ends return the inputs; a NaN stays in its row"""
    shape, f = (4, 972), 0.3
    a = rnd(shape, 63)
    b = rnd(shape, 64)
    b[0] = 1.5 * a[0]
    b[0, :5] = torch.nextafter(b[0, :5], torch.full((5,), float("inf")))       # near-parallel, not parallel
    b[1] = 0.0
    b[2] = -2.0 * a[2]
    _, wa, wb = R.slerp(a.double(), b.double(), float(torch.tensor(f).float()))
    lin = (float(1.0 - torch.tensor(f).float().double()), float(torch.tensor(f).float()))
    assert wa[:3].tolist() == [lin[0]] * 3 and abs(float(wa[3]) - lin[0]) > 1e-3       # what the restatement says about these rows
    out, w = vd.slerp(a.to(DEV), b.to(DEV), f, return_weights=True)
    want = torch.tensor(lin, dtype=F64).float()
    assert torch.equal(w[:3].cpu(), want.expand(3, 2)) and not torch.equal(w[3].cpu(), want)
    ends0, ends1 = vd.slerp(a.to(DEV), b.to(DEV), 0.0), vd.slerp(a.to(DEV), b.to(DEV), 1.0)
    assert float((ends0.cpu() - a).abs().max()) <= 2.0 ** -23 * float(a.abs().max())
    assert float((ends1.cpu() - b).abs().max()) <= 2.0 ** -23 * float(b.abs().max())
    bad = a.clone()
    bad[3, 7] = NAN                                               # a row on the spherical branch: its norm, so both its weights
    o2 = vd.slerp(bad.to(DEV), b.to(DEV), f)
    assert bool(torch.isnan(o2[3]).all()) and torch.equal(o2[:3], out[:3])


# ------------------------------------------------------------------------------------------------ 6. one real network
def _tiny(vd):
    from oracle.cases import TINY, make_weights
    case = TINY["tinyA"]                                          # attention, class labels
    model = vd.UNet(**case["cfg"])
    model.load_state_dict(make_weights(case["cfg"]), strict=True)
    return model.to(DEV).eval(), case


def test_real_network_and_distillation_object(vd):
    """T = 4 through the tinyA UNet.  The replay sees states that differ from the inversion's by fp32 rounding, a few 2^-24, which the
    network and four steps may amplify; a wrong map, scale or order is off by O(1).  Bound: 1e-4 of the image's scale (an amplification
    of ~1e3 over the rounding), stated before the first GPU run."""
    model, case = _tiny(vd)
    B, R_, T = 2, case["R"], 4
    shp = (B, 3, R_, R_)
    y = torch.tensor([1.0, 4.0])
    gd = _gd(T, "v", "fixed_large", 1.0)
    x0 = rnd(shp, 53, 0.6).clamp(-1, 1).to(DEV)
    scale = float(x0.abs().max())
    x_start, maps = gd.p_invert_noise(model, x0, label=y, seed=5)
    assert maps.shape == (T,) + shp and bool(torch.isfinite(maps).all())
    back = gd.p_sample_replay(model, x_start, maps, label=y)
    err = float((back - x0.cpu()).abs().max())
    print(f"[invert -> replay, tinyA, T={T}] {err:.3e} (scale {scale:.3e})")
    assert back.device.type == "cpu" and err <= 1e-4 * scale, err
    edit = gd.p_sample_replay(model, x_start, maps, label=torch.tensor([2.0, 3.0]))
    assert bool(torch.isfinite(edit).all()) and float((edit - x0.cpu()).abs().max()) > 10 * max(err, FLOOR)
    lat = gd.p_encode(model, x0, label=y, order=2)
    assert lat.shape == shp and lat.is_cuda and bool(torch.isfinite(lat).all())
    mid = vd.slerp(lat, lat.flip(0), 0.5)
    assert mid.shape == shp and bool(torch.isfinite(mid).all())
    dd = vd.DistillationDiffusion(model, T, logsnr_fn=gd.logsnr_fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="snr_trunc")
    xs_d, maps_d = dd.p_invert_noise(model, x0, label=y, seed=5)
    back_d = dd.p_sample_replay(model, xs_d, maps_d, label=y)
    err_d = float((back_d - x0.cpu()).abs().max())
    print(f"[invert -> replay, tinyA, DistillationDiffusion] {err_d:.3e}")
    assert err_d <= 1e-4 * scale, err_d
    cpu_model = vd.UNet(**case["cfg"]).eval()                     # parameters on the CPU
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_invert_noise(cpu_model, x0, label=y, seed=5)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_replay(cpu_model, x_start, maps, label=y)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_encode(cpu_model, x0, label=y)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_invert_noise(model, x0.cpu(), label=y, seed=5)
