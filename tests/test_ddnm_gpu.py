"""DDNM null-space restoration on the GPU: the one kernel vd_ddnm_step against the float64 restatement of tests/ddnm_ref.py, its exact
properties, and the chains of ``GaussianDiffusion.p_sample_ddnm``.

Shapes, step rows, the stand-in network and the input recipe are those of tests/test_dps_gpu.py (imported, not copied): C*HW = 75 odd and
scalar, a one-channel mask a wide access would straddle, a non-square image, one block per channel (down8 on 8x8), both grey channel
counts; clipped predictions are kept 1e-3 off +-1.  The yardstick of the kernel's error is that file's ``held``: the same arithmetic as
plain fp32 torch ops on the GPU (ddnm_ref's functions on fp32 GPU tensors) -- the kernel may be at most 2x as far from fp64, plus 4 ulp of
the row's scale.  Every operand of a kernel launch lies between sentinel bands, at offsets 0 and 1 float (the wide and the scalar form).
Needs an MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ddnm_ref as R                                              # noqa: E402
import dps_ref as DR                                              # noqa: E402
import test_dps_gpu as D                                          # noqa: E402  (CASES, ROWS, Stub, case_inputs, guarded, held: imported, not copied)

pytestmark = pytest.mark.gpu
DEV = "cuda"
MOTS = D.MOTS
W_GUIDE = D.W_GUIDE
NAN = float("nan")
LAM = 0.7


@pytest.fixture(scope="module")
def vd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import v_diffusion
    from v_diffusion import _hip
    _hip.lib()
    return v_diffusion


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def run(H, k, xt, out, noise, meas, mask, lam, op, par, mot, cfg, last, clip, offset=0, alias=False, want_sum=True):
    """(xn, xdup, sumsq) of one vd_ddnm_step launch on device copies placed ``offset`` floats into sentinel-banded buffers; asserts that
    no band was written and no input changed"""
    B, C, Hh, Ww = xt.shape
    (xd, ok_x), (od, ok_o), (md, ok_m) = (D.placed(t, offset) for t in (xt, out, meas))
    nd, ok_z = (None, lambda: True) if noise is None else D.placed(noise, offset)
    kd, ok_k = (None, lambda: True) if mask is None else D.placed(mask, offset)
    xn, ok_n = (xd, ok_x) if alias else D.guarded(xt.shape, offset)
    xdup, ok_d = D.guarded((2 * B,) + tuple(xt.shape[1:]), offset) if cfg else (None, lambda: True)
    ss, ok_s = D.guarded((B,), offset) if want_sum else (None, lambda: True)
    H.ddnm_step(xd, od, nd, md, kd, list(k), lam, H.OUT_TYPES[mot], cfg, last, clip, H.DPS_OPS[op], par or 0, xn, xdup, ss, B, C, Hh, Ww)
    torch.cuda.synchronize()
    assert all(f() for f in (ok_x, ok_o, ok_m, ok_z, ok_k, ok_n, ok_d, ok_s)), "guard band written"
    assert same_bits(od.cpu(), out) and same_bits(md.cpu(), meas) and (alias or same_bits(xd.cpu(), xt))
    assert (noise is None or same_bits(nd.cpu(), noise)) and (mask is None or same_bits(kd.cpu(), mask))
    return xn.clone(), None if xdup is None else xdup.clone(), None if ss is None else ss.clone()


def both_forms(H, *a, **kw):
    """the launch at offsets 0 (16-byte aligned: the wide accesses where the shape allows them) and 1 float (scalar): the same bits"""
    xn, xdup, ss = run(H, *a, **kw)
    x1, d1, s1 = run(H, *a, offset=1, **kw)
    assert same_bits(x1, xn) and (xdup is None or same_bits(d1, xdup)) and (ss is None or same_bits(s1, ss)), "offset 1 float: other bits"
    return xn, xdup, ss


d64 = lambda t: None if t is None else t.double()
gpu = lambda t: None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize("last", (False, True), ids=("step", "last"))
@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("case", D.CASES, ids=list(D.CASES))
def test_kernel_against_fp64(vd, case, mot, cfg, clip, last):
    """the first, an interior and the last row of the 8-step table and a row of the 1024-step table (weights near 1), DDPM and DDIM
    coefficients; xn and sumsq by the yardstick, at both offsets"""
    from v_diffusion import _hip as H
    shape, op, par = D.CASES[case]
    both = mot == "both"
    for T, i, ddim in D.ROWS:
        k = D.step_row(T, i, mot, W_GUIDE if cfg else 0.0, ddim, clip)
        xt, out, noise, mask, meas, _ = D.case_inputs(case, mot, cfg, clip, T, i, ddim, 17 + i)
        what = f"{case} {mot} {'guided' if cfg else 'plain'} {'clip' if clip else 'noclip'} T={T} i={i} last={int(last)}"
        xn, xdup, ss = both_forms(H, k, xt, out, noise, meas, mask, LAM, op, par, mot, cfg, last, clip)
        ref = R.step(k, d64(xt), d64(out), d64(noise), d64(meas), op, LAM, par, d64(mask), both, cfg, last, clip)
        cmp = R.step(k, gpu(xt), gpu(out), gpu(noise), gpu(meas), op, LAM, par, gpu(mask), both, cfg, last, clip)
        D.held("xn", xn, cmp["xn"], ref["xn"], what)
        D.held("sumsq", ss, cmp["sumsq"], ref["sumsq"], what)
        assert not same_bits(xn.cpu(), R.step(k, xt, out, noise, meas, op, 0.0, par, mask, both, cfg, last, clip)["xn"]), "no correction made"
        if cfg:
            assert same_bits(xdup[0::2], xn) and same_bits(xdup[1::2], xn)


# ------------------------------------------------------------------------------------------------ 2. exact properties
PROP_CASES = ("mask75", "mask972", "mask100one", "mask100C", "down2", "down8", "gray3", "gray4")


def sample_step(H, k, xt, out, noise, mot, cfg, last, clip):
    return D.run_sample_step(H, k, xt, out, noise, mot, cfg, last, clip)


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("case", PROP_CASES)
def test_exact_properties(vd, case, mot, cfg):
    from v_diffusion import _hip as H
    shape, op, par = D.CASES[case]
    T, i = 8, 3
    k = D.step_row(T, i, mot, W_GUIDE if cfg else 0.0, False)
    xt, out, noise, mask, meas, _ = D.case_inputs(case, mot, cfg, True, T, i, False, 5)
    for last in (False, True):
        for nz in (noise, None) if last else (noise,):
            kk = list(k)
            if nz is None:
                kk[5] = 0.0
            args = (kk, xt, out, nz, meas, mask, LAM, op, par, mot, cfg, last, True)
            base, bdup = sample_step(H, kk, xt, out, nz, mot, cfg, last, True)
            # lam = 0: vd_sample_step's bits, whatever meas and mask hold (the mask is not read: NaN is no mask value)
            junk_m = None if mask is None else torch.full_like(mask, NAN)
            x0, d0, _ = both_forms(H, kk, xt, out, nz, torch.full_like(meas, NAN), junk_m, 0.0, op, par, mot, cfg, last, True, want_sum=False)
            assert same_bits(x0, base) and (not cfg or same_bits(d0, bdup))
            # ... and with the sum asked for, the sum is the step's and xn still vd_sample_step's
            x0s, _, s0 = both_forms(H, kk, xt, out, nz, meas, mask, 0.0, op, par, mot, cfg, last, True)
            assert same_bits(x0s, base)
            # the step proper: the same call gives the same bits; aliasing; the duplicate; the optional sum
            xn, xdup, ss = both_forms(H, *args)
            assert not same_bits(xn, base) and bool(torch.isfinite(xn).all()) and bool((ss > 0).all()) and same_bits(ss, s0)
            for kw in (dict(), dict(alias=True), dict(offset=1, alias=True), dict(want_sum=False), dict(offset=2)):
                x2, d2, s2 = run(H, *args, **kw)
                assert same_bits(x2, xn) and (not cfg or same_bits(d2, xdup)) and (s2 is None or same_bits(s2, ss)), kw
            if cfg:
                assert same_bits(xdup[0::2], xn) and same_bits(xdup[1::2], xn)
            if op != "mask":
                continue
            # an element that was not measured (M = 0) with NaN in meas: xn and sumsq stay finite, xn there is the lam = 0 value, and
            # nothing else notices
            hole = mask.expand(shape) == 0
            assert bool(hole.any()) and bool((~hole).any())
            x3, _, s3 = both_forms(H, kk, xt, out, nz, torch.where(hole, torch.full_like(meas, NAN), meas), mask, LAM, op, par, mot, cfg, last,
                                   True)
            assert same_bits(x3, xn) and same_bits(s3, ss) and same_bits(x3.cpu()[hole], base.cpu()[hole])


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("case", ("mask75", "mask100one", "mask100C", "mask972"))
def test_a_measured_pixel_of_the_last_step_is_the_measurement(vd, case, cfg):
    """mask M = 1, last step, lam = 1, no noise term: xn == meas bitwise; M = 0 keeps the prediction; with a noise term or lam < 1 the
    select is off"""
    from v_diffusion import _hip as H
    shape, op, par = D.CASES[case]
    k = list(D.step_row(8, 0, "v", W_GUIDE if cfg else 0.0, False))
    assert k[5] == 0.0
    xt, out, noise, mask, meas, _ = D.case_inputs(case, "v", cfg, True, 8, 0, False, 17)
    one, hole = (mask.expand(shape) == 1), (mask.expand(shape) == 0)
    assert bool(one.any()) and bool(hole.any()) and bool((~one & ~hole).any())
    base, _ = sample_step(H, k, xt, out, None, "v", cfg, True, True)
    for nz in (None, noise):                                      # (k[5] = 0: a noise that is given adds nothing)
        xn, _, _ = both_forms(H, k, xt, out, nz, meas, mask, 1.0, op, par, "v", cfg, True, True)
        assert same_bits(xn.cpu()[one], meas[one]) and same_bits(xn.cpu()[hole], base.cpu()[hole])
    k5 = list(k)
    k5[5] = 0.25
    xn, _, _ = both_forms(H, k5, xt, out, noise, meas, mask, 1.0, op, par, "v", cfg, True, True)
    assert not same_bits(xn.cpu()[one], meas[one])
    xn, _, _ = both_forms(H, k, xt, out, None, meas, mask, 0.5, op, par, "v", cfg, True, True)
    assert not same_bits(xn.cpu()[one], meas[one])


@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", ("v", "both"))
@pytest.mark.parametrize("case", ("down2", "down4", "down8", "gray3", "gray4"))
def test_the_null_space_part_is_the_network_s(vd, case, mot, cfg):
    """the two means on the last step: xn - A^+ A xn against g - A^+ A g of the fp64 prediction g, by the yardstick -- the correction
    moves the range-space part only -- and A xn against the measurement"""
    from v_diffusion import _hip as H
    shape, op, par = D.CASES[case]
    k = list(D.step_row(8, 0, mot, W_GUIDE if cfg else 0.0, False))
    xt, out, _, mask, meas, _ = D.case_inputs(case, mot, cfg, True, 8, 0, False, 17)
    null = lambda x: x - R.pinv(op, DR.apply_A(op, x, par), tuple(x.shape), par)
    xn, _, _ = both_forms(H, k, xt, out, None, meas, None, 1.0, op, par, mot, cfg, True, True)
    ref = R.step(k, d64(xt), d64(out), None, d64(meas), op, 1.0, par, None, mot == "both", cfg, True, True)
    cmp = R.step(k, gpu(xt), gpu(out), None, gpu(meas), op, 1.0, par, None, mot == "both", cfg, True, True)
    D.held("null-space part", null(xn.cpu().double()), null(cmp["xn"].cpu().double()), null(ref["g"]), f"{case} {mot} cfg={int(cfg)}")
    assert float(null(ref["g"]).abs().max()) > 0.05
    D.held("A xn", DR.apply_A(op, xn.cpu().double(), par), DR.apply_A(op, cmp["xn"].cpu().double(), par), d64(meas), f"{case} {mot}")


def test_wrapper_refuses_bad_arguments(vd):
    from v_diffusion import _hip as H
    z = lambda *s: torch.zeros(s, device=DEV)
    k = [0.8, -0.6, 0.0, 0.3, 0.7, 0.1, 0.0, 0.0]
    stp = lambda **kw: H.ddnm_step(*{**dict(xt=z(1, 3, 4, 4), out=z(1, 3, 4, 4), noise=z(1, 3, 4, 4), meas=z(1, 3, 4, 4), mask=z(1, 1, 4, 4),
                                            k=k, lam=1.0, mot=0, cfg=0, last=0, clip=1, op=0, par=1, xn=z(1, 3, 4, 4), xdup=None, ss=None,
                                            n=1, C=3, H=4, W=4), **kw}.values())
    stp()
    for kw, msg in ((dict(op=3), "bad op"), (dict(mot=5), "model_out_type"), (dict(mask=None), "null"), (dict(meas=None), "null"),
                    (dict(xn=None), "null"), (dict(par=2), "channels"), (dict(op=1, par=3), "down-sampling"),
                    (dict(op=1, par=8), "down-sampling"), (dict(n=0), "empty"), (dict(W=0), "empty"), (dict(noise=None), "noise")):
        with pytest.raises(H.HipError, match=msg):
            stp(**kw)
    with pytest.raises(H.HipError, match="CPU tensor"):
        stp(xt=torch.zeros(1, 3, 4, 4))
    stp(op=2, mask=None, meas=z(1, 1, 4, 4), ss=z(1))                     # the mask belongs to op 0 only
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. chains on the stand-in network
T_CHAIN, CHAIN_SHAPE = 8, (2, 3, 8, 8)
OPS = (("mask", 1), ("down", 2), ("gray", None))


def chain_setup(vd, op, par, guided, noisy=0.0):
    """(gd, label, mask, operator, measurement on the GPU) of a chain test: a mask with exact 0, exact 1 and a value between"""
    gd = D.make_gd(vd, T_CHAIN, "v", 1.0 if guided else 0.0)
    y = torch.arange(1, CHAIN_SHAPE[0] + 1, dtype=torch.float32) if guided else None
    mask = None
    if op == "mask":
        mask = torch.zeros((1, 1) + CHAIN_SHAPE[2:])
        mask[..., : CHAIN_SHAPE[3] // 2] = 1.0
        mask[..., CHAIN_SHAPE[3] // 2] = 0.5
    operator = D.operator_of(op, par, mask)
    clean = D.rnd(CHAIN_SHAPE, 31, 0.6).clamp(-1, 1)
    meas = vd.dps_measure(clean, operator)
    if noisy:
        meas = meas + noisy * D.rnd(tuple(meas.shape), 33)
    return gd, y, mask, operator, meas.to(DEV)


def fp64_chains(vd, gd, sched, draws, meas, op, par, mask, y, guided, ddim=False, **kw):
    """(the fp64 chain, the same chain as fp32 torch ops on the GPU) over the replayed draws"""
    row = lambda i: gd._step_coefs(i, ddim, True)
    jrow = lambda i, j: vd.jump_coefs(gd.logsnr_fn, gd.sample_timesteps, i, j)
    c = lambda t: None if t is None else t.detach().cpu().double()
    ref = R.chain(D.Stub(), c(draws[0]), c(meas), op, sched, row, jrow, [c(n) for n in draws[1:]], par=par, mask=c(mask), y=c(y), cfg=guided,
                  **kw)
    cmp = R.chain(D.Stub(), draws[0], meas, op, sched, row, jrow, draws[1:], par=par, mask=gpu(mask), y=gpu(y), cfg=guided, **kw)
    return ref, cmp


@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("op,par", OPS)
def test_chain_against_fp64_and_consistency(vd, op, par, guided):
    """T = 8, seeded, noiseless: the sampler against the fp64 chain over the replayed draws by the error of the same chain as fp32 torch
    ops; the residual norms; and the final image reproduces the measurement"""
    T, shape, seed = T_CHAIN, CHAIN_SHAPE, 29
    gd, y, mask, operator, meas = chain_setup(vd, op, par, guided)
    calls = []
    got, res = gd.p_sample_ddnm(D.Stub(calls=calls), meas, operator, shape, label=y, seed=seed, return_residuals=True)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape and not got.requires_grad
    assert calls == [(i + 1) / T for i in reversed(range(T))]                      # one network call per step
    assert res.is_cuda and res.dtype == torch.float32 and tuple(res.shape) == (T, shape[0]) and bool(torch.isfinite(res).all())
    draws = D.replay(seed, shape, T + 1)
    sched = list(range(T, -1, -1))
    (ref, rsum), (cmp, csum) = fp64_chains(vd, gd, sched, draws, meas, op, par, mask, y, guided)
    scale = float(ref.abs().max())
    es, ec = float((got.cpu().double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    print(f"[ddnm chain {op} {'guided' if guided else 'plain'} T={T}] sampler {es:.3e}  composition {ec:.3e}  (scale {scale:.3e})")
    assert es <= 2.0 * ec + D.FLOOR * scale, (es, ec)
    D.held("residual norms", res, torch.stack(csum).sqrt(), torch.stack(rsum).sqrt(), f"ddnm chain {op}")
    assert same_bits(got, gd.p_sample_ddnm(D.Stub(), meas, operator, shape, label=y, seed=seed, lam=[1.0] * T))      # the rule, noiseless
    # Consistency.  The last launch forms, per measurement element, A g (its fp64 sum narrowed to fp32: 1 rounding; the division by the
    # count: 1), r = meas - A g (1, of a value up to |meas| + |A g|: 2 units of the scale) and xn = fma(lam, d, g) (1; for a mask d = r / M
    # is one more, undone by A's M up to that rounding): at most 6 roundings of half an ulp, 2^-24 each, of the largest of |meas|, |xn| and
    # the clip's bound 1 + 2 w on |g|.
    M = None if mask is None else gpu(mask).double()
    back = DR.apply_A(op, got.double(), par, M)
    scale = max(float(meas.abs().max()), float(got.abs().max()), 1.0 + 2.0 * gd.w_guide * guided)
    taken = torch.ones_like(back, dtype=torch.bool) if M is None else M.expand(shape) > 0
    worst = float((back - meas.double())[taken].abs().max())
    print(f"[ddnm consistency {op}] |A x - y| {worst:.3e}  bound {6 * 2.0 ** -24 * scale:.3e}")
    assert worst <= 6 * 2.0 ** -24 * scale
    if M is not None:
        one = (M.expand(shape) == 1)
        assert same_bits(got[one], meas[one])
    plain = gd.p_sample_ddnm(D.Stub(), meas, operator, shape, label=y, seed=seed, lam=0.0)
    assert float((meas.double() - DR.apply_A(op, plain.double(), par, M))[taken].abs().max()) > 1e-2      # ... and lam = 0 does not


@pytest.mark.parametrize("ddim", (False, True), ids=("ddpm", "ddim"))
@pytest.mark.parametrize("guided", (False, True), ids=("plain", "guided"))
def test_lam_zero_is_p_sample(vd, guided, ddim):
    gd, y, mask, operator, meas = chain_setup(vd, "mask", 1, guided)
    got = gd.p_sample_ddnm(D.Stub(), torch.full_like(meas, NAN), operator, CHAIN_SHAPE, label=y, seed=7, lam=0.0, use_ddim=ddim)
    want = gd.p_sample(D.Stub(), CHAIN_SHAPE, label=y, device=DEV, seed=7, use_ddim=ddim)
    assert got.is_cuda and same_bits(got.cpu(), want)
    some = gd.p_sample_ddnm(D.Stub(), meas, operator, CHAIN_SHAPE, label=y, seed=7, use_ddim=ddim)
    assert not same_bits(some.cpu(), want) and bool(torch.isfinite(some).all())
    dd = vd.DistillationDiffusion(D.Stub(), T_CHAIN, logsnr_fn=gd.logsnr_fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="snr_trunc")
    s = dd.p_sample_ddnm(D.Stub(), meas, operator, CHAIN_SHAPE, label=y, seed=7)
    assert tuple(s.shape) == CHAIN_SHAPE and bool(torch.isfinite(s).all())


@pytest.mark.parametrize("op,par", OPS)
def test_noisy_measurement_follows_the_rule(vd, monkeypatch, op, par):
    """sigma_y > 0: the chain runs, and the lam and the noise scale every launch received are ``ddnm_rule``'s of the step's row"""
    from v_diffusion import _hip as H
    sigma = 0.5                      # (T = 8: the step to index 1 has noise scale 0.336 < c2 sigma = 0.377, the earlier ones cover theirs)
    gd, y, mask, operator, meas = chain_setup(vd, op, par, False, noisy=sigma)
    seen = []
    real = H.ddnm_step

    def recording(xt, out, noise, meas_, mask_, k8, lam, mot, cfg, last, *rest):
        seen.append((list(k8), lam, bool(last)))
        return real(xt, out, noise, meas_, mask_, k8, lam, mot, cfg, last, *rest)
    monkeypatch.setattr(H, "ddnm_step", recording)
    got = gd.p_sample_ddnm(D.Stub(), meas, operator, CHAIN_SHAPE, seed=3, sigma_y=sigma)
    monkeypatch.undo()
    assert bool(torch.isfinite(got).all()) and len(seen) == T_CHAIN
    lams = []
    for (k8, lam, last), i in zip(seen, reversed(range(T_CHAIN))):
        row, _ = gd._step_coefs(i, False, True)
        want_lam, want_ns = vd.ddnm_rule(row[4], row[5], sigma, i == 0)
        assert last == (i == 0) and lam == want_lam and k8[5] == want_ns and k8[:5] + k8[6:] == list(row[:5]) + list(row[6:]), i
        assert (c := row[4] * lam * sigma) ** 2 + k8[5] ** 2 <= row[5] ** 2 * (1 + 1e-12) + 1e-30, (i, c)
        lams.append(lam)
    assert lams[-1] == 0.0 and any(0.0 < l < 1.0 for l in lams) and any(l == 1.0 for l in lams), lams
    draws = D.replay(3, CHAIN_SHAPE, T_CHAIN + 1)
    (ref, _), (cmp, _) = fp64_chains(vd, gd, list(range(T_CHAIN, -1, -1)), draws, meas, op, par, mask, None, False, sigma_y=sigma)
    es, ec = float((got.cpu().double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    assert es <= 2.0 * ec + D.FLOOR * float(ref.abs().max()), (es, ec)


def test_time_travel_draw_order_and_call_count(vd, monkeypatch):
    """(jump_length, resamplings) = (2, 2): one generator seeded on the device; the initial state, then one image-shaped draw per
    transition and nothing else; T + (r - 1) j P network calls; the chain against fp64 over the replayed draws"""
    import v_diffusion.restore as restore          # (the chain is opened, and every draw made, there)
    T, shape, seed, j, r = T_CHAIN, CHAIN_SHAPE, 13, 2, 2
    gd, y, mask, operator, meas = chain_setup(vd, "down", 2, False)
    sched = vd.resampling_schedule(T, j, r)
    P = len(range(j, T - j + 1, j))
    steps = sum(b < a for a, b in zip(sched, sched[1:]))
    assert steps == T + (r - 1) * j * P and len(sched) - 1 - steps == (r - 1) * P
    seen, calls = [], []
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
    got, res = gd.p_sample_ddnm(D.Stub(calls=calls), meas, operator, shape, seed=seed, jump_length=j, resamplings=r, return_residuals=True)
    monkeypatch.undo()
    want = D.replay(seed, shape, len(sched))
    assert len(seen) == len(sched) and len({id(g) for g, _ in seen}) == 1 and seen[0][0] is not None and seen[0][0].device.type == "cuda"
    assert all(tuple(t.shape) == shape and torch.equal(t, w) for (_, t), w in zip(seen, want))
    assert calls == [a / T for a, b in zip(sched, sched[1:]) if b < a] and len(calls) == steps and tuple(res.shape) == (steps, shape[0])
    (ref, _), (cmp, _) = fp64_chains(vd, gd, sched, want, meas, "down", 2, None, None, False)
    es, ec = float((got.cpu().double() - ref).abs().max()), float((cmp.cpu().double() - ref).abs().max())
    assert es <= 2.0 * ec + D.FLOOR * float(ref.abs().max()), (es, ec)


def test_return_residuals_is_the_root_of_a_direct_launch(vd, monkeypatch):
    """the (reverse steps, B) tensor: each row the square root of the sumsq a direct launch on the step's operands gives"""
    from v_diffusion import _hip as H
    gd, y, mask, operator, meas = chain_setup(vd, "mask", 1, True)
    launches = []
    real = H.ddnm_step

    def recording(xt, out, noise, *rest):
        launches.append((xt.clone(), out.clone(), noise.clone(), rest))
        return real(xt, out, noise, *rest)
    monkeypatch.setattr(H, "ddnm_step", recording)
    got, res = gd.p_sample_ddnm(D.Stub(), meas, operator, CHAIN_SHAPE, label=y, seed=11, return_residuals=True)
    monkeypatch.undo()
    assert tuple(res.shape) == (T_CHAIN, CHAIN_SHAPE[0]) and len(launches) == T_CHAIN
    for n, (xt, out, noise, rest) in enumerate(launches):
        meas_, mask_, k8, lam, mot, cfg, last, clip, op, par, xn, xdup, ss, B, C, Hh, Ww = rest
        direct = torch.empty(B, device=DEV)
        real(xt, out, noise, meas_, mask_, k8, lam, mot, cfg, last, clip, op, par, torch.empty_like(xt), None, direct, B, C, Hh, Ww)
        assert same_bits(res[n], direct.sqrt()), n
    alone = gd.p_sample_ddnm(D.Stub(), meas, operator, CHAIN_SHAPE, label=y, seed=11)
    assert torch.is_tensor(alone) and same_bits(alone, got)


def test_gpu_refusals(vd):
    shape = CHAIN_SHAPE
    gd = D.make_gd(vd, 2)
    meas = torch.zeros((2, 1, 8, 8), device=DEV)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_ddnm(D.Stub(), meas, ("gray",), shape, device="cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_ddnm(D.Stub(), meas.cpu(), ("gray",), shape)
    with pytest.raises(ValueError, match="measurement"):
        gd.p_sample_ddnm(D.Stub(), meas, ("down", 2), shape)
    with pytest.raises(ValueError, match="use_ddim"):
        gd.p_sample_ddnm(D.Stub(), meas, ("gray",), shape, sigma_y=0.1, use_ddim=True)
    with pytest.raises(ValueError, match="lam"):
        gd.p_sample_ddnm(D.Stub(), meas, ("gray",), shape, lam=[1.0])
    x = gd.p_sample_ddnm(D.Stub(), meas, ("gray",), shape, seed=1)                             # and after the refusals it runs
    assert bool(torch.isfinite(x).all())
