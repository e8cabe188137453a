"""Learned variances on the GPU: vd_bpd_terms_lv / vd_bpd_bwd_lv, vd_hybrid_loss_fwd / _bwd and vd_sample_step_lv through the C ABI
against tests/learned_ref.py in fp64 (its fp32 evaluation is the natural-noise yardstick, the Sweep rule and the floors of
test_diffusion_kernels_gpu.py), and train_loss / HotPathTrainer / calc_all_bpd / p_sample around a small UNet with Cp + C output
channels.  Need an MI355X."""
import math

import pytest
import torch

import learned_ref as lref
from test_diffusion_kernels_gpu import (BIG, DEV, SIZES, H, StubNet, Sweep, clip_is_decisive, close, cosine, guarded, rnd,       # noqa: F401
                                        rows_close, t_passes)

pytestmark = pytest.mark.gpu

MOT_CLIP = [(mot, clip) for mot in ("v", "both", "eps") for clip in (False, True)]
FL_KL, FL_NLL, FL_PRED, FL_MSE, FL_GRAD = 2e-5, 1e-4, 2e-6, 1e-5, 2e-5
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def make_gd(T, mot, loss="kl", w_guide=0.0, rw="snr_trunc", **kw):
    import v_diffusion as vd
    return vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T, mot, "learned", rw, loss, w_guide=w_guide, p_uncond=0.0, **kw)


def cp_of(mot, C):
    return C * (2 if mot == "both" else 1)


def saturate(nu):
    """nu = 3 * N(0, 1) with the last two rows at +12 and -12, where the sigmoid saturates"""
    nu = nu * 3.0
    nu[-2], nu[-1] = 12.0, -12.0
    return nu


def lv_inputs(mot, size, s, t, seed):
    """bpd_inputs of test_diffusion_kernels_gpu.py with Cp + C output channels"""
    from oracle import diffusion_ref as dref
    n, Cc, Hh, Ww = size
    x0 = (rnd(n, Cc, Hh, Ww, seed=seed + 1).clamp(-1, 1) * 127.5).round() / 127.5
    x0[0, :, :2], x0[1, :, :2] = 1.0, -1.0                    # the cut-off branches of the discretised likelihood
    eps = rnd(n, Cc, Hh, Ww, seed=seed + 2)
    ls, lt = cosine()(s).float().reshape(-1, 1, 1, 1), cosine()(t).float().reshape(-1, 1, 1, 1)
    xt = dref.q_sample(x0, lt, eps)
    out = torch.cat([rnd(n, cp_of(mot, Cc), Hh, Ww, seed=seed + 3) * 0.7, saturate(rnd(n, Cc, Hh, Ww, seed=seed + 5))], dim=1)
    return x0, eps, xt, out, ls, lt, rnd(n, seed=seed + 4)


def lv_reference(mot, clip, x0, xt, out, ls, lt, dt, use_kl=None, gl=None):
    """(kl, nll, x0_hat, unclipped x0_hat, d sum(gl * where(use_kl, kl, nll)) / d out) of learned_ref in dtype dt"""
    from oracle import diffusion_ref as dref
    o = out.detach().to(dt, copy=True).requires_grad_(gl is not None)
    kl, nll, px0, _ = lref.terms(o, x0.to(dt), xt.to(dt), ls, lt, mot, clip)
    raw = dref.predictions(mot, xt.to(dt), lref.split(o, mot)[0], lt.to(dt))[0]
    grad = None
    if gl is not None:
        grad, = torch.autograd.grad((torch.where(use_kl, kl, nll) * gl.to(dt)).sum(), o)
    return kl.detach(), nll.detach(), px0.detach(), raw.detach(), grad


def halves(t, mot, C):
    return t[:, :cp_of(mot, C)], t[:, cp_of(mot, C):]


def run_terms(H, gd, mot, clip, x0, xt, out, ls, lt, use_kl, gl, mean_grad=True):
    """both kernels on guarded outputs: (kl, nll, pred, mse, dout)"""
    n, Cc, Hh, Ww = x0.shape
    dv = lambda a: a.to(DEV)
    coef = gd._bpd_coefs(dv(ls), dv(lt))
    (kl, k1), (nll, k2), (mse, k3) = (guarded((n,)) for _ in range(3))
    pred, k4 = guarded(tuple(x0.shape))
    H.bpd_terms_lv(dv(x0), dv(xt), dv(out), coef, H.OUT_TYPES[mot], clip, kl, nll, pred, mse, n, Cc, Hh * Ww)
    dout, k5 = guarded(tuple(out.shape))
    H.bpd_bwd_lv(dv(x0), dv(xt), dv(out), coef, dv(use_kl.float()), dv(gl), H.OUT_TYPES[mot], clip, mean_grad, dout, n, Cc, Hh * Ww)
    torch.cuda.synchronize()
    assert k1() and k2() and k3() and k4() and k5(), "a learned-variance bound kernel wrote outside its outputs"
    return kl, nll, pred, mse, dout


def l2_rows(what, d, ref, rows, bound=3e-2):
    """decoder-NLL rows: each row against the fp32 autograd of the same expression in L2 (ill-conditioned in the reference itself:
    check_bpd_mid of test_diffusion_kernels_gpu.py); returns the worst figure"""
    worst = 0.0
    for r in rows:
        rel = (d[r].double() - ref[r].double()).norm().item() / max(ref[r].double().norm().item(), 1e-300)
        worst = max(worst, rel)
        assert rel <= bound, f"{what} row {r}: L2 {rel:.3e}"
    return worst


def check_lv_mid(H, sw, mot, clip, size, seed):
    n, Cc, Hh, Ww = size
    s = 0.3 + 0.1 * (torch.arange(n, dtype=torch.float64) % 6)              # the mid-chain variances of check_bpd_mid
    use_kl = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 1.0]).repeat((n + 5) // 6)[:n] != 0
    x0, _, xt, out, ls, lt, gl = lv_inputs(mot, size, s, s + 0.125, seed)
    kl64, nll64, p64, raw64, g64 = lv_reference(mot, clip, x0, xt, out, ls, lt, torch.float64, use_kl, gl)
    kl32, nll32, _, _, g32 = lv_reference(mot, clip, x0, xt, out, ls, lt, torch.float32, use_kl, gl)
    if clip:
        assert clip_is_decisive(raw64, use_kl) == (True, True), "clip case without both live and dead pixels"
    gd = make_gd(8, mot)
    kl, nll, pred, mse, dout = run_terms(H, gd, mot, clip, x0, xt, out, ls, lt, use_kl, gl)
    rows_close(sw, kl, kl64, kl32, floor=FL_KL, name="kl")
    rows_close(sw, nll, nll64, nll32, floor=FL_NLL, name="nll")
    rows_close(sw, pred, p64, None, floor=FL_PRED, name="pred")
    rows_close(sw, mse, ((p64 - x0.double()) ** 2).flatten(1).mean(1), None, floor=FL_MSE, name="mse")
    d = dout.cpu()
    (dp, dn), (gp64, gn64), (gp32, gn32) = halves(d, mot, Cc), halves(g64, mot, Cc), halves(g32, mot, Cc)
    klr, nlr = [r for r in range(n) if use_kl[r]], [r for r in range(n) if not use_kl[r]]
    for r in klr:
        sw.close(dp[r:r + 1], gp64[r:r + 1], gp32[r:r + 1], floor=FL_GRAD, name=f"d kl / d pred row {r}")
        sw.close(dn[r:r + 1], gn64[r:r + 1], gn32[r:r + 1], floor=FL_GRAD, name=f"d kl / d nu row {r}")
    wp, wn = l2_rows("d nll / d pred", dp, gp32, nlr), l2_rows("d nll / d nu", dn, gn32, nlr)
    print(f"[bpd_lv mid {mot} clip={clip} {size}] worst d nll row L2: prediction half {wp:.3e}, nu half {wn:.3e}")
    # the stop-gradient form: exact zeros on the prediction channels, the same nu bits
    d0 = run_terms(H, gd, mot, clip, x0, xt, out, ls, lt, use_kl, gl, mean_grad=False)[4].cpu()
    assert bool((d0[:, :cp_of(mot, Cc)] == 0).all()), "mean_grad = 0 left a prediction-channel gradient"
    assert torch.equal(d0[:, cp_of(mot, Cc):], dn), "the nu gradient depends on mean_grad"
    assert bool(dn[klr].abs().max() > 0) and bool(dp[klr].abs().max() > 0)


@pytest.mark.parametrize("size", SIZES, ids=ids)
@pytest.mark.parametrize("mot,clip", MOT_CLIP)
def test_bpd_lv_mid_chain(H, mot, clip, size):
    """KL, decoder NLL, x0_hat, its squared error and both halves of both gradients at the mid-chain variances of check_bpd_mid; the
    decoder-NLL gradient (ill-conditioned in the reference: fp32 against fp64 autograd differs by 0.33 / 0.61 in row L2 for the
    prediction / nu half) against the fp32 autograd of the same expression in row L2 under 3e-2, both halves"""
    sw = Sweep(f"bpd_lv mid {mot} clip={clip} {size}")
    check_lv_mid(H, sw, mot, clip, size, seed=620)
    sw.done()


def test_bpd_lv_grid_wraps(H):
    """(no clip at this size: among 1.5 million pixels some x0_hat always lies within rounding of the clip bound)"""
    sw = Sweep(f"bpd_lv mid both {BIG}")
    check_lv_mid(H, sw, "both", False, BIG, seed=700)
    sw.done()


@pytest.mark.parametrize("size", SIZES, ids=ids)
@pytest.mark.parametrize("mot,clip", MOT_CLIP)
def test_bpd_lv_schedule_ends(H, mot, clip, size):
    """per-row logsnr_t from +20 to -20 and s = max(t - 1/8, 0): as test_bpd_terms_schedule_ends, KL and its gradient (both halves) on
    the rows with s != 0, x0_hat and its squared error on every row, the fp32 oracle's own error the yardstick"""
    n, Cc, Hh, Ww = size
    sw = Sweep(f"bpd_lv ends {mot} clip={clip} {size}")
    gd = make_gd(8, mot)
    dead = live = False
    for p, t in enumerate(t_passes(n)):
        s = (t - 0.125).clamp(min=0.0)
        use_kl = s != 0
        x0, _, xt, out, ls, lt, gl = lv_inputs(mot, size, s, t, seed=800 + 10 * p)
        kl64, _, p64, raw64, g64 = lv_reference(mot, clip, x0, xt, out, ls, lt, torch.float64, use_kl, gl)
        kl32, _, p32, _, g32 = lv_reference(mot, clip, x0, xt, out, ls, lt, torch.float32, use_kl, gl)
        if clip:
            dead, live = (a or b for a, b in zip((dead, live), clip_is_decisive(raw64, use_kl)))
        kl, _, pred, mse, dout = run_terms(H, gd, mot, clip, x0, xt, out, ls, lt, use_kl, gl)
        tag = f"pass {p}"
        rows_close(sw, pred, p64, p32, floor=FL_PRED, name=f"pred {tag}")
        rows_close(sw, mse, ((p64 - x0.double()) ** 2).flatten(1).mean(1), ((p32 - x0) ** 2).flatten(1).mean(1), floor=FL_MSE, name=f"mse {tag}")
        d = dout.cpu()
        (dp, dn), (gp64, gn64), (gp32, gn32) = halves(d, mot, Cc), halves(g64, mot, Cc), halves(g32, mot, Cc)
        for r in range(n):
            if use_kl[r]:
                sw.close(kl[r:r + 1], kl64[r:r + 1], kl32[r:r + 1], floor=FL_KL, name=f"kl {tag} row {r}")
                sw.close(dp[r:r + 1], gp64[r:r + 1], gp32[r:r + 1], floor=FL_GRAD, name=f"d kl / d pred {tag} row {r}")
                sw.close(dn[r:r + 1], gn64[r:r + 1], gn32[r:r + 1], floor=FL_GRAD, name=f"d kl / d nu {tag} row {r}")
    assert not clip or (dead and live), "clip case without both live and dead pixels in the rows whose gradient is compared"
    sw.done()


def test_decoder_well_conditioned(H):
    """the decoder NLL and its gradient where fp64 is a fair yardstick: T = 8, the s = 0 row (lvmin = -20, delta = 16.73), nu such that
    the model sigma lies in [1/255, 4/255] (frac in [0.53, 0.70]) and a v-output with x0_hat - x0 ~ N(0, (2/255)^2).  On these inputs
    the fp32 reference is within 1.6e-4 (NLL) and 6e-5 / 1.4e-4 (gradient, L2 / max-norm) of fp64, finite everywhere; ordinary rule."""
    from oracle import diffusion_ref as dref
    size = n, Cc, Hh, Ww = (4, 3, 33, 17)
    s, t = torch.zeros(n, dtype=torch.float64), torch.full((n,), 0.125, dtype=torch.float64)
    x0, _, xt, out, ls, lt, gl = lv_inputs("v", size, s, t, seed=900)
    _, _, lvmin, delta = lref.lv_coefs(ls, lt)
    assert float(lvmin[0]) == pytest.approx(-20.0, abs=1e-3) and float(delta[0]) == pytest.approx(16.73, abs=5e-3)
    u = torch.rand(size, generator=torch.Generator().manual_seed(901), dtype=torch.float64)
    lv = 2.0 * torch.log((1.0 + 3.0 * u) / 255.0)
    frac = (lv - lvmin.double()) / delta.double()
    assert 0.53 <= float(frac.min()) and float(frac.max()) <= 0.70
    a, sg = dref.alpha_sigma(lt.double())
    v = (a * xt.double() - (x0.double() + rnd(*size, seed=902, dtype=torch.float64) * (2.0 / 255.0))) / sg
    out = torch.cat([v, torch.logit(frac)], dim=1).float()
    use_kl = torch.zeros(n, dtype=torch.bool)
    _, nll64, _, _, g64 = lv_reference("v", False, x0, xt, out, ls, lt, torch.float64, use_kl, gl)
    _, nll32, _, _, g32 = lv_reference("v", False, x0, xt, out, ls, lt, torch.float32, use_kl, gl)
    assert bool(torch.isfinite(g32).all()) and bool(torch.isfinite(g64).all())
    _, nll, _, _, dout = run_terms(H, make_gd(8, "v"), "v", False, x0, xt, out, ls, lt, use_kl, gl)
    sw = Sweep("decoder, well conditioned")
    rows_close(sw, nll, nll64, nll32, floor=FL_NLL, name="nll")
    d = dout.cpu()
    for name, (a_, b_, c_) in (("pred", (d[:, :3], g64[:, :3], g32[:, :3])), ("nu", (d[:, 3:], g64[:, 3:], g32[:, 3:]))):
        rows_close(sw, a_, b_, c_, floor=FL_GRAD, name=f"d nll / d {name}")
        print(f"[decoder, well conditioned] d nll / d {name}: max err {float((a_.double() - b_).abs().max()):.3e} on scale {float(b_.abs().max()):.3e}")
    sw.done()


# ================================================================================================ hybrid loss
HYBRID_PAIRS = [("v", "snr_trunc"), ("v", "snr_1plus"), ("v", "constant"), ("v", "snr"), ("both", "snr_trunc"), ("eps", "snr_trunc"),
                ("eps", "snr")]


def run_hybrid(H, gd, mot, rw, vlb, x0, eps, xt, out, ls, lt, use_kl, gl):
    n, Cc, Hh, Ww = x0.shape
    dv = lambda a: a.to(DEV)
    coef = gd._bpd_coefs(dv(ls), dv(lt))
    l32 = dv(lt.reshape(-1).contiguous())
    (loss, k1), (aux, k2), (dout, k3) = guarded((n,)), guarded((n, 4)), guarded(tuple(out.shape))
    args = (dv(x0), dv(eps), dv(xt), dv(out), l32, coef, dv(use_kl.float()))
    H.hybrid_loss_fwd(*args, H.OUT_TYPES[mot], H.REWEIGHTS[rw], vlb, loss, aux, n, Cc, Hh * Ww)
    H.hybrid_loss_bwd(*args, aux, dv(gl), H.OUT_TYPES[mot], H.REWEIGHTS[rw], vlb, dout, n, Cc, Hh * Ww)
    torch.cuda.synchronize()
    assert k1() and k2() and k3(), "a hybrid kernel wrote outside its outputs"
    return loss, aux, dout


def check_hybrid(H, sw, mot, rw, size, seed, vlb=0.05):
    n, Cc, Hh, Ww = size
    s = 0.3 + 0.1 * (torch.arange(n, dtype=torch.float64) % 6)
    use_kl = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 1.0]).repeat((n + 5) // 6)[:n] != 0
    x0, eps, xt, out, ls, lt, gl = lv_inputs(mot, size, s, s + 0.125, seed)
    ref = {}
    for dt in (torch.float64, torch.float32):
        o = out.to(dt, copy=True).requires_grad_(True)
        lo = lref.hybrid_loss(o, x0.to(dt), eps.to(dt), xt.to(dt), ls, lt, use_kl, mot, rw, vlb)
        g, = torch.autograd.grad((lo * gl.to(dt)).sum(), o)
        ref[dt] = (lo.detach(), g)
    gd = make_gd(8, mot, "hybrid", rw=rw)
    loss, aux, dout = run_hybrid(H, gd, mot, rw, vlb, x0, eps, xt, out, ls, lt, use_kl, gl)
    rows_close(sw, loss, ref[torch.float64][0], ref[torch.float32][0], floor=FL_MSE, name="loss")
    d = dout.cpu()
    (dp, dn), (gp64, gn64), (gp32, gn32) = (halves(a, mot, Cc) for a in (d, ref[torch.float64][1], ref[torch.float32][1]))
    rows_close(sw, dp, gp64, gp32, floor=FL_GRAD, name="d loss / d pred")
    klr, nlr = [r for r in range(n) if use_kl[r]], [r for r in range(n) if not use_kl[r]]
    for r in klr:
        sw.close(dn[r:r + 1], gn64[r:r + 1], gn32[r:r + 1], floor=FL_GRAD, name=f"d loss / d nu row {r}")
    worst = l2_rows("d loss / d nu (decoder rows)", dn, gn32, nlr)
    print(f"[hybrid {mot}/{rw} {size}] decoder rows, nu half against fp32 autograd: worst row L2 {worst:.3e}")
    # the bound terms in aux are the lv kernel's
    kl64, nll64, _, _, _ = lv_reference(mot, False, x0, xt, out, ls, lt, torch.float64)
    kl32, nll32, _, _, _ = lv_reference(mot, False, x0, xt, out, ls, lt, torch.float32)
    rows_close(sw, aux[:, 2], kl64, kl32, floor=FL_KL, name="aux kl")
    rows_close(sw, aux[:, 3], nll64, nll32, floor=FL_NLL, name="aux nll")
    return gd, (x0, eps, xt, out, ls, lt, use_kl, gl), d


@pytest.mark.parametrize("size", SIZES, ids=ids)
@pytest.mark.parametrize("mot,rw", HYBRID_PAIRS)
def test_hybrid_loss_and_gradient(H, mot, rw, size):
    """loss and the whole Cp + C gradient against the fp64 autograd of learned_ref.hybrid_loss (mean detached in the bound term), every
    reweight; then the stop-gradient without tolerances: calls that differ only in nu, vlb_weight and use_kl give bitwise the same
    prediction-channel gradient, and vlb_weight = 0 a nu gradient of exact zeros"""
    n, Cc = size[:2]
    sw = Sweep(f"hybrid {mot}/{rw} {size}")
    gd, (x0, eps, xt, out, ls, lt, use_kl, gl), d = check_hybrid(H, sw, mot, rw, size, seed=1000)
    sw.done()
    Cp = cp_of(mot, Cc)
    out2 = out.clone()
    out2[:, Cp:] = saturate(rnd(*x0.shape, seed=1234)).flip(0)
    _, _, d2 = run_hybrid(H, gd, mot, rw, 0.7, x0, eps, xt, out2, ls, lt, ~use_kl, gl)
    assert torch.equal(d2.cpu()[:, :Cp], d[:, :Cp]), "the prediction-channel gradient depends on nu, vlb_weight or use_kl"
    assert not torch.equal(d2.cpu()[:, Cp:], d[:, Cp:])
    _, _, d3 = run_hybrid(H, gd, mot, rw, 0.0, x0, eps, xt, out, ls, lt, use_kl, gl)
    assert bool((d3.cpu()[:, Cp:] == 0).all()) and torch.equal(d3.cpu()[:, :Cp], d[:, :Cp])
    # the mse part is vd_loss_fwd / vd_loss_bwd on the prediction channels copied out
    dv = lambda a: a.to(DEV)
    l32, pc = dv(lt.reshape(-1).contiguous()), dv(out[:, :Cp].contiguous())
    loss0, aux0, dl0 = torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV), torch.empty_like(pc)
    H.loss_fwd(dv(x0), dv(eps), dv(xt), pc, l32, H.OUT_TYPES[mot], H.REWEIGHTS[rw], loss0, aux0, n, Cc, x0[0, 0].numel())
    H.loss_bwd(dv(x0), dv(eps), dv(xt), pc, l32, aux0, dv(gl), H.OUT_TYPES[mot], H.REWEIGHTS[rw], dl0, n, Cc, x0[0, 0].numel())
    close(d[:, :Cp], dl0.cpu().double(), None, floor=1e-6, name="prediction channels against vd_loss_bwd")


def test_hybrid_grid_wraps(H):
    sw = Sweep(f"hybrid both/snr_trunc {BIG}")
    check_hybrid(H, sw, "both", "snr_trunc", BIG, seed=1100)
    sw.done()


# ================================================================================================ reverse step
def lv_step_inputs(shape, mot, cfg, step, T, seed=0):
    from oracle import diffusion_ref as dref
    B, C, Hh, Ww = shape
    x0, eps = rnd(B, C, Hh, Ww, seed=seed + 1).clamp(-1, 1), rnd(B, C, Hh, Ww, seed=seed + 2)
    lt = cosine()(torch.full((B,), (step + 1) / T, dtype=torch.float64)).float().reshape(-1, 1, 1, 1)
    xt = dref.q_sample(x0, lt, eps)
    rows = B * (1 + cfg)
    out = torch.cat([rnd(rows, cp_of(mot, C), Hh, Ww, seed=seed + 3 + cfg) * 0.8, saturate(rnd(rows, C, Hh, Ww, seed=seed + 7))], dim=1)
    y = torch.arange(1, B + 1, dtype=torch.float32) if cfg else None
    return xt, out, rnd(B, C, Hh, Ww, seed=seed + 5), y


def run_lv_step(H, gd, xt_d, out_d, noise_d, mot, cfg, step, use_ddim, clip, shape, xn=None, xdup=None):
    B, C, Hh, Ww = shape
    k10, _ = gd._step_coefs(step, use_ddim, clip)
    xn = torch.empty(shape, device=DEV) if xn is None else xn
    H.sample_step_lv(xt_d, out_d, None if use_ddim else noise_d, k10, H.OUT_TYPES[mot], cfg, step == 0, clip, xn, xdup, B, C, Hh * Ww)
    return xn


def misaligned(t):
    """a copy of t that starts 4 bytes past a 16-byte boundary: the scalar form of a kernel that picks its form by alignment"""
    buf = torch.empty(t.numel() + 1, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("shape", [(5, 3, 8, 8), (3, 3, 33, 17), (2, 1, 5, 3)], ids=ids)
@pytest.mark.parametrize("mot", ["v", "both", "eps"])
def test_sample_step_lv_vs_ref(H, mot, shape):
    """vd_sample_step_lv with the 10 coefficients of _step_coefs against learned_ref.p_sample_step in fp64 over {guidance off, w = 1.5}
    x steps {0, 1, T/2, T-1} x T {8, 1000} x {DDPM, DDIM} x {clip off, on}; where the wide form runs (C*HW % 4 == 0) the scalar form,
    reached through a misaligned state, gives the same bits; without noise the result is vd_sample_step's on the prediction channels"""
    B, C, Hh, Ww = shape
    sw = Sweep(f"sample_step_lv {mot} {shape}")
    for cfg in (0, 1):
        w = 1.5 if cfg else 0.0
        for T in (8, 1000):
            gd = make_gd(T, mot, w_guide=w)
            for step in (0, 1, T // 2, T - 1):
                xt, out, noise, y = lv_step_inputs(shape, mot, cfg, step, T)
                xt_d, out_d, noise_d = xt.to(DEV), out.to(DEV), noise.to(DEV)
                for use_ddim in (False, True):
                    for clip in (False, True):
                        kw = dict(model_out_type=mot, w_guide=w, use_ddim=use_ddim, clip=clip)
                        ref = {dt: lref.p_sample_step(lambda *_: out.to(dt), cosine(), xt.to(dt), step, T, y, noise.to(dt), **kw)
                               for dt in (torch.float64, torch.float32)}
                        xn, ok = guarded(shape)
                        xdup, dup_ok = guarded((2 * B, C, Hh, Ww)) if cfg else (None, lambda: True)
                        run_lv_step(H, gd, xt_d, out_d, noise_d, mot, cfg, step, use_ddim, clip, shape, xn=xn, xdup=xdup)
                        torch.cuda.synchronize()
                        assert ok() and dup_ok(), "sample_step_lv wrote outside its outputs"
                        name = f"cfg={cfg} T={T} step={step} ddim={use_ddim} clip={clip}"
                        sw.close(xn, ref[torch.float64], ref[torch.float32], name=name)
                        if cfg:
                            assert torch.equal(xdup[0::2], xn) and torch.equal(xdup[1::2], xn)
                        if (C * Hh * Ww) % 4 == 0 and clip:
                            assert xt_d.data_ptr() % 16 == 0 and out_d.data_ptr() % 16 == 0 and noise_d.data_ptr() % 16 == 0
                            wide = run_lv_step(H, gd, xt_d, out_d, noise_d, mot, cfg, step, use_ddim, clip, shape)
                            scalar = run_lv_step(H, gd, misaligned(xt_d), out_d, noise_d, mot, cfg, step, use_ddim, clip, shape)
                            assert wide.data_ptr() % 16 == 0 and torch.equal(wide, scalar) and torch.equal(wide, xn), f"wide != scalar: {name}"
                # noise = None: vd_sample_step on the prediction channels copied to a contiguous tensor, bit for bit
                k10, _ = gd._step_coefs(step, False)
                k8 = list(k10[:8])
                k8[5] = 0.0
                Cp = cp_of(mot, C)
                a, b = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
                H.sample_step_lv(xt_d, out_d, None, k10, H.OUT_TYPES[mot], cfg, step == 0, True, a, None, B, C, Hh * Ww)
                H.sample_step(xt_d, out_d[:, :Cp].contiguous(), None, k8, H.OUT_TYPES[mot], cfg, step == 0, True, b, None, B, C, Hh * Ww)
                assert torch.equal(a, b), f"noise=None differs from vd_sample_step: cfg={cfg} T={T} step={step}"
    sw.done()


def test_sample_step_lv_grid_wraps_and_refusals(H):
    shape, mot, cfg = (128, 3, 64, 64), "both", 1
    B, C, Hh, Ww = shape
    gd = make_gd(1000, mot, w_guide=1.5)
    xt, out, noise, y = lv_step_inputs(shape, mot, cfg, 500, 1000)
    ref = {dt: lref.p_sample_step(lambda *_: out.to(dt), cosine(), xt.to(dt), 500, 1000, y, noise.to(dt), model_out_type=mot, w_guide=1.5)
           for dt in (torch.float64, torch.float32)}
    x, x_ok = guarded(shape)
    xdup, dup_ok = guarded((2 * B, C, Hh, Ww))
    x.copy_(xt)
    run_lv_step(H, gd, x, out.to(DEV), noise.to(DEV), mot, cfg, 500, False, True, shape, xn=x, xdup=xdup)      # in place, as a chain may
    close(x, ref[torch.float64], ref[torch.float32], name="128x3x64x64 in place")
    assert torch.equal(xdup[0::2], x) and torch.equal(xdup[1::2], x) and x_ok() and dup_ok()
    k10, _ = gd._step_coefs(500, False)
    small = torch.zeros((2, 3, 4, 4), device=DEV)
    for bad in (lambda: H.sample_step_lv(small, torch.zeros((2, 9, 4, 4), device=DEV), None, k10, 7, 0, False, True, small.clone(), None, 2, 3, 16),
                lambda: H.sample_step_lv(small, torch.zeros((2, 9, 4, 4), device=DEV), None, k10, 3, 0, False, True, small.clone(), small.clone(), 2, 3, 16),
                lambda: H.bpd_terms_lv(small, small, torch.zeros((2, 6, 4, 4), device=DEV), None, 0, False, small, small, None, None, 2, 3, 16),
                lambda: H.hybrid_loss_fwd(small, small, small, torch.zeros((2, 9, 4, 4), device=DEV), small, small, small, 3, 0, 0.1, small, small, 2, 3, 16)):
        with pytest.raises(H.HipError):
            bad()


# ================================================================================================ network level
@pytest.fixture(scope="module")
def net6():
    """tinyA with out_channels = 6 (v-prediction + variance channels) and the deterministic weights of the oracle"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return build6()


def build6():
    import v_diffusion as vd
    from oracle.cases import TINY, make_weights
    cfg = dict(TINY["tinyA"]["cfg"], out_channels=6)
    m = vd.UNet(**cfg)
    m.load_state_dict(make_weights(cfg), strict=True)
    return m.to(DEV)


def case6(seed=3):
    from oracle import detrand
    from oracle.cases import TINY, make_inputs
    case = TINY["tinyA"]
    x0, t, y = make_inputs(case["cfg"], 3, case["R"], case["label"], seed=seed)
    x0 = (x0.clamp(-1, 1) * 127.5).round() / 127.5
    t[0] = 0.05                                                   # snaps to 1/T: the decoder row
    return x0, t, y.clamp(min=1), detrand.normal("noise", tuple(x0.shape), seed)


@pytest.mark.parametrize("loss_type", ["hybrid", "kl"])
def test_train_loss_on_the_networks_own_output(H, net6, loss_type):
    """train_loss and d loss / d out (captured with a hook) against learned_ref on the output the network gave"""
    from oracle import diffusion_ref as dref
    T = 8
    gd = make_gd(T, "v", loss_type)
    assert gd.vlb_weight == 0.008
    net6.train()
    x0, t, y, noise = case6()
    seen = {}

    def den(x, tt, yy):
        o = net6(x, tt, yy)
        seen["x"], seen["t"], seen["out"] = x.detach().cpu(), tt.detach().cpu(), o.detach().cpu()
        o.register_hook(lambda g: seen.__setitem__("grad", g.detach().cpu()))
        return o
    gl = torch.tensor([0.5, -1.25, 2.0])
    loss = gd.train_loss(den, x0.to(DEV), t.to(DEV), y.to(DEV), noise.to(DEV))
    (loss * gl.to(DEV)).sum().backward()
    tg = torch.ceil(t * T) / T
    s = (tg - 1.0 / T).clamp(min=0.0)
    assert torch.equal(seen["t"], tg) and float(s[0]) == 0.0 and bool((s[1:] > 0).all()) and seen["out"].shape[1] == 6
    ls, lt = cosine()(s).float().reshape(-1, 1, 1, 1), cosine()(tg).float().reshape(-1, 1, 1, 1)
    ref = {}
    for dt in (torch.float64, torch.float32):
        o = seen["out"].to(dt, copy=True).requires_grad_(True)
        xt = dref.q_sample(x0.to(dt), lt.to(dt), noise.to(dt))
        if loss_type == "hybrid":
            lo = lref.hybrid_loss(o, x0.to(dt), noise.to(dt), xt, ls, lt, s != 0, "v", "snr_trunc", gd.vlb_weight)
        else:
            kl, nll, _, _ = lref.terms(o, x0.to(dt), xt, ls, lt, "v")
            lo = torch.where(s != 0, kl, nll)
        g, = torch.autograd.grad((lo * gl.to(dt)).sum(), o)
        ref[dt] = (lo.detach(), g)
    sw = Sweep(f"train_loss {loss_type}")
    close(seen["x"], dref.q_sample(x0.double(), lt.double(), noise.double()), None, floor=1e-6, name="x_t")
    rows_close(sw, loss.detach(), ref[torch.float64][0], ref[torch.float32][0], floor=FL_KL if loss_type == "kl" else FL_MSE, name="loss")
    d, g64, g32 = seen["grad"], ref[torch.float64][1], ref[torch.float32][1]
    for r in (1, 2):                                              # KL rows
        sw.close(d[r:r + 1, :3], g64[r:r + 1, :3], g32[r:r + 1, :3], floor=FL_GRAD, name=f"d loss / d pred row {r}")
        sw.close(d[r:r + 1, 3:], g64[r:r + 1, 3:], g32[r:r + 1, 3:], floor=FL_GRAD, name=f"d loss / d nu row {r}")
    if loss_type == "hybrid":                                     # decoder row: the prediction half is the mse gradient alone
        sw.close(d[0:1, :3], g64[0:1, :3], g32[0:1, :3], floor=FL_GRAD, name="d loss / d pred row 0")
        l2_rows("d loss / d nu", d[:, 3:], g32[:, 3:], [0])
    else:
        l2_rows("d loss / d out", d, g32, [0])
    sw.done()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net6.parameters())
    net6.zero_grad(set_to_none=True)


def test_train_loss_rules(H, net6):
    """the channel check comes before any launch; "mse" keeps its assert; the label drop of the mse branch applies to "hybrid" only"""
    import v_diffusion as vd
    x0, t, y, noise = case6()
    args = (x0.to(DEV), t.to(DEV), y.to(DEV), noise.to(DEV))
    three = lambda x, tt, yy: x * 1.0
    for loss_type in ("hybrid", "kl"):
        with pytest.raises(RuntimeError, match="3 \\+ 3 channels"):
            make_gd(8, "v", loss_type).train_loss(three, *args)
    with pytest.raises(RuntimeError, match="6 \\+ 3 channels"):
        make_gd(8, "both", "hybrid").train_loss(net6, *args)
    with pytest.raises(RuntimeError, match="3 \\+ 3 channels"):
        make_gd(8, "v").calc_all_bpd(three, x0.to(DEV), y.to(DEV))
    with pytest.raises(RuntimeError, match="3 \\+ 3 channels"):
        make_gd(8, "v").p_sample(three, (2, 3, 8, 8), device=DEV, seed=1)
    with pytest.raises(AssertionError):
        make_gd(8, "v", "mse").train_loss(net6, *args)
    with pytest.raises(NotImplementedError, match="use_graph"):
        make_gd(8, "v").p_sample(net6, (2, 3, 16, 16), device=DEV, seed=1, use_graph=True)
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    net6.eval()
    for loss_type, dropped in (("hybrid", True), ("kl", False)):
        gd = vd.GaussianDiffusion(fn, 8, "v", "learned", "snr_trunc", loss_type, p_uncond=1.0)
        yy = y.to(DEV).clone()
        with torch.no_grad():
            gd.train_loss(net6, x0.to(DEV), t.to(DEV), yy, noise.to(DEV))
        assert bool((yy == 0).all()) == dropped


def test_hot_path_trainer_step(H, net6):
    """HotPathTrainer takes such a diffusion unchanged: one step runs, the loss is finite and the parameters move"""
    from v_diffusion.trainer import HotPathTrainer
    model = build6().train()                                      # a model of its own: the step changes the weights
    tr = HotPathTrainer(model, make_gd(8, "v", "hybrid"), lr=1e-3, warmup=0, timesteps=8)
    before = [p.detach().clone() for p in model.parameters()]
    x0, _, y, _ = case6()
    loss = tr.step(x0.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    moved = [not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters())]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters()) and sum(moved) >= len(moved) - 2
    last = dict(model.named_parameters())
    out_w = [k for k in last if last[k].shape[:1] == (6,)]
    assert out_w and all(not torch.equal(last[k].detach(), dict(net6.named_parameters())[k].detach()) for k in out_w), "the output layer did not move"


def test_calc_all_bpd_columns(H, net6):
    """T = 4, fixed generator: every column is learned_ref's term on the replayed draws and the network's own output"""
    from oracle import diffusion_ref as dref
    T = 4
    gd = make_gd(T, "v")
    net6.eval()
    x0, _, y, _ = case6()
    outs = []

    def den(x, tt, yy):
        o = net6(x, tt, yy)
        outs.append(o.detach().cpu())
        return o
    with torch.no_grad():
        total, terms, prior, mse = gd.calc_all_bpd(den, x0.to(DEV), y.to(DEV), clip_denoised=True, generator=torch.Generator(DEV).manual_seed(5))
    g = torch.Generator(DEV).manual_seed(5)
    draws = [torch.empty(x0.shape, device=DEV).normal_(generator=g).cpu() for _ in range(T)]            # steps T-1 ... 0
    assert terms.shape == (3, T) and mse.shape == (3, T) and bool(torch.isfinite(total).all())
    sw = Sweep("calc_all_bpd")
    for j, i in enumerate(range(T - 1, -1, -1)):
        ls = cosine()(torch.full((3,), i / T, dtype=torch.float64)).float().reshape(-1, 1, 1, 1)
        lt = cosine()(torch.full((3,), (i + 1) / T, dtype=torch.float64)).float().reshape(-1, 1, 1, 1)
        ref = {}
        for dt in (torch.float64, torch.float32):
            xt = dref.q_sample(x0.to(dt), lt.to(dt), draws[j].to(dt))
            kl, nll, px0, _ = lref.terms(outs[j].to(dt), x0.to(dt), xt, ls, lt, "v", clip=True)
            ref[dt] = (kl if i > 0 else nll, ((px0 - x0.to(dt)) ** 2).flatten(1).mean(1))
        rows_close(sw, terms[:, i], ref[torch.float64][0], ref[torch.float32][0], floor=FL_KL if i > 0 else FL_NLL, name=f"term {i}")
        rows_close(sw, mse[:, i], ref[torch.float64][1], ref[torch.float32][1], floor=FL_MSE, name=f"mse {i}")
    sw.done()
    close(total, (terms.sum(1) + prior).cpu().double(), None, floor=1e-6, name="total")


@pytest.mark.parametrize("labels", [False, True], ids=["nolabel", "guided"])
@pytest.mark.parametrize("use_ddim", [False, True], ids=["ancestral", "ddim"])
def test_p_sample_replays_the_draw_stream(H, net6, use_ddim, labels):
    """p_sample(seed=...) equals a step-by-step replay of its documented draw stream -- x_T, then one image-shaped draw per step from
    the same generator, also for DDIM -- through learned_ref.p_sample_step around the same network (1e-4 absolute, the bound of the
    T = 8 chain tests of test_unet_gpu.py), reproduces bit for bit, and p_sample_progressive returns the guided x0 prediction"""
    T, shape, w = 8, (3, 3, 16, 16), 1.0
    gd = make_gd(T, "v", w_guide=w)
    net6.eval()
    y = torch.tensor([1.0, 7.0, 10.0]) if labels else None
    a = gd.p_sample(net6, shape, label=y, device=DEV, seed=11, use_ddim=use_ddim)
    b = gd.p_sample(net6, shape, label=y, device=DEV, seed=11, use_ddim=use_ddim)
    assert a.device.type == "cpu" and torch.equal(a, b) and bool(torch.isfinite(a).all())
    g = torch.Generator(DEV).manual_seed(11)
    x = torch.randn(shape, device=DEV, generator=g).cpu()
    draws = [torch.empty(shape, device=DEV).normal_(generator=g).cpu() for _ in range(T)]
    with torch.no_grad():
        den = lambda xx, tt, yy: net6(xx.float().to(DEV), tt.to(DEV), None if yy is None else yy.to(DEV)).cpu()
        preds = []
        for j, step in enumerate(reversed(range(T))):
            x, p = lref.p_sample_step(den, cosine(), x, step, T, y, draws[j], model_out_type="v", w_guide=w, use_ddim=use_ddim, clip=True,
                                      return_pred=True)
            preds.append(p)
    err = float((a - x).abs().max())
    print(f"[p_sample learned ddim={use_ddim} labels={labels}] end of chain differs by {err:.3e}")
    assert err <= 1e-4
    c, pr = gd.p_sample_progressive(net6, shape, label=y, device=DEV, seed=11, use_ddim=use_ddim, pred_freq=1)
    assert torch.equal(c, a) and pr.shape == (T,) + shape
    for j, step in enumerate(reversed(range(T))):
        assert float((pr[step] - preds[j]).abs().max()) <= 1e-4, f"x0 prediction of step {step}"
    if not use_ddim:
        d = gd.p_sample(net6, shape, label=y, device=DEV, seed=11, use_ddim=True)
        assert not torch.equal(d, a)
    u8 = gd.p_sample_uint8_async(net6, shape, label=y, device=DEV, seed=11, use_ddim=use_ddim).tensor()
    want = (a * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    assert int((u8.to(torch.int16) - want.to(torch.int16)).abs().max()) <= 1                      # (round-to-nearest vs truncation at .5 ties)
    # the (B,) step tensor API: uniform steps take the fused kernel, mixed steps the tensor composition; same numbers
    xt = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    yd = None if y is None else y.to(DEV)
    gen = lambda: torch.Generator(DEV).manual_seed(4)
    with torch.no_grad():
        u = gd.p_sample_step(net6, xt, torch.full((3,), 5, device=DEV), yd, generator=gen(), use_ddim=use_ddim)
        m = gd.p_sample_step(net6, xt, torch.tensor([5, 5, 0], device=DEV), yd, generator=gen(), use_ddim=use_ddim)
    assert float((u[:2] - m[:2]).abs().max()) <= 1e-4 and bool(torch.isfinite(m).all())
