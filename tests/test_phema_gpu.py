"""Post-hoc EMA on the device: vd_adamw_emas against the entries it extends (bit for bit) and against the fp64 recurrence of
tests/phema_ref.py, vd_ema_combine against exact sums, and the trainer / optim.PowerEMA / posthoc_ema paths built on them.

Bounds.  One shadow step e' = e + r (p' - e) rounds the subtraction, the product and the sum: |e' - e'_64| <= (2u + u^2) r |p' - e| + u |e'_64|,
u = 2^-24, doubled (phema_ref.shadow_step_bound); p' is the kernel's own fp32 result and r the fp32 rate.  Over several steps the fp64
recurrence is fed the kernel's own p sequence and the error must stay within the SUM of the per-step bounds: an EMA is a contraction
(0 < r <= 1), it does not amplify what earlier steps left.  The combination is one fp64 fma chain rounded to fp32 once:
|out - exact| <= ulp32(exact) / 2 + k 2^-53 sum_j |w_j s_j|.

All data comes from seeded CPU generators.  Needs an MI355X."""
import fractions
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phema_ref as R                                              # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
PRODUCT = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, wd=0.01)
DECAY = 0.9999
SIGMAS4 = (0.05, 0.10, 0.075, 0.15)
KEYS = ("p", "m", "v", "ema")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


@pytest.fixture(scope="module")
def P(H):
    from v_diffusion import phema
    return phema


def randn(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).float()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def state(n, seed):
    return {"p": randn(n, seed), "m": randn(n, seed + 1, 0.05), "v": randn(n, seed + 2, 0.05).square(), "ema": randn(n, seed + 3)}


def launch(H, d, g, *, k, gnorm_sq, max_norm, mode, rng, flag=None, steps=None, pema=None, rates=None, n_pema=None):
    """one update of the device state d at the product's constants: through vd_adamw_ema / vd_adamw_ema_flagged without ``pema``, through
    vd_adamw_emas with it.  mode 0 / 1 / 2: r_mode; "flag": the device-decided range"""
    b1, b2 = PRODUCT["betas"]
    args = (d["p"], g, d["m"], d["v"], d["ema"], gnorm_sq, max_norm, PRODUCT["lr"], b1, b2, PRODUCT["eps"], PRODUCT["wd"],
            1 - b1 ** k, 1 - b2 ** k, DECAY)
    r_bc = (1 - b1 ** (k - 1), 1 - b2 ** (k - 1)) if mode == 2 else (1.0, 1.0)
    if pema is None:
        if mode == "flag":
            H.adamw_ema_flagged(*args, rng[0], rng[1], flag, steps)
        else:
            H.adamw_ema(*args, r_lo=rng[0], r_hi=rng[1], r_mode=mode, r_bc1=r_bc[0], r_bc2=r_bc[1])
    elif mode == "flag":
        H.adamw_emas(*args, pema, rates, rng[0], rng[1], r_flag=flag, r_steps=steps, n_pema=n_pema)
    else:
        H.adamw_emas(*args, pema, rates, rng[0], rng[1], mode, r_bc[0], r_bc[1], n_pema=n_pema)


def check_shadow_step(e_new, e_old, p_new, rate, what):
    """one power-shadow step against fp64 within the documented bound; returns the worst error / bound"""
    r = float(np.float32(rate))
    e_old, p_new = e_old.double().cpu().numpy(), p_new.double().cpu().numpy()
    want = e_old + r * (p_new - e_old)
    bound = R.shadow_step_bound(r, p_new, e_old, want)
    err = np.abs(e_new.double().cpu().numpy() - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), f"{what}: error / bound {worst:.3f}"
    return worst


# ------------------------------------------------------------------------------------------------ vd_adamw_emas against the existing entries
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, 65539])
def test_emas_equals_the_existing_entries_bit_for_bit(H, P, n):
    """p, m, v, ema and r_steps of vd_adamw_emas equal vd_adamw_ema / vd_adamw_ema_flagged on copies of the same inputs, with 1, 2 and 4
    power shadows; every shadow of every case is within the one-step bound of fp64"""
    cpu, g = state(n, 100 + n), randn(n, 99 + n, 0.1).to(DEV)
    shadows0 = [randn(n, 200 + n + j) for j in range(4)]
    gsq = torch.zeros(1, device=DEV)
    H.sumsq(g, gsq)
    rng = (min(5, n), min(22, n))                                  # cuts a group of four
    k, t = 3, 7
    rates = [P.power_ema_rate(t, P.sigma_rel_to_gamma(s)) for s in SIGMAS4]
    worst = 0.0
    for clip in (True, False):
        for with_ema in (True, False):
            for mode, flagv in ((0, None), (1, None), (2, None), ("flag", 0.0), ("flag", 1.0)):
                def fresh():
                    d = {key: cpu[key].clone().to(DEV) for key in KEYS}
                    if not with_ema:
                        d["ema"] = None
                    flag = torch.full((1,), flagv, device=DEV) if flagv is not None else None
                    steps = torch.full((1,), 2, dtype=torch.int32, device=DEV) if flagv is not None else None
                    return d, flag, steps
                kw = dict(k=k, gnorm_sq=gsq if clip else None, max_norm=1.0 if clip else 0.0, mode=mode, rng=rng)
                ref, rflag, rsteps = fresh()
                launch(H, ref, g, flag=rflag, steps=rsteps, **kw)
                for npe in (1, 2, 4):
                    d, flag, steps = fresh()
                    pema = [e.clone().to(DEV) for e in shadows0[:npe]]
                    launch(H, d, g, flag=flag, steps=steps, pema=pema, rates=rates[:npe], **kw)
                    what = f"n {n} clip {clip} ema {with_ema} mode {mode} flag {flagv} shadows {npe}"
                    for key in KEYS:
                        if d[key] is not None:
                            assert same_bits(d[key], ref[key]), f"{what}: {key} differs from the existing entry"
                    if steps is not None:
                        assert int(steps) == int(rsteps) == (3 if flagv > 0 else 2), what
                    for j in range(npe):
                        worst = max(worst, check_shadow_step(pema[j], shadows0[j], d["p"], rates[j], f"{what} shadow {j}"))
    print(f"[n {n}] worst shadow error / bound {worst:.3f}")


@pytest.mark.parametrize("t0", [0, 100000])
def test_power_shadows_over_24_steps(H, P, t0):
    """24 updates at t = t0 + 1 .. t0 + 24: the fp64 recurrence over the kernel's own p sequence, within the sum of the per-step bounds"""
    n, sig = 65539, (0.05, 0.10)
    gam = [P.sigma_rel_to_gamma(s) for s in sig]
    d = {key: v.to(DEV) for key, v in state(n, 31).items()}
    pema = [randn(n, 41 + j).to(DEV) for j in range(2)]
    e64 = [e.double().cpu().numpy() for e in pema]
    budget = [np.zeros(n) for _ in pema]
    gsq = torch.zeros(1, device=DEV)
    for i in range(24):
        g = randn(n, 500 + i, 0.1).to(DEV)
        H.sumsq(g, gsq)
        t = t0 + i + 1
        rates = [P.power_ema_rate(t, x) for x in gam]
        before = [e.double().cpu().numpy() for e in pema]
        launch(H, d, g, k=i + 1, gnorm_sq=gsq if i % 2 == 0 else None, max_norm=1.0 if i % 2 == 0 else 0.0, mode=0, rng=(0, 0), pema=pema,
               rates=rates)
        p_new = d["p"].double().cpu().numpy()
        for j in range(2):
            r = float(np.float32(rates[j]))
            assert abs(r - (1.0 - R.beta(t, gam[j]))) <= U * r + 1e-15          # the fp32 rate is the restatement's, rounded once
            e64[j] = p_new.copy() if r == 1.0 else e64[j] + r * (p_new - e64[j])
            budget[j] += R.shadow_step_bound(r, p_new, before[j], e64[j])
    for j in range(2):
        err = np.abs(pema[j].double().cpu().numpy() - e64[j])
        print(f"[t0 {t0}] sigma_rel {sig[j]}: max error {err.max():.3e}, worst error / summed bound {(err / budget[j]).max():.3f}")
        assert (err <= budget[j]).all()


def test_a_rate_of_one_selects(H, P):
    n = 257
    cpu, g = state(n, 7), randn(n, 8, 0.1).to(DEV)
    d = {key: cpu[key].clone().to(DEV) for key in KEYS}
    nan, other = torch.full((n,), float("nan"), device=DEV), randn(n, 9).to(DEV)
    launch(H, d, g, k=1, gnorm_sq=None, max_norm=0.0, mode=0, rng=(0, 0), pema=[nan, other], rates=[1.0, 0.25])
    assert same_bits(nan, d["p"])                                  # selected: the NaN shadow was not read
    assert all(torch.isfinite(d[key]).all() for key in KEYS) and torch.isfinite(other).all()
    nan.fill_(float("nan"))
    launch(H, d, g, k=2, gnorm_sq=None, max_norm=0.0, mode=0, rng=(0, 0), pema=[nan, other], rates=[0.999, 0.25])
    assert torch.isnan(nan).all()                                  # a rate below 1 keeps the NaN, in that shadow only
    assert all(torch.isfinite(d[key]).all() for key in KEYS) and torch.isfinite(other).all()


def test_emas_refusals_leave_every_buffer_untouched(H, P):
    n = 257
    cpu, g = state(n, 17), randn(n, 18, 0.1).to(DEV)
    d = {key: cpu[key].clone().to(DEV) for key in KEYS}
    sh = [randn(n, 19 + j).to(DEV) for j in range(5)]
    sh0 = [e.clone() for e in sh]
    kw = dict(k=2, gnorm_sq=None, max_norm=0.0, mode=0, rng=(0, 0))
    cases = {"n_pema 0": dict(pema=[], rates=[]), "n_pema 5": dict(pema=sh, rates=[0.5] * 5),
             "null shadow": dict(pema=[sh[0], None], rates=[0.5, 0.5]), "rate 0": dict(pema=sh[:2], rates=[0.5, 0.0]),
             "rate 1.5": dict(pema=sh[:1], rates=[1.5]), "alias m": dict(pema=[sh[0], d["m"]], rates=[0.5, 0.5]),
             "alias a part of m": dict(pema=[d["m"][4:]], rates=[0.5]), "two shadows alias": dict(pema=[sh[0], sh[0]], rates=[0.5, 0.5]),
             "bad range": dict(pema=sh[:1], rates=[0.5], mode=1, rng=(5, n + 1))}
    for what, c in cases.items():
        with pytest.raises(H.HipError, match="vd_adamw_emas"):
            launch(H, d, g, **{**kw, **c})
        torch.cuda.synchronize()
        assert all(same_bits(d[key], cpu[key].to(DEV)) for key in KEYS), what
        assert all(same_bits(a, b) for a, b in zip(sh, sh0)), what


# ------------------------------------------------------------------------------------------------ vd_ema_combine
def weights_like_a_reconstruction(k, seed):
    """signs mixed, sum 1, sum |w| <= 10"""
    if k == 1:
        return [1.0]
    r = np.random.default_rng(seed).standard_normal(k)
    r[0], r[1] = abs(r[0]), -abs(r[1])
    w = r * (4.0 / np.abs(r).sum())
    w += (1.0 - w.sum()) / k
    w[-1] += 1.0 - w.sum()
    assert abs(w.sum() - 1.0) < 1e-14 and np.abs(w).sum() <= 10 and (w > 0).any() and (w < 0).any()
    return [float(x) for x in w]


def check_combination(out, srcs, w, acc=None):
    """|out - exact| <= ulp32(exact) / 2 + k 2^-53 sum |w_j s_j|: Fractions on 256 sampled elements, numpy.longdouble on all"""
    k, n = len(srcs), out.numel()
    got = out.double().cpu().numpy()
    xs = [s.cpu().numpy() for s in srcs]
    exact, mag = R.combine_longdouble(xs, w)
    if acc is not None:
        exact, mag = exact + acc.astype(np.longdouble), mag + np.abs(acc)
    bound = 0.5 * R.ulp32(exact.astype(np.float64)) + k * 2.0 ** -53 * mag
    err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
    assert (err <= bound).all(), f"k {k} n {n}: worst error / bound {(err / bound).max():.3f}"
    idx = np.unique(np.linspace(0, n - 1, min(n, 256)).astype(np.int64))
    for i, ex in zip(idx, R.combine_fraction(xs, w, idx, acc)):
        b = fractions.Fraction(float(R.ulp32(float(ex)))) / 2 + fractions.Fraction(k * 2.0 ** -53) * fractions.Fraction(float(mag[i]))
        assert abs(fractions.Fraction(float(got[i])) - ex) <= b, (k, n, int(i))
    return float((err / bound).max())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 65539])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_combine_against_exact_sums(H, n, k):
    srcs = [randn(n, 1000 + 37 * k + j).to(DEV) for j in range(k)]
    w = weights_like_a_reconstruction(k, k)
    out, again = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    H.ema_combine(out, None, srcs, w)
    H.ema_combine(again, None, srcs, w)
    assert same_bits(out, again)                                   # the same call, the same bits
    worst = check_combination(out, srcs, w)
    print(f"[k {k} n {n}] worst error / bound {worst:.3f}")
    # the one-element-per-lane form (a base that is not 16-byte aligned) gives the same bits
    shifted = [torch.empty(n + 1, device=DEV)[1:].copy_(s) for s in srcs]
    H.ema_combine(again.zero_(), None, shifted, w)
    assert same_bits(out, again)
    # one-hot weights return that source bit for bit, NaN in every other source
    hot = [torch.full((n,), float("nan"), device=DEV) for _ in range(k)]
    hot[k // 2] = srcs[k // 2]
    H.ema_combine(again.zero_(), None, hot, [1.0 if j == k // 2 else 0.0 for j in range(k)])
    assert same_bits(again, srcs[k // 2])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 65539])
def test_combine_chained_through_acc_is_the_same_chain(H, n):
    srcs = [randn(n, 3000 + j).to(DEV) for j in range(5)]
    w = weights_like_a_reconstruction(5, 77)
    one, two = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    acc1, acc = torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    H.ema_combine(one, None, srcs, w)
    H.ema_combine(None, acc, srcs[:2], w[:2])
    H.ema_combine(two, acc, srcs[2:], w[2:])
    assert same_bits(one, two)                                     # 5 in one launch == 2 + 3 through acc
    H.ema_combine(None, acc1, srcs, w)
    assert torch.equal(acc1.view(torch.int64), acc.view(torch.int64)) and same_bits(acc.float(), one)
    start = randn(n, 3100).double().to(DEV)                        # a non-zero starting accumulator enters the chain first
    keep = start.clone()
    H.ema_combine(two, start, srcs, w)
    check_combination(two, srcs, w, acc=keep.cpu().numpy())


def test_combine_refusals(H):
    n = 16
    srcs = [randn(n, 50 + j).to(DEV) for j in range(33)]
    out = torch.full((n,), 3.0, device=DEV)
    for bad_src, bad_out in (([], out), (srcs, out), (srcs[:2], None)):       # k = 0, k = 33, neither out nor acc
        with pytest.raises(H.HipError, match="vd_ema_combine"):
            H.ema_combine(bad_out, None, bad_src, [0.5] * len(bad_src))
    with pytest.raises(H.HipError, match="aliases"):
        H.ema_combine(out, None, [out, srcs[0]], [0.5, 0.5])
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 3.0


def test_posthoc_ema_forty_snapshots_in_chunks(H, P, tmp_path):
    """40 snapshots (half of them on disk), chunk = 16: three launches chained through the accumulator equal the single exact combination
    within the one-chain bound, and equal a two-chunk run bit for bit"""
    n, gam = 1023, P.sigma_rel_to_gamma(0.10)
    layout = [("w", 0, (31, 33))]
    snaps, flats = [], []
    for i in range(40):
        f = torch.cat([randn(n, 7000 + i), torch.zeros(1)])
        s = P.make_snapshot(8 * (i + 1), (0.10,), layout, n + 1, [f])
        flats.append(f)
        if i % 2:
            path = str(tmp_path / f"snap{i}.pt")
            torch.save(s, path)
            s = path
        snaps.append(s)
    got = P.posthoc_ema(snaps, 0.075, chunk=16)
    assert list(got) == ["w"] and got["w"].shape == (31, 33) and got["w"].is_cuda and got["w"].dtype == torch.float32
    w = P.solve_weights([8 * (i + 1) for i in range(40)], [gam] * 40, 320, P.sigma_rel_to_gamma(0.075))
    check_combination(got["w"].reshape(-1), [f[:n] for f in flats], [float(x) for x in w])
    assert same_bits(got["w"], P.posthoc_ema(snaps, 0.075, chunk=32)["w"])
    assert same_bits(P.posthoc_ema(snaps, 0.10, t=160)["w"], flats[19][:n].view(31, 33).to(DEV))     # a stored profile: selected
    with pytest.raises(ValueError, match="layout"):
        P.posthoc_ema(snaps + [P.make_snapshot(400, (0.10,), [("w", 0, (33, 31))], n + 1, [flats[0]])], 0.075)


# ------------------------------------------------------------------------------------------------ trainer
def tiny_trainer(cfg, **kw):
    import v_diffusion
    from oracle.cases import make_weights
    from v_diffusion.trainer import HotPathTrainer
    model = v_diffusion.UNet(**cfg)
    model.load_state_dict(make_weights(cfg))
    model.to(DEV).train()
    gd = v_diffusion.GaussianDiffusion(v_diffusion.get_logsnr_schedule("cosine"), 8, "v", "fixed_large", "snr_trunc", "mse", p_uncond=0.0)
    return HotPathTrainer(model, gd, lr=2e-4, betas=(0.9, 0.999), weight_decay=0.01, warmup=0, grad_norm=1.0, ema_decay=0.9999, **kw)


def tiny_batch(cfg, label):
    from oracle.cases import TINY, make_inputs
    x, _, y = make_inputs(cfg, 4, TINY["tinyA"]["R"], label, seed=5)
    return x.clamp(-1, 1).to(DEV), (y.to(DEV) if label else None)


def twin_steps(cfg, label, ys, extra=None):
    """twin trainers from the same seeds, one tracking (0.05, 0.10); returns them and the per-step records of the tracking one"""
    a, b = tiny_trainer(cfg, ema_sigma_rels=(0.05, 0.10)), tiny_trainer(cfg)
    assert b.flat.pema == [] and len(a.flat.pema) == 2 and all(same_bits(e, a.flat.p) for e in a.flat.pema)
    x, y = tiny_batch(cfg, label)
    rec = []
    for i, use_y in enumerate(ys):
        losses = []
        for tr in (a, b):
            torch.manual_seed(1234 + i)                            # dropout seeds come from the default generator
            losses.append(tr.step(x, y if use_y else None))
        assert float(losses[0]) == float(losses[1]), f"step {i}: the loss moved"
        rec.append((a.flat.p.clone(), [e.clone() for e in a.flat.pema]))
        if extra is not None:
            extra(i, a)
    for key in ("p", "m", "v", "ema"):
        assert same_bits(getattr(a.flat, key), getattr(b.flat, key)), f"{key} moved with the power shadows on"
    assert a.flat.pema_updates == len(ys) and a.flat.ema_updates == b.flat.ema_updates == len(ys)
    return a, b, x, y, rec


def check_recorded_shadows(P, a, rec):
    for j, g in enumerate(a.flat.pema_gammas):
        e64, budget, before = None, 0.0, None
        for i, (p, shadows) in enumerate(rec):
            r = float(np.float32(P.power_ema_rate(i + 1, g)))
            p64 = p.double().cpu().numpy()
            prev = p64 if before is None else before                # (the shadows start as p; the first rate is 1 and selects)
            e64 = p64.copy() if i == 0 else e64 + r * (p64 - e64)
            budget = budget + R.shadow_step_bound(r, p64, prev, e64)
            before = shadows[j].double().cpu().numpy()
        err = np.abs(before - e64)
        assert (err <= budget).all(), f"shadow {j}: worst error / bound {(err / np.maximum(budget, 1e-300)).max():.3f}"
        assert same_bits(rec[0][1][j], rec[0][0])                  # t = 1: the shadow IS theta_1


@pytest.mark.parametrize("conditional", [True, False], ids=["tinyA", "tinyA_without_classes"])
def test_trainer_twins_and_checkpoints(H, P, tmp_path, conditional):
    """tinyA with labels in every step (class-conditional: the device-flagged form of the tail), and the same network without its class
    embedding (the host-decided form, r_mode 0)"""
    from oracle.cases import TINY
    cfg = TINY["tinyA"]["cfg"] if conditional else dict(TINY["tinyA"]["cfg"], num_classes=0)
    label = TINY["tinyA"]["label"] if conditional else None
    snaps = []
    a, b, x, y, rec = twin_steps(cfg, label, [conditional] * 6, extra=lambda i, tr: snaps.append(tr.ema_snapshot()) if i in (1, 3, 5) else None)
    assert (a.flat.cls_range is not None) == conditional
    check_recorded_shadows(P, a, rec)
    # ema_weights(sigma_rel) points the module at that shadow and back, also when the body raises
    name, q = next(iter(a.model.named_parameters()))
    home = q.data_ptr()
    with a.ema_weights(sigma_rel=0.10):
        inside = q.data_ptr()
        assert inside == a.flat.pema[1].data_ptr() + 4 * a.flat.offsets[name]
    assert inside != home and q.data_ptr() == home
    with pytest.raises(ZeroDivisionError):
        with a.ema_weights(sigma_rel=0.05):
            1 / 0
    assert q.data_ptr() == home
    with a.ema_weights():
        assert q.data_ptr() not in (home, inside)
    with pytest.raises(KeyError):
        with a.ema_weights(sigma_rel=0.07):
            pass
    with pytest.raises(KeyError):
        with b.ema_weights(sigma_rel=0.10):
            pass
    # the snapshots of steps 2, 4, 6 -> the step-4 profile, bit for bit: the one-hot path end to end
    assert [s["t"] for s in snaps] == [2, 4, 6] and snaps[0]["sigma_rels"] == [0.05, 0.10] and snaps[0]["numel"] == a.flat.numel
    path = str(tmp_path / "snap6.pt")
    assert a.ema_snapshot(path)["t"] == 6 and torch.load(path, weights_only=True)["t"] == 6
    got = P.posthoc_ema([snaps[0], snaps[1], path], 0.10, t=4)
    assert set(got) == set(a.flat.names)
    for k in a.flat.names:
        assert same_bits(got[k], a.flat.view(rec[3][1][1], k)), k
    a.model.load_state_dict(got, strict=False)                     # ... and it loads as a state_dict
    # checkpoints: "ema_power" only with the feature; a fresh trainer resumes with bit-equal shadows
    sd_a, sd_b = a.state_dicts(), b.state_dicts()
    assert set(sd_b) == {"model", "optimizer", "ema", "scheduler"} and set(sd_a) == set(sd_b) | {"ema_power"}
    assert sd_a["ema_power"]["sigma_rels"] == [0.05, 0.10] and sd_a["ema_power"]["num_updates"] == 6
    assert [set(s) for s in sd_a["ema_power"]["shadows"]] == [set(sd_a["model"])] * 2
    sd_a["rng"] = a.gather_rng_states()
    c = tiny_trainer(cfg, ema_sigma_rels=(0.05, 0.10))
    c.load_checkpoint(sd_a)
    assert c.flat.pema_updates == 6 and all(same_bits(u, v) for u, v in zip(a.flat.pema, c.flat.pema))
    for i in range(2):
        for tr in (a, c):
            torch.manual_seed(99 + i)
            tr.step(x, y)
    assert same_bits(a.flat.p, c.flat.p) and all(same_bits(u, v) for u, v in zip(a.flat.pema, c.flat.pema))
    with pytest.raises(RuntimeError, match="sigma_rels"):
        tiny_trainer(cfg, ema_sigma_rels=(0.05, 0.15)).load_checkpoint(sd_a)
    d = tiny_trainer(cfg, ema_sigma_rels=(0.05, 0.10))
    with pytest.warns(UserWarning, match="ema_power"):              # a checkpoint without the profiles: they start at the loaded weights, t = 0
        d.load_checkpoint(sd_b)
    assert d.flat.pema_updates == 0 and all(same_bits(e, d.flat.p) for e in d.flat.pema)
    for bad in ((), (0.05, 0.05), (0.05, 0.06, 0.07, 0.08, 0.09)):
        with pytest.raises(ValueError):
            tiny_trainer(cfg, ema_sigma_rels=bad)


def test_trainer_twins_class_conditional_through_the_flagged_form(H, P):
    from oracle.cases import TINY
    case = TINY["tinyA"]
    a, b, _, _, rec = twin_steps(case["cfg"], case["label"], [True, False, True, True, False, True])
    assert a.flat.cls_range is not None and a.flat.cls_steps == b.flat.cls_steps == 4
    check_recorded_shadows(P, a, rec)


def test_trainer_without_the_feature_launches_what_it_launched(H, monkeypatch):
    from oracle.cases import TINY
    cfg = dict(TINY["tinyA"]["cfg"], num_classes=0)
    tr = tiny_trainer(cfg)
    monkeypatch.setattr(H, "adamw_emas", lambda *a, **k: pytest.fail("vd_adamw_emas launched without ema_sigma_rels"))
    x, _ = tiny_batch(cfg, None)
    tr.step(x, None)
    with pytest.raises(RuntimeError, match="ema_sigma_rels"):
        tr.ema_snapshot()


# ------------------------------------------------------------------------------------------------ optim.PowerEMA
def test_power_ema_over_a_fused_adamw_store(H, P):
    from v_diffusion import optim
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3)).to(DEV)
    opt = optim.FusedAdamW(model.parameters(), lr=1e-2, betas=(0.9, 0.999), weight_decay=0.01)
    pe = optim.PowerEMA(model)
    assert pe.sigma_rels == (0.05, 0.10) and pe._store is not None
    x = randn(40, 5).view(8, 5).to(DEV)
    e64, budget, before = [None, None], [0.0, 0.0], [None, None]
    for i in range(5):
        opt.zero_grad(set_to_none=True)
        model(x).square().mean().backward()
        opt.step()
        pe.update()
        p64 = opt.p.double().cpu().numpy()
        for j, g in enumerate(pe.gammas):
            r = float(np.float32(P.power_ema_rate(i + 1, g)))
            e64[j] = p64.copy() if i == 0 else e64[j] + r * (p64 - e64[j])
            budget[j] = budget[j] + R.shadow_step_bound(r, p64, p64 if i == 0 else before[j], e64[j])
            before[j] = pe._flat[j].double().cpu().numpy()
    for j in range(2):
        assert (np.abs(before[j] - e64[j]) <= budget[j]).all()
    raw = opt.p.clone()
    pe.apply(0.10)
    assert same_bits(opt.p, pe._flat[1]) and same_bits(model[0].weight.data, pe.shadows[1]["0.weight"])
    pe.restore()
    assert same_bits(opt.p, raw)
    with pe:
        assert same_bits(opt.p, pe._flat[0])
    assert same_bits(opt.p, raw)
    with pytest.raises(KeyError):
        pe.apply(0.2)
    sd = pe.state_dict()
    assert sd["num_updates"] == 5 and sd["sigma_rels"] == [0.05, 0.10] and set(sd["shadows"][0]) == {k for k, _ in model.named_parameters()}
    snap = pe.snapshot()
    assert snap["t"] == 5 and snap["numel"] == opt.flat.numel
    got = P.posthoc_ema([snap], 0.05)
    for k, v in pe.shadows[0].items():
        assert same_bits(got[k], v), k
