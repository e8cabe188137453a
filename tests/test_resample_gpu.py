"""Loss-aware timestep resampling on the GPU: vd_lsm_draw / vd_lsm_update through the C ABI against the numpy restatement
tests/lsm_ref.py, the LossSecondMomentResampler object, and HotPathTrainer with a resampler on the tiny learned-variance UNet (one
rank and two).  Need an MI355X.

Bounds.  cdf: delta = (2 T + 16) 2^-53 absolute -- twice the worst-case error of summing T positive fp64 terms that end at 1 (the
kernel's sum and the restatement's, in different orders) plus the roundings of the square root, the divisions and the mixture.  An
index may differ from the restatement's only where u lies within delta of an edge; the tests assert that no u they use does.
Weights: one fp32 ulp (q agrees to ~1e-13 relative; the rounding to fp32 may fall either way).  Everything else is exact."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lsm_ref
from test_diffusion_kernels_gpu import DEV, H, guarded, rnd                   # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS, KS, BS = (1, 2, 7, 64, 1000, 4097), (1, 10), (1, 5, 4096)
TOP = float(np.nextafter(1.0, 0.0))
SENTINEL = -12345.0


def delta(T):
    return (2 * T + 16) * 2.0 ** -53


def guarded_as(shape, dtype):
    """``guarded`` for a 4- or 8-byte dtype: the payload of ``guarded`` starts at an odd float offset, so one float is skipped (and
    checked here) to keep an 8-byte type aligned"""
    words = math.prod(shape) * (torch.empty((), dtype=dtype).element_size() // 4)
    flat, ok = guarded((words + 1,))
    body = flat[1:].view(dtype).view(shape)
    return body, lambda: ok() and float(flat[0]) == SENTINEL


@functools.lru_cache(maxsize=None)
def warmed(T, K, eps=0.001, special=None):
    """a warmed-up restatement with a log-uniform history in [1e-6, 1e2], its probabilities and running sum, computed once"""
    r = lsm_ref.Ref(T, K, eps)
    rng = np.random.default_rng(1000 * T + K)
    r.hist[:] = np.exp(rng.uniform(math.log(1e-6), math.log(1e2), size=(T, K))).astype(np.float32)
    if special == "huge":
        r.hist[T // 2] = 1e30                                      # squares overflow fp32, not fp64
    if special == "zero":
        r.hist[:] = 0.0                                            # S = 0: the uniform fallback
    r.count[:] = K
    return r, r.probabilities(), r.cdf()


@functools.lru_cache(maxsize=None)
def uniforms(T, B):
    return np.random.default_rng(77 * T + B).random(B)


def device_state(r):
    (hist, hk), (count, ck), (pos, pk) = guarded(r.hist.shape), guarded_as(r.count.shape, torch.int32), guarded_as(r.pos.shape, torch.int32)
    hist.copy_(torch.from_numpy(r.hist))
    count.copy_(torch.from_numpy(r.count))
    pos.copy_(torch.from_numpy(r.pos))
    return hist, count, pos, lambda: hk() and ck() and pk()


def run_draw(H, r, hist, count, u):
    """vd_lsm_draw on guarded outputs: (cdf, t, idx, w) as numpy"""
    B = len(u)
    (cdf, k0), (t, k1), (idx, k2), (w, k3) = (guarded_as((r.T,), torch.float64), guarded_as((B,), torch.float64),
                                              guarded_as((B,), torch.int32), guarded((B,)))
    H.lsm_draw(hist, count, torch.from_numpy(np.ascontiguousarray(u)).to(DEV), cdf, t, idx, w, r.T, r.K, B, r.eps)
    torch.cuda.synchronize()
    assert k0() and k1() and k2() and k3(), "vd_lsm_draw wrote outside its outputs"
    return cdf.cpu().numpy(), t.cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy()


def edge_distance(u, C):
    """distance of every u to the nearest C_i (C non-decreasing)"""
    j = np.searchsorted(C, u)
    lo, hi = C[np.maximum(j - 1, 0)], C[np.minimum(j, len(C) - 1)]
    return np.minimum(np.abs(u - lo), np.abs(u - hi))


def check_warm_draw(H, r, q, C, Bs):
    T = r.T
    d = delta(T)
    hist, count, _, state_ok = device_state(r)
    width = np.diff(C, prepend=0.0)
    assert bool((width > 4 * d).all()), "an interval of the reference distribution is too narrow for the midpoint test"
    mids, ends = C - 0.5 * width, np.array([0.0, TOP])
    worst = 0.0
    for u in [uniforms(T, B) for B in Bs] + [mids, ends]:
        cdf, t, idx, w = run_draw(H, r, hist, count, u)
        worst = max(worst, float(np.abs(cdf - C).max()))
        assert np.abs(cdf - C).max() <= d, f"cdf off by {np.abs(cdf - C).max():.3e} > delta {d:.3e}"
        if u is not ends:                                         # (the largest double below 1 sits on the last edge; its index is T - 1 on either side)
            assert edge_distance(u, C).min() > d, "a u lies within delta of an edge: pick another seed"
        _, ridx, rw = r.draw(u)
        assert np.array_equal(idx, ridx), f"indices differ at {np.nonzero(idx != ridx)[0][:5]}"
        assert idx.dtype == np.int32 and w.dtype == np.float32 and t.dtype == np.float64
        assert bool((np.abs(w.astype(np.float64) - rw.astype(np.float64)) <= np.spacing(rw).astype(np.float64)).all()), "weight off by more than one fp32 ulp"
        assert np.array_equal(t, (idx.astype(np.float64) + 1.0) / T)
        if u is mids:
            assert np.array_equal(idx, np.arange(T, dtype=np.int32)), "a midpoint did not return its own interval"
        if u is ends:
            assert idx.tolist() == [0, T - 1]
        again = run_draw(H, r, hist, count, u)
        assert all(np.array_equal(a, b) for a, b in zip((cdf, t, idx, w), again)), "two calls differ"
    assert state_ok() and np.array_equal(hist.cpu().numpy(), r.hist) and np.array_equal(count.cpu().numpy(), r.count), "the draw changed the history"
    return worst


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T", TS)
def test_draw_warmed_up(H, T, K):
    r, q, C = warmed(T, K)
    worst = check_warm_draw(H, r, q, C, BS)
    print(f"[lsm draw T={T} K={K}] cdf within {worst / delta(T):.3f} delta of the sequential sum")


@pytest.mark.parametrize("special,T,K,eps", [("huge", 7, 10, 0.001), ("huge", 1000, 10, 0.001), ("zero", 7, 10, 0.001), ("zero", 4097, 1, 0.001),
                                             (None, 64, 10, 0.0), (None, 1000, 10, 1.0)])
def test_draw_special_histories(H, special, T, K, eps):
    """a row of 1e30 (its squares overflow fp32, not fp64), an all-zero history (uniform fallback), and the ends of uniform_prob"""
    r, q, C = warmed(T, K, eps, special)
    assert bool(np.isfinite(q).all())
    if special == "zero" or eps == 1.0:
        assert np.array_equal(q, np.full(T, 1.0 / T))
    if special == "huge":
        assert q[T // 2] > 0.99
    check_warm_draw(H, r, q, C, (5, 4096))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T", TS)
def test_draw_not_warmed_up(H, T, K):
    """one count entry at K - 1: idx = floor(u T), w = 1 exactly, whatever the history holds"""
    r0, _, _ = warmed(T, K)
    r = lsm_ref.Ref(T, K, 0.001)
    r.hist[:] = r0.hist
    r.count[:] = K
    r.count[T // 3] = K - 1
    hist, count, _, state_ok = device_state(r)
    for u in [uniforms(T, B) for B in BS] + [np.array([0.0, TOP])]:
        cdf, t, idx, w = run_draw(H, r, hist, count, u)
        assert np.array_equal(idx, np.minimum(T - 1, np.floor(u * T)).astype(np.int32))
        assert bool((w == 1.0).all()) and np.array_equal(t, (idx.astype(np.float64) + 1.0) / T)
        assert np.array_equal(cdf, (np.arange(T) + 1.0) / T)
    assert state_ok()


# ================================================================================================ update
def rows_for(T, n, seed):
    """n rows with NaN, +Inf, -Inf losses and indices -1 and T mixed in"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, T, size=n).astype(np.int32)
    loss = np.exp(rng.uniform(math.log(1e-6), math.log(1e2), size=n)).astype(np.float32)
    r = np.arange(n)
    loss[r % 17 == 3] = np.nan
    loss[r % 19 == 5] = np.inf
    loss[r % 23 == 7] = -np.inf
    idx[r % 29 == 11] = -1
    idx[r % 31 == 2] = T
    return idx, loss


def started(T, K, seed):
    """a restatement in mid-life: random history, counts in [0, K], positions in [0, K)"""
    rng = np.random.default_rng(seed)
    r = lsm_ref.Ref(T, K)
    r.hist[:] = rng.standard_normal((T, K)).astype(np.float32)
    r.count[:] = rng.integers(0, K + 1, size=T)
    r.pos[:] = rng.integers(0, K, size=T)
    return r


def run_update(H, hist, count, pos, idx, loss, T, K):
    H.lsm_update(hist, count, pos, torch.from_numpy(idx).to(DEV), torch.from_numpy(loss).to(DEV), len(idx), T, K)


def same_state(r, hist, count, pos):
    torch.cuda.synchronize()
    return (np.array_equal(hist.cpu().numpy().view(np.int32), r.hist.view(np.int32)) and np.array_equal(count.cpu().numpy(), r.count)
            and np.array_equal(pos.cpu().numpy(), r.pos))


@pytest.mark.parametrize("T,K,n", [(3, 2, 300), (1000, 10, 1), (1000, 10, 128), (1000, 10, 8192), (4097, 10, 5), (1000, 10, 0), (1, 1, 40),
                                   (257, 3, 1025)])
def test_update_equals_the_sequential_loop(H, T, K, n):
    r = started(T, K, seed=T + n)
    hist, count, pos, state_ok = device_state(r)
    idx, loss = rows_for(T, n, seed=3 * T + n)
    if n >= 32:
        assert np.isnan(loss).any() and np.isposinf(loss).any() and np.isneginf(loss).any() and (idx == -1).any() and (idx == T).any()
    run_update(H, hist, count, pos, idx, loss, T, K)
    r.update(idx, loss)
    assert same_state(r, hist, count, pos), "state differs from the sequential loop"
    assert state_ok(), "vd_lsm_update wrote outside hist / count / pos"


def test_update_skips_and_splits(H):
    """a call of bad rows only changes nothing; two consecutive calls equal one call on the concatenated rows"""
    T, K = 1000, 10
    r = started(T, K, seed=9)
    hist, count, pos, state_ok = device_state(r)
    bad_i, bad_l = np.array([5, -1, T, 7, 8], dtype=np.int32), np.array([np.nan, 1.0, 1.0, np.inf, -np.inf], dtype=np.float32)
    run_update(H, hist, count, pos, bad_i, bad_l, T, K)
    assert same_state(r, hist, count, pos)
    idx, loss = rows_for(T, 1500, seed=10)
    one = device_state(r)
    run_update(H, hist, count, pos, idx[:700], loss[:700], T, K)
    run_update(H, hist, count, pos, idx[700:], loss[700:], T, K)
    run_update(H, *one[:3], idx, loss, T, K)
    r.update(idx, loss)
    assert same_state(r, hist, count, pos) and same_state(r, *one[:3]) and state_ok() and one[3]()


# ================================================================================================ the object
def test_object_round_trip_and_probabilities(H):
    import v_diffusion as vd
    T, K = 1000, 10
    a = vd.LossSecondMomentResampler(T, device=DEV)
    assert a.hist.shape == (T, K) and a.hist.dtype == torch.float32 and a.count.dtype == torch.int32 and a.pos.dtype == torch.int32
    assert a.cdf.dtype == torch.float64 and not a.warmed_up and float(a.hist.abs().sum()) == 0.0
    r = lsm_ref.Ref(T, K, 0.001)
    assert np.array_equal(a.probabilities().cpu().numpy(), np.full(T, 1.0 / T))
    rng = np.random.default_rng(4)
    for _ in range(12):                                           # ~12 visits per timestep: warmed up with every ring wrapped
        idx = rng.permutation(T).astype(np.int32)
        loss = np.exp(rng.uniform(math.log(1e-4), math.log(10.0), size=T)).astype(np.float32)
        a.update(torch.from_numpy(idx).to(DEV), torch.from_numpy(loss).to(DEV))
        r.update(idx, loss)
    assert a.warmed_up and r.warmed_up() and same_state(r, a.hist, a.count, a.pos)
    q = a.probabilities()
    assert q.dtype == torch.float64 and q.is_cuda
    assert bool((np.abs(q.cpu().numpy() - r.probabilities()) <= delta(T) * r.probabilities()).all())
    b = vd.LossSecondMomentResampler(T, uniform_prob=0.5, device=DEV)
    b.load_state_dict(a.state_dict())
    assert b.uniform_prob == a.uniform_prob and same_state(r, b.hist, b.count, b.pos)
    ga, gb = torch.Generator(DEV).manual_seed(3), torch.Generator(DEV).manual_seed(3)
    da, db = a.draw(128, generator=ga), b.draw(128, generator=gb)
    assert all(torch.equal(x, y) for x, y in zip(da, db)) and torch.equal(a.cdf, b.cdf)
    # the stream contract: one rand of B doubles
    g = torch.Generator(DEV).manual_seed(3)
    u = torch.rand((128,), dtype=torch.float64, device=DEV, generator=g)
    assert all(torch.equal(x, y) for x, y in zip(da, a.draw(128, u=u))) and torch.equal(ga.get_state(), g.get_state())
    _, ridx, rw = r.draw(u.cpu().numpy())
    assert np.array_equal(da[1].cpu().numpy(), ridx) and len(set(ridx.tolist())) > 16
    for T2, K2 in ((T + 1, K), (T, K + 1)):
        with pytest.raises(RuntimeError):
            vd.LossSecondMomentResampler(T2, history_per_term=K2, device=DEV).load_state_dict(a.state_dict())


# ================================================================================================ the trainer
T8 = 8


def build6():
    """tinyA with six output channels (v-prediction + variance channels) and the oracle's deterministic weights"""
    import v_diffusion as vd
    from oracle.cases import TINY, make_weights
    cfg = dict(TINY["tinyA"]["cfg"], out_channels=6)
    m = vd.UNet(**cfg)
    m.load_state_dict(make_weights(cfg), strict=True)
    return m.to(DEV).train()


def make_gd():
    import v_diffusion as vd
    return vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T8, "v", "learned", "snr_trunc", "kl", w_guide=0.0, p_uncond=0.0)


def batch(seed=3):
    from oracle.cases import TINY, make_inputs
    case = TINY["tinyA"]
    x0, _, y = make_inputs(case["cfg"], 3, case["R"], case["label"], seed=seed)
    return ((x0.clamp(-1, 1) * 127.5).round() / 127.5).to(DEV), y.clamp(min=1).to(DEV)


def trainer(**kw):
    from v_diffusion.trainer import HotPathTrainer
    return HotPathTrainer(build6(), make_gd(), lr=1e-3, warmup=0, timesteps=T8, **kw)


def skewed(K=10):
    """a warmed-up, strongly non-uniform history over T8 timesteps"""
    r = lsm_ref.Ref(T8, K, 0.001)
    r.hist[:] = (10.0 ** np.linspace(-3, 1, T8))[:, None].astype(np.float32) * np.linspace(0.5, 1.5, K)[None, :].astype(np.float32)
    r.count[:] = K
    r.pos[:] = np.arange(T8) % K
    return r


def load_into(sampler, r):
    sampler.load_state_dict({"hist": torch.from_numpy(r.hist), "count": torch.from_numpy(r.count), "pos": torch.from_numpy(r.pos),
                             "history_per_term": r.K, "uniform_prob": r.eps})


def replay(B, shape):
    """the documented stream of a resampled draw from a fresh rank-0 generator: one fp64 rand(B), then the noise"""
    g = torch.Generator(DEV).manual_seed(8191)
    u = torch.rand((B,), dtype=torch.float64, device=DEV, generator=g)
    noise = torch.empty(shape, device=DEV).normal_(generator=g)
    return u, noise


def test_trainer_uniform_is_the_default(H):
    x, y = batch()
    a, b = trainer(), trainer(schedule_sampler="uniform")
    assert a.sampler is None and b.sampler is None and "schedule_sampler" not in a.state_dicts()
    for _ in range(2):
        la, lb = a.step(x, y), b.step(x, y)
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    assert torch.equal(a.flat.p, b.flat.p) and torch.equal(a.generator.get_state(), b.generator.get_state())


def test_trainer_cold_resampler(H):
    """before the history is warmed up the step is a uniform one drawn from a double: the loss is the mean of train_loss on the
    replayed draw (1e-6 relative: the same kernels through a second copy of the model, summed in another order), and the history
    afterwards is the restatement's update with those losses"""
    x, y = batch()
    tr = trainer(schedule_sampler="loss-second-moment")
    assert tr.sampler.num_timesteps == T8 and tr.sampler.history_per_term == 10
    u, noise = replay(x.shape[0], x.shape)
    r = lsm_ref.Ref(T8, 10, 0.001)
    t, idx, w = r.draw(u.cpu().numpy())
    per = make_gd().train_loss(build6(), x_0=x, t=torch.from_numpy(t).to(DEV), y=y, noise=noise).detach()      # (the training forward, as the step runs)
    loss = tr.step(x, y)
    torch.cuda.synchronize()
    assert per.shape == (3,) and abs(float(loss) - float(per.double().mean())) <= 1e-6 * abs(float(per.double().mean()))
    r.update(idx, per.cpu().numpy())
    assert same_state(r, tr.sampler.hist, tr.sampler.count, tr.sampler.pos)
    assert float(tr.stats.extract()["loss"]) == pytest.approx(float(loss), rel=1e-6)


def test_trainer_warm_resampler_loss_and_gradient(H):
    """a warmed, strongly non-uniform history: the loss is dot(per, w) / B with w = 1 / (T q_idx) far from one, the flat gradient is
    the gradient of (train_loss * w).mean() through a second copy of the model (relative L2 1e-6), the history moves on"""
    import v_diffusion as vd
    x, y = batch()
    r = skewed()
    sm = vd.LossSecondMomentResampler(T8, device=DEV)
    load_into(sm, r)
    tr = trainer(schedule_sampler=sm)
    assert tr.sampler is sm and sm.warmed_up
    u, noise = replay(x.shape[0], x.shape)
    t, idx, w = r.draw(u.cpu().numpy())
    assert float(np.abs(w - 1.0).max()) > 0.2, "the weights of this history are too close to one to test the reweighting"
    m2 = build6()
    per = make_gd().train_loss(m2, x_0=x, t=torch.from_numpy(t).to(DEV), y=y, noise=noise)
    want = (per * torch.from_numpy(w).to(DEV)).mean()
    want.backward()
    loss = tr.step(x, y)
    torch.cuda.synchronize()
    want = float(want.detach())
    assert abs(float(loss) - want) <= 1e-6 * abs(want)
    g2 = dict(m2.named_parameters())
    num = sum(float((tr.flat.grad_views[k].double() - g2[k].grad.double()).square().sum()) for k in tr.flat.names)
    den = sum(float(g2[k].grad.double().square().sum()) for k in tr.flat.names)
    rel = math.sqrt(num / den)
    print(f"[lsm trainer] weighted gradient against the second route: relative L2 {rel:.3e}")
    assert den > 0 and rel <= 1e-6
    r.update(idx, per.detach().cpu().numpy())
    assert same_state(r, sm.hist, sm.count, sm.pos)
    # injected t / noise: the index comes from t, the weights from the keyword (ones by default), the history still moves
    t_in = torch.tensor([1.0, 4.0, 8.0], dtype=torch.float64, device=DEV) / T8
    m3 = build6()
    m3.load_state_dict(tr.model.state_dict())
    per_in = make_gd().train_loss(m3, x_0=x, t=t_in, y=y, noise=noise).detach()
    wk = torch.tensor([0.5, 2.0, 1.0], device=DEV)
    loss_in = tr.step(x, y, update=False, t=t_in, noise=noise, weights=wk)
    torch.cuda.synchronize()
    want_in = float((per_in.double() * wk.double()).mean())
    assert abs(float(loss_in) - want_in) <= 1e-6 * abs(want_in)
    r.update(np.array([0, 3, 7], dtype=np.int32), per_in.cpu().numpy())
    assert same_state(r, sm.hist, sm.count, sm.pos)


def test_trainer_checkpoint_carries_the_history(H, tmp_path):
    import v_diffusion as vd
    x, y = batch()
    a = trainer(schedule_sampler="loss-second-moment")
    load_into(a.sampler, skewed())
    a.step(x, y)
    path = str(tmp_path / "lsm.pt")
    a.save_checkpoint(path)
    ckpt = torch.load(path, map_location="cpu")
    assert set(ckpt["schedule_sampler"]) == {"hist", "count", "pos", "history_per_term", "uniform_prob"}
    b = trainer(schedule_sampler="loss-second-moment")
    b.load_checkpoint(path)
    assert torch.equal(a.sampler.hist, b.sampler.hist) and torch.equal(a.sampler.pos, b.sampler.pos) and torch.equal(a.sampler.count, b.sampler.count)
    (ta, na), (tb, nb) = a.draw(x), b.draw(x)
    assert torch.equal(ta, tb) and torch.equal(na, nb) and all(torch.equal(p, q) for p, q in zip(a._drawn, b._drawn))
    assert float((a._drawn[1] - 1.0).abs().max()) > 0.2
    # a checkpoint without the key loads and leaves the history alone; a uniform trainer ignores the key
    c = trainer(schedule_sampler="loss-second-moment")
    c.load_checkpoint({k: v for k, v in ckpt.items() if k != "schedule_sampler"})
    assert not c.sampler.warmed_up and float(c.sampler.hist.abs().sum()) == 0.0
    d = trainer()
    d.load_checkpoint(ckpt)
    assert d.sampler is None and torch.equal(d.flat.p, a.flat.p)
    with pytest.raises(ValueError):
        trainer(schedule_sampler=vd.LossSecondMomentResampler(T8 + 1, device=DEV))


def test_two_ranks_hold_one_history(H, tmp_path):
    """two data-parallel ranks on the one GPU over gloo: after two steps both replicas hold bitwise the same history, and it is the
    restatement's update on the rank-ordered concatenation of the rows each rank reported"""
    out = str(tmp_path / "lsm_dp2.pt")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29581", os.path.join(ROOT, "tests", "lsm_dp_worker.py"), "--out", out, "--steps", "2"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    got = torch.load(out)
    ranks = got["ranks"]
    r = lsm_ref.Ref(got["T"], got["K"])
    assert len(ranks) == 2 and all(len(rk["rows"]) == 2 for rk in ranks)
    for s in range(2):
        for rk in ranks:
            idx, per = rk["rows"][s]
            assert idx.shape == (got["B"],) and per.shape == (got["B"],) and bool(torch.isfinite(per).all())
            r.update(idx.numpy(), per.numpy())
    assert not torch.equal(ranks[0]["rows"][0][0], ranks[1]["rows"][0][0]) or not torch.equal(ranks[0]["rows"][1][0], ranks[1]["rows"][1][0])
    for rk in ranks:
        assert np.array_equal(rk["hist"].numpy().view(np.int32), r.hist.view(np.int32)), "a replica's history differs from the restatement"
        assert np.array_equal(rk["count"].numpy(), r.count) and np.array_equal(rk["pos"].numpy(), r.pos)
    assert int(r.count.sum()) > 0
