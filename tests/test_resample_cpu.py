"""Loss-aware timestep resampling without a GPU: the invariants of the numpy restatement tests/lsm_ref.py (the yardstick of
test_resample_gpu.py), the constructor's checks and the export."""
import math

import numpy as np
import pytest

import lsm_ref


def filled(T, K, eps, seed):
    r = lsm_ref.Ref(T, K, eps)
    rng = np.random.default_rng(seed)
    r.hist[:] = np.exp(rng.uniform(math.log(1e-6), math.log(1e2), size=(T, K))).astype(np.float32)
    r.count[:] = K
    return r


@pytest.mark.parametrize("T,K", [(1, 1), (7, 10), (1000, 10), (4097, 1)])
@pytest.mark.parametrize("eps", [0.0, 0.001, 1.0])
def test_probabilities_sum_to_one(T, K, eps):
    r = filled(T, K, eps, seed=T + K)
    q, C = r.probabilities(), r.cdf()
    assert q.shape == (T,) and bool((q >= 0).all())
    assert abs(C[-1] - 1.0) <= T * 2.0 ** -53 and abs(math.fsum(q) - 1.0) <= T * 2.0 ** -53
    assert bool((np.diff(C) >= 0).all())
    if eps == 1.0:
        assert np.array_equal(q, np.full(T, 1.0 / T))


def test_uniform_prob_one_draws_like_the_uniform_grid():
    """with eps = 1 the warmed-up draw is the cold one: idx = floor(u T) wherever u T is not within rounding of an integer, w = 1 to
    one fp32 ulp"""
    T = 1000
    r = filled(T, 10, 1.0, seed=5)
    u = np.random.default_rng(6).random(4096)
    frac = u * T - np.floor(u * T)
    assert bool(((frac > 1e-9) & (frac < 1 - 1e-9)).all())
    t, idx, w = r.draw(u)
    assert np.array_equal(idx, np.floor(u * T).astype(np.int32))
    assert np.array_equal(t, (idx + 1.0) / T)
    assert bool((np.abs(w - 1.0) <= 2.0 ** -23).all())
    cold = lsm_ref.Ref(T, 10, 0.001)
    t2, idx2, w2 = cold.draw(u)
    assert np.array_equal(idx2, idx) and np.array_equal(t2, t) and bool((w2 == 1.0).all()) and w2.dtype == np.float32


def test_draw_edges():
    r = filled(7, 10, 0.001, seed=1)
    top = np.nextafter(1.0, 0.0)
    _, idx, _ = r.draw(np.array([0.0, top]))
    assert idx.tolist() == [0, 6]
    _, idx, _ = lsm_ref.Ref(7).draw(np.array([0.0, top]))
    assert idx.tolist() == [0, 6]
    zero = lsm_ref.Ref(5, 2, 0.001)
    zero.count[:] = 2                                              # warmed up on an all-zero history: the uniform fallback
    assert np.array_equal(zero.probabilities(), np.full(5, 0.2))
    big = filled(5, 2, 0.001, seed=2)
    big.hist[3] = 1e30                                             # squares overflow fp32, not fp64
    q = big.probabilities()
    assert bool(np.isfinite(q).all()) and q[3] > 0.99


def test_ring_wraps_in_row_order():
    """T = 3, K = 2, nine rows: the table by hand"""
    r = lsm_ref.Ref(3, 2)
    r.update([0, 1, 0, 0, 2, 1, 0, 1, 1], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0])
    # t = 0 sees 1, 3, 4, 7: slots [1, 3] -> [4, 3] -> [4, 7], next slot 0; t = 1 sees 2, 6, 8, 9: [2, 6] -> [8, 6] -> [8, 9], next 0; t = 2 sees 5
    assert r.hist.tolist() == [[4.0, 7.0], [8.0, 9.0], [5.0, 0.0]]
    assert r.pos.tolist() == [0, 0, 1] and r.count.tolist() == [2, 2, 1]
    assert not r.warmed_up()
    r.update([2], [0.5])
    assert r.warmed_up() and r.hist[2].tolist() == [5.0, 0.5] and r.pos[2] == 0


def test_bad_rows_are_skipped():
    r = lsm_ref.Ref(3, 2)
    r.update([0, 1, 2, -1, 3, 1], [float("nan"), float("inf"), float("-inf"), 1.0, 2.0, 7.0])
    assert r.hist.tolist() == [[0.0, 0.0], [7.0, 0.0], [0.0, 0.0]]
    assert r.count.tolist() == [0, 1, 0] and r.pos.tolist() == [0, 1, 0]


def test_constructor_checks_and_export():
    import v_diffusion as vd
    assert "LossSecondMomentResampler" in vd.__all__ and "LossSecondMomentResampler" in vd._HOT and callable(vd.LossSecondMomentResampler)
    for kw in (dict(num_timesteps=0), dict(num_timesteps=65537), dict(num_timesteps=8, history_per_term=0),
               dict(num_timesteps=8, uniform_prob=-0.1), dict(num_timesteps=8, uniform_prob=1.5)):
        with pytest.raises(ValueError):
            vd.LossSecondMomentResampler(device="cpu", **kw)
    with pytest.raises(RuntimeError, match="must live on an MI355X"):
        vd.LossSecondMomentResampler(8, device="cpu")


def test_trainer_refuses_resampling_without_a_grid():
    """checked before any device work: no model, no GPU needed"""
    from v_diffusion.trainer import HotPathTrainer
    with pytest.raises(ValueError, match="timesteps > 0"):
        HotPathTrainer(None, None, timesteps=0, schedule_sampler="loss-second-moment")
    with pytest.raises(ValueError, match="schedule_sampler"):
        HotPathTrainer(None, None, timesteps=8, schedule_sampler="importance")
