"""CPU-side checks of v_diffusion.metrics.kid_score and v_diffusion.metrics.inception_score: both import without a GPU, the subset
draw is the documented one, and every argument check raises before any device work (there is no device on this tier: a check
that came too late would surface as the RuntimeError of the missing GPU instead of the ValueError asked for here)."""
import numpy as np
import pytest
import torch


def test_modules_import_without_a_gpu_and_stay_off_the_star_surface():
    import v_diffusion.metrics as M
    from v_diffusion.metrics import inception_score as I, kid_score as K
    assert callable(K.subset_indices) and callable(K.polynomial_mmd) and callable(K.kernel_inception_distance)
    assert callable(I.inception_score)
    for name in ("kernel_inception_distance", "polynomial_mmd", "subset_indices", "inception_score", "KID", "InceptionScore"):
        assert name not in M.__all__


def test_subset_indices_draw_order_and_shape():
    from v_diffusion.metrics.kid_score import subset_indices
    ix, iy = subset_indices(50, 70, 4, 20, seed=5)
    assert ix.dtype == np.int32 and iy.dtype == np.int32 and ix.shape == (4, 20) and iy.shape == (4, 20)
    jx, jy = subset_indices(50, 70, 4, 20, seed=5)
    assert np.array_equal(ix, jx) and np.array_equal(iy, jy)
    kx, _ = subset_indices(50, 70, 4, 20, seed=6)
    assert not np.array_equal(ix, kx)
    for row in list(ix) + list(iy):
        assert len(set(row.tolist())) == 20
    assert ix.min() >= 0 and ix.max() < 50 and iy.min() >= 0 and iy.max() < 70 and iy.max() >= 50     # (seed 5 reaches Y's upper rows)
    # the definition: one RandomState(seed); per subset X's choice first, then Y's
    rng = np.random.RandomState(5)
    for s in range(4):
        assert np.array_equal(ix[s], rng.choice(50, 20, replace=False))
        assert np.array_equal(iy[s], rng.choice(70, 20, replace=False))
    # a full-size subset is a permutation
    px, _ = subset_indices(20, 20, 2, 20, seed=0)
    assert sorted(px[1].tolist()) == list(range(20))


def test_kid_argument_checks_before_device_work():
    from v_diffusion.metrics import kid_score as K
    x, y = torch.zeros(40, 32), torch.zeros(30, 32)
    with pytest.raises(ValueError, match="feature lengths"):
        K.kernel_inception_distance(x, torch.zeros(30, 48), subsets=2, subset_size=8)
    with pytest.raises(ValueError, match="feature lengths"):
        K.polynomial_mmd(x, torch.zeros(30, 48))
    with pytest.raises(ValueError, match="multiples of 16"):
        K.polynomial_mmd(torch.zeros(40, 24), torch.zeros(30, 24))
    with pytest.raises(ValueError, match="multiples of 16"):
        K.kernel_inception_distance(torch.zeros(40, 8), torch.zeros(30, 8), subsets=2, subset_size=8)
    with pytest.raises(ValueError, match="subset_size"):
        K.kernel_inception_distance(x, y, subsets=2, subset_size=1)
    with pytest.raises(ValueError, match="subset_size"):
        K.kernel_inception_distance(x, y, subsets=2, subset_size=31)          # fits X, not Y
    with pytest.raises(ValueError, match="subset_size"):
        K.kernel_inception_distance(x, y)                                       # the default 1000 does not fit either
    with pytest.raises(ValueError, match="subset_size"):
        K.subset_indices(40, 30, 2, 41)
    for degree in (0, 9, 2.5):
        with pytest.raises(ValueError, match="degree"):
            K.polynomial_mmd(x, y, degree=degree)
        with pytest.raises(ValueError, match="degree"):
            K.kernel_inception_distance(x, y, subsets=2, subset_size=8, degree=degree)
    with pytest.raises(ValueError, match="at least 2 rows"):
        K.polynomial_mmd(torch.zeros(1, 32), y)
    with pytest.raises(ValueError, match="floating-point"):
        K.polynomial_mmd(torch.zeros(40, 32, dtype=torch.int32), y)
    # with valid arguments the first thing to fail on this tier is the missing device
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.polynomial_mmd(x, y, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.kernel_inception_distance(x, y, subsets=2, subset_size=8, device="cpu")


def test_kid_index_checks_before_device_work():
    from v_diffusion import _hip
    from v_diffusion.metrics import kid_score as K
    x, y = torch.zeros(40, 32), torch.zeros(30, 32)
    good_x, good_y = np.zeros((2, 8), dtype=np.int32), np.zeros((2, 8), dtype=np.int32)
    kid = lambda ix, iy: K.kernel_inception_distance(x, y, indices=(ix, iy), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):                      # the good pair passes every host check
        kid(good_x, good_y)
    for bad in (good_x.astype(np.int64), good_x.astype(np.float32), good_x[0], good_x.reshape(2, 2, 4), good_x.tolist(),
                torch.from_numpy(good_x), np.zeros((2, 0), dtype=np.int32)):
        with pytest.raises(ValueError, match="int32 array of shape"):
            kid(bad, good_y)
        with pytest.raises(ValueError, match="int32 array of shape"):
            kid(good_x, bad)
    with pytest.raises(ValueError, match="different numbers of subsets"):
        kid(good_x, np.zeros((3, 8), dtype=np.int32))
    with pytest.raises(ValueError, match="at least 2 rows"):
        kid(np.zeros((2, 1), dtype=np.int32), good_y)
    with pytest.raises(ValueError, match="pair"):
        K.kernel_inception_distance(x, y, indices=good_x[0, 0], device="cpu")
    for n, idx, who in ((40, good_x, "ix"), (30, good_y, "iy")):
        for value in (n, -1, n + 1000, np.iinfo(np.int32).min):
            bad = idx.copy()
            bad[1, 3] = value
            with pytest.raises(ValueError, match=rf"{who} must lie in \[0, {n}\)"):
                kid(bad, good_y) if who == "ix" else kid(good_x, bad)
            with pytest.raises(ValueError, match="must lie in"):
                _hip.kid_indices(bad, n)
        edge = idx.copy()
        edge[1, 3] = n - 1                                                     # the last row is in range
        assert _hip.kid_indices(edge, n) is edge


def test_inception_score_argument_checks_before_device_work():
    from v_diffusion.metrics.inception_score import inception_score
    with pytest.raises(ValueError, match="splits"):
        inception_score(torch.zeros(5, 10), splits=6)
    with pytest.raises(ValueError, match="splits"):
        inception_score(torch.zeros(5, 10), splits=0)
    with pytest.raises(ValueError, match="classes"):
        inception_score(torch.zeros(5, 1), splits=1)
    with pytest.raises(ValueError, match="floating-point"):
        inception_score(torch.zeros(5, 10, dtype=torch.int64), splits=1)
    with pytest.raises(ValueError, match="floating-point"):
        inception_score(torch.zeros(5), splits=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        inception_score(torch.zeros(5, 10), splits=5, device="cpu")
