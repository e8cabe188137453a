"""v_diffusion.metrics.fid_score on the MI355X: the fp64 statistics and product kernels (csrc/fid.hip) against fp64 numpy, and
the statistics / distances of the reference recorded in tests/golden/fid_stats.npz (tests/make_golden_fid.py).

Tolerance model of the statistics (u = 2^-53, N rows in total, truth covariance t and mean mu from np.cov(ddof=1) / np.mean of
the fp64 copy): the kernel forms x - shift in fp64 and its products are exact, so only the sums round; a sum of N terms carries
at most N u sum|terms|, the mean |(x_a - s_a)(x_b - s_b)| is at most sqrt(t_aa t_bb) up to the shift, and a factor 8 covers the
shift and the finalise step:
    |cov_ab - t_ab|  <= 8 N u sqrt(t_aa t_bb)
    |mean_a - mu_a|  <= 8 N u sqrt(t_aa) + 2^-52 |mu_a|
Products: |C_ij - (A^T B)_ij| <= 2 k u sum_k |A_ki| |B_kj|.
Distance: against the fp64 eigen formulation evaluated in numpy here (fd_eigen), the native value may be off by the larger of
10 x the reference's own gap to that formulation (recorded in the fixture; the factor allows for the device products summing in
another order than LAPACK's) and the floor 64 d u (tr S1 + tr S2); the recorded reference value must lie within the same amount."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "fid_stats.npz")) as g:
        g = {k: g[k] for k in g.files}
    il = np.tril_indices(192)
    for i in (1, 2):
        c = np.zeros((192, 192))
        c[il] = g[f"rd_cov{i}_tril"]
        g[f"rd_cov{i}"] = c + np.tril(c, -1).T
    return g


def fd_eigen(mu1, s1, mu2, s2):
    w, v = np.linalg.eigh(s1)
    r = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh((m + m.T) * 0.5)
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def make_features(n, d, seed):
    rng = np.random.default_rng(seed)
    scale = 0.05 + rng.random(d)
    mix = rng.normal(size=(8, d))
    x = 1.0 + rng.random(d) + scale * rng.normal(size=(n, d)) + 0.3 * rng.normal(size=(n, 8)) @ mix
    return x.astype(np.float32)


def split(x, sizes):
    assert sum(sizes) == x.shape[0]
    out, i = [], 0
    for b in sizes:
        out.append(x[i:i + b])
        i += b
    return out


def device_stats(batches, ldx=None):
    """(mean, cov) as numpy from vd_fid_shift / vd_fid_accum over the batches and fid_score.finalize"""
    from v_diffusion import _hip
    from v_diffusion.metrics import fid_score as F
    d = batches[0].shape[1]
    shift, total = torch.zeros(d, dtype=torch.float64, device=DEV), torch.zeros(d, dtype=torch.float64, device=DEV)
    outer = torch.zeros(d, d, dtype=torch.float64, device=DEV)
    count = 0
    for b in batches:
        x = torch.from_numpy(np.ascontiguousarray(b)).to(DEV)
        if ldx is not None:
            wide = torch.full((x.shape[0], ldx), float("nan"), dtype=torch.float32, device=DEV)   # the padding is never read
            wide[:, :d] = x
            x = wide[:, :d]
            assert x.stride(0) == ldx
        if count == 0:
            _hip.fid_shift(x, shift)
        _hip.fid_accum(x, shift, total, outer)
        count += x.shape[0]
    mean, cov = F.finalize(shift, total, outer, count)
    return mean.cpu().numpy(), cov.cpu().numpy()


def check_stats(what, mean, cov, mu, t, n, extra_mean=0.0, extra_cov=0.0):
    sd = np.sqrt(np.diag(t))
    cov_tol = 8.0 * n * U * np.outer(sd, sd) + extra_cov
    mean_tol = 8.0 * n * U * sd + 2.0 ** -52 * np.abs(mu) + extra_mean
    ec, em = np.abs(cov - t), np.abs(mean - mu)
    print(f"{what}: N = {n}, worst cov error / bound = {np.max(ec / cov_tol):.3e}, worst mean error / bound = {np.max(em / mean_tol):.3e}")
    assert (ec <= cov_tol).all(), f"{what}: covariance off by {np.max(ec / cov_tol):.3e} x the bound"
    assert (em <= mean_tol).all(), f"{what}: mean off by {np.max(em / mean_tol):.3e} x the bound"
    return cov_tol


def truth(x):
    x = x.astype(np.float64)
    return x.mean(axis=0), np.cov(x, rowvar=False, ddof=1)


# d = 16 / 80 / 144: below one 64-column tile, a partial last tile; the other rows are the smallest shapes that reach several tiles,
# row counts off the k step (1 included), accumulation across calls and a strided input
@pytest.mark.parametrize("d,sizes,ldx", [(64, [1, 1], None), (64, [3, 5], None), (192, [130, 1, 257, 512], None), (2048, [37], None),
                                         (2048, [512, 512], None), (64, [257], 80), (16, [5, 2], None), (80, [70], None),
                                         (144, [17, 33], 148)])
def test_statistics_against_fp64_numpy(d, sizes, ldx):
    n = sum(sizes)
    x = make_features(n, d, seed=1000 * d + n)
    mu, t = truth(x)
    mean, cov = device_stats(split(x, sizes), ldx)
    tol = check_stats(f"d={d} {sizes} ldx={ldx}", mean, cov, mu, t, n)
    assert np.array_equal(cov, cov.T), "covariance is not bitwise symmetric"
    mean2, cov2 = device_stats(split(x, sizes), ldx)
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2), "a second identical run differs"
    other = [n] if len(sizes) > 1 else ([n - n // 3, n // 3] if n >= 3 else [n])
    if other != sizes:
        mean3, cov3 = device_stats(split(x, other), ldx)
        check_stats(f"d={d} {other} ldx={ldx}", mean3, cov3, mu, t, n)
        assert (np.abs(cov3 - cov) <= tol).all(), "two batch splits disagree beyond the bound"


def test_shift_keeps_the_covariance_of_offset_data():
    """columns 100 + 0.01 z: raw second moments would carry N u 1e4 ~ 1e-9 against covariance entries of 1e-4"""
    n, d = 1000, 64
    rng = np.random.default_rng(7)
    x = (100.0 + 0.01 * rng.normal(size=(n, d))).astype(np.float32)
    centred = x.astype(np.float64) - 100.0                      # exact: the truth carries no centring error of its own
    mu, t = 100.0 + centred.mean(axis=0), np.cov(centred, rowvar=False, ddof=1)
    for sizes in ([n], [130, 1, 257, 612]):
        mean, cov = device_stats(split(x, sizes))
        check_stats(f"offset data {sizes}", mean, cov, mu, t, n)


@pytest.mark.parametrize("k,m,n", [(64, 64, 64), (192, 64, 192), (148, 192, 16)])
def test_atb_f64_against_numpy(k, m, n):
    from v_diffusion import _hip
    rng = np.random.default_rng(k + m + n)
    a, b = rng.normal(size=(k, m)), rng.normal(size=(k, n)) + 0.25
    c = _hip.atb_f64(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    tol = 2.0 * k * U * (np.abs(a).T @ np.abs(b))
    err = np.abs(c - a.T @ b)
    print(f"atb {k}x{m}x{n}: worst error / bound = {np.max(err / tol):.3e}")
    assert c.shape == (m, n) and (err <= tol).all()
    # strided operands: the same product out of wider buffers
    wa, wb = torch.zeros(k, m + 6, dtype=torch.float64, device=DEV), torch.zeros(k, n + 2, dtype=torch.float64, device=DEV)
    wa[:, :m], wb[:, :n] = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    assert np.array_equal(_hip.atb_f64(wa[:, :m], wb[:, :n]).cpu().numpy(), c)


@pytest.mark.parametrize("pair", ["ab", "rd", "same"])
def test_distance_against_the_eigen_formulation_and_the_reference(golden, pair):
    from v_diffusion.metrics import fid_score as F
    g = golden
    if pair == "ab":
        args, ref, gap = (g["mean_a"], g["cov_a"], g["mean_b"], g["cov_b"]), float(g["fd_ab"]), float(g["gap_ab"])
    elif pair == "rd":
        args, ref, gap = (g["rd_mean1"], g["rd_cov1"], g["rd_mean2"], g["rd_cov2"]), float(g["fd_rd"]), float(g["gap_rd"])
    else:
        args, ref, gap = (g["mean_a"], g["cov_a"], g["mean_a"], g["cov_a"]), 0.0, 0.0      # identical statistics: distance 0
    d = args[0].shape[0]
    allowed = max(10.0 * gap, 64.0 * d * U * (np.trace(args[1]) + np.trace(args[3])))
    fd = F.calc_fd(*args)
    yard = fd_eigen(*args)
    print(f"{pair}: native {fd:.15g}, eigen formulation {yard:.15g}, reference {ref:.15g}; |native - yardstick| = {abs(fd - yard):.3e}, "
          f"|native - reference| = {abs(fd - ref):.3e}, allowed {allowed:.3e}")
    assert isinstance(fd, float)
    assert abs(fd - yard) <= allowed
    assert abs(fd - ref) <= allowed


class StandIn(torch.nn.Module):
    """x [B, d] -> [x as a B x d x 1 x 1 map]"""

    def forward(self, x):
        return [x[:, :, None, None]]


class Maps(torch.nn.Module):
    """x [B, d, H, W] -> [x]"""

    def forward(self, x):
        return [x]


def fixture_batches(g, x):
    sizes = [int(b) for b in g["batches"]]
    return split(x, sizes + [x.shape[0] - sum(sizes)])


def test_inception_statistics_end_to_end(golden):
    from v_diffusion.metrics import fid_score as F
    g = golden
    xa = g["x_a"]
    n = xa.shape[0]
    stats = F.InceptionStatistics(model=StandIn(), activation_dim=64, device=DEV)
    with pytest.raises(AssertionError):
        stats.get_statistics()                                  # count = 0
    for b in fixture_batches(g, xa):
        assert stats(torch.from_numpy(b).to(DEV)) is None
    assert stats.count == n and isinstance(stats.count, int)
    mean, cov = stats.get_statistics()
    assert mean.dtype == np.float64 and cov.dtype == np.float64 and mean.shape == (64,) and cov.shape == (64, 64)
    check_stats("fixture set A against the reference", mean, cov, g["mean_a"], g["cov_a"], n)

    # update(features) is forward without the model; reset() clears everything
    direct = F.InceptionStatistics(model=StandIn(), activation_dim=64, device=DEV)
    for b in fixture_batches(g, xa):
        direct.update(torch.from_numpy(b))
    mean_u, cov_u = direct.get_statistics()
    assert np.array_equal(mean_u, mean) and np.array_equal(cov_u, cov)
    stats.reset()
    assert stats.count == 0
    stats(torch.from_numpy(xa[:1]).to(DEV))
    with pytest.raises(AssertionError):
        stats.get_statistics()                                  # count = 1
    stats.reset()
    for b in fixture_batches(g, xa):
        stats(torch.from_numpy(b).to(DEV))
    mean_r, cov_r = stats.get_statistics()
    assert np.array_equal(mean_r, mean) and np.array_equal(cov_r, cov)

    # 2 x 2 maps whose spatial mean is set A up to the fp32 rounding of a +- e.  The truth pools in fp64 without rounding; the module
    # rounds the pooled value once to fp32, |e_ia| <= 2^-24 |x_ia|, which moves the mean by at most E_a = 2^-24 max_i |x_ia| and, by
    # Cauchy-Schwarz on the centred sums, cov_ab by at most c (E_a sd_b + sd_a E_b) + c^2 E_a E_b with c = sqrt(N / (N - 1))
    rng = np.random.default_rng(11)
    e1, e2 = (0.2 * rng.normal(size=xa.shape)).astype(np.float32), (0.1 * rng.normal(size=xa.shape)).astype(np.float32)
    maps = np.stack([xa + e1, xa - e1, xa + e2, xa - e2], axis=-1).reshape(n, 64, 2, 2).astype(np.float32)
    pooled = maps.astype(np.float64).mean(axis=(2, 3))
    mu, t = pooled.mean(axis=0), np.cov(pooled, rowvar=False, ddof=1)
    big = 2.0 ** -24 * np.abs(pooled).max(axis=0)
    sd, c = np.sqrt(np.diag(t)), np.sqrt(n / (n - 1.0))
    extra_cov = c * (np.outer(big, sd) + np.outer(sd, big)) + c * c * np.outer(big, big)
    pooling = F.InceptionStatistics(model=Maps(), activation_dim=64, device=DEV)
    for b in fixture_batches(g, maps):
        pooling(torch.from_numpy(b).to(DEV))
    mean_p, cov_p = pooling.get_statistics()
    check_stats("2 x 2 maps", mean_p, cov_p, mu, t, n, extra_mean=big, extra_cov=extra_cov)


def test_validation_on_the_device():
    from v_diffusion import _hip
    from v_diffusion.metrics import fid_score as F
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    with pytest.raises(_hip.HipError, match="multiple of 16"):
        _hip.fid_accum(torch.ones(4, 24, device=DEV), z(24), z(24), z(24, 24))
    with pytest.raises(_hip.HipError, match="multiple of 16"):
        _hip.fid_shift(torch.ones(4, 8, device=DEV), z(8))
    with pytest.raises(_hip.HipError, match="multiple of 4"):
        _hip.fid_accum(torch.ones(4, 18, device=DEV)[:, :16], z(16), z(16), z(16, 16))
    with pytest.raises(_hip.HipError, match="multiples of 16"):
        _hip.atb_f64(z(8, 24), z(8, 16))
    with pytest.raises(_hip.HipError):
        _hip.fid_accum(torch.ones(4, 16), z(16), z(16), z(16, 16))               # CPU tensor
    with pytest.raises(ValueError, match="activation_dim"):
        F.InceptionStatistics(model=StandIn(), activation_dim=24, device=DEV)
    stats = F.InceptionStatistics(model=StandIn(), activation_dim=128, device=DEV)
    with pytest.raises(ValueError, match="activation_dim"):
        stats(torch.ones(4, 64, device=DEV))                                     # the model returns 64 activations per sample
    assert stats.count == 0

    # non-finite activations propagate into row / column c and entry c only, and get_statistics() refuses the result
    x = make_features(40, 64, seed=3)
    clean = F.InceptionStatistics(model=StandIn(), activation_dim=64, device=DEV)
    clean.update(torch.from_numpy(x))
    mean0, cov0 = clean.get_statistics()
    for bad in (float("nan"), float("inf")):
        y = x.copy()
        y[5, 9] = bad
        stats = F.InceptionStatistics(model=StandIn(), activation_dim=64, device=DEV)
        stats.update(torch.from_numpy(y))
        with pytest.raises(ValueError, match="not finite"):
            stats.get_statistics()
        mean, cov = (v.cpu().numpy() for v in F.finalize(stats._shift, stats._sum, stats._outer, stats.count))
        hit = np.zeros((64, 64), dtype=bool)
        hit[9, :] = hit[:, 9] = True
        assert not np.isfinite(cov[hit]).any() and not np.isfinite(mean[9])
        assert np.array_equal(cov[~hit], cov0[~hit]) and np.array_equal(np.delete(mean, 9), np.delete(mean0, 9))
