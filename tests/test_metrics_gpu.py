"""v_diffusion.metrics on the MI355X: the fused k-NN kernels (csrc/metrics.hip) against an fp64 numpy oracle in this file, and the
precision / recall of the reference on tests/golden/metrics_pr.npz (tests/make_golden_metrics.py).

Tolerance model: the kernels compute d2 = |x|^2 + |y|^2 - 2 x.y in fp32 from fp16 operands; |d2 - d2_fp64| <= 1e-5 (|x|^2 + |y|^2).
Decisions (fp16 rounding of a radius, a hit) are compared exactly wherever the fp64 value is farther than that band from the
decision boundary, and the number of disagreements is bounded by the number of rows inside the band."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
REL = 1e-5


def clustered(n, d, seed, k=16, spread=0.3, scale=1.0):
    rng = np.random.default_rng(seed)
    centers = rng.normal(0.0, scale, (k, d))
    x = centers[rng.integers(0, k, n)] + rng.normal(0.0, spread * scale, (n, d))
    return x.astype(np.float16)


def d2_fp64(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    xx, yy = (x * x).sum(1), (y * y).sum(1)
    return np.maximum(xx[:, None] + yy[None, :] - 2.0 * x @ y.T, 0.0), xx, yy


def kth_gpu(x, y, kth):
    from v_diffusion import _hip
    q = _hip.features_f16(torch.from_numpy(x).to(DEV))
    c = q if y is None else _hip.features_f16(torch.from_numpy(y).to(DEV))
    return _hip.knn_kth_f16(q, _hip.rows_sqnorm_f16(q), c, _hip.rows_sqnorm_f16(c), kth).cpu().numpy().astype(np.float64)


def check_kth(x, y, kth, got):
    """got (fp32 distances) against fp64: d2 within the band; the fp16 rounding exact outside it"""
    d2, xx, yy = d2_fp64(x, x if y is None else y)
    ref = np.sort(d2, axis=1)[:, kth - 1]
    tol = REL * (xx + yy.max())
    err = np.abs(got ** 2 - ref)
    assert (err <= tol).all(), f"kth={kth}: worst d2 error {(err - tol).max():.3e} over the band"
    lo = np.sqrt(np.maximum(ref - tol, 0)).astype(np.float16)
    hi = np.sqrt(ref + tol).astype(np.float16)
    sure = lo == hi
    g16 = got.astype(np.float32).astype(np.float16)
    assert (g16[sure] == lo[sure]).all(), f"kth={kth}: fp16 radius differs outside the rounding band"
    return sure


def hit_bands(d2, xx, yy, r):
    """fp64 decision per row for 'some j: sqrt(d2_ij) <= r_j': (certain hit, certain miss); the rest lie in the band"""
    r2 = r.astype(np.float64) ** 2
    tol = REL * (xx[:, None] + yy[None, :]) + 2.0 ** -22 * r2[None, :]
    m = d2 - r2[None, :]
    return (m < -tol).any(1), (m > tol).all(1)


@pytest.mark.parametrize("n,d,kth", [(n, d, k) for n, d in [(1000, 4096), (777, 200), (2048, 64), (5, 3)] for k in (2, 4, 8, 16)
                                     if k <= n])
def test_radii_against_fp64(n, d, kth):
    x = clustered(n, d, seed=n + d)
    got = kth_gpu(x, None, kth)
    sure = check_kth(x, None, kth, got)
    assert sure.mean() > 0.5                 # the exact fp16 comparison covers most rows


@pytest.mark.parametrize("kth,c", [(4, 4), (4, 3), (8, 9), (8, 7), (16, 16), (2, 1)])
def test_multiplicity(kth, c):
    """every row repeated c times: kth <= c gives exactly 0; kth = c + 1 the distance to the nearest other row"""
    base = clustered(60, 96, seed=7)
    x = np.repeat(base, c, axis=0)
    got = kth_gpu(x, None, kth)
    if kth <= c:
        assert (got == 0).all()
    else:
        d2, xx, _ = d2_fp64(x, base)
        d2[np.arange(len(x)), np.arange(len(x)) // c] = np.inf
        if kth == c + 1:
            ref = d2.min(1)
            assert (np.abs(got ** 2 - ref) <= REL * (xx + xx.max())).all()
        check_kth(x, None, kth, got)


@pytest.mark.parametrize("nq,nc,kth", [(4, None, 4), (16, None, 16), (127, None, 4), (129, None, 8), (255, None, 16),
                                       (257, None, 4), (129, 127, 4), (1, 300, 16), (300, 1, 1), (130, 16, 16)])
def test_tails_and_cross_sets(nq, nc, kth):
    x = clustered(nq, 128, seed=nq)
    y = None if nc is None else clustered(nc, 128, seed=1000 + nc)
    got = kth_gpu(x, y, kth)
    check_kth(x, y, kth, got)


def test_coverage_against_fp64_and_calc_pr():
    from v_diffusion.metrics import ManifoldBuilder, calc_pr
    from v_diffusion import _hip
    real = clustered(1500, 256, seed=11, spread=0.35)
    # half on the real set's centres (same seed) with another spread, half on centres of its own
    gen = np.concatenate([clustered(550, 256, seed=11, spread=0.38), clustered(550, 256, seed=12, spread=0.3)])[::-1].copy()
    mr = ManifoldBuilder(features=torch.from_numpy(real), nhood_size=3).manifold
    mg = ManifoldBuilder(features=torch.from_numpy(gen), nhood_size=3).manifold
    p, r = calc_pr(mg, mr, 10000, 10000, DEV)
    assert p.dtype == torch.float32 and p.dim() == 0 and p.device.type == "cpu"
    for q, s, m_s, got in ((gen, real, mr, float(p)), (real, gen, mg, float(r))):
        d2, xx, yy = d2_fp64(q, s)
        sure_hit, sure_miss = hit_bands(d2, xx, yy, m_s.kth.numpy())
        qd = _hip.features_f16(torch.from_numpy(q).to(DEV))
        sd = _hip.features_f16(torch.from_numpy(s).to(DEV))
        hits = _hip.manifold_hits_f16(qd, _hip.rows_sqnorm_f16(qd), sd, _hip.rows_sqnorm_f16(sd),
                                      m_s.kth.to(DEV, torch.float32)).cpu().numpy().astype(bool)
        assert hits[sure_hit].all() and not hits[sure_miss].any()
        band = (~sure_hit & ~sure_miss).sum()
        assert abs(got - hits.mean()) < 1e-6
        assert abs(got - sure_hit.mean()) <= band / len(q) + 1e-6
        assert 0.05 < got < 0.99


def test_full_scale_no_nxn_buffer_and_bitwise_repeatable():
    from v_diffusion.metrics import ManifoldBuilder, calc_pr
    g = torch.Generator(device=DEV).manual_seed(5)
    centers = torch.randn(400, 4096, device=DEV, generator=g)

    def feats(n):
        idx = torch.randint(0, 400, (n,), device=DEV, generator=g)
        return (centers[idx] + 0.5 * torch.randn(n, 4096, device=DEV, generator=g)).half().cpu()
    f_real, f_gen = feats(50000), feats(40000)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    b1 = ManifoldBuilder(features=f_real, nhood_size=3)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 2 << 30
    m_real = b1.manifold
    m_gen = ManifoldBuilder(features=f_gen, nhood_size=3).manifold
    p1, r1 = calc_pr(m_gen, m_real, 10000, 10000, None)
    del b1
    m_real2 = ManifoldBuilder(features=f_real, nhood_size=3).manifold
    p2, r2 = calc_pr(m_gen, m_real2, 10000, 10000, None)
    assert torch.equal(m_real.kth, m_real2.kth) and float(p1) == float(p2) and float(r1) == float(r2)

    rng = np.random.default_rng(0)
    rows = rng.choice(50000, 64, replace=False)
    xr, xa = f_real.numpy(), f_real.numpy()
    d2, xx, yy = d2_fp64(xr[rows], xa)
    ref = np.sort(d2, axis=1)[:, 3]
    got = m_real.kth.numpy()[rows].astype(np.float64)
    tol = REL * (xx + yy.max())
    lo = np.sqrt(np.maximum(ref - tol, 0)).astype(np.float16)
    hi = np.sqrt(ref + tol).astype(np.float16)
    sure = lo == hi
    assert (m_real.kth.numpy()[rows][sure] == lo[sure]).all()
    assert (np.abs(got - np.sqrt(ref)) <= 2.0 ** -9 * np.sqrt(ref) + 1e-6).all()

    # hit flags of 64 generated rows (the precision direction) against fp64
    from v_diffusion import _hip
    grows = rng.choice(40000, 64, replace=False)
    d2, xx, yy = d2_fp64(f_gen.numpy()[grows], xa)
    sure_hit, sure_miss = hit_bands(d2, xx, yy, m_real.kth.numpy())
    qd = _hip.features_f16(f_gen[grows].to(DEV))
    sd = _hip.features_f16(f_real.to(DEV))
    hits = _hip.manifold_hits_f16(qd, _hip.rows_sqnorm_f16(qd), sd, _hip.rows_sqnorm_f16(sd),
                                  m_real.kth.to(DEV, torch.float32)).cpu().numpy().astype(bool)
    assert hits[sure_hit].all() and not hits[sure_miss].any()
    assert 0.0 <= float(p1) <= 1.0 and 0.0 <= float(r1) <= 1.0


def test_reference_golden():
    from v_diffusion.metrics import Manifold, ManifoldBuilder, calc_pr
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics_pr.npz"))
    xr, xg = g["x_real"], g["x_gen"]
    for k in (3, 5):
        for x, name in ((xr, "real"), (xg, "gen")):
            kth = ManifoldBuilder(features=torch.from_numpy(x), nhood_size=k).kth.numpy()
            ref = g[f"kth{k}_{name}"]
            ulp = np.spacing(np.abs(ref)).astype(np.float64)
            assert (np.abs(kth.astype(np.float64) - ref.astype(np.float64)) <= 5 * ulp).all(), (k, name)
        mr = Manifold(torch.from_numpy(xr), torch.from_numpy(g[f"kth{k}_real"]))
        mg = Manifold(torch.from_numpy(xg), torch.from_numpy(g[f"kth{k}_gen"]))
        p, r = calc_pr(mg, mr, 700, 600, DEV)
        for q, s, rad, got, want in ((xg, xr, g[f"kth{k}_real"], float(p), float(g[f"precision{k}"])),
                                     (xr, xg, g[f"kth{k}_gen"], float(r), float(g[f"recall{k}"]))):
            # the reference rounds each distance to fp16: its band is an fp16 ulp of the distance wide
            d = np.sqrt(d2_fp64(q, s)[0])
            m = d - rad.astype(np.float64)[None, :]
            w = np.spacing(d.astype(np.float16)).astype(np.float64) + REL * d
            band = (~((m < -w).any(1)) & ~((m > w).all(1))).sum()
            assert abs(got - want) <= band / len(q) + 1e-6, (k, got, want, band)


def test_input_validation_on_device():
    from v_diffusion.metrics import ManifoldBuilder
    bad = torch.from_numpy(clustered(50, 64, seed=1))
    bad[3, 5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ManifoldBuilder(features=bad, nhood_size=3)
    with pytest.raises(ValueError, match="nearest neighbour"):
        ManifoldBuilder(features=torch.from_numpy(clustered(3, 64, seed=1)), nhood_size=3)
