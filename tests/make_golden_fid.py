"""Writes tests/golden/fid_stats.npz: the reference's FID statistics and distances (v_diffusion/metrics/fid_score.py) on seeded
feature sets, run on the CPU.  Run once where a checkout of the reference exists:

    PYTHONDONTWRITEBYTECODE=1 VDIFF_REFERENCE_ROOT=/path/to/v-diffusion-torch python tests/make_golden_fid.py

The module is loaded by file path under a throw-away package name with stub modules for what it imports and this run does not
use (torchvision's transforms, requests when absent, the sibling Inception network).  Contents:
  x_a [1000, 64], x_b [800, 64]    fp32 feature sets (positive, non-zero means, decaying spectrum; values representable in fp16
                                   so that the file stays small)
  batches                          the uneven batch sizes the sets were fed in (130, 1, 257, rest)
  mean_a, cov_a, mean_b, cov_b     the reference's InceptionStatistics result on each (stand-in model x -> [x[:, :, None, None]])
  fd_ab, gap_ab                    the reference's calc_fd(A, B); |that - the fp64 eigen formulation in numpy (fd_eigen below)|
  rd_mean1, rd_cov1_tril, rd_mean2, rd_cov2_tril
                                   a rank-deficient pair at d = 192 (N1 = 150 < d, N2 = 1000): means and the packed lower triangles
                                   (np.tril_indices order) of the exactly symmetric covariances
  fd_rd, gap_rd                    as above for that pair"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fid_stats.npz")
BATCHES = (130, 1, 257)


def fd_eigen(mu1, s1, mu2, s2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum sqrt(max(lambda(R S2 R), 0)), R = S1^(1/2) from a symmetric eigen-decomposition"""
    w, v = np.linalg.eigh(s1)
    r = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh((m + m.T) * 0.5)
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def features(n, d, seed, offset):
    """positive features: a decaying spectrum mixed by a random rotation, shifted away from 0, rounded to fp16-representable fp32"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    scale = 0.5 * 0.93 ** np.arange(d)
    x = (rng.normal(size=(n, d)) * scale) @ q.T + offset + 0.3 * rng.random(d)
    x = np.abs(x)
    return x.astype(np.float16).astype(np.float32)


def load_reference():
    root = os.environ.get("VDIFF_REFERENCE_ROOT")
    path = os.path.join(root or "", "v_diffusion", "metrics", "fid_score.py")
    if not root or not os.path.exists(path):
        sys.exit("set VDIFF_REFERENCE_ROOT to a checkout of the reference")

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Anything:
        def __init__(self, *a, **k):
            pass

    try:
        import torchvision  # noqa: F401
    except ImportError:
        tr = stub("torchvision.transforms", Compose=_Anything, Resize=_Anything, Normalize=_Anything, ToTensor=_Anything,
                  InterpolationMode=types.SimpleNamespace(BILINEAR="bilinear"))
        stub("torchvision", transforms=tr)
    try:
        import requests  # noqa: F401
    except ImportError:
        stub("requests")
    pkg = stub("_ref_fid_pkg")
    pkg.__path__ = []
    stub("_ref_fid_pkg.inception", InceptionV3=type("InceptionV3", (), {"BLOCK_INDEX_BY_DIM": {64: 0, 192: 1, 768: 2, 2048: 3}}))
    spec = importlib.util.spec_from_file_location("_ref_fid_pkg.fid_score", path)
    ref = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = ref
    spec.loader.exec_module(ref)
    return ref


class StandIn(torch.nn.Module):
    def forward(self, x):
        return [x[:, :, None, None]]


def reference_statistics(ref, x):
    stats = ref.InceptionStatistics(model=StandIn(), activation_dim=x.shape[1], device=torch.device("cpu"))
    i = 0
    for b in BATCHES + (x.shape[0] - sum(BATCHES),):
        stats(torch.from_numpy(x[i:i + b]))
        i += b
    mean, cov = stats.get_statistics()
    return mean.copy(), cov.copy()


def main():
    ref = load_reference()
    out = {"batches": np.array(BATCHES, dtype=np.int64)}
    xa, xb = features(1000, 64, 20261017, 1.5), features(800, 64, 20261018, 1.4)
    out["x_a"], out["x_b"] = xa, xb
    out["mean_a"], out["cov_a"] = reference_statistics(ref, xa)
    out["mean_b"], out["cov_b"] = reference_statistics(ref, xb)
    pairs = {"ab": (out["mean_a"], out["cov_a"], out["mean_b"], out["cov_b"])}

    y1, y2 = features(150, 192, 20261019, 1.5).astype(np.float64), features(1000, 192, 20261020, 1.45).astype(np.float64)
    stats = []
    for y in (y1, y2):
        cov = np.cov(y, rowvar=False)
        stats += [y.mean(axis=0), (cov + cov.T) * 0.5]
    pairs["rd"] = tuple(stats)
    il = np.tril_indices(192)
    out["rd_mean1"], out["rd_cov1_tril"], out["rd_mean2"], out["rd_cov2_tril"] = stats[0], stats[1][il], stats[2], stats[3][il]

    for name, p in pairs.items():
        fd = float(ref.calc_fd(*p))
        out[f"fd_{name}"] = np.float64(fd)
        out[f"gap_{name}"] = np.float64(abs(fd - fd_eigen(*p)))
        print(f"{name}: reference calc_fd {fd:.15g}, eigen formulation off by {out[f'gap_' + name]:.3e} "
              f"({out[f'gap_' + name] / (np.trace(p[1]) + np.trace(p[3])):.3e} of the traces)")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
