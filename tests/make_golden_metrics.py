"""Writes tests/golden/metrics_pr.npz: the reference's precision / recall (v_diffusion/metrics/precision_recall.py) on two seeded
fp16 feature sets, run on the CPU.  Run once where a checkout of the reference exists:

    VDIFF_REFERENCE_ROOT=/path/to/v-diffusion-torch python tests/make_golden_metrics.py

The module is imported by file path (its package __init__ would pull in the FID / Inception code).  CPU torch has no fp16
torch.cdist, so for fp16 CPU operands the script computes it in fp32 and rounds the distances to fp16 -- the dtype the
reference's device path returns.  Contents: x_real [1500, 128], x_gen [1200, 128] (fp16), kth{3,5}_{real,gen} (fp16 radii of
nhood_size 3 and 5) and precision{3,5} / recall{3,5} (calc_pr of gen against real)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "metrics_pr.npz")
D = 128


def feature_sets():
    """real: 12 Gaussian clusters; generated: 8 of them slightly shifted, a little wider plus 3 clusters of its own"""
    rng = np.random.default_rng(20261015)
    centers = rng.normal(0.0, 1.0, (12, D))
    real = centers[rng.integers(0, 12, 1500)] + rng.normal(0.0, 0.35, (1500, D))
    own = rng.normal(0.0, 1.0, (3, D))
    gc = np.concatenate([centers[:8] + rng.normal(0.0, 0.05, (8, D)), own])
    lab = rng.integers(0, 11, 1200)
    gen = gc[lab] + rng.normal(0.0, 0.355, (1200, D))
    return real.astype(np.float16), gen.astype(np.float16)


def main():
    root = os.environ.get("VDIFF_REFERENCE_ROOT")
    path = os.path.join(root or "", "v_diffusion", "metrics", "precision_recall.py")
    if not root or not os.path.exists(path):
        sys.exit("set VDIFF_REFERENCE_ROOT to a checkout of the reference")
    spec = importlib.util.spec_from_file_location("ref_precision_recall", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    cdist = torch.cdist

    def cdist_cpu_half(a, b, *args, **kw):
        if a.dtype == torch.float16 and a.device.type == "cpu":
            return cdist(a.float(), b.float(), *args, **kw).half()
        return cdist(a, b, *args, **kw)
    torch.cdist = cdist_cpu_half

    real, gen = feature_sets()
    out = {"x_real": real, "x_gen": gen}
    for k in (3, 5):
        mr = ref.ManifoldBuilder(features=torch.from_numpy(real), nhood_size=k, row_batch_size=700, col_batch_size=600).manifold
        mg = ref.ManifoldBuilder(features=torch.from_numpy(gen), nhood_size=k, row_batch_size=700, col_batch_size=600).manifold
        p, r = ref.calc_pr(mg, mr, row_batch_size=700, col_batch_size=600, device=torch.device("cpu"))
        out[f"kth{k}_real"], out[f"kth{k}_gen"] = mr.kth.numpy(), mg.kth.numpy()
        out[f"precision{k}"], out[f"recall{k}"] = np.float32(p), np.float32(r)
        print(f"nhood_size {k}: precision {float(p):.4f} recall {float(r):.4f}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
