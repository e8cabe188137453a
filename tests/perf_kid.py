"""KID and Inception Score of v_diffusion.metrics (csrc/kid.hip) at the shapes people report, and KID against the materialising route.
    python tests/perf_kid.py
Line 1: vd_kid_sums at 100 subsets x 1000 rows, d = 2 048, indices already drawn: ms from device events after a warm-up (mean of
3, the index upload included), fp64 TFLOP/s on the algorithmic 2 d per kernel value (m (m - 1) / 2 + m (m - 1) / 2 + m^2 values per
subset: the symmetric halves are not computed), and kernel_inception_distance end to end (draw + upload + launch + host), wall clock.
Line 2: the materialising route on the same GPU and the same subsets: per subset gather the rows, three fp64 torch.matmul, cube,
mask the diagonal, sum; ms, the ratio to line 1 and the largest relative difference of the sums.
Line 3: polynomial_mmd over whole sets of 50 000 x 50 000, d = 2 048 (one launch, 1.22 M tiles; the Gram matrices would be 3 x 20 GB).
Line 4: inception_score at 50 000 x 1 008, 10 splits: ms and the logits' read rate."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "v-diffusion-torch_amd"))
from v_diffusion import _hip as H                                   # noqa: E402
from v_diffusion.metrics import inception_score as I, kid_score as K  # noqa: E402

dev = torch.device("cuda", 0)
N, D, SUBSETS, M, CLASSES = 50000, 2048, 100, 1000, 1008


def timeit(fn, n=3):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def features(seed, shift):
    g = torch.Generator(device=dev).manual_seed(seed)
    mix = torch.randn(64, D, device=dev, generator=g)
    x = shift + torch.rand(D, device=dev, generator=g) + 0.2 * torch.randn(N, D, device=dev, generator=g) \
        + 0.1 * torch.randn(N, 64, device=dev, generator=g) @ mix
    return x.abs().float().contiguous()


def materialised(x, y, ix, iy):
    out = torch.empty(ix.shape[0], 3, dtype=torch.float64, device=dev)
    gamma = 1.0 / x.shape[1]
    for s in range(ix.shape[0]):
        xs, ys = x[ix[s]].double(), y[iy[s]].double()
        for kind, (a, b) in enumerate(((xs, xs), (ys, ys), (xs, ys))):
            k = (gamma * torch.matmul(a, b.T) + 1.0) ** 3
            out[s, kind] = k.sum() - k.diagonal().sum() if kind < 2 else k.sum()
    return out


def main():
    x, y = features(1, 0.5), features(2, 0.55)
    ix, iy = K.subset_indices(N, N, SUBSETS, M, seed=0)
    t = timeit(lambda: H.kid_sums(x, y, ix, iy))
    values = SUBSETS * (M * (M - 1.0) + M * M)
    t0 = time.perf_counter()
    kid = K.kernel_inception_distance(x, y, SUBSETS, M, device=dev)
    t_all = (time.perf_counter() - t0) * 1e3
    print(f"KID {SUBSETS} x {M} d={D}: vd_kid_sums {t:8.2f} ms, {2.0 * D * values / t / 1e9:6.2f} fp64 TF/s algorithmic; "
          f"kernel_inception_distance end to end {t_all:8.1f} ms = {kid.mean:.6e} +- {kid.std:.2e}", flush=True)

    dix, diy = torch.from_numpy(ix).to(dev).long(), torch.from_numpy(iy).to(dev).long()
    t_mat = timeit(lambda: materialised(x, y, dix, diy))
    a, b = H.kid_sums(x, y, ix, iy), materialised(x, y, dix, diy)
    print(f"materialising route (gather, 3 fp64 torch.matmul, cube, sum per subset): {t_mat:8.2f} ms ({t_mat / t:.2f}x the fused launch); "
          f"sums agree to {float(((a - b).abs() / b.abs()).max()):.2e} relative", flush=True)

    t_whole = timeit(lambda: H.kid_sums(x, y), n=1)
    whole = float(N) * (N - 1) + float(N) * N
    print(f"polynomial_mmd {N} x {N} d={D}: {t_whole:9.1f} ms, {2.0 * D * whole / t_whole / 1e9:6.2f} fp64 TF/s algorithmic, "
          f"MMD^2 = {K.polynomial_mmd(x, y, device=dev):.6e}", flush=True)

    g = torch.Generator(device=dev).manual_seed(3)
    logits = (3.0 * torch.randn(N, CLASSES, device=dev, generator=g)).contiguous()
    t_is = timeit(lambda: H.is_scores(logits, 10))
    res = I.inception_score(logits, 10, device=dev)
    print(f"inception_score {N} x {CLASSES}, 10 splits: {t_is:7.3f} ms ({4.0 * N * CLASSES / t_is / 1e6:.1f} GB/s of logits), "
          f"IS = {res.mean:.4f} +- {res.std:.4f}", flush=True)


if __name__ == "__main__":
    main()
