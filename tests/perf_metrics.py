"""Fused k-NN passes of v_diffusion.metrics (csrc/metrics.hip) at eval.py's shape, and against the reference-style path.
    python tests/perf_metrics.py
Line 1: radius pass (kth = nhood_size + 1 = 4) and coverage pass at N = 50 000, D = 4 096: ms from device events after a warm-up,
algorithmic TFLOP/s = 2 N^2 D / time, and its share of the 2.5 PF dense fp16 spec peak.
Line 2: both passes at N = 20 000 next to the reference's path at that size (torch.cdist on the GPU in 10 000 x 10 000 fp16 blocks,
.cpu(), CPU kthvalue of each fp32-widened 10 000-row band: reference precision_recall.py:50-62 and :156-164)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "v-diffusion-torch_amd"))
from v_diffusion import _hip as H        # noqa: E402

dev = torch.device("cuda", 0)
PEAK = 2.5e15


def timeit(fn, n=3):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def feats(n, d, g):
    centers = torch.randn(256, d, device=dev, generator=g)
    idx = torch.randint(0, 256, (n,), device=dev, generator=g)
    return H.features_f16((centers[idx] + 0.5 * torch.randn(n, d, device=dev, generator=g)).half())


def fused(n, d=4096, kth=4):
    g = torch.Generator(device=dev).manual_seed(1)
    x = feats(n, d, g)
    sq = H.rows_sqnorm_f16(x)
    kt = H.knn_kth_f16(x, sq, x, sq, kth)
    r = kt.half().float()
    t_k = timeit(lambda: H.knn_kth_f16(x, sq, x, sq, kth))
    t_h = timeit(lambda: H.manifold_hits_f16(x, sq, x, sq, r))
    return x, t_k, t_h


def reference_style(x, kth=4, blk=10000):
    out = []
    for rb in x.split(blk):
        band = torch.cat([torch.cdist(rb.unsqueeze(0), cb.unsqueeze(0)).squeeze(0).cpu() for cb in x.split(blk)], dim=1)
        out.append(band.float().kthvalue(kth, dim=1).values.half())
    return torch.cat(out)


def main():
    n = 50000
    _, t_k, t_h = fused(n)
    fl = 2.0 * n * n * 4096
    print(f"N={n} D=4096 kth=4: radius {t_k:8.2f} ms {fl / t_k / 1e9:6.1f} TF/s ({fl / t_k / 1e-3 / PEAK:.3f} of peak) | "
          f"coverage {t_h:8.2f} ms {fl / t_h / 1e9:6.1f} TF/s ({fl / t_h / 1e-3 / PEAK:.3f} of peak)", flush=True)
    n = 20000
    x, t_k, t_h = fused(n)
    xs = x[:, :4096].contiguous()
    reference_style(xs[:2000])                 # warm-up (cdist kernels, host allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reference_style(xs)
    torch.cuda.synchronize()
    t_ref = (time.perf_counter() - t0) * 1e3
    print(f"N={n} D=4096 kth=4: radius {t_k:8.2f} ms | coverage {t_h:8.2f} ms | reference-style cdist + .cpu() + kthvalue "
          f"{t_ref:9.1f} ms ({t_ref / t_k:.0f}x the fused radius pass)", flush=True)


if __name__ == "__main__":
    main()
