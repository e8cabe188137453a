"""FID statistics and distance of v_diffusion.metrics.fid_score (csrc/fid.hip) at eval.py's shape, and against the reference-style path.
    python tests/perf_fid.py
Line 1: the statistics pass at N = 50 000, d = 2 048 in batches of 512 (98 vd_fid_accum launches): ms from device events after a
warm-up (mean of 3), fp64 TFLOP/s on the algorithmic 2 N d^2, and the accumulator traffic of 2 * 8 d^2 bytes per launch.
Line 2: the same device tensors through the reference-style path, once: .cpu().numpy() per batch, np.mean / np.cov in fp64 and a
running merge of mean and covariance (reference fid_score.py:106-125), wall clock; the ratio to line 1.
Line 3: calc_fd at d = 2 048 split into its device products and its host eigen-solves, next to the reference formulation
(scipy.linalg.sqrtm of the product) when scipy imports."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "v-diffusion-torch_amd"))
from v_diffusion import _hip as H                       # noqa: E402
from v_diffusion.metrics import fid_score as F          # noqa: E402

dev = torch.device("cuda", 0)
N, D, B = 50000, 2048, 512


def timeit(fn, n=3):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def features():
    g = torch.Generator(device=dev).manual_seed(1)
    mix = torch.randn(64, D, device=dev, generator=g)
    x = 0.5 + torch.rand(D, device=dev, generator=g) + 0.2 * torch.randn(N, D, device=dev, generator=g) \
        + 0.1 * torch.randn(N, 64, device=dev, generator=g) @ mix
    return x.abs().float().contiguous()


def native_pass(batches, shift, total, outer):
    total.zero_(); outer.zero_()
    H.fid_shift(batches[0], shift)
    for b in batches:
        H.fid_accum(b, shift, total, outer)


def reference_style(batches):
    mean, var, count = np.zeros(D), np.zeros((D, D)), 0
    for b in batches:
        act = b.cpu().numpy()
        m, v, n = np.mean(act, axis=0, dtype=np.float64), np.cov(act, rowvar=False, ddof=0, dtype=np.float64), act.shape[0]
        a = n / (count + n)
        if count == 0:
            mean, var = m, v
        else:
            diff = m - mean
            mean = mean + a * diff
            var += a * (v - var)
            var += a * (1 - a) * np.outer(diff, diff)
        count += n
    return mean, var * count / (count - 1)


def main():
    x = features()
    batches = list(x.split(B))
    shift, total = torch.zeros(D, dtype=torch.float64, device=dev), torch.zeros(D, dtype=torch.float64, device=dev)
    outer = torch.zeros(D, D, dtype=torch.float64, device=dev)
    t = timeit(lambda: native_pass(batches, shift, total, outer))
    fl, traffic = 2.0 * N * D * D, 2.0 * 8 * D * D * len(batches)
    print(f"N={N} d={D} batches of {B}: {len(batches)} vd_fid_accum launches {t:8.2f} ms, {fl / t / 1e9:6.2f} fp64 TF/s algorithmic "
          f"(2 N d^2), accumulator traffic {traffic / 1e9:.2f} GB = {traffic / t / 1e9:.2f} TB/s", flush=True)
    mean, cov = F.finalize(shift, total, outer, N)
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()

    reference_style(batches[:2])                                    # warm-up (host allocator, BLAS threads)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rmean, rcov = reference_style(batches)
    t_ref = (time.perf_counter() - t0) * 1e3
    print(f"reference-style .cpu() + np.cov + running merge: {t_ref:9.1f} ms ({t_ref / t:.1f}x the native pass); statistics agree to "
          f"{np.abs(cov - rcov).max():.2e} (cov) {np.abs(mean - rmean).max():.2e} (mean)", flush=True)

    # distance between the statistics of the two halves
    stats = []
    for half in (batches[:49], batches[49:]):
        native_pass(half, shift, total, outer)
        m, c = F.finalize(shift, total, outer, sum(b.shape[0] for b in half))
        stats += [m.cpu().numpy(), c.cpu().numpy()]
    s1, s2 = torch.from_numpy(stats[1]), torch.from_numpy(stats[3])
    F.calc_fd(*stats)                                               # warm-up
    t0 = time.perf_counter()
    fd = F.calc_fd(*stats)
    t_fd = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    w, v = torch.linalg.eigh(s1)
    torch.linalg.eigvalsh(s2)
    t_host = (time.perf_counter() - t0) * 1e3
    q = (v * w.clamp_min(0).pow(0.25)).T.contiguous().to(dev)
    s2d = s2.to(dev)
    r = H.atb_f64(q, q)
    t_dev = timeit(lambda: H.atb_f64(q, q)) + timeit(lambda: H.atb_f64(H.atb_f64(s2d, r), r))
    line = (f"calc_fd d={D}: {t_fd:8.1f} ms in all = {fd:.6f}; host eigen-solves (eigh + eigvalsh) {t_host:8.1f} ms, three device products "
            f"{t_dev:6.2f} ms ({3 * 2.0 * D ** 3 / t_dev / 1e9:.2f} fp64 TF/s)")
    try:
        from scipy import linalg
        t0 = time.perf_counter()
        covmean, _ = linalg.sqrtm(stats[1].dot(stats[3]), disp=False)
        diff = stats[0] - stats[2]
        ref = float(diff.dot(diff) + np.trace(stats[1]) + np.trace(stats[3]) - 2 * np.trace(covmean.real))
        t_sq = (time.perf_counter() - t0) * 1e3
        line += f" | scipy sqrtm formulation {t_sq:9.1f} ms = {ref:.6f} ({t_sq / t_fd:.1f}x)"
    except ImportError:
        line += " | scipy sqrtm formulation: not measured (scipy does not import)"
    print(line, flush=True)


if __name__ == "__main__":
    main()
