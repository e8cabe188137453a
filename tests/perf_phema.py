"""Post-hoc EMA measurements (not a test).  The sides of each comparison alternate inside one run; each figure is the median of ROUNDS
windows of ITERS calls (device events) with the smallest and largest window beside it, as tests/perf_consistency.py does.

  tail      flat buffers of the CIFAR-10 network's size: (a) vd_adamw_ema with the classic shadow, (b) vd_adamw_emas with two power
            shadows, (c) vd_adamw_ema followed by two torch.Tensor.lerp_ calls
  combine   vd_ema_combine at k = 16 against 16 fp32 ATen ``add_(src, alpha=w)`` passes, in GB/s of source bytes; posthoc_ema from 64
            snapshots on disk end to end, the time of reading and copying the same files alone beside it
  step      the CIFAR-10 B = 128 HotPathTrainer.step with ema_sigma_rels=(0.05, 0.10) against None, a trainer pair alternating

python tests/perf_phema.py [tail] [combine] [step] [--iters N]        (default: all three)"""
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]
import torch
import v_diffusion
from v_diffusion import _hip as H, phema
from bench import build_model, CIFAR

dev = torch.device("cuda", 0)
ITERS = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 50
PARTS = [a for a in sys.argv[1:] if a in ("tail", "combine", "step")] or ["tail", "combine", "step"]
ROUNDS = 7
N = 60_800_000 // 4 * 4


def window(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                       # us per call


def compare(label, iters=ITERS, **sides):
    for f in sides.values():                                      # warm-up: code objects, allocator
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, f in sides.items():                                 # alternate
            us[k].append(window(f, iters))
    print(label + ":  " + "   ".join(f"{k} {statistics.median(v):9.1f} us [{min(v):.1f} .. {max(v):.1f}]" for k, v in us.items()), flush=True)
    return {k: statistics.median(v) for k, v in us.items()}


def tail():
    p, g, m, v, ema, e1, e2 = (torch.randn(N, device=dev) * s for s in (1, 0.01, 0.01, 0.01, 1, 1, 1))
    v.abs_()
    gsq = torch.zeros(1, device=dev)
    H.sumsq(g, gsq)
    rates = [phema.power_ema_rate(100000, phema.sigma_rel_to_gamma(s)) for s in (0.05, 0.10)]
    a = (p, g, m, v, ema, gsq, 1.0, 2e-4, 0.9, 0.999, 1e-8, 0.001, 1 - 0.9 ** 1000, 1 - 0.999 ** 1000, 0.9999)

    def classic():
        H.adamw_ema(*a)

    def fused():
        H.adamw_emas(*a, [e1, e2], rates)

    def classic_then_lerps():
        H.adamw_ema(*a)
        e1.lerp_(p, rates[0])
        e2.lerp_(p, rates[1])
    us = compare(f"tail, n = {N}", a_adamw_ema=classic, b_adamw_emas_2=fused, c_adamw_ema_2_lerp=classic_then_lerps)
    for k, byts in (("a_adamw_ema", 36), ("b_adamw_emas_2", 52), ("c_adamw_ema_2_lerp", 60)):
        print(f"    {k}: {byts} B/parameter -> {byts * N / us[k] / 1e6:.2f} TB/s")


def combine():
    k = 16
    srcs = [torch.randn(N, device=dev) for _ in range(k)]
    w = [float(x) for x in torch.randn(k, dtype=torch.float64)]
    out, ref = torch.empty(N, device=dev), torch.empty(N, device=dev)

    def fused():
        H.ema_combine(out, None, srcs, w)

    def aten():
        ref.zero_()
        for s, x in zip(srcs, w):
            ref.add_(s, alpha=x)
    us = compare(f"combine, k = {k}, n = {N}", iters=max(ITERS // 5, 4), vd_ema_combine=fused, aten_16_add=aten)
    print("    source bytes: " + "   ".join(f"{name} {k * 4 * N / t / 1e3:.0f} GB/s" for name, t in us.items()))
    print(f"    max |fp64-accumulated - fp32 sequential| = {float((out - ref).abs().max()):.3e} (values O(4))")
    del srcs
    # 64 snapshots on disk (32 times x 2 profiles each = 64 sources) -> one profile, end to end
    with tempfile.TemporaryDirectory() as d:
        paths, flats = [], [torch.randn(N), torch.randn(N)]
        files = 32 if shutil.disk_usage(d).free > 24e9 else 4      # (a small scratch disk: fewer files, said in the line printed)
        for i in range(files):
            s = phema.make_snapshot(1000 * (i + 1), (0.05, 0.10), [("w", 0, (N,))], N, flats)
            paths.append(os.path.join(d, f"s{i}.pt"))
            torch.save(s, paths[-1])
        def load_only():                                           # what posthoc_ema reads and copies, without the combination
            for path in paths:
                for flat in torch.load(path, map_location="cpu", mmap=True, weights_only=True)["flat"]:
                    flat.to(dev)
            torch.cuda.synchronize()

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        load = timed(load_only)                                    # (first: it also warms the page cache for the run below)
        load = timed(load_only)
        total = timed(lambda: phema.posthoc_ema(paths, 0.075, chunk=16))
        print(f"posthoc_ema, {files} files x 2 profiles = {2 * files} sources of {N} ({files * 8 * N / 1e9:.1f} GB on disk, page cache warm): {total:.2f} s end to end; "
              f"reading the same files and copying them to the device alone takes {load:.2f} s")


def step():
    from v_diffusion.trainer import HotPathTrainer
    B = 128
    gd = v_diffusion.GaussianDiffusion(v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0), 50, "v", "fixed_medium", "snr_trunc", "mse",
                                       intp_frac=0.3, w_guide=1.0, p_uncond=0.1)
    kw = dict(lr=2e-4, weight_decay=0.001, warmup=1000, grad_norm=1.0, ema_decay=0.9999, use_ema=True)
    plain = HotPathTrainer(build_model(dev, cfg=CIFAR).train(), gd, **kw)
    power = HotPathTrainer(build_model(dev, cfg=CIFAR).train(), gd, ema_sigma_rels=(0.05, 0.10), **kw)
    g = torch.Generator(dev).manual_seed(4321)
    x = torch.rand((B, 3, 32, 32), device=dev, generator=g) * 2 - 1
    y = torch.randint(1, 11, (B,), device=dev, generator=g).float()
    compare(f"CIFAR-10 B = {B} train step", iters=max(ITERS // 5, 4), ema_sigma_rels_None=lambda: plain.step(x, y),
            ema_sigma_rels_2=lambda: power.step(x, y))


for name in PARTS:
    {"tail": tail, "combine": combine, "step": step}[name]()
