"""Dynamic thresholding in the DPM-Solver++ sampler on the CIFAR config (not a test): per-launch time of vd_solver_step_dyn beside
vd_solver_step(clip=1) in the same process -- at 128 x 3 x 32 x 32 and 64 x 3 x 64 x 64, guided, and at batch 1, where one workgroup
works alone -- and end-to-end images/s and ms/step of p_sample_solver, static clip against dynamic threshold, at 20 and at 50 steps,
guided, B = 128.  The dynamic launch reads a sample's input rows five times (four selection passes and the update) where the static
one reads them once; the bar is relative to the static path of the same run: at B = 128 the time it adds per step (difference of the
launch medians) must be smaller than the static chain's own run-to-run spread of ms/step.  Every figure is taken ROUNDS times, the
versions alternating, and printed as median [min .. max].
python tests/perf_threshold.py [rounds]"""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]
import torch
import v_diffusion
from v_diffusion import _hip as H
from bench import build_model, CIFAR

dev = torch.device("cuda", 0)
W, Q = 1.5, 0.995
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
fn = v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0)


def timed(f, iters, warm=20):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v, unit, scale=1.0):
    return f"{statistics.median(v) * scale:8.2f} {unit} [{min(v) * scale:.2f} .. {max(v) * scale:.2f}]"


# ---- the two update kernels alone, on stand-in network outputs, coefficients of step 25 of 50
k = v_diffusion.solver_coefs(fn, 50, order=2, model_out_type="v", w_guide=W)[0][25].tolist()
added_us = None
for B, RES in ((128, 32), (64, 64), (1, 32)):
    x, hist, xn = (torch.randn((B, 3, RES, RES), device=dev) for _ in range(3))
    out, xdup = (torch.randn((2 * B, 3, RES, RES), device=dev) for _ in range(2))
    r = v_diffusion.threshold_rank(3 * RES * RES, Q)
    static = lambda: H.solver_step(x, out, hist, k, 0, True, True, xn, xdup, B, 3, RES * RES)
    dynamic = lambda: H.solver_step_dyn(x, out, hist, k, 0, True, r, math.inf, None, xn, xdup, B, 3, RES * RES)
    ts, td = [], []
    for _ in range(ROUNDS):
        ts.append(timed(static, 500))
        td.append(timed(dynamic, 500))
    ms, md = statistics.median(ts), statistics.median(td)
    if (B, RES) == (128, 32):
        added_us = (md - ms) * 1e3
    print(f"{B:3d} x 3 x {RES} x {RES} guided: vd_solver_step(clip=1) {spread(ts, 'us', 1e3)}   vd_solver_step_dyn {spread(td, 'us', 1e3)}   "
          f"added {(md - ms) * 1e3:.2f} us", flush=True)

# ---- whole chains through the CIFAR network
B, RES = 128, 32
model = build_model(dev, cfg=CIFAR).eval()
lab = torch.randint(1, 11, (B,), device=dev).float()
shape = (B, 3, RES, RES)
gd = v_diffusion.GaussianDiffusion(fn, 50, "v", "fixed_large", "snr_trunc", "mse", w_guide=W)


def chain(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(T, clip):
    return lambda: gd.p_sample_solver(model, shape, label=lab, device=dev, seed=1, steps=T, clip_denoised=clip)


runs = {f"p_sample_solver {name}, {T} steps": (T, run(T, clip)) for T in (20, 50) for name, clip in (("static ", True), ("dynamic", "dynamic"))}
run(4, True)()                                                                       # warm-up of every shape
run(4, "dynamic")()
secs = {name: [] for name in runs}
for _ in range(max(3, ROUNDS)):
    for name, (_, f) in runs.items():
        secs[name].append(chain(f))
noise_us = math.inf
for name, (T, _) in runs.items():
    v = secs[name]
    per_step = [s / T for s in v]
    if "static" in name:
        noise_us = min(noise_us, (max(per_step) - min(per_step)) * 1e6)
    print(f"{name:34s}: {spread([B / s for s in v], 'images/s')}   {spread(per_step, 'ms/step', 1e3)}", flush=True)
print(f"added per step at B = 128: {added_us:.2f} us;  static chain's run-to-run spread of ms/step (the smaller of the two chains'): "
      f"{noise_us:.2f} us  ->  {'within the noise' if added_us < noise_us else 'ABOVE the noise'}", flush=True)
