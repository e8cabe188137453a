"""The DPM-Solver++(2M) sampler on the CIFAR config (not a test): per-launch time of vd_solver_step beside vd_sample_step in the same
process, at the sampling shape (128 x 3 x 32 x 32, guided) and at batch 1, and end-to-end images/s of p_sample(use_ddim=True) at 50
steps against p_sample_solver at 50 and at 20 steps.  vd_solver_step moves 8 image-units per element (x_t, two output rows, hist in;
hist, x_next, two duplicated rows out) against vd_sample_step's 7, so its time is held against vd_sample_step's of the same run
times 8/7.  Every figure is taken ROUNDS times, the versions alternating, and printed as median [min .. max].
python tests/perf_solver.py [rounds]"""
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
RES, W = 32, 1.0
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
gd = v_diffusion.GaussianDiffusion(fn, 50, "v", "fixed_large", "snr_trunc", "mse", w_guide=W)
k_ddim, _ = gd._step_coefs(25, use_ddim=True)
k_solver = v_diffusion.solver_coefs(fn, 50, order=2, model_out_type="v", w_guide=W)[0][25].tolist()
for B in (128, 1):
    x, hist, noise, xn = (torch.randn((B, 3, RES, RES), device=dev) for _ in range(4))
    out, xdup = (torch.randn((2 * B, 3, RES, RES), device=dev) for _ in range(2))
    solver = lambda: H.solver_step(x, out, hist, k_solver, 0, True, True, xn, xdup, B, 3, RES * RES)
    ddim = lambda: H.sample_step(x, out, noise, k_ddim, 0, True, False, True, xn, xdup, B, 3, RES * RES)
    ts, td = [], []
    for _ in range(ROUNDS):
        ts.append(timed(solver, 500))
        td.append(timed(ddim, 500))
    ms, md = statistics.median(ts), statistics.median(td)
    print(f"B={B:3d} guided: vd_solver_step {spread(ts, 'us', 1e3)}   vd_sample_step {spread(td, 'us', 1e3)}   "
          f"ratio of medians {ms / md:.3f} (bytes 8/7 = {8 / 7:.3f})", flush=True)

# ---- whole chains through the CIFAR network
B = 128
model = build_model(dev, cfg=CIFAR).eval()
lab = torch.randint(1, 11, (B,), device=dev).float()
shape = (B, 3, RES, RES)


def chain(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


runs = {"p_sample DDIM, 50 steps": (50, lambda: gd.p_sample(model, shape, label=lab, device=dev, seed=1, use_ddim=True)),
        "p_sample_solver 2M, 50 steps": (50, lambda: gd.p_sample_solver(model, shape, label=lab, device=dev, seed=1, steps=50)),
        "p_sample_solver 2M, 20 steps": (20, lambda: gd.p_sample_solver(model, shape, label=lab, device=dev, seed=1, steps=20))}
gd.p_sample_solver(model, shape, label=lab, device=dev, seed=1, steps=4)             # warm-up of every shape
gd.p_sample(model, shape, label=lab, device=dev, seed=1, use_ddim=True)
secs = {name: [] for name in runs}
for _ in range(max(3, ROUNDS // 2 + 1)):
    for name, (_, f) in runs.items():
        secs[name].append(chain(f))
for name, (T, _) in runs.items():
    v = secs[name]
    print(f"{name:30s}: {spread([B / s for s in v], 'images/s')}   {spread([s / T for s in v], 'ms/step', 1e3)}", flush=True)
