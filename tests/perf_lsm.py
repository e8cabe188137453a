"""Loss-aware timestep resampling (not a test): time of the two launches beside what they replace, in the same process, at T = 1000,
K = 10 -- a draw of B = 128 and an update of n = 128 rows (one rank's step) and of n = 1024 rows (eight ranks' gathered rows):
  * vd_lsm_draw + vd_lsm_update, as LossSecondMomentResampler issues them;
  * the ATen composition on the device: hist.double().square().mean(1).sqrt(), normalise and mix, cumsum, searchsorted, gather for the
    weights, and an index_put_-based history write (which, unlike the kernel, keeps ONE row of a timestep that occurs several times);
  * a host-numpy resampler in the manner of improved-diffusion: losses and indices copied to the host, the history in numpy,
    np.searchsorted on the host, indices and weights copied back -- its .cpu() round trips drain the launch queue.
Then HotPathTrainer.step on the CIFAR-10 model at B = 128, the uniform draw against "loss-second-moment" (a warmed-up history) on ONE
trainer whose sampler is switched off and on, the two alternating.  Every figure is taken ROUNDS times and printed as median [min .. max]; times are device events around
back-to-back calls (a host clock around a synchronised loop for the host-numpy version), so they include launch gaps the way a step sees
them.  The expectation to check is that the resampler's cost per step is noise against the step.
python tests/perf_lsm.py [rounds]"""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]
import numpy as np
import torch
import v_diffusion
from v_diffusion.trainer import HotPathTrainer
from bench import build_model, CIFAR

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ITERS, T, K, B, EPS = 200, 1000, 10, 128, 0.001


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


def wall(f, iters, warm=20):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def spread(v, unit, scale=1.0):
    return f"{statistics.median(v) * scale:8.2f} {unit} [{min(v) * scale:.2f} .. {max(v) * scale:.2f}]"


# ------------------------------------------------------------------------------------------------ the launches and what they replace
rng = np.random.default_rng(0)
hist0 = np.exp(rng.uniform(math.log(1e-4), math.log(10.0), size=(T, K))).astype(np.float32)
sm = v_diffusion.LossSecondMomentResampler(T, K, EPS, device=dev)
warm = {"hist": torch.from_numpy(hist0), "count": torch.full((T,), K, dtype=torch.int32), "pos": torch.zeros(T, dtype=torch.int32),
        "history_per_term": K, "uniform_prob": EPS}
g = torch.Generator(dev).manual_seed(1)
u = torch.rand((B,), dtype=torch.float64, device=dev, generator=g)
state = {}

for n in (B, 1024):
    sm.load_state_dict(warm)                                       # the three versions start from the same history: their first draws are compared
    rows_idx = torch.randint(T, (n,), device=dev, generator=g).to(torch.int32)
    rows_loss = torch.rand((n,), device=dev, generator=g) + 0.1
    hist_a, pos_a = torch.from_numpy(hist0).to(dev), torch.zeros(T, dtype=torch.int64, device=dev)
    hist_h, pos_h = hist0.copy(), np.zeros(T, dtype=np.int64)

    def fused():
        state["fused"] = sm.draw(B, u=u)
        sm.update(rows_idx, rows_loss)

    def aten():
        m = hist_a.double().square().mean(1).sqrt()
        q = (1.0 - EPS) * m / m.sum() + EPS / T
        idx = torch.searchsorted(torch.cumsum(q, 0), u, right=True).clamp_(max=T - 1)
        state["aten"] = ((idx + 1).double() / T, idx, (1.0 / (T * q[idx])).float())
        i = rows_idx.long()
        hist_a.index_put_((i, pos_a[i]), rows_loss)
        pos_a.index_put_((i,), (pos_a[i] + 1) % K)

    def host():
        m = np.sqrt((hist_h.astype(np.float64) ** 2).mean(1))
        q = (1.0 - EPS) * m / m.sum() + EPS / T
        idx = np.minimum(np.searchsorted(np.cumsum(q), u.cpu().numpy(), side="right"), T - 1)
        state["host"] = (torch.from_numpy((idx + 1.0) / T).to(dev), torch.from_numpy(idx).to(dev),
                         torch.from_numpy((1.0 / (T * q[idx])).astype(np.float32)).to(dev))
        for i, l in zip(rows_idx.cpu().numpy().tolist(), rows_loss.cpu().numpy().tolist()):
            hist_h[i, pos_h[i]] = l
            pos_h[i] = (pos_h[i] + 1) % K

    fused(), aten(), host()
    torch.cuda.synchronize()
    same = float((state["fused"][1].long() != state["aten"][1]).float().mean()), float((state["fused"][1].long() != state["host"][1]).float().mean())
    tf, ta, th = [], [], []
    for _ in range(ROUNDS):
        tf.append(timed(fused, ITERS))
        ta.append(timed(aten, ITERS))
        th.append(wall(host, 50, warm=5))
    print(f"T={T} K={K} draw B={B} + update n={n}: vd_lsm_draw + vd_lsm_update {spread(tf, 'us', 1e3)}   ATen composition {spread(ta, 'us', 1e3)}   "
          f"host numpy with .cpu() round trips {spread(th, 'us', 1e3)}   (first-call indices differing from the kernel's: ATen {same[0]:.3f}, host {same[1]:.3f})",
          flush=True)
td, tu = [], []
for _ in range(ROUNDS):
    td.append(timed(lambda: sm.draw(B, u=u), ITERS))
    tu.append(timed(lambda: sm.update(rows_idx, rows_loss), ITERS))
print(f"alone: draw B={B} {spread(td, 'us', 1e3)}   update n=1024 {spread(tu, 'us', 1e3)}", flush=True)

# ------------------------------------------------------------------------------------------------ the train step
TS = 1000
x = torch.rand((B, 3, 32, 32), device=dev) * 2 - 1
lab = torch.randint(1, 11, (B,), device=dev).float()
diffusion = v_diffusion.GaussianDiffusion(v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0), TS, "v", "fixed_medium", "snr_trunc", "mse",
                                          intp_frac=0.3, w_guide=1.0, p_uncond=0.1)
tr = HotPathTrainer(build_model(dev, cfg=CIFAR).train(), diffusion, lr=2e-4, weight_decay=0.001, warmup=1000, grad_norm=1.0, ema_decay=0.9999,
                    use_ema=True, timesteps=TS, schedule_sampler="loss-second-moment")
tr.sampler.load_state_dict(sm.state_dict())                        # warmed up: the step takes the weighted path
assert tr.sampler.warmed_up
# ONE trainer, its sampler switched off and on (sampler None is the uniform code path): two model instances in one process differ by more
# than the resampler costs
modes = {"uniform": None, "loss-second-moment": tr.sampler}
steps = {k: [] for k in modes}
for _ in range(ROUNDS):
    for name, sampler in modes.items():
        tr.sampler = sampler
        steps[name].append(timed(lambda: tr.step(x, lab.clone()), 20, warm=5))
mu, ml = statistics.median(steps["uniform"]), statistics.median(steps["loss-second-moment"])
print(f"HotPathTrainer.step CIFAR-10 B={B} T={TS}: uniform {spread(steps['uniform'], 'ms')}   loss-second-moment {spread(steps['loss-second-moment'], 'ms')}   "
      f"delta of medians {1e3 * (ml - mu):+.0f} us = {100 * (ml / mu - 1):+.2f} % of the uniform step", flush=True)
