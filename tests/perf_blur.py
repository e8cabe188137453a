"""The blur operator of Diffusion Posterior Sampling (not a test): two measurements, every figure taken ROUNDS times with the versions
alternating and printed as median [min .. max]; times are device events around ITERS back-to-back calls, so they include launch gaps the
way a chain sees them.  No figure is a threshold.

1. The residual launch vdx_dps_residual_blur at 128 x 3 x 32 x 32 under 9 x 9 taps and at 32 x 3 x 64 x 64 under 33 x 33 taps (both
   bounds), plain and guided, beside the fp32 ATen composition of the same quantity with autograd for the cotangents (reflect pad +
   depthwise conv2d; loss -> autograd.grad) and beside vd_dps_residual with a mask on the same inputs in the same run.  The launch is
   checked against the composition before it is timed.
2. One full DPS step of the CIFAR-10 network at B = 128 (network call with tape, residual launch, input-only backward pass, step launch)
   as ``p_sample_dps`` runs it, with the 9 x 9 Gaussian blur beside a mask: a chain of STEPS steps, divided by STEPS.
python tests/perf_blur.py [rounds] [launches|step]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd"), os.path.join(ROOT, "tests")]
import torch
import torch.nn.functional as F
import v_diffusion
from v_diffusion import _hip as H
import dps_ref as R

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
fn = v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0)


def timed(f, iters, warm):
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


def aten_A(x, taps):
    C, (kh, kw) = x.shape[1], taps.shape
    return F.conv2d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2), mode="reflect"), taps.expand(C, 1, kh, kw), groups=C)


def launches():
    T, STEP = 50, 25
    for (B, C, RES), taps, iters in (((128, 3, 32), v_diffusion.gaussian_kernel(9, 1.5).to(dev), 100),
                                     ((32, 3, 64), (torch.randn(33, 33, device=dev) / 33.0 ** 2), 10)):
        shape = (B, C, RES, RES)
        for cfg in (False, True):
            gd = v_diffusion.GaussianDiffusion(fn, T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0 if cfg else 0.0)
            k8, _ = gd._step_coefs(STEP, use_ddim=False)
            k8 = torch.tensor(k8, dtype=torch.float64).float().tolist()
            rows = B * (1 + cfg)
            xt, out = torch.randn(shape, device=dev), 0.8 * torch.randn((rows,) + shape[1:], device=dev)
            mask = (torch.rand((B, 1, RES, RES), device=dev) < 0.5).float()
            meas = aten_A(0.6 * torch.randn(shape, device=dev), taps)
            dout, dxt, ss = torch.empty_like(out), torch.empty_like(xt), torch.empty(B, device=dev)
            state = {}

            def blur():
                H.dps_residual_blur(xt, out, meas, taps, k8, 0, cfg, True, dout, dxt, ss, None, B, C, RES, RES)

            def masked():
                H.dps_residual(xt, out, meas, mask, k8, 0, cfg, True, H.DPS_OPS["mask"], 1, dout, dxt, ss, None, B, C, RES, RES)

            def composed():
                with torch.enable_grad():
                    xg, og = xt.detach().requires_grad_(True), out.detach().requires_grad_(True)
                    r = meas - aten_A(R.guided(k8, xg, og, False, cfg, True)[0], taps)
                    l = 0.5 * (r * r).reshape(B, -1).sum(dim=1)
                    state["gx"], state["go"] = torch.autograd.grad(l.sum(), (xg, og))
                state["ss"] = 2.0 * l.detach()

            composed()
            blur()
            torch.cuda.synchronize()
            worst = max(float((dout - state["go"]).abs().max()), float((dxt - state["gx"]).abs().max()))
            assert worst <= 1e-4 and float(((ss - state["ss"]).abs() / state["ss"]).max()) <= 1e-4, worst
            tb, tm, tc = [], [], []
            for _ in range(ROUNDS):
                tb.append(timed(blur, iters, 3))
                tm.append(timed(masked, iters, 3))
                tc.append(timed(composed, iters, 3))
            print(f"{B} x {C} x {RES} x {RES}, {taps.shape[0]} x {taps.shape[1]} taps, {'guided' if cfg else 'plain '}: vdx_dps_residual_blur "
                  f"{spread(tb, 'us', 1e3)}   ATen + autograd {spread(tc, 'us', 1e3)}   vd_dps_residual (mask) {spread(tm, 'us', 1e3)}   "
                  f"blur / ATen {statistics.median(tb) / statistics.median(tc):.3f}   (max difference {worst:.1e})", flush=True)


def full_step():
    from oracle.cases import CIFAR_COND, make_weights
    B, STEPS = 128, 4
    model = v_diffusion.UNet(**CIFAR_COND)
    model.load_state_dict(make_weights(CIFAR_COND), strict=True)
    model.to(dev).eval()
    shape = (B, 3, 32, 32)
    gd = v_diffusion.GaussianDiffusion(fn, STEPS, "v", "fixed_large", "snr_trunc", "mse", w_guide=0.0)
    y = torch.ones(B, device=dev)
    clean = (0.6 * torch.randn(shape, device=dev)).clamp(-1, 1)
    ops = {"blur": ("blur", v_diffusion.gaussian_kernel(9, 1.5)), "mask": ("mask", (torch.rand((B, 1, 32, 32), device=dev) < 0.5).float())}
    meas = {name: v_diffusion.dps_measure(clean, op) for name, op in ops.items()}
    run = {name: (lambda name=name: gd.p_sample_dps(model, meas[name], ops[name], shape, label=y, seed=3, zeta=0.5)) for name in ops}
    times = {name: [] for name in ops}
    for _ in range(ROUNDS):
        for name in ops:
            times[name].append(timed(run[name], 3, 1) / STEPS)
    print(f"CIFAR-10 network, B = {B}, one DPS step (a chain of {STEPS}, per step): blur 9 x 9 {spread(times['blur'], 'ms')}   "
          f"mask {spread(times['mask'], 'ms')}   ratio of medians {statistics.median(times['blur']) / statistics.median(times['mask']):.3f}",
          flush=True)


if __name__ == "__main__":
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    if which in ("all", "launches"):
        launches()
    if which in ("all", "step"):
        full_step()
