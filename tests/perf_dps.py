"""Diffusion Posterior Sampling (not a test): two measurements, every figure taken ROUNDS times with the versions alternating and printed
as median [min .. max]; times are device events around ITERS back-to-back calls, so they include launch gaps the way a chain sees them.

1. The backward pass of the CIFAR-10 network at B = 128 on ONE tape: the input-gradient-only pass (``UNetEngine.backward(tape, dout,
   None, need_dx=True)``, what ``UNet.forward_vjp`` and the frozen-network autograd node run) beside the full pass with ``need_dx=True``
   (what a frozen network asked for d/dx paid before).  The two d/dx are checked bit for bit before they are timed.  The expectation to
   check is only that the input-only pass is faster.
2. The two launches of a DPS step, vd_dps_residual + vd_dps_step, at 128 x 3 x 32 x 32, guided and plain, for the three operators, beside
   the fp32 ATen composition of the same arithmetic with autograd for the cotangents (tests/dps_ref.py: loss -> autograd.grad -> step), on
   stand-in network outputs and a stand-in input gradient.  Both are checked against each other before they are timed.
python tests/perf_dps.py [rounds]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd"), os.path.join(ROOT, "tests")]
import torch
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


def backward_passes():
    from oracle.cases import CIFAR_COND, make_inputs, make_weights
    B = 128
    model = v_diffusion.UNet(**CIFAR_COND)
    model.load_state_dict(make_weights(CIFAR_COND), strict=True)
    model.to(dev).eval()
    eng = model.engine()
    x, t, y = (v.to(dev) for v in make_inputs(CIFAR_COND, B, 32, "single", seed=9))
    with torch.no_grad():
        out, tape = eng.forward(x, t, y, False, True)
        d4 = torch.randn_like(out)
        d4[..., 3:] = 0.0                                          # (the padding channel of the NHWC output gradient)
        G = eng.new_grads()
        full = lambda: eng.backward(tape, d4, G, need_dx=True)
        only = lambda: eng.backward(tape, d4, None, need_dx=True)
        a, b = full(), only()
        torch.cuda.synchronize()
        assert torch.equal(a, b), float((a - b).abs().max())
        tf, to = [], []
        for _ in range(ROUNDS):
            tf.append(timed(full, 10, 3))
            to.append(timed(only, 10, 3))
    print(f"CIFAR-10 network, B = {B}, backward on one tape: full pass (need_dx) {spread(tf, 'ms')}   input-only pass {spread(to, 'ms')}   "
          f"ratio of medians {statistics.median(to) / statistics.median(tf):.3f}   (d/dx bit for bit equal)", flush=True)


def launches():
    B, C, RES, T, STEP, ITERS = 128, 3, 32, 50, 25, 300
    shape = (B, C, RES, RES)
    for op, par in (("mask", 1), ("down", 4), ("gray", None)):
        for cfg in (False, True):
            gd = v_diffusion.GaussianDiffusion(fn, T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0 if cfg else 0.0)
            k8, _ = gd._step_coefs(STEP, use_ddim=False)
            k8 = torch.tensor(k8, dtype=torch.float64).float().tolist()
            rows = B * (1 + cfg)
            xt, noise = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
            out, dxin = 0.8 * torch.randn((rows,) + shape[1:], device=dev), 0.3 * torch.randn((rows,) + shape[1:], device=dev)
            mask = (torch.rand((B, 1, RES, RES), device=dev) < 0.5).float() if op == "mask" else None
            meas = R.apply_A(op, 0.6 * torch.randn(shape, device=dev), par, mask)
            dout, dxt, ss, xn = torch.empty_like(out), torch.empty_like(xt), torch.empty(B, device=dev), torch.empty_like(xt)
            xdup = torch.empty((2 * B,) + shape[1:], device=dev) if cfg else None
            state = {}

            def fused():
                H.dps_residual(xt, out, meas, mask, k8, 0, cfg, True, H.DPS_OPS[op], par or 0, dout, dxt, ss, None, B, C, RES, RES)
                H.dps_step(xt, out, noise, dxin, dxt, ss, k8, 0.5, 0, cfg, False, True, xn, xdup, B, C, RES * RES)

            def composed():
                with torch.enable_grad():
                    xg, og = xt.detach().requires_grad_(True), out.detach().requires_grad_(True)
                    l = R.loss(k8, xg, og, meas, op, par, mask, False, cfg, True)
                    gx, go = torch.autograd.grad(l.sum(), (xg, og))
                x = R.step(k8, xt, out, noise, dxin, gx, 2.0 * l.detach(), 0.5, False, cfg, False, True)
                state["x"], state["go"] = x, go
                if cfg:
                    state["dup"] = x.repeat_interleave(2, dim=0)

            fused()
            composed()
            torch.cuda.synchronize()
            worst = float((xn - state["x"]).abs().max())
            assert worst <= 1e-4 and float((dout - state["go"]).abs().max()) <= 1e-5, worst
            tf, tc = [], []
            for _ in range(ROUNDS):
                tf.append(timed(fused, ITERS, 20))
                tc.append(timed(composed, ITERS, 20))
            print(f"{B} x {C} x {RES} x {RES} {op:4s} {'guided' if cfg else 'plain '}: vd_dps_residual + vd_dps_step {spread(tf, 'us', 1e3)}   "
                  f"ATen + autograd {spread(tc, 'us', 1e3)}   ratio of medians {statistics.median(tf) / statistics.median(tc):.3f}   "
                  f"(max difference {worst:.1e})", flush=True)


if __name__ == "__main__":
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    if which in ("all", "backward"):
        backward_passes()
    if which in ("all", "launches"):
        launches()
