"""DDNM null-space restoration (not a test): two measurements, every figure taken ROUNDS times with the versions alternating and printed
as median [min .. max]; times are device events around ITERS back-to-back calls, so they include launch gaps the way a chain sees them.

1. The one launch of a DDNM step, vd_ddnm_step, at 128 x 3 x 32 x 32, guided and plain, for the three operators, beside vd_sample_step on
   the same operands in the same run (what the launch costs on top of the ordinary step) and beside the fp32 ATen composition of the same
   arithmetic (tests/ddnm_ref.py ``step``), on stand-in network outputs.  Kernel and composition are checked against each other before
   they are timed.
2. One full DDNM step -- the network's forward and vd_ddnm_step -- beside one full DPS step -- the taped forward, vd_dps_residual, the
   input-gradient-only backward pass and vd_dps_step -- of the CIFAR-10 network at B = 128, with the same operator.
Nothing is asserted on the times.
python tests/perf_ddnm.py [rounds] [all|launches|steps]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd"), os.path.join(ROOT, "tests")]
import torch
import v_diffusion
from v_diffusion import _hip as H
import ddnm_ref as R
import dps_ref as DR

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
fn = v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0)
OPS = (("mask", 1), ("down", 4), ("gray", None))


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


def launches():
    B, C, RES, T, STEP, ITERS, LAM = 128, 3, 32, 50, 25, 300, 1.0
    shape = (B, C, RES, RES)
    for op, par in OPS:
        for cfg in (False, True):
            gd = v_diffusion.GaussianDiffusion(fn, T, "v", "fixed_large", "snr_trunc", "mse", w_guide=1.0 if cfg else 0.0)
            k8, _ = gd._step_coefs(STEP, use_ddim=False)
            k8 = torch.tensor(k8, dtype=torch.float64).float().tolist()
            rows = B * (1 + cfg)
            xt, noise = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
            out = 0.8 * torch.randn((rows,) + shape[1:], device=dev)
            mask = (torch.rand((B, 1, RES, RES), device=dev) < 0.5).float() if op == "mask" else None
            meas = DR.apply_A(op, 0.6 * torch.randn(shape, device=dev), par, mask)
            ss, xn, xs = torch.empty(B, device=dev), torch.empty_like(xt), torch.empty_like(xt)
            xdup = torch.empty((2 * B,) + shape[1:], device=dev) if cfg else None
            state = {}

            def fused():
                H.ddnm_step(xt, out, noise, meas, mask, k8, LAM, 0, cfg, False, True, H.DPS_OPS[op], par or 0, xn, xdup, ss, B, C, RES, RES)

            def nosum():
                H.ddnm_step(xt, out, noise, meas, mask, k8, LAM, 0, cfg, False, True, H.DPS_OPS[op], par or 0, xn, xdup, None, B, C, RES, RES)

            def plain():
                H.sample_step(xt, out, noise, k8, 0, cfg, False, True, xs, xdup, B, C, RES * RES)

            def composed():
                res = R.step(k8, xt, out, noise, meas, op, LAM, par, mask, False, cfg, False, True)
                state["x"], state["ss"] = res["xn"], res["sumsq"]
                if cfg:
                    state["dup"] = res["xn"].repeat_interleave(2, dim=0)

            fused()
            composed()
            torch.cuda.synchronize()
            worst = float((xn - state["x"]).abs().max())
            assert worst <= 1e-4 and float(((ss - state["ss"]) / state["ss"]).abs().max()) <= 1e-5, worst
            tf, tn, tp, tc = [], [], [], []
            for _ in range(ROUNDS):
                tf.append(timed(fused, ITERS, 20))
                tp.append(timed(plain, ITERS, 20))
                tn.append(timed(nosum, ITERS, 20))
                tc.append(timed(composed, ITERS, 20))
            print(f"{B} x {C} x {RES} x {RES} {op:4s} {'guided' if cfg else 'plain '}: vd_ddnm_step {spread(tf, 'us', 1e3)}   without sumsq "
                  f"{spread(tn, 'us', 1e3)}   vd_sample_step {spread(tp, 'us', 1e3)}   ATen {spread(tc, 'us', 1e3)}   over vd_sample_step "
                  f"{(statistics.median(tf) - statistics.median(tp)) * 1e3:+.2f} us   ratio to ATen "
                  f"{statistics.median(tf) / statistics.median(tc):.3f}   (max difference {worst:.1e})", flush=True)


def steps():
    from oracle.cases import CIFAR_COND, make_inputs, make_weights
    B, C, RES, T, STEP = 128, 3, 32, 50, 25
    shape = (B, C, RES, RES)
    model = v_diffusion.UNet(**CIFAR_COND)
    model.load_state_dict(make_weights(CIFAR_COND), strict=True)
    model.to(dev).eval()
    gd = v_diffusion.GaussianDiffusion(fn, T, "v", "fixed_large", "snr_trunc", "mse", w_guide=0.0)
    k8, t_net = gd._step_coefs(STEP, use_ddim=False)
    x, _, y = (v.to(dev) for v in make_inputs(CIFAR_COND, B, RES, "single", seed=9))
    t = torch.full((B,), t_net, dtype=torch.float64, device=dev)
    noise = torch.randn(shape, device=dev)
    xn, dxt, ss = torch.empty_like(x), torch.empty_like(x), torch.empty(B, device=dev)
    with torch.no_grad(), model.engine().fixed_weights():
        for op, par in OPS:
            mask = (torch.rand((B, 1, RES, RES), device=dev) < 0.5).float() if op == "mask" else None
            meas = DR.apply_A(op, 0.6 * torch.randn(shape, device=dev), par, mask)
            dout = torch.empty(shape, device=dev)

            def forward():
                return model(x, t, y).to(torch.float32).contiguous()

            def ddnm():
                out = forward()
                H.ddnm_step(x, out, noise, meas, mask, k8, 1.0, 0, False, False, True, H.DPS_OPS[op], par or 0, xn, None, ss, B, C, RES, RES)

            def dps():
                out, vjp = model.forward_vjp(x, t, y)
                out = out.to(torch.float32).contiguous()
                H.dps_residual(x, out, meas, mask, k8, 0, False, True, H.DPS_OPS[op], par or 0, dout, dxt, ss, None, B, C, RES, RES)
                H.dps_step(x, out, noise, vjp(dout), dxt, ss, k8, 0.5, 0, False, False, True, xn, None, B, C, RES * RES)

            tw, tn, td = [], [], []
            for _ in range(ROUNDS):
                tw.append(timed(forward, 10, 3))
                tn.append(timed(ddnm, 10, 3))
                td.append(timed(dps, 10, 3))
            print(f"CIFAR-10 network, B = {B}, {op:4s}: forward alone {spread(tw, 'ms')}   DDNM step {spread(tn, 'ms')}   DPS step "
                  f"{spread(td, 'ms')}   DDNM : DPS ratio of medians {statistics.median(tn) / statistics.median(td):.3f}", flush=True)


if __name__ == "__main__":
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    if which in ("all", "launches"):
        launches()
    if which in ("all", "steps"):
        steps()
