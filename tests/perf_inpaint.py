"""The RePaint reverse step (not a test): per-step time of the one launch of vd_inpaint_step beside what a user composes today from
the existing pieces -- vd_sample_step, ATen ops for ak*known + bk*knoise and for the mask blend, and repeat_interleave for the next
guided input -- in the same process, on stand-in network outputs, at 128 x 3 x 32 x 32 and 64 x 3 x 64 x 64, with and without cfg,
for a mask shared by the channels.  Both versions produce the next state (and, guided, its duplicated copy) from the same inputs and
are checked against each other before they are timed.  Every figure is taken ROUNDS times, the versions alternating, and printed as
median [min .. max]; times are device events around ITERS back-to-back steps, so they include launch gaps the way a chain sees them.
The expectation to check is that the single launch is not slower than the composition.
python tests/perf_inpaint.py [rounds]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]
import torch
import v_diffusion
from v_diffusion import _hip as H

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ITERS, W, T, STEP = 500, 1.0, 50, 25
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


for B, RES in ((128, 32), (64, 64)):
    for cfg in (False, True):
        gd = v_diffusion.GaussianDiffusion(fn, T, "v", "fixed_large", "snr_trunc", "mse", w_guide=W if cfg else 0.0)
        k8, _ = gd._step_coefs(STEP, use_ddim=False)
        ak, bk = v_diffusion.known_coefs(fn, T, STEP)
        shape, HW = (B, 3, RES, RES), RES * RES
        x, noise, known, knoise, xn, xn2 = (torch.randn(shape, device=dev) for _ in range(6))
        out = torch.randn((B * (1 + cfg),) + shape[1:], device=dev)
        xdup = torch.empty((2 * B,) + shape[1:], device=dev) if cfg else None
        mask = (torch.rand((B, 1, RES, RES), device=dev) < 0.5).float()
        state = {}

        def fused():
            H.inpaint_step(x, out, noise, known, mask, knoise, list(k8) + [ak, bk], 0, cfg, False, True, 1, xn, xdup, B, 3, HW)

        def composed():
            H.sample_step(x, out, noise, k8, 0, cfg, False, True, xn2, None, B, 3, HW)
            kn = ak * known + bk * knoise
            merged = mask * kn + (1.0 - mask) * xn2
            state["x"] = merged
            if cfg:
                state["dup"] = merged.repeat_interleave(2, dim=0)

        fused()
        composed()
        torch.cuda.synchronize()
        worst = float((xn - state["x"]).abs().max())
        assert worst <= 1e-4 and (not cfg or torch.equal(xdup[0::2], xn)), worst
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(timed(fused, ITERS))
            tc.append(timed(composed, ITERS))
        mf, mc = statistics.median(tf), statistics.median(tc)
        print(f"{B:3d} x 3 x {RES} x {RES} {'guided' if cfg else 'plain '}: vd_inpaint_step {spread(tf, 'us', 1e3)}   "
              f"vd_sample_step + ATen {spread(tc, 'us', 1e3)}   ratio of medians {mf / mc:.3f}   (max difference {worst:.1e})", flush=True)
