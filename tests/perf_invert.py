"""The noise-space inversion step (not a test): per-step time of the one launch of vd_noise_extract beside the four-op composition it
replaces -- vd_forward_jump for x_i = ak*x_0 + bk*eps, vd_sample_step without noise for the guided mean, ATen subtract and divide for
the map, and repeat_interleave for the next guided input -- in the same process, on stand-in network outputs, at 128 x 3 x 32 x 32,
guided and plain.  Both versions produce the next state, the map (and, guided, the duplicated copy) from the same inputs and are
checked against each other before they are timed.  Every figure is taken ROUNDS times, the versions alternating, and printed as
median [min .. max]; times are device events around ITERS back-to-back steps, so they include launch gaps the way a chain sees them.
The expectation to check is that the single launch is not slower than the composition.  The last line times vd_slerp_rows on the same
shape beside the ATen expression of the same formula (fp32 sums).
python tests/perf_invert.py [rounds]"""
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


B, RES = 128, 32
shape, HW = (B, 3, RES, RES), RES * RES
for cfg in (True, False):
    gd = v_diffusion.GaussianDiffusion(fn, T, "v", "fixed_large", "snr_trunc", "mse", w_guide=W if cfg else 0.0)
    k8, _ = gd._step_coefs(STEP, use_ddim=False)
    ak, bk = v_diffusion.known_coefs(fn, T, STEP)
    x, x0, eps, xs, z, xs2, mean = (torch.randn(shape, device=dev) for _ in range(7))
    out = torch.randn((B * (1 + cfg),) + shape[1:], device=dev)
    xdup = torch.empty((2 * B,) + shape[1:], device=dev) if cfg else None
    k_mean = list(k8)
    k_mean[5] = 0.0
    state = {}

    def fused():
        H.noise_extract(x, out, x0, eps, list(k8) + [ak, bk], 0, cfg, False, True, xs, z, xdup, B, 3, HW)

    def composed():
        H.forward_jump(x0, eps, (ak, bk), xs2, None, B, 3 * HW)
        H.sample_step(x, out, None, k_mean, 0, cfg, False, True, mean, None, B, 3, HW)
        state["z"] = (xs2 - mean) / k8[5]
        if cfg:
            state["dup"] = xs2.repeat_interleave(2, dim=0)

    fused()
    composed()
    torch.cuda.synchronize()
    worst = float((z - state["z"]).abs().max() / z.abs().max())
    assert worst <= 1e-5 and torch.equal(xs, xs2) and (not cfg or torch.equal(xdup[0::2], xs)), worst
    tf, tc = [], []
    for _ in range(ROUNDS):
        tf.append(timed(fused, ITERS))
        tc.append(timed(composed, ITERS))
    mf, mc = statistics.median(tf), statistics.median(tc)
    print(f"{B:3d} x 3 x {RES} x {RES} {'guided' if cfg else 'plain '}: vd_noise_extract {spread(tf, 'us', 1e3)}   "
          f"jump + vd_sample_step + ATen {spread(tc, 'us', 1e3)}   ratio of medians {mf / mc:.3f}   (max relative difference {worst:.1e})",
          flush=True)

a, b, o = (torch.randn(shape, device=dev) for _ in range(3))
state = {}


def fused_slerp():
    H.slerp_rows(a, b, 0.3, o, None, B, 3 * HW)


def composed_slerp():
    af, bf = a.reshape(B, -1), b.reshape(B, -1)
    w = torch.acos(((af * bf).sum(1) / (af.norm(dim=1) * bf.norm(dim=1))).clamp(-1, 1))
    s = torch.sin(w)
    state["o"] = (torch.sin(0.7 * w) / s).reshape(B, 1, 1, 1) * a + (torch.sin(0.3 * w) / s).reshape(B, 1, 1, 1) * b


fused_slerp()
composed_slerp()
torch.cuda.synchronize()
worst = float((o - state["o"]).abs().max())
assert worst <= 1e-4, worst
tf, tc = [], []
for _ in range(ROUNDS):
    tf.append(timed(fused_slerp, ITERS))
    tc.append(timed(composed_slerp, ITERS))
print(f"{B:3d} x 3 x {RES} x {RES} slerp : vd_slerp_rows {spread(tf, 'us', 1e3)}   ATen {spread(tc, 'us', 1e3)}   "
      f"ratio of medians {statistics.median(tf) / statistics.median(tc):.3f}   (max difference {worst:.1e})", flush=True)
