"""Same-box A/B of the two F(4x4,3x3) input gradients (not a test): the fused kernel (wino43_conv_kernel<., false>, reads dy) against the
planes form GIVEN dM (pack + 36 plane GEMMs + overlap-add: what a training step adds once its weight gradient has made dM), three
alternating rounds per geometry, operands at the scale of a real step (garbage or zeros change the clock of power-bound kernels).
   python tests/perf_dgrad_planes.py [--out FILE]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "v-diffusion-torch_amd"))
from v_diffusion import _hip as H

DEV = "cuda"
ROUNDS, ITERS, SETTLE_S = 3, 200, 1.0        # (a window of a few milliseconds measures the clock ramp: 0.05 ms of drift on 0.45 ms at ITERS = 20)
# (nimg, H, W, Cin, Cout) of the convolution: its input gradient is a K = Cout -> N = Cin product
GEOMS = ((128, 32, 32, 256, 256), (128, 32, 32, 512, 256), (128, 16, 16, 256, 256), (128, 16, 16, 512, 256), (64, 32, 32, 256, 256),
         (64, 32, 32, 512, 256))


def timeit(fn, n=ITERS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"# fused F(4x4,3x3) input gradient vs planes given dM (pack + 36 plane GEMMs + overlap-add); ms per call, {ROUNDS} alternating "
             f"rounds of {ITERS} calls; dM pass = vd_conv3x3_wino43_dy_image alone (the step runs it for the weight gradient either way)",
             f"# {torch.cuda.get_device_name(0)}"]
    lib = H.lib()
    for nimg, Hh, Ww, Cin, Cout in GEOMS:
        g = torch.Generator(DEV).manual_seed(1)
        dy = torch.randn((nimg, Hh, Ww, Cout), device=DEV, generator=g) * 0.05
        w = torch.randn((Cout, Cin, 3, 3), device=DEV, generator=g) * (9 * Cin) ** -0.5
        u43 = torch.empty(lib.vd_wino43_u_floats(Cout, Cin), device=DEV)
        H.wino43_pack(w, Cout, Cin, u43)
        dm = torch.empty(lib.vd_conv3x3_wino43_dm_floats(nimg, Hh, Ww, Cout), device=DEV)
        dxf, dxp = torch.empty(nimg, Hh, Ww, Cin, device=DEV), torch.empty(nimg, Hh, Ww, Cin, device=DEV)
        H.conv3x3_wino43_dy_image(dy, Cout, nimg, Hh, Ww, Cout, dm)
        fused = lambda: H.conv3x3_dgrad_wino43(dy, Cout, u43, dxf, Cin, nimg, Hh, Ww, Cin, Cout)
        planes = lambda: H.conv3x3_wino43_dgrad_planes(dm, w, dxp, Cin, nimg, Hh, Ww, Cin, Cout)
        t_end = time.perf_counter() + SETTLE_S          # both forms back to back until the clock has settled under this load
        while time.perf_counter() < t_end:
            fused()
            planes()
            torch.cuda.synchronize()
        tf, tp = [], []
        for _ in range(ROUNDS):
            tf.append(timeit(fused))
            tp.append(timeit(planes))
        tdm = timeit(lambda: H.conv3x3_wino43_dy_image(dy, Cout, nimg, Hh, Ww, Cout, dm))
        H.PROFILE = []
        for _ in range(5):
            planes()
        torch.cuda.synchronize()
        rec, H.PROFILE = H.PROFILE, None
        ph = [min(e0.elapsed_time(e1) for _, _, e0, e1 in rec[i::3]) for i in range(3)]
        form = H.tile_fields(lib.vd_gemm_last_tile())[1:]
        diff = ((dxp - dxf).norm() / dxf.norm()).item()
        spread = max(tf) - min(tf)
        gain = sum(tf) / ROUNDS - sum(tp) / ROUNDS
        verdict = "planes faster" if gain > spread else ("planes slower" if -gain > spread else "inside the spread")
        lines.append(f"{nimg}x{Hh}x{Ww} K={Cout} -> N={Cin} ({nimg * (Hh // 4) * (Ww // 4)} tiles, GEMM form {form}): fused "
                     + " ".join(f"{t:.3f}" for t in tf) + " | planes " + " ".join(f"{t:.3f}" for t in tp)
                     + f" [pack {ph[0]:.3f} + gemm {ph[1]:.3f} + overlap-add {ph[2]:.3f}] | mean gain {gain:+.3f} ms, fused spread {spread:.3f}: "
                     f"{verdict} | dM pass {tdm:.3f} | rel-L2 planes vs fused {diff:.2e}")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
