"""The UniPC node launch at the CIFAR sampling shape (not a test): per-launch time of vd_unipc_step at 128 x 3 x 32 x 32, guided and
plain, beside the fp32 ATen composition of the same ordered arithmetic (tests/unipc_ref.py::node on device tensors, the history shift
and the duplicated rows included) and beside vd_solver_step in the same process.  vd_unipc_step moves 12 image-units per element when
guided (x_t, two output rows, three history images in; three history images, x_next, two duplicated rows out) against vd_solver_step's
8, and 9 against 5 when plain.  Every figure is taken ROUNDS times, the versions alternating, and printed as median [min .. max].
python tests/perf_unipc.py [rounds]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd"), os.path.join(ROOT, "tests")]
import torch
import v_diffusion
from v_diffusion import _hip as H
import unipc_ref as U

dev = torch.device("cuda", 0)
B, C, RES, W = 128, 3, 32, 1.0
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


for cfg in (True, False):
    w = W if cfg else 0.0
    k_unipc = v_diffusion.unipc_coefs(fn, 50, order=3, variant="bh2", corrector=True, model_out_type="v", w_guide=w)[0][25].tolist()
    k_solver = v_diffusion.solver_coefs(fn, 50, order=2, model_out_type="v", w_guide=w)[0][25].tolist()
    x, h0, h1, h2, xn = (torch.randn((B, C, RES, RES), device=dev) for _ in range(5))
    out = torch.randn(((1 + cfg) * B, C, RES, RES), device=dev)
    xdup = torch.empty_like(out) if cfg else None
    st = {"h": (h0.clone(), h1.clone(), h2.clone())}

    def unipc():
        H.unipc_step(x, out, h0, h1, h2, k_unipc, 0, cfg, True, xn, xdup, None, B, C, RES * RES)

    def solver():
        H.solver_step(x, out, h0, k_solver, 0, cfg, True, xn, xdup, B, C, RES * RES)

    def aten():
        a, b, c = st["h"]
        oc, ou = (out[0::2], out[1::2]) if cfg else (out, None)
        nx, _, g = U.node(k_unipc, x, oc, ou, a, b, c, cfg=cfg, clip=True)
        st["h"] = (g, a, b)
        return nx.repeat_interleave(2, dim=0) if cfg else nx

    tu, ts, ta = [], [], []
    for _ in range(ROUNDS):
        tu.append(timed(unipc, 500))
        ts.append(timed(solver, 500))
        ta.append(timed(aten, 200))
    mu, ms, ma = (statistics.median(v) for v in (tu, ts, ta))
    units = (12, 8) if cfg else (9, 5)
    print(f"B={B} {'guided' if cfg else 'plain '}: vd_unipc_step {spread(tu, 'us', 1e3)}   ATen composition {spread(ta, 'us', 1e3)} "
          f"({ma / mu:.1f}x)   vd_solver_step {spread(ts, 'us', 1e3)}   unipc/solver {mu / ms:.3f} (bytes {units[0]}/{units[1]} = "
          f"{units[0] / units[1]:.3f})", flush=True)
