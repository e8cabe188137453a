"""Same-box, same-process A/B of the 128x256 split-operand GEMM form against the 128x128 one (not a test), real random operands:
the eight launches of profiles/r06_presplit_price.txt, the M = 32 768 launches with N = 768 and N = 512, and the batched attention
products at L = 1024 (hd = 64, 6 heads, 16 images: Q.K^T and dP have N = L and can take the form; P.V, dV, dQ, dK have N = hd = 64 and
cannot -- they are listed with their 128x128 time only).

Per shape the two forms are ALTERNATED in blocks of 25 launches, ROUNDS blocks each (>= 200 timed launches per form after warm-up); a block
is timed with one event pair.  Reported: median block time per launch, the spread (max - min over the blocks of that form), and the
in-kernel shader clock each form holds when it runs alone back to back (tests/probe/clock_witness.hip beside it, as in
tests/probe/clock_by_kernel.py).  "wide wins" = the difference of the medians exceeds the larger of the two spreads.

    python tests/perf_gemm_wide.py > profiles/<round>_gemm_wide_ab.txt
"""
import ctypes
import os
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "v-diffusion-torch_amd"))
from v_diffusion import _hip as H   # noqa: E402

DEV = "cuda"
BLOCK, ROUNDS = 25, int(os.environ.get("VD_PERF_ROUNDS", "10"))
WIT_SO = os.path.join(HERE, "probe", "libclock_witness.so")
if not os.path.exists(WIT_SO):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-shared", "-fPIC", os.path.join(HERE, "probe", "clock_witness.hip"),
                           "-o", WIT_SO])
wit = ctypes.CDLL(WIT_SO)
wit.launch_clock_witness.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p]
wit.launch_clock_witness.restype = ctypes.c_int
side = torch.cuda.Stream()
NWG, NSAMP, PERIOD = 8, 200, 100_000          # one witness per XCD, 200 stamps 1 ms apart (100 MHz ticks)


def clock_of(fn, lead_s=0.6):
    """MHz the chip holds while fn runs alone back to back (median over the XCDs)"""
    buf = torch.zeros(NWG * NSAMP * 2, dtype=torch.int64, device=DEV)
    done = torch.cuda.Event()
    n, t0, launched = 0, time.perf_counter(), False
    while True:
        for _ in range(20):
            fn()
        n += 20
        if not launched and time.perf_counter() - t0 >= lead_s:
            with torch.cuda.stream(side):
                assert wit.launch_clock_witness(buf.data_ptr(), NWG, NSAMP, PERIOD, side.cuda_stream) == 0
                done.record(side)
            launched = True
        if launched and done.query():
            break
        if n % 200 == 0:
            torch.cuda.current_stream().synchronize()
    torch.cuda.synchronize()
    t = buf.view(NWG, NSAMP, 2).double().cpu()
    return float(((t[:, -1, 0] - t[:, 0, 0]) / (t[:, -1, 1] - t[:, 0, 1]) * 100.0).median())


def block_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(BLOCK):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / BLOCK


def ab(name, flops, make):
    """make(tile) -> launch closure; prints one line"""
    f128, fw = make(128), make(H.TILE_WIDE)
    codes = []
    for f in (f128, fw):
        if f is None:
            codes.append(0)
            continue
        for _ in range(10):
            f()
        torch.cuda.synchronize()
        codes.append(H.lib().vd_gemm_last_tile())
    t = {0: [], 1: []}
    for _ in range(ROUNDS):
        for i, f in enumerate((f128, fw)):
            if f is not None:
                t[i].append(block_ms(f))
    med = lambda v: sorted(v)[len(v) // 2]
    m0, s0, c0 = med(t[0]), max(t[0]) - min(t[0]), clock_of(f128)
    line = f"{name:46s} 128x128 [{codes[0]}] {m0 * 1e3:8.1f} us (spread {s0 * 1e3:5.1f}) {c0:5.0f} MHz {flops / m0 / 1e9:6.1f} TF"
    if fw is None:
        print(line + " | 128x256: N % 256 != 0, no such form", flush=True)
        return
    m1, s1, c1 = med(t[1]), max(t[1]) - min(t[1]), clock_of(fw)
    verdict = "wide wins" if m0 - m1 > max(s0, s1) else ("wide loses" if m1 - m0 > max(s0, s1) else "inside the spread")
    print(line + f" | 128x256 [{codes[1]}] {m1 * 1e3:8.1f} us (spread {s1 * 1e3:5.1f}) {c1:5.0f} MHz {flops / m1 / 1e9:6.1f} TF | {(m1 / m0 - 1) * 100:+5.1f} %  {verdict}",
          flush=True)


g = torch.Generator(DEV).manual_seed(1)
rn = lambda *s: torch.randn(s, device=DEV, generator=g)


def plain(M, N, K, bk):
    A, B, C, bias = rn(M, K), (rn(N, K) if bk == H.ROW else rn(K, N)) * K ** -0.5, torch.empty((M, N), device=DEV), rn(N)
    return lambda tile: (lambda: H.gemm(A, B, C, M, N, K, a_kind=H.ROW, b_kind=bk, lda=K, ldb=B.shape[1], ldc=N,
                                        bias=bias if bk == H.ROW else None, tile=tile))


print(f"# {os.path.basename(__file__)}: blocks of {BLOCK} launches, {ROUNDS} alternated blocks per form; time = median block, spread = max - min over the "
      f"blocks of one form; clock = in-kernel shader clock of the form looped alone; TF = fp32-equivalent TFLOP/s; library {H.LIB_PATH}")
for name, M, N, K, bk in (("fwd qkv  32x32", 131072, 768, 256, H.ROW), ("fwd proj 32x32", 131072, 256, 256, H.ROW),
                          ("fwd skip 32x32", 131072, 256, 512, H.ROW), ("fwd qkv  16x16", 32768, 768, 256, H.ROW),
                          ("dgrad qkv 32x32", 131072, 256, 768, H.COL), ("dgrad proj 32x32", 131072, 256, 256, H.COL),
                          ("dgrad skip 32x32", 131072, 512, 256, H.COL), ("dgrad qkv 16x16", 32768, 256, 768, H.COL),
                          ("dgrad skip 16x16", 32768, 512, 256, H.COL), ("fwd skip-like 16x16", 32768, 512, 256, H.ROW)):
    ab(f"{name:20s} M={M:6d} N={N:4d} K={K:4d}", 2.0 * M * N * K, plain(M, N, K, bk))
    torch.cuda.empty_cache()

# batched attention products at L = 1024, as engine.py passes them: qkv [B][L][3 hid], P [B][nh][L][L]
Bz, nh, L, hd = 16, 6, 1024, 64
hid, ld = nh * hd, 3 * nh * hd
qkv, dO = rn(Bz, L, ld), rn(Bz, L, hid)
P = torch.softmax(rn(Bz, nh, L, L), -1)
S, O, dqkv = torch.empty_like(P), torch.empty((Bz, L, hid), device=DEV), torch.empty((Bz, L, ld), device=DEV)
q, k, v = qkv[0, 0, 0:], qkv[0, 0, hid:], qkv[0, 0, 2 * hid:]
dq, dk, dv = dqkv[0, 0, 0:], dqkv[0, 0, hid:], dqkv[0, 0, 2 * hid:]
sP, sQ, sO = (nh * L * L, L * L), (L * ld, hd), (L * hid, hd)
kw = dict(batch=Bz * nh, nh=nh)
fl = 2.0 * Bz * nh * L * L * hd
wide_only = lambda f: (lambda tile: f(tile))
no_wide = lambda f: (lambda tile: f(tile) if tile == 128 else None)
ab("attn Q.K^T  L=1024 hd=64 batch 96", fl, wide_only(lambda tile: (lambda: H.gemm(q, k, S, L, L, hd, a_kind=H.ROW, b_kind=H.ROW, lda=ld, ldb=ld, ldc=L, sA=sQ,
                                                                                     sB=sQ, sC=sP, alpha=hd ** -0.5, tile=tile, **kw))))
ab("attn dP     L=1024 hd=64 batch 96", fl, wide_only(lambda tile: (lambda: H.gemm(dO, v, S, L, L, hd, a_kind=H.ROW, b_kind=H.ROW, lda=hid, ldb=ld, ldc=L, sA=sO,
                                                                                     sB=sQ, sC=sP, tile=tile, **kw))))
ab("attn P.V    L=1024 hd=64 batch 96", fl, no_wide(lambda tile: (lambda: H.gemm(P, v, O, L, hd, L, a_kind=H.ROW, b_kind=H.COL, lda=L, ldb=ld, ldc=hid, sA=sP,
                                                                                   sB=sQ, sC=sO, tile=tile, **kw))))
ab("attn dV     L=1024 hd=64 batch 96", fl, no_wide(lambda tile: (lambda: H.gemm(P, dO, dv, L, hd, L, a_kind=H.COL, b_kind=H.COL, lda=L, ldb=hid, ldc=ld, sA=sP,
                                                                                   sB=sO, sC=sQ, tile=tile, **kw))))
