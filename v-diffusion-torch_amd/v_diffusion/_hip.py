"""ctypes binding of libvdiff_hip.so (C ABI: include/vdiff_hip.h, include/vdiff_phema.h for the post-hoc EMA entries and
include/vdiff_blur.h, prefix vdx_, for the blur operator of DPS).

PyTorch is used only for device memory and streams: every function here takes torch CUDA(HIP) tensors,
passes raw pointers + the current stream to the HIP library and returns nothing the library allocated.
There is NO fallback: a missing library, a CPU tensor or a non-zero return code raises.
"""
import ctypes as C
import os
import re

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "vdiff_hip.h")
PHEMA_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "vdiff_phema.h")      # the post-hoc EMA entries: a table of their own
BLUR_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "vdiff_blur.h")        # the blur operator of DPS: a table and a prefix of its own
LIB_PATH = os.environ.get("VDIFF_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libvdiff_hip.so")   # (override: A/B builds)

ROW, COL, IM2COL = 0, 1, 2
TILE_WIDE = 128256            # gemm(tile=...): force the 128x256 split-operand form (N % 256 == 0); 128 keeps the 128x128 tiles
RS_NONE, RS_DOWN, RS_UP = 0, 1, 2
OUT_TYPES = {"v": 0, "x0": 1, "eps": 2, "both": 3}
REWEIGHTS = {"constant": 0, "snr": 1, "snr_trunc": 2, "snr_1plus": 3}

_i32, _i64, _f32, _vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class GemmDesc(C.Structure):
    _fields_ = [("A", _vp), ("B", _vp), ("C", _vp), ("bias", _vp), ("R", _vp),
                ("M", _i32), ("N", _i32), ("K", _i32), ("a_kind", _i32), ("b_kind", _i32),
                ("lda", _i64), ("ldb", _i64), ("ldc", _i64), ("ldr", _i64),
                ("batch", _i32), ("nh", _i32),
                ("sAb", _i64), ("sAh", _i64), ("sBb", _i64), ("sBh", _i64),
                ("sCb", _i64), ("sCh", _i64), ("sRb", _i64), ("sRh", _i64),
                ("alpha", _f32), ("accumulate", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32),
                ("splitk", _i32), ("ws", _vp), ("ws_bytes", _i64), ("tile", _i32),
                ("colsum", _vp), ("colsum_accumulate", _i32), ("stats", _vp), ("stats_hw", _i32), ("sBias", _i64)]


_BY_VALUE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
             "float": C.c_float, "double": C.c_double}
_RETURNS = {**_BY_VALUE, "int": C.c_int, "const char*": C.c_char_p}
_STRUCTS = {"vd_gemm_desc": GemmDesc}          # `const <struct>*` parameters bound to their ctypes mirror; every other pointer is c_void_p
_DECL = re.compile(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(vd_\w+)\s*\(([^()]*)\)\s*;")
BLUR_PREFIX = "vdx_"


def _parse_header(text, prefix="vd_"):
    """The declarations of the C header whose names start with ``prefix``: ({name: (return type, [parameter, ...])} of the product entries,
    the same of the entries inside #ifdef VD_PROBES ... #endif), each in header order, types and parameters as whitespace-normalised C text
    ("const float* xt")."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    decl = _DECL if prefix == "vd_" else re.compile(_DECL.pattern.replace("vd_", re.escape(prefix)))
    tables = ({}, {})
    for i, part in enumerate(re.split(r"#ifdef\s+VD_PROBES\b(.*?)#endif", text, flags=re.S)):       # odd parts: inside the #ifdef
        decls = decl.findall(part)
        if len(decls) != len(re.findall(r"\b" + re.escape(prefix) + r"\w+\s*\(", part)):
            raise RuntimeError(f"{HEADER_PATH}: a {prefix}* declaration is not of the form `type {prefix}name(parameters);`")
        for ret, name, params in decls:
            if name in tables[0] or name in tables[1]:
                raise RuntimeError(f"{HEADER_PATH}: {name} is declared twice")
            params = [" ".join(q.split()) for q in params.split(",")]
            tables[i % 2][name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return tables


def _ctypes_of(name, ret, params):
    """(restype, [argtypes]) of one parsed declaration.  A by-value type outside _BY_VALUE / _RETURNS raises: there is no default type."""
    def arg(q):
        ctype = q.rpartition(" ")[0]
        if "*" in q:
            m = re.fullmatch(r"const (\w+)\*", ctype)
            return C.POINTER(_STRUCTS[m.group(1)]) if m and m.group(1) in _STRUCTS else _vp
        if ctype not in _BY_VALUE:
            raise RuntimeError(f"{HEADER_PATH}: {name}: no ctypes type for the parameter `{q}`")
        return _BY_VALUE[ctype]
    if ret not in _RETURNS:
        raise RuntimeError(f"{HEADER_PATH}: {name}: no ctypes type for the return type `{ret}`")
    return _RETURNS[ret], [arg(q) for q in params]


def _header_signatures(path=None, prefix="vd_"):
    path = path or HEADER_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the ctypes binding is read from the C header of the source tree")
    with open(path) as f:
        tables = _parse_header(f.read(), prefix)
    return [{name: _ctypes_of(name, *decl) for name, decl in t.items()} for t in tables]


# name -> (restype, [argtypes]) of every entry point the header declares.  PROBE_EXPORTS: the extra entry points of libvdiff_hip_probe.so
# (built with -DVD_PROBES; tests/probe/*.py load it through VDIFF_HIP_LIB): bound when the loaded library has them, absent from the product
# library
_SIGNATURES, PROBE_EXPORTS = _header_signatures()
EXPORTS = tuple(_SIGNATURES)
# the same for include/vdiff_phema.h (vd_adamw_emas, vd_ema_combine): bound by the same rule, required of the library like the rest
def _phema_signatures(path=None):
    """the product table of include/vdiff_phema.h; a name vdiff_hip.h declares too is named, not bound twice (_parse_header sees one header)"""
    path = path or PHEMA_HEADER_PATH
    table, probe = _header_signatures(path)
    twice = sorted((set(table) | set(probe)) & (set(_SIGNATURES) | set(PROBE_EXPORTS)))
    if twice or probe:
        raise RuntimeError(f"{path}: {twice or sorted(probe)} also declared in {HEADER_PATH}" if twice else f"{path}: probe entries belong in {HEADER_PATH}")
    return table


PHEMA_SIGNATURES = _phema_signatures()


# the same for include/vdiff_blur.h (vdx_dps_residual_blur, vdx_blur_planes), under its own prefix
def _blur_signatures(path=None):
    """the product table of include/vdiff_blur.h: its vdx_* declarations.  It declares no vd_* name (those belong to the two recorded
    tables above) and no probe entry, and those two headers declare no vdx_* name: no name stands in two headers"""
    path = path or BLUR_HEADER_PATH
    table, probe = _header_signatures(path, BLUR_PREFIX)
    other = [n for t in _header_signatures(path) for n in t]
    if other or probe:
        raise RuntimeError(f"{path}: {other} belong in {HEADER_PATH} or {PHEMA_HEADER_PATH}: this header declares {BLUR_PREFIX}* names only"
                           if other else f"{path}: probe entries belong in {HEADER_PATH}")
    for elsewhere in (HEADER_PATH, PHEMA_HEADER_PATH):
        stray = [n for t in _header_signatures(elsewhere, BLUR_PREFIX) for n in t]
        if stray:
            raise RuntimeError(f"{elsewhere}: {stray} belong in {BLUR_HEADER_PATH}")
    return table


BLUR_SIGNATURES = _blur_signatures()

_lib = None


def lib():
    """Load the HIP library (raises if it has not been built -- there is no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (or make -C v-diffusion-torch_amd/csrc). "
                "The v_diffusion hot path has no CPU/PyTorch fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in (*_SIGNATURES.items(), *PHEMA_SIGNATURES.items(), *BLUR_SIGNATURES.items()):
            fn = getattr(l, name)           # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        for name, (res, args) in PROBE_EXPORTS.items():
            if hasattr(l, name):
                fn = getattr(l, name)
                fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


class HipError(RuntimeError):
    pass


_CPU_TENSOR = "v_diffusion HIP op received a CPU tensor: the hot path runs on an MI355X only (no CPU fallback)"


def _check(rc, what):
    if rc != 0:
        raise HipError(f"{what} failed (rc={rc}): {lib().vd_last_error().decode(errors='replace')}")


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError(_CPU_TENSOR)
    if t.dtype not in (torch.float32, torch.float64, torch.uint8, torch.int32):
        raise HipError(f"unsupported dtype {t.dtype}")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def _host_floats(k, n):
    """the `const float*` argument of an entry point that reads n coefficients on the host: a ctypes array of them, or None (NULL) for None"""
    return None if k is None else (_f32 * n)(*[float(v) for v in k])


def _table_ptr(table):
    """device pointer of the int64 item table of a *_batched entry point"""
    assert table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()
    return table.data_ptr()


_ws_cache = {}

# When set to a list, the matmul-shaped wrappers append (kernel_name, flops, start_event, end_event) per launch
# (bench.py uses it for the live roofline figure; events sit on the stream the kernels are launched on).  Names are the
# rocprofv3 kernel names: gemm_dma_kernel<BM, BN, a_kind, b_kind, splitk, KT, TR> with kinds 0 = ROW, 1 = COL, 2 = IM2COL
# (TR = transposed-accumulator epilogue, taken by launches without output statistics).
PROFILE = None
PROFILE_BYTES = {}            # kernel name -> [algorithmic bytes (operands read + written once) summed over its recorded launches, launches]
_KIND = {0: "ROW", 1: "COL", 2: "IM2COL"}


def _note_bytes(name, nbytes):
    if PROFILE is not None:
        e = PROFILE_BYTES.setdefault(name, [0.0, 0])
        e[0] += float(nbytes)
        e[1] += 1


def tile_fields(code):
    """vd_gemm_last_tile code (csrc/common.h: vd_tile_code) -> (transposed epilogue, split-operand form, K tile [0: register-staged kernel], BM, BN)"""
    flags = code // 100000000
    return bool(flags & 1), flags >= 2, (code // 1000000) % 100, (code // 1000) % 1000, code % 1000


class _Timed:
    """event pair around a launch; with PROFILE set, a clean exit appends (*_record(), start_event, end_event)"""
    def __init__(self, name, amount, rename=None):
        self.name, self.amount, self.rename = name, amount, rename

    def __enter__(self):
        if PROFILE is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROFILE is not None and exc[0] is None:
            self.e1.record()
            PROFILE.append(self._record() + (self.e0, self.e1))


class _TimedTile(_Timed):
    """(rocprof name of the tile-engine instantiation that ran, from vd_gemm_last_tile; flops)"""
    def _record(self):
        tr, spl, kt, bm, bn = tile_fields(lib().vd_gemm_last_tile())
        name = self.name.format(tile=f"{bm}, {bn}", kt=f"{kt}, {'true' if tr else 'false'}")
        if spl:
            name = name.replace("gemm_dma_kernel", "gemm_split_kernel")
        if spl and (bm, bn) == (256, 256):          # round 6: the 8-wave 256x256 form of the grouped weight-gradient launches (its rocprof name)
            name = "wgrad_planes256_kernel" + name[name.index(">") + 1:]
        if kt == 0:
            name = name.replace("gemm_dma_kernel", "gemm_kernel").replace(", 0, false>", ">")
        return name, self.amount


class _TimedName(_Timed):
    """(fixed kernel name, flops): launches whose instantiation does not come from vd_gemm_last_tile"""
    def _record(self):
        return self.name, self.amount


class _TimedBytes(_Timed):
    """HBM-bound launch: ("hbm:<rocprof kernel name>", algorithmic bytes = operands read + written once).  ``rename`` (optional) is
    called after the launch and returns the name of the instantiation that ran."""
    def _record(self):
        return "hbm:" + (self.rename() if self.rename else self.name), float(self.amount)


def _two_parts(parts):
    """[(part, C, chunks)] of one or two channel-concatenated sources -> the six arguments of the *_from_partials entry points"""
    (p1, c1, k1), (p2, c2, k2) = parts[0], (parts[1] if len(parts) > 1 else (None, 0, 0))
    return ptr(p1), c1, k1, ptr(p2), c2, k2


def _resampled(H, W, resample):
    """(Ho, Wo) of an (H, W) image behind the RS_* resampling of the GroupNorm-apply kernels: the one statement of that rule (the engine
    sizes its buffers by it; a host helper, not a launch wrapper, hence not among the public names)"""
    return (H // 2, W // 2) if resample == RS_DOWN else ((H * 2, W * 2) if resample == RS_UP else (H, W))


def _resampled_hw(H, W, resample):
    Ho, Wo = _resampled(H, W, resample)
    return Ho * Wo


def _wgrad_args(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, dbias, Cin_w, Cout_w, accumulate, ws):
    return (ptr(x), ldx, ptr(dy), lddy, nimg, H, W, Cin, Cout, ptr(dw), ptr(dbias), Cin_w, Cout_w, int(accumulate), ws.data_ptr(),
            ws.numel() * 4)


def workspace(nbytes, device, tag="default"):
    """Per-(device, stream, tag) scratch buffer, grown on demand.  Kernels on one stream are ordered, so a scratch
    region can be reused by the next launch on the same stream."""
    key = (device, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((max(int(nbytes), 1 << 20) + 3) // 4, dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


# ----------------------------------------------------------------------------------------------- wrappers
def gemm(A, B, Cm, M, N, K, *, a_kind=ROW, b_kind=ROW, lda, ldb, ldc, bias=None, R=None, ldr=0, batch=1, nh=1,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), sR=(0, 0), alpha=1.0, accumulate=False, splitk=1, tile=0, colsum=None,
         colsum_accumulate=False, stats=None, stats_hw=0, sBias=0):
    d = GemmDesc()
    d.A, d.B, d.C, d.bias, d.R = ptr(A), ptr(B), ptr(Cm), ptr(bias), ptr(R)
    d.M, d.N, d.K, d.a_kind, d.b_kind = M, N, K, a_kind, b_kind
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.batch, d.nh = batch, nh
    (d.sAb, d.sAh), (d.sBb, d.sBh), (d.sCb, d.sCh), (d.sRb, d.sRh) = sA, sB, sC, sR
    d.alpha, d.accumulate = alpha, int(accumulate)
    d.splitk, d.tile = splitk, tile
    d.colsum, d.colsum_accumulate = ptr(colsum), int(colsum_accumulate)
    d.stats, d.stats_hw = ptr(stats), stats_hw
    d.sBias = sBias
    if splitk > 1:
        ws = workspace(splitk * (M * N + M) * 4, A.device, "splitk")
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    with _TimedTile("gemm_dma_kernel<{tile}, " + f"{a_kind}, {b_kind}, " + ("true, {kt}>" if splitk > 1 else "false, {kt}>"),
                2.0 * M * N * K * batch):
        _check(lib().vd_gemm(C.byref(d), stream()), "vd_gemm")


GROUP_MAX = 36
GROUPED_WGRAD = os.environ.get("VD_GROUPED_WGRAD", "1") != "0"   # A/B switch: 0 = one launch per weight-gradient GEMM


def gemm_grouped_wgrad(entries, M, N, K, lda, ldb, ldc, splitk):
    """entries: [(A = dY rows [K][M], B = X rows [K][N], C = dW [M][N], colsum = dbias [M] or None)], at most GROUP_MAX, all of one shape:
    C = A^T B (+ colsum) for every entry in ONE launch (vd_gemm_grouped_wgrad)"""
    n = len(entries)
    assert 0 < n <= GROUP_MAX
    arr = lambda i: (_vp * n)(*[ptr(e[i]) for e in entries])
    has_cs = entries[0][3] is not None
    assert all((e[3] is not None) == has_cs for e in entries)
    S = max(1, int(splitk))
    ws = workspace(lib().vd_gemm_grouped_wgrad_ws_bytes(n, M, N, S), entries[0][0].device, "splitk")
    with _TimedTile("gemm_dma_kernel<{tile}, 1, 1, true, 32, true, true>", 2.0 * M * N * K * n):
        _check(lib().vd_gemm_grouped_wgrad(arr(0), arr(1), arr(2), arr(3) if has_cs else None, n, M, N, K, lda, ldb, ldc, S,
                                           ws.data_ptr(), ws.numel() * 4, stream()), "vd_gemm_grouped_wgrad")


def last_row_tile():
    """BM of the calling thread's last vd_gemm / vd_conv3x3 launch (chunk size of its output statistics = BM/2)"""
    return tile_fields(lib().vd_gemm_last_tile())[3]


def stats_part_numel(nimg, HW, Cc):
    """floats needed for the GroupNorm partials of an (nimg, HW, Cc) output, whatever row tile the launch picks"""
    return nimg * max(HW // 32, 1) * 2 * Cc


def gn_stats_from_partials(parts, nimg, HW, stats, G=32, eps=1e-6):
    """parts: [(part, C, chunks)] for one or two channel-concatenated sources"""
    _check(lib().vd_gn_stats_from_partials(*_two_parts(parts), nimg, HW, G, eps, ptr(stats), stream()),
           "vd_gn_stats_from_partials")


def gn_coef_from_partials(parts, nimg, HW, gamma, beta, film, coef, G=32, eps=1e-6):
    _check(lib().vd_gn_coef_from_partials(*_two_parts(parts), nimg, HW, G, eps, ptr(gamma), ptr(beta), ptr(film),
                                          ptr(coef), stream()), "vd_gn_coef_from_partials")


WINO = os.environ.get("VD_WINO", "1") != "0"      # A/B switch: 0 sends every 3x3 convolution to the direct implicit GEMM


def wino_supported(nimg, H, W, Cin, Cout, ldx, ldy, ldres=0):
    return WINO and bool(lib().vd_conv3x3_wino_supported(nimg, H, W, Cin, Cout, ldx, ldy, ldres))


def wino_pack(w, Cout, Cin, uf=None, ud=None):
    _check(lib().vd_wino_pack(ptr(w), Cout, Cin, ptr(uf), ptr(ud), stream()), "vd_wino_pack")


def wino_pack_batched(table, n, total_blocks):
    _check(lib().vd_wino_pack_batched(_table_ptr(table), n, total_blocks, stream()), "vd_wino_pack_batched")


def conv3x3_wino(x, ldx, U, bias, y, ldy, nimg, H, W, Cin, Cout, res=None, ldres=0, stats_part=None):
    """Winograd F(2x2,3x3) form (see vd_conv3x3_wino); `flops` recorded = the direct convolution's (algorithmic) count, of
    which the matrix cores execute 4/9"""
    with _TimedName("wino_conv_kernel<{tw}, {ns}, {st}, false, 0>", 2.0 * nimg * H * W * Cout * 9 * Cin) as t:
        _check(lib().vd_conv3x3_wino(ptr(x), ldx, ptr(U), ptr(bias), ptr(res), ldres, ptr(y), ldy, nimg, H, W, Cin, Cout,
                                     ptr(stats_part), stream()), "vd_conv3x3_wino")
        if PROFILE is not None:
            k = lib().vd_wino_last_kernel()
            if k < 0:                       # the 128-tile ("wide") form
                k = -k
                t.name = f"wino_conv_wide_kernel<{k // 2000}, {(k // 2) % 1000}, {'true' if k & 1 else 'false'}>"
            else:
                t.name = t.name.format(tw=k // 2000, ns=(k // 2) % 1000, st="true" if k & 1 else "false")
            _note_bytes(t.name, 4.0 * (nimg * H * W * (Cin + Cout + (Cout if res is not None else 0)) + 16 * Cout * Cin))


def mfma_calibrate(seconds=1.5, blocks=256, iters=20000):
    """Run the register-only fp32 MFMA loop of vd_mfma_calibrate back to back for `seconds` (the part's clock settles under load) and
    return (in-kernel clock in MHz, TFLOP/s) of the last launch: a figure bench lines from different boxes can be normalised by."""
    import time
    sink = torch.zeros(1, device="cuda")
    stamps = torch.zeros(2 * blocks, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_end = time.perf_counter() + seconds
    ms = 0.0
    while True:
        e0.record()
        _check(lib().vd_mfma_calibrate(sink.data_ptr(), stamps.data_ptr(), blocks, iters, 12345, stream()), "vd_mfma_calibrate")
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if time.perf_counter() >= t_end:
            break
    st = stamps.view(blocks, 2).double().cpu()
    mhz = float((st[:, 0] / st[:, 1].clamp(min=1)).median()) * 100.0
    tflops = blocks * 8 * iters * 16 * 2048.0 / (ms * 1e-3) / 1e12
    return mhz, tflops


WINO43 = os.environ.get("VD_WINO43", "1") != "0"  # A/B switch: 0 keeps the input gradients on F(2x2,3x3)
WINO43_MIN_W = int(os.environ.get("VD_WINO43_MIN_W", "16"))   # A/B switch: 32 keeps the 16x16 layers on F(2x2,3x3)


# occupancy rule between F(4x4,3x3) and F(2x2,3x3) (vd_conv3x3_wino43_preferred: small batches keep the finer F(2x2,3x3) items);
# VD_WINO43_OCC=0: F(4x4,3x3) wherever served (A/B switch)
WINO43_OCC = os.environ.get("VD_WINO43_OCC", "1") != "0"


def wino43_preferred(nimg, H, W, N):
    return not WINO43_OCC or bool(lib().vd_conv3x3_wino43_preferred(nimg, H, W, N))


def wino43_supported(nimg, H, W, Cin, Cout, lddy, lddx):
    """input gradient of a Cin -> Cout convolution on (nimg, H, W) images through F(4x4,3x3)?"""
    return (WINO and WINO43 and W >= WINO43_MIN_W and bool(lib().vd_conv3x3_dgrad_wino43_supported(nimg, H, W, Cin, Cout, lddy, lddx))
            and wino43_preferred(nimg, H, W, Cin))


def wino43_pack(w, Cout, Cin, U43):
    _check(lib().vd_wino43_pack(ptr(w), Cout, Cin, ptr(U43), stream()), "vd_wino43_pack")


def wino43_pack_batched(table, n, total_blocks):
    _check(lib().vd_wino43_pack_batched(_table_ptr(table), n, total_blocks, stream()), "vd_wino43_pack_batched")


# forward convolutions of the 16x16 / 32x32 / 64-wide layers through F(4x4,3x3) with the dyadic interpolation points (csrc/wino43.hip:
# 1.78x fewer matrix-core cycles than F(2x2,3x3), ~2x its output error, inside the stated 2e-5 bound); VD_WINO43_FWD=0 keeps F(2x2,3x3)
WINO43_FWD = os.environ.get("VD_WINO43_FWD", "1") != "0"


def wino43_fwd_supported(nimg, H, W, Cin, Cout, ldx, ldy, ldres=0):
    return (WINO and WINO43_FWD and bool(lib().vd_conv3x3_wino43_fwd_supported(nimg, H, W, Cin, Cout, ldx, ldy, ldres))
            and wino43_preferred(nimg, H, W, Cout))


def wino43_pack_fwd(w, Cout, Cin, U43f):
    _check(lib().vd_wino43_pack_fwd(ptr(w), Cout, Cin, ptr(U43f), stream()), "vd_wino43_pack_fwd")


def wino43_fwd_chunk_rows(H, W):
    return int(lib().vd_conv3x3_wino43_fwd_chunk_rows(H, W))


def conv3x3_wino43_fwd(x, ldx, U43f, bias, y, ldy, nimg, H, W, Cin, Cout, res=None, ldres=0, stats_part=None):
    """y = conv3x3(x, w) + bias (+ res) as Winograd F(4x4,3x3) (vd_conv3x3_wino43_fwd); `flops` recorded = the direct convolution's
    (algorithmic) count, of which the matrix cores execute 1/4"""
    name = f"wino43_conv_kernel<{W // 4}, true>"
    with _TimedName(name, 2.0 * nimg * H * W * Cout * 9 * Cin):
        _check(lib().vd_conv3x3_wino43_fwd(ptr(x), ldx, ptr(U43f), ptr(bias), ptr(res), ldres, ptr(y), ldy, nimg, H, W, Cin, Cout,
                                           ptr(stats_part), stream()), "vd_conv3x3_wino43_fwd")
    _note_bytes(name, 4.0 * (nimg * H * W * (Cin + Cout + (Cout if res is not None else 0)) + 36 * Cout * Cin))


# forward 3x3 convolutions through PLANES (csrc/wino43.hip: V transform -> 36 plane GEMMs on the split-operand tile engine -> output
# transform) where vd_conv3x3_fwd_planes_preferred says they beat the fused kernel; a training forward keeps V on the tape and the weight
# gradient skips its input transform.  CONV_PLANES (VD_CONV_PLANES): "0" never, "1" by that rule, "2" wherever supported (tests, A/B runs)
CONV_PLANES = os.environ.get("VD_CONV_PLANES", "1")


def conv3x3_fwd_planes_preferred(nimg, H, W, Cin, Cout, training):
    return bool(lib().vd_conv3x3_fwd_planes_preferred(nimg, H, W, Cin, Cout, int(bool(training))))


def conv_planes_supported(nimg, H, W, Cin, Cout, ldx, ldy, ldres=0, training=False):
    """does the forward convolution of this call go through planes?  A training forward (``training``: the tape keeps V in place of the
    input) also needs the F(4x4,3x3) weight gradient, the only reader of V, to serve the geometry."""
    if CONV_PLANES == "0" or not (WINO and WINO43_FWD):
        return False
    if not lib().vd_conv3x3_wino43_fwd_planes_supported(nimg, H, W, Cin, Cout, ldx, ldy, ldres):
        return False
    if training and not wgrad43_supported(nimg, H, W, Cin, Cout, Cin, Cout):
        return False
    return CONV_PLANES == "2" or conv3x3_fwd_planes_preferred(nimg, H, W, Cin, Cout, training)


def conv3x3_wino43_fwd_planes(x, ldx, w, bias, y, ldy, nimg, H, W, Cin, Cout, res=None, ldres=0, stats_part=None, v=None):
    """y = conv3x3(x, w) + bias (+ res) through planes (vd_conv3x3_wino43_fwd_planes); ``w``: the raw [Cout][Cin][3][3] kernel.  ``v``: the
    tensor that receives V (vd_conv3x3_wino43_v_floats floats; a training forward keeps it for the weight gradient) -- None: scratch."""
    nv = lib().vd_conv3x3_wino43_v_floats(nimg, H, W, Cin)
    if v is None:
        v = workspace(nv * 4, x.device, "planes_v")
    assert v.numel() >= nv and w.is_contiguous() and tuple(w.shape) == (Cout, Cin, 3, 3)
    ws = workspace(lib().vd_conv3x3_wino43_fwd_planes_ws_bytes(nimg, H, W, Cin, Cout), x.device, "planes")
    args = (ptr(x), ldx, ptr(w), ptr(bias), ptr(res), ldres, ptr(y), ldy, nimg, H, W, Cin, Cout, ptr(stats_part), ptr(v), ws.data_ptr(),
            ws.numel() * 4)
    phase = lambda ph: _check(lib().vd_conv3x3_wino43_fwd_planes(*args, ph, stream()), "vd_conv3x3_wino43_fwd_planes")
    if PROFILE is None:
        phase(7)
        return
    T = nimg * (H // 4) * (W // 4)
    with _TimedBytes("wino43_wgrad_transform_kernel", 4.0 * nimg * H * W * Cin * (1 + 2.25)):
        phase(1)
    # the 36 planes as ONE batched launch of the tile engine, recorded under that instantiation's name with the work it EXECUTES (a quarter
    # of the direct convolution's 2*M*N*K: the name carries no tag a reader could scale by)
    with _TimedTile("gemm_dma_kernel<{tile}, 0, 0, false, {kt}>", 2.0 * 36 * T * Cout * Cin):
        phase(2)
    _note_bytes(PROFILE[-1][0], 4.0 * 36.0 * (T * (Cin + Cout) + Cout * Cin))
    with _TimedBytes("wino43_out_transform_kernel", 4.0 * (36.0 * T * Cout + nimg * H * W * Cout * (2 if res is not None else 1))):
        phase(4)


# input gradients through PLANES (csrc/wino43.hip: dM = A dY A^T, the image the weight gradient makes of dy anyway -> 36 plane GEMMs on the
# split-operand tile engine -> overlap-add pass) in training steps whose forward kept V: dy is transformed once for both gradients.
# DGRAD_PLANES (VD_DGRAD_PLANES): "0" never, "1" where vd_conv3x3_dgrad_planes_preferred says it beats the fused kernel, "2" wherever supported
DGRAD_PLANES = os.environ.get("VD_DGRAD_PLANES", "1")


def dgrad_planes_supported(nimg, H, W, Cin, Cout, lddy, lddx):
    """does the input gradient of this Cin -> Cout call (dy at pitch lddy, dx at pitch lddx) go through planes, GIVEN that its forward kept V?
    The F(4x4,3x3) weight gradient, the other reader of dM, must serve the geometry too."""
    if DGRAD_PLANES == "0" or not (WINO and WINO43):
        return False
    if lddy % 4 or not lib().vd_conv3x3_wino43_dgrad_planes_supported(nimg, H, W, Cin, Cout, lddx):
        return False
    if not wgrad43_supported(nimg, H, W, Cin, Cout, Cin, lddy):
        return False
    return DGRAD_PLANES == "2" or bool(lib().vd_conv3x3_dgrad_planes_preferred(nimg, H, W, Cin, Cout, 1))


def conv3x3_wino43_dy_image(dy, lddy, nimg, H, W, Cout, dm):
    """dm = A dY A^T (vd_conv3x3_wino43_dy_image): the image of dy both gradients of a planes layer read"""
    assert dm.numel() >= lib().vd_conv3x3_wino43_dm_floats(nimg, H, W, Cout)
    with _TimedBytes("wino43_wgrad_transform_kernel", 4.0 * nimg * H * W * Cout * (1 + 2.25)):
        _check(lib().vd_conv3x3_wino43_dy_image(ptr(dy), lddy, nimg, H, W, Cout, ptr(dm), stream()), "vd_conv3x3_wino43_dy_image")


def conv3x3_wgrad_wino43_vm(v, dm, nimg, H, W, Cin, Cout, dw, Cin_w, Cout_w, accumulate=False, dbias=None):
    """F(4x4,3x3) weight gradient with both images given (vd_conv3x3_wgrad_wino43_vm): the 36 grouped GEMMs and the fold alone"""
    assert v.numel() == lib().vd_conv3x3_wino43_v_floats(nimg, H, W, Cin) and dm.numel() >= lib().vd_conv3x3_wino43_dm_floats(nimg, H, W, Cout)
    ws = workspace(lib().vd_conv3x3_wgrad_wino43_ws_bytes(nimg, H, W, Cin, Cout), dm.device, "wgrad43")
    args = (ptr(v), ptr(dm), nimg, H, W, Cin, Cout, ptr(dw), ptr(dbias), Cin_w, Cout_w, int(accumulate), ws.data_ptr(), ws.numel() * 4)
    phase = lambda ph: _check(lib().vd_conv3x3_wgrad_wino43_vm(*args, ph, stream()), "vd_conv3x3_wgrad_wino43_vm")
    if PROFILE is None:
        phase(7)
        return
    with _TimedTile("gemm_dma_kernel<{tile}, 1, 1, true, {kt}, true> " + W43_WGRAD_TAG, 2.0 * nimg * H * W * Cout * 9 * Cin):
        phase(2)
    _note_bytes(PROFILE[-1][0], 4.0 * (36.0 * nimg * (H // 4) * (W // 4) * (Cin + Cout) + 36.0 * Cout * Cin))
    with _TimedName("wino43_wgrad_finish_kernel", 0.0):
        phase(4)


def conv3x3_wino43_dgrad_planes(dm, w, dx, lddx, nimg, H, W, Cin, Cout):
    """dx = input gradient of the Cin -> Cout 3x3 convolution through planes (vd_conv3x3_wino43_dgrad_planes); ``dm``: the image of dy from
    conv3x3_wino43_dy_image, ``w``: the raw [Cout][Cin][3][3] kernel"""
    assert dm.numel() >= lib().vd_conv3x3_wino43_dm_floats(nimg, H, W, Cout) and w.is_contiguous() and tuple(w.shape) == (Cout, Cin, 3, 3)
    ws = workspace(lib().vd_conv3x3_wino43_dgrad_planes_ws_bytes(nimg, H, W, Cin, Cout), dm.device, "dgrad_planes")
    args = (ptr(dm), ptr(w), ptr(dx), lddx, nimg, H, W, Cin, Cout, ws.data_ptr(), ws.numel() * 4)
    phase = lambda ph: _check(lib().vd_conv3x3_wino43_dgrad_planes(*args, ph, stream()), "vd_conv3x3_wino43_dgrad_planes")
    if PROFILE is None:
        phase(7)
        return
    T = nimg * (H // 4) * (W // 4)
    with _TimedBytes("wino43_pack_planes_t_kernel", 4.0 * (9 + 36) * Cout * Cin):
        phase(1)
    # the 36 planes as ONE batched launch of the tile engine, under that instantiation's name with the work it EXECUTES
    with _TimedTile("gemm_dma_kernel<{tile}, 0, 0, false, {kt}>", 2.0 * 36 * T * Cout * Cin):
        phase(2)
    _note_bytes(PROFILE[-1][0], 4.0 * 36.0 * (T * (Cin + Cout) + Cout * Cin))
    with _TimedBytes("wino43_in_transpose_kernel", 4.0 * (36.0 * T * Cin + nimg * H * W * Cin)):
        phase(4)


def conv3x3_dgrad_wino43(dy, lddy, U43, dx, lddx, nimg, H, W, Cin, Cout):
    """dx = input gradient of the Cin -> Cout 3x3 convolution (Winograd F(4x4,3x3), see vd_conv3x3_dgrad_wino43); `flops` recorded =
    the direct convolution's (algorithmic) count, of which the matrix cores execute 1/4"""
    with _TimedName(f"wino43_conv_kernel<{W // 4}, false>", 2.0 * nimg * H * W * Cout * 9 * Cin):
        _check(lib().vd_conv3x3_dgrad_wino43(ptr(dy), lddy, ptr(U43), ptr(dx), lddx, nimg, H, W, Cin, Cout, stream()),
               "vd_conv3x3_dgrad_wino43")
    _note_bytes(f"wino43_conv_kernel<{W // 4}, false>", 4.0 * (nimg * H * W * (Cin + Cout) + 36 * Cout * Cin))


def conv3x3(x, ldx, wpack, bias, y, ldy, nimg, H, W, Cin, Cout, res=None, ldres=0, accumulate=False, stats_part=None):
    with _TimedTile("gemm_dma_kernel<{tile}, 2, 0, false, {kt}>", 2.0 * nimg * H * W * Cout * 9 * Cin):
        _check(lib().vd_conv3x3(ptr(x), ldx, ptr(wpack), ptr(bias), ptr(res), ldres, ptr(y), ldy, nimg, H, W, Cin, Cout,
                                int(accumulate), ptr(stats_part), stream()), "vd_conv3x3")


def conv3x3_wgrad_wino(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, Cin_w, Cout_w, accumulate=False, dbias=None):
    nb = lib().vd_conv3x3_wgrad_wino_ws_bytes(nimg, H, W, Cin, Cout)
    ws = workspace(nb, x.device, "wgrad")
    args = _wgrad_args(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, dbias, Cin_w, Cout_w, accumulate, ws)
    if PROFILE is None:
        _check(lib().vd_conv3x3_wgrad_wino(*args, stream()), "vd_conv3x3_wgrad_wino")
        return
    # per-kernel timing: the MFMA kernel and the plane reduction get their own event pairs (same kernels, same order)
    tws = min(W // 2, 16)
    with _TimedName(f"wino_wgrad_kernel<{tws}, {'true' if dbias is not None else 'false'}>", 2.0 * nimg * H * W * Cout * 9 * Cin):
        _check(lib().vd_conv3x3_wgrad_wino_phase(*args, 1, stream()), "vd_conv3x3_wgrad_wino_phase")
    with _TimedName("wino_wgrad_reduce_kernel", 0.0):
        _check(lib().vd_conv3x3_wgrad_wino_phase(*args, 2, stream()), "vd_conv3x3_wgrad_wino_phase")


# weight gradients on a side stream beside the input-gradient / GroupNorm chain of backward (engine._cwgrad): -0.9 ms per CIFAR step,
# -7 ms per CelebA step, same-box A/B; VD_WGRAD_STREAM=0 keeps everything on one stream
WGRAD_STREAM = os.environ.get("VD_WGRAD_STREAM", "1") != "0"
# slab count of the grouped 1x1 / linear weight gradients from vd_gemm_grouped_wgrad_auto_split (whole residency rounds: -0.5 ms per CIFAR
# step against the fixed 1024-workgroup rule, same-box A/B); VD_GROUPED_AUTO_SPLIT=0: that rule
GROUPED_AUTO_SPLIT = os.environ.get("VD_GROUPED_AUTO_SPLIT", "1") != "0"
# data-parallel runs (a gradient reducer listens to backward): report gradients ready after every residual / attention block (1) or at
# UNet-level boundaries only (0: fewer, larger grouped weight-gradient launches; buckets leave in bursts)
GN_FOLD = os.environ.get("VD_GN_FOLD", "1") != "0"       # A/B switch: 0 = statistics finalize and apply as two launches
GN_FOLD_MAX_CHUNKS = int(os.environ.get("VD_GN_FOLD_MAX_CHUNKS", "8"))     # most chunks per image the folded form re-reduces per workgroup
READY_PER_BLOCK = os.environ.get("VD_READY_PER_BLOCK", "0") != "0"
# a training forward outside the flat-buffer trainer returns a CHAIN of autograd nodes cut at the engine's progress points, so that the
# reference's own DDP(model) (train.py:141-148) sees gradients -- and launches its bucket all-reduces -- while backward still runs
# (models/unet.py::_SegFn); 0 = one node for the whole network (A/B switch: same kernels, same results bit for bit, no overlap)
AUTOGRAD_CHAIN = os.environ.get("VD_AUTOGRAD_CHAIN", "1") != "0"
WINO43_WGRAD = os.environ.get("VD_WINO43_WGRAD", "1") != "0"   # A/B switch: 0 keeps every weight gradient on F(2x2,3x3)
# fewest 4x4-output tiles (= K of the 36 GEMMs) it is picked for: 512 = 8x8 images at batch 128 (256 -> 256: x1.17, 768 -> 768: x1.41 over the fused
# F(2x2,3x3) kernel, same-box A/B tests/perf_wgrad43.py); the library serves nothing below 512
WINO43_WGRAD_MIN_TILES = int(os.environ.get("VD_WINO43_WGRAD_MIN_TILES", "512"))


W43_WGRAD_TAG = "[36 planes of the F(4x4,3x3) weight gradient]"


def wgrad43_supported(nimg, H, W, Cin, Cout, ldx, lddy):
    return (WINO and WINO43_WGRAD and nimg * (H // 4) * (W // 4) >= WINO43_WGRAD_MIN_TILES
            and bool(lib().vd_conv3x3_wgrad_wino43_supported(nimg, H, W, Cin, Cout, ldx, lddy)))


def conv3x3_wgrad_wino43(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, Cin_w, Cout_w, accumulate=False, dbias=None, v=None):
    """F(4x4,3x3) weight gradient, unfused (vd_conv3x3_wgrad_wino43): transforms -> 36 grouped GEMMs -> finish.  ``v``: the V image of x
    that conv3x3_wino43_fwd_planes left behind -- the transform pass then runs its dy half alone (x is not read and may be None)"""
    nb = lib().vd_conv3x3_wgrad_wino43_ws_bytes(nimg, H, W, Cin, Cout)
    ws = workspace(nb, dy.device, "wgrad43")
    if v is not None:
        assert v.numel() == lib().vd_conv3x3_wino43_v_floats(nimg, H, W, Cin)
        vargs = (ptr(v), ptr(dy), lddy, nimg, H, W, Cin, Cout, ptr(dw), ptr(dbias), Cin_w, Cout_w, int(accumulate), ws.data_ptr(),
                 ws.numel() * 4)
        phase = lambda ph: _check(lib().vd_conv3x3_wgrad_wino43_v(*vargs, ph, stream()), "vd_conv3x3_wgrad_wino43_v")
    else:
        args = _wgrad_args(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, dbias, Cin_w, Cout_w, accumulate, ws)
        phase = lambda ph: _check(lib().vd_conv3x3_wgrad_wino43_phase(*args, ph, stream()), "vd_conv3x3_wgrad_wino43_phase")
    if PROFILE is None:
        if v is not None:
            phase(7)
        else:
            _check(lib().vd_conv3x3_wgrad_wino43(*args, stream()), "vd_conv3x3_wgrad_wino43")
        return
    with _TimedBytes("wino43_wgrad_transform_kernel", 4.0 * nimg * H * W * ((Cin if v is None else 0) + Cout) * (1 + 2.25)):
        phase(1)
    # the 36 planes run as ONE grouped launch of the tile engine: recorded under that instantiation's rocprof name (from vd_gemm_last_tile),
    # tagged so that the bench knows its recorded work is the direct convolution's 2*M*N*K, of which the planes execute 1/4
    with _TimedTile("gemm_dma_kernel<{tile}, 1, 1, true, {kt}, true> " + W43_WGRAD_TAG, 2.0 * nimg * H * W * Cout * 9 * Cin) as t:
        phase(2)
    # (its operands are the transformed images: 36 planes of [tiles][Cin] and [tiles][Cout], read once, + the 36 x Cout x Cin result)
    _note_bytes(PROFILE[-1][0], 4.0 * (36.0 * nimg * (H // 4) * (W // 4) * (Cin + Cout) + 36.0 * Cout * Cin))
    with _TimedName("wino43_wgrad_finish_kernel", 0.0):
        phase(4)


def conv3x3_wgrad(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, Cin_w, Cout_w, accumulate=False, dbias=None, direct=False, v=None):
    """weight (and bias) gradient of the 3x3 convolution: Winograd-domain kernels wherever the geometry is served -- F(4x4,3x3)
    unfused for the large layers, F(2x2,3x3) fused otherwise (VD_WINO=0 or direct=True: the implicit GEMM over pixels).  ``v``: the forward
    through planes kept V in place of x (conv_planes_supported(training=True) promised the F(4x4,3x3) weight gradient for this geometry)"""
    if v is not None:
        if direct or not wgrad43_supported(nimg, H, W, Cin, Cout, Cin, lddy):
            raise HipError("conv3x3_wgrad: a V image was kept for a geometry the F(4x4,3x3) weight gradient does not serve")
        return conv3x3_wgrad_wino43(None, Cin, dy, lddy, nimg, H, W, Cin, Cout, dw, Cin_w, Cout_w, accumulate, dbias, v=v)
    if not direct and wgrad43_supported(nimg, H, W, Cin, Cout, ldx, lddy):
        return conv3x3_wgrad_wino43(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, Cin_w, Cout_w, accumulate, dbias)
    if WINO and not direct and lib().vd_conv3x3_wgrad_wino_supported(nimg, H, W, Cin, Cout, ldx, lddy):
        return conv3x3_wgrad_wino(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, Cin_w, Cout_w, accumulate, dbias)
    nb = lib().vd_conv3x3_wgrad_ws_bytes(nimg, H, W, Cin, Cout)
    ws = workspace(nb, x.device, "wgrad")
    args = _wgrad_args(x, ldx, dy, lddy, nimg, H, W, Cin, Cout, dw, dbias, Cin_w, Cout_w, accumulate, ws)
    flops = 2.0 * nimg * H * W * Cout * 9 * Cin
    if PROFILE is None:
        _check(lib().vd_conv3x3_wgrad(*args, stream()), "vd_conv3x3_wgrad")
        return
    # per-kernel timing: the MFMA kernel and the slab reduction get their own event pairs (same kernels, same order)
    with _TimedTile("gemm_dma_kernel<{tile}, 1, 2, true, {kt}>", flops):
        _check(lib().vd_conv3x3_wgrad_phase(*args, 1, stream()), "vd_conv3x3_wgrad_phase")
    with _TimedTile("reduce_slabs_oihw_kernel", 0.0):
        _check(lib().vd_conv3x3_wgrad_phase(*args, 2, stream()), "vd_conv3x3_wgrad_phase")


def im2col3x3(x, ldx, xc, nimg, H, W, Cc):
    _check(lib().vd_im2col3x3(ptr(x), ldx, ptr(xc), nimg, H, W, Cc, stream()), "vd_im2col3x3")


def tap_gather(z, ldz, bias, out, ldo, nimg, H, W, Cout):
    _check(lib().vd_tap_gather(ptr(z), ldz, ptr(bias), ptr(out), ldo, nimg, H, W, Cout, stream()), "vd_tap_gather")


def tap_spread(dy, lddy, dz, ldz, nimg, H, W, Cout):
    _check(lib().vd_tap_spread(ptr(dy), lddy, ptr(dz), ldz, nimg, H, W, Cout, stream()), "vd_tap_spread")


def thin_wgrad_finish(g, Cout_w, Cin, Cin_w, dw, accumulate=False, colsum=None, cs_stride=1, cs_off=0, dbias=None):
    _check(lib().vd_thin_wgrad_finish(ptr(g), Cout_w, Cin, Cin_w, ptr(dw), int(accumulate), ptr(colsum), cs_stride, cs_off,
                                      ptr(dbias), stream()), "vd_thin_wgrad_finish")


def pack_conv3x3(w, Cout_w, Cin_w, wf=None, Cin_p=0, wd=None, Cout_p=0):
    _check(lib().vd_pack_conv3x3(ptr(w), Cout_w, Cin_w, ptr(wf), Cin_p, ptr(wd), Cout_p, stream()), "vd_pack_conv3x3")


def pack_conv3x3_batched(table, n, total_blocks):
    """table: int64 device tensor [n][8], see vd_pack_conv3x3_batched"""
    _check(lib().vd_pack_conv3x3_batched(_table_ptr(table), n, total_blocks, stream()), "vd_pack_conv3x3_batched")


def gn_stats(x, ldx, nimg, HW, Cc, stats, G=32, eps=1e-6):
    nb = lib().vd_gn_ws_bytes(nimg, HW, Cc)
    ws = workspace(nb, x.device, "gn")
    _check(lib().vd_gn_stats(ptr(x), ldx, nimg, HW, Cc, G, eps, ptr(stats), ws.data_ptr(), ws.numel() * 4, stream()),
           "vd_gn_stats")


def _gn_bwd_name():
    k = lib().vd_gn_bwd_last_kernel()
    if k > 0:
        split, k = k // 100000000, k % 100000000         # (sibling workgroups per image slab: the SPLIT form of round 5)
        nt, k = k >= 1000000, k % 1000000
        return f"gn_bwd_fused_kernel<{k // 10000}, {k % 10000}, {'true' if nt else 'false'}, {'true' if split else 'false'}>"
    return "gn_bwd_apply_kernel (two-pass form)" if k < 0 else "gn_bwd_apply_kernel (resample)"


def gn_apply(x, ldx, stats, gamma, beta, film, act, p_drop, seed, resample, y, ldy, nimg, H, W, Cc, coef, G=32):
    with _TimedBytes("gn_apply_kernel" if gamma is not None else "gn_apply_kernel (resample)", 4.0 * nimg * Cc * (H * W + _resampled_hw(H, W, resample))):
        _gn_apply(x, ldx, stats, gamma, beta, film, act, p_drop, seed, resample, y, ldy, nimg, H, W, Cc, coef, G)


def gn_apply_from_partials(x, ldx, parts, gamma, beta, film, act, p_drop, seed, resample, y, ldy, nimg, H, W, Cc, coef, G=32, eps=1e-6):
    """statistics from the producers' partial sums + apply in one launch (vd_gn_apply_from_partials); parts: [(part, C, chunks)] x 1 or 2"""
    with _TimedBytes("gn_apply_kernel", 4.0 * nimg * Cc * (H * W + _resampled_hw(H, W, resample))):
        _check(lib().vd_gn_apply_from_partials(ptr(x), ldx, *_two_parts(parts), ptr(gamma), ptr(beta), ptr(film), int(act),
                                               float(p_drop), int(seed), resample, ptr(y), ldy, nimg, H, W, Cc, G, eps, ptr(coef), stream()),
               "vd_gn_apply_from_partials")


def _gn_apply(x, ldx, stats, gamma, beta, film, act, p_drop, seed, resample, y, ldy, nimg, H, W, Cc, coef, G=32):
    _check(lib().vd_gn_apply(ptr(x), ldx, ptr(stats), ptr(gamma), ptr(beta), ptr(film), int(act), float(p_drop), int(seed),
                             resample, ptr(y), ldy, nimg, H, W, Cc, G, ptr(coef), stream()), "vd_gn_apply")


def gn_apply_bwd(dy, lddy, x, ldx, coef, gamma, beta, film, act, p_drop, seed, resample, add, ldadd, dx, lddx,
                 accumulate_dx, dfilm, dgamma, dbeta, accumulate_params, nimg, H, W, Cc, G=32, pgb_keep=None):
    """pgb_keep ([nimg][2][Cc] floats): leave the per-image dgamma / dbeta terms there for one gn_param_sums_batched launch over
    all norms of the backward pass instead of summing them here (dgamma / dbeta are then not touched)"""
    nb = lib().vd_gn_ws_bytes(nimg, H * W, Cc)
    ws = workspace(nb, dy.device, "gn")
    nbytes = 4.0 * nimg * Cc * (_resampled_hw(H, W, resample) + H * W * (1 + (gamma is not None) + (add is not None) + bool(accumulate_dx)))
    with _TimedBytes("gn_apply_bwd", nbytes, rename=_gn_bwd_name):
        if pgb_keep is not None:
            _check(lib().vd_gn_apply_bwd_keep(ptr(dy), lddy, ptr(x), ldx, ptr(coef), ptr(gamma), ptr(beta), ptr(film), int(act),
                                              float(p_drop), int(seed), resample, ptr(add), ldadd, ptr(dx), lddx, int(accumulate_dx),
                                              ptr(dfilm), ptr(pgb_keep), nimg, H, W, Cc, G, ws.data_ptr(), ws.numel() * 4, stream()),
                   "vd_gn_apply_bwd_keep")
        else:
            _gn_apply_bwd_call(dy, lddy, x, ldx, coef, gamma, beta, film, act, p_drop, seed, resample, add, ldadd, dx, lddx,
                               accumulate_dx, dfilm, dgamma, dbeta, accumulate_params, nimg, H, W, Cc, G, ws)


def gn_param_sums_batched(table, n, total_blocks):
    _check(lib().vd_gn_param_sums_batched(_table_ptr(table), n, total_blocks, stream()), "vd_gn_param_sums_batched")


def _gn_apply_bwd_call(dy, lddy, x, ldx, coef, gamma, beta, film, act, p_drop, seed, resample, add, ldadd, dx, lddx,
                       accumulate_dx, dfilm, dgamma, dbeta, accumulate_params, nimg, H, W, Cc, G, ws):
    _check(lib().vd_gn_apply_bwd(ptr(dy), lddy, ptr(x), ldx, ptr(coef), ptr(gamma), ptr(beta), ptr(film), int(act),
                                 float(p_drop), int(seed), resample, ptr(add), ldadd, ptr(dx), lddx, int(accumulate_dx),
                                 ptr(dfilm), ptr(dgamma), ptr(dbeta), int(accumulate_params), nimg, H, W, Cc, G,
                                 ws.data_ptr(), ws.numel() * 4, stream()), "vd_gn_apply_bwd")


def colsum(x, ldx, M, N, out, accumulate=False):
    nb = lib().vd_colsum_ws_bytes(M, N)
    ws = workspace(nb, x.device, "colsum")
    _check(lib().vd_colsum(ptr(x), ldx, M, N, ptr(out), int(accumulate), ws.data_ptr(), ws.numel() * 4, stream()), "vd_colsum")


def axpby(x, ldx, alpha, y, ldy, beta, rows, Cc):
    _check(lib().vd_axpby(ptr(x), ldx, alpha, ptr(y), ldy, beta, rows, Cc, stream()), "vd_axpby")


def silu(x, y):
    _check(lib().vd_silu(ptr(x), ptr(y), x.numel(), stream()), "vd_silu")


def silu_bwd(x, dy, dx, accumulate=False):
    _check(lib().vd_silu_bwd(ptr(x), ptr(dy), ptr(dx), x.numel(), int(accumulate), stream()), "vd_silu_bwd")


def softmax_rows(s, rows, L):
    _check(lib().vd_softmax_rows(ptr(s), rows, L, stream()), "vd_softmax_rows")


def softmax_rows_bwd(p, dp, rows, L, alpha):
    _check(lib().vd_softmax_rows_bwd(ptr(p), ptr(dp), rows, L, alpha, stream()), "vd_softmax_rows_bwd")


FUSED_ATTN = os.environ.get("VD_FUSED_ATTN", "1")            # A/B switch: 0 = three-launch attention everywhere, 2 = fused wherever served


def attn_supported(L, hd, backward):
    """is the geometry served by the fused kernels (csrc/attn.hip: L % 64 == 0, head dim 64 / 128 / 256, forward and backward)?"""
    return FUSED_ATTN != "0" and bool(lib().vd_attn_supported(L, hd, int(backward)))


def attn_use_fused(L, hd, rows, training):
    """Which attention path a block takes.  Inference: the fused forward wherever it is served (faster at every measured shape).
    Training (forward + backward with recomputation: 9 products where the three-launch path runs 6) by same-box measurement at
    batch 128 (tests/perf_attn.py, MI355X): head dim 64 fused except at L = 256 (0.144 vs 0.128 ms); head dim 128 / 256 unfused (the
    backward kernels hold Q/dO or K/V fragments of the whole head dim in registers: one wave per SIMD at head dim 256 -- L = 1024:
    5.3 vs 3.6 ms) -- unless the materialised [rows, L, L] maps would not be reasonable to keep (>= 4 GiB each), where the fused
    path is the only sensible one.  VD_FUSED_ATTN=2 forces the fused kernels wherever served (parity tests of the whole step)."""
    if not attn_supported(L, hd, training):
        return False
    if not training or FUSED_ATTN == "2":
        return True
    if 4.0 * rows * L * L >= float(1 << 32):
        return True
    return hd == 64 and L != 256


def attn_fwd(q, k, v, ld, o, ldo, lse, B, nh, L, hd, scale):
    """fused softmax(scale q k^T) v; FLOPs recorded = the two products (4 L^2 hd per image and head)"""
    with _TimedName(f"attn_fwd_kernel<{hd}>", 4.0 * B * nh * L * L * hd):
        _check(lib().vd_attn_fwd(ptr(q), ptr(k), ptr(v), ld, ptr(o), ldo, ptr(lse), B, nh, L, hd, scale, stream()), "vd_attn_fwd")


def attn_bwd(q, k, v, ld, o, ldo, dout, lddo, lse, delta, dq, dk, dv, ldd, B, nh, L, hd, scale):
    """backward of attn_fwd (recomputes the probabilities).  FLOPs recorded are ALGORITHMIC: the four products of the backward
    (dP, dQ to the first kernel, dV, dK to the second; 2 L^2 hd each per image and head) -- the kernels execute 3 + 4 = 7 of
    them (the logits in both, dP again in the second), so their executed MFMA rate is 7/4 of the recorded one"""
    args = (ptr(q), ptr(k), ptr(v), ld, ptr(o), ldo, ptr(dout), lddo, ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), ldd, B, nh, L, hd,
            scale)
    if PROFILE is None:
        _check(lib().vd_attn_bwd(*args, stream()), "vd_attn_bwd")
        return
    unit = 2.0 * B * nh * L * L * hd
    with _TimedName(f"attn_bwd_dq_kernel<{hd}>", 2 * unit):
        _check(lib().vd_attn_bwd_phase(*args, 1, stream()), "vd_attn_bwd_phase")
    with _TimedName(f"attn_bwd_dkv_kernel<{hd}>", 2 * unit):
        _check(lib().vd_attn_bwd_phase(*args, 2, stream()), "vd_attn_bwd_phase")


def nchw_to_nhwc(x, y, nimg, Cc, H, W, ldy):
    _check(lib().vd_nchw_to_nhwc(ptr(x), ptr(y), nimg, Cc, H, W, ldy, stream()), "vd_nchw_to_nhwc")


def nhwc_to_nchw(x, ldx, y, nimg, Cc, H, W):
    _check(lib().vd_nhwc_to_nchw(ptr(x), ldx, ptr(y), nimg, Cc, H, W, stream()), "vd_nhwc_to_nchw")


def images_to_uint8_hwc(x, out, n, Cc, HW):
    _check(lib().vd_images_to_uint8_hwc(ptr(x), ptr(out), n, Cc, HW, stream()), "vd_images_to_uint8_hwc")


def images_from_uint8_hwc(u8, flip, out, n, Cc, H, W):
    _check(lib().vd_images_from_uint8_hwc(ptr(u8), ptr(flip), ptr(out), n, Cc, H, W, stream()), "vd_images_from_uint8_hwc")


def timestep_embedding(t, out, n, dim, scale=1000.0):
    if t.dtype != torch.float64:
        raise HipError("timestep_embedding expects fp64 timesteps")
    _check(lib().vd_timestep_embedding(ptr(t), ptr(out), n, dim, scale, stream()), "vd_timestep_embedding")


def class_embed(y, w, bias, temb, n, emb, ncls):
    _check(lib().vd_class_embed(ptr(y), ptr(w), ptr(bias), ptr(temb), n, emb, ncls, stream()), "vd_class_embed")


def class_embed_bwd(y, dtemb, dw, dbias, n, emb, ncls, accumulate=False):
    _check(lib().vd_class_embed_bwd(ptr(y), ptr(dtemb), ptr(dw), ptr(dbias), n, emb, ncls, int(accumulate), stream()),
           "vd_class_embed_bwd")


def multitag_norm(y, out, n, ncls):
    _check(lib().vd_multitag_norm(ptr(y), ptr(out), n, ncls, stream()), "vd_multitag_norm")


def q_sample(x0, eps, logsnr, xt, n, Cc, HW):
    _check(lib().vd_q_sample(ptr(x0), ptr(eps), ptr(logsnr), ptr(xt), n, Cc, HW, stream()), "vd_q_sample")


def loss_fwd(x0, eps, xt, out, logsnr, mot, rw, loss, aux, n, Cc, HW):
    _check(lib().vd_loss_fwd(ptr(x0), ptr(eps), ptr(xt), ptr(out), ptr(logsnr), mot, rw, ptr(loss), ptr(aux), n, Cc, HW,
                             stream()), "vd_loss_fwd")


def loss_bwd(x0, eps, xt, out, logsnr, aux, gloss, mot, rw, dout, n, Cc, HW):
    _check(lib().vd_loss_bwd(ptr(x0), ptr(eps), ptr(xt), ptr(out), ptr(logsnr), ptr(aux), ptr(gloss), mot, rw, ptr(dout),
                             n, Cc, HW, stream()), "vd_loss_bwd")


def bpd_terms(x0, xt, out, coef, mot, clip, kl, nll, pred, mse, n, Cc, HW):
    _check(lib().vd_bpd_terms(ptr(x0), ptr(xt), ptr(out), ptr(coef), mot, int(clip), ptr(kl), ptr(nll), ptr(pred), ptr(mse),
                              n, Cc, HW, stream()), "vd_bpd_terms")


def bpd_bwd(x0, xt, out, coef, use_kl, gloss, mot, clip, dout, n, Cc, HW):
    _check(lib().vd_bpd_bwd(ptr(x0), ptr(xt), ptr(out), ptr(coef), ptr(use_kl), ptr(gloss), mot, int(clip), ptr(dout),
                            n, Cc, HW, stream()), "vd_bpd_bwd")


def sample_step(xt, out, noise, k8, mot, cfg, last, clip, xn, xdup, n, Cc, HW, k_dev=None):
    """k8: 8 host floats, or None with k_dev = device tensor of 8 floats (graph-replayable form)"""
    arr = _host_floats(k8, 8)
    _check(lib().vd_sample_step(ptr(xt), ptr(out), ptr(noise), arr, ptr(k_dev), mot, int(cfg), int(last), int(clip), ptr(xn),
                                ptr(xdup), n, Cc, HW, stream()), "vd_sample_step")


def bpd_terms_lv(x0, xt, out, coef, mot, clip, kl, nll, pred, mse, n, Cc, HW):
    """bpd_terms for a learned-variance output (Cp + C channels; coef slots 5, 6 = lvmin, delta)"""
    _check(lib().vd_bpd_terms_lv(ptr(x0), ptr(xt), ptr(out), ptr(coef), mot, int(clip), ptr(kl), ptr(nll), ptr(pred), ptr(mse),
                                 n, Cc, HW, stream()), "vd_bpd_terms_lv")


def bpd_bwd_lv(x0, xt, out, coef, use_kl, gloss, mot, clip, mean_grad, dout, n, Cc, HW):
    """dout has Cp + C channels; mean_grad = False writes zeros to the prediction channels"""
    _check(lib().vd_bpd_bwd_lv(ptr(x0), ptr(xt), ptr(out), ptr(coef), ptr(use_kl), ptr(gloss), mot, int(clip), int(mean_grad), ptr(dout),
                               n, Cc, HW, stream()), "vd_bpd_bwd_lv")


def hybrid_loss_fwd(x0, eps, xt, out, logsnr, coef, use_kl, mot, rw, vlb_weight, loss, aux, n, Cc, HW):
    """loss = mse on the prediction channels + vlb_weight * bound term; aux: n x 4 floats"""
    _check(lib().vd_hybrid_loss_fwd(ptr(x0), ptr(eps), ptr(xt), ptr(out), ptr(logsnr), ptr(coef), ptr(use_kl), mot, rw, float(vlb_weight),
                                    ptr(loss), ptr(aux), n, Cc, HW, stream()), "vd_hybrid_loss_fwd")


def hybrid_loss_bwd(x0, eps, xt, out, logsnr, coef, use_kl, aux, gloss, mot, rw, vlb_weight, dout, n, Cc, HW):
    _check(lib().vd_hybrid_loss_bwd(ptr(x0), ptr(eps), ptr(xt), ptr(out), ptr(logsnr), ptr(coef), ptr(use_kl), ptr(aux), ptr(gloss), mot, rw,
                                    float(vlb_weight), ptr(dout), n, Cc, HW, stream()), "vd_hybrid_loss_bwd")


def sample_step_lv(xt, out, noise, k10, mot, cfg, last, clip, xn, xdup, n, Cc, HW):
    """sample_step for a learned-variance output; k10: 10 host floats (slot 5 = lvmin, slot 8 = delta); noise may be None"""
    arr = _host_floats(k10, 10)
    _check(lib().vd_sample_step_lv(ptr(xt), ptr(out), ptr(noise), arr, mot, int(cfg), int(last), int(clip), ptr(xn), ptr(xdup),
                                   n, Cc, HW, stream()), "vd_sample_step_lv")


def distill_mid(zt, tout, coef, tmot, cfg, clip, xhat, dhat, zmid, zdup, n, Cc, HW):
    _check(lib().vd_distill_mid(ptr(zt), ptr(tout), ptr(coef), tmot, int(cfg), int(clip), ptr(xhat), ptr(dhat), ptr(zmid), ptr(zdup),
                                n, Cc, HW, stream()), "vd_distill_mid")


def distill_loss_fwd(xhat, dhat, zmid, tout, zt, sout, coef, tmot, smot, cfg, clip, loss, resid, xtilde, n, Cc, HW):
    _check(lib().vd_distill_loss_fwd(ptr(xhat), ptr(dhat), ptr(zmid), ptr(tout), ptr(zt), ptr(sout), ptr(coef), tmot, smot, int(cfg), int(clip),
                                     ptr(loss), ptr(resid), ptr(xtilde), n, Cc, HW, stream()), "vd_distill_loss_fwd")


def distill_loss_bwd(resid, coef, gloss, smot, dout, n, Cc, HW):
    _check(lib().vd_distill_loss_bwd(ptr(resid), ptr(coef), ptr(gloss), smot, ptr(dout), n, Cc, HW, stream()), "vd_distill_loss_bwd")


CONSIST_METRICS = {"l2": 0, "huber": 1}


def consist_mid(zt, tout, coef, tmot, cfg, clip, zs, dz, xhat, n, Cc, HW):
    """xhat may be None"""
    _check(lib().vd_consist_mid(ptr(zt), ptr(tout), ptr(coef), tmot, int(cfg), int(clip), ptr(zs), ptr(dz), ptr(xhat), n, Cc, HW, stream()),
           "vd_consist_mid")


def consist_pair(x0, eps, coef, zt, zs, dz, n, Cc, HW):
    _check(lib().vd_consist_pair(ptr(x0), ptr(eps), ptr(coef), ptr(zt), ptr(zs), ptr(dz), n, Cc, HW, stream()), "vd_consist_pair")


def consist_loss_fwd(zt, zs, dz, sout, tout, coef, mot, metric, huber_c, loss, resid, aux, target, n, Cc, HW):
    """metric: 0 l2, 1 pseudo-Huber with the absolute constant huber_c; target may be None"""
    _check(lib().vd_consist_loss_fwd(ptr(zt), ptr(zs), ptr(dz), ptr(sout), ptr(tout), ptr(coef), mot, int(metric), float(huber_c), ptr(loss),
                                     ptr(resid), ptr(aux), ptr(target), n, Cc, HW, stream()), "vd_consist_loss_fwd")


def consist_loss_bwd(resid, coef, gloss, aux, mot, dout, n, Cc, HW):
    _check(lib().vd_consist_loss_bwd(ptr(resid), ptr(coef), ptr(gloss), ptr(aux), mot, ptr(dout), n, Cc, HW, stream()), "vd_consist_loss_bwd")


def ema_track_batched(table, n, total_blocks, decay):
    """table: int64 device tensor [n][8], see vd_ema_track_batched"""
    _check(lib().vd_ema_track_batched(_table_ptr(table), n, total_blocks, float(decay), stream()), "vd_ema_track_batched")


def solver_step(xt, out, hist, k8, mot, cfg, clip, xn, xdup, n, Cc, HW, k_dev=None):
    """k8: 8 host floats, or None with k_dev = device tensor of 8 floats (graph-replayable form)"""
    arr = _host_floats(k8, 8)
    _check(lib().vd_solver_step(ptr(xt), ptr(out), ptr(hist), arr, ptr(k_dev), mot, int(cfg), int(clip), ptr(xn), ptr(xdup),
                                n, Cc, HW, stream()), "vd_solver_step")


def unipc_step(xt, out, h0, h1, h2, k16, mot, cfg, clip, xn, xdup, xc_out, n, Cc, HW, k_dev=None):
    """one UniPC node: k16 = 16 host floats, or None with k_dev = device tensor of 16 floats (graph-replayable form); h0, h1, h2 = the
    last three guided predictions, shifted in place; xc_out (optional) receives the corrected state"""
    arr = _host_floats(k16, 16)
    _check(lib().vd_unipc_step(ptr(xt), ptr(out), ptr(h0), ptr(h1), ptr(h2), arr, ptr(k_dev), mot, int(cfg), int(clip), ptr(xn), ptr(xdup),
                               ptr(xc_out), n, Cc, HW, stream()), "vd_unipc_step")


def abs_kth_rows(x, n, N, r, kth):
    """kth[b] = the element of rank r of |x[b]| over n rows of N floats (vd_abs_kth_rows: exact radix select)"""
    _check(lib().vd_abs_kth_rows(ptr(x), n, int(N), int(r), ptr(kth), stream()), "vd_abs_kth_rows")


def solver_step_dyn(xt, out, hist, k8, mot, cfg, r, s_max, s_out, xn, xdup, n, Cc, HW, k_dev=None):
    """solver_step with the guided prediction thresholded at its rank-r magnitude (s_max = inf: no cap); s_out optional, n floats"""
    arr = _host_floats(k8, 8)
    _check(lib().vd_solver_step_dyn(ptr(xt), ptr(out), ptr(hist), arr, ptr(k_dev), mot, int(cfg), int(r), float(s_max), ptr(s_out),
                                    ptr(xn), ptr(xdup), n, Cc, HW, stream()), "vd_solver_step_dyn")


def inpaint_step(xt, out, noise, known, mask, knoise, k10, mot, cfg, last, clip, mask_c, xn, xdup, n, Cc, HW, k_dev=None):
    """sample_step merged with ak*known + bk*knoise by the mask (n x mask_c x HW floats, mask_c 1 or C; 1 keeps the known image).
    k10: sample_step's 8 host floats + (ak, bk), or None with k_dev = device tensor of 10 floats (graph-replayable form)"""
    arr = _host_floats(k10, 10)
    _check(lib().vd_inpaint_step(ptr(xt), ptr(out), ptr(noise), ptr(known), ptr(mask), ptr(knoise), arr, ptr(k_dev), mot, int(cfg),
                                 int(last), int(clip), int(mask_c), ptr(xn), ptr(xdup), n, Cc, HW, stream()), "vd_inpaint_step")


def forward_jump(x, noise, k2, xn, xdup, n, N, k_dev=None):
    """xn = a*x + b*noise over n rows of N floats (xdup optional: 2n interleaved rows); k2 = (a, b) host floats, or None with k_dev"""
    arr = _host_floats(k2, 2)
    _check(lib().vd_forward_jump(ptr(x), ptr(noise), arr, ptr(k_dev), ptr(xn), ptr(xdup), n, int(N), stream()), "vd_forward_jump")


def noise_extract(xt, out, x0, eps, k10, mot, cfg, last, clip, xs, z, xdup, n, Cc, HW, k_dev=None):
    """xs = ak*x0 + bk*eps and the noise map z = (xs - guided mean of sample_step)/k[5] (vd_noise_extract).  k10: inpaint_step's ten host
    floats, or None with k_dev = device tensor of 10 floats; eps may be None when bk = 0; xs may alias xt"""
    arr = _host_floats(k10, 10)
    _check(lib().vd_noise_extract(ptr(xt), ptr(out), ptr(x0), ptr(eps), arr, ptr(k_dev), mot, int(cfg), int(last), int(clip), ptr(xs),
                                  ptr(z), ptr(xdup), n, Cc, HW, stream()), "vd_noise_extract")


def slerp_rows(a, b, frac, out, w_out, n, N, frac_dev=None):
    """out = spherical interpolation of n pairs of rows of N floats (vd_slerp_rows); frac = one host float, or None with frac_dev =
    device tensor of n floats; w_out optional, n x 2 floats"""
    arr = _host_floats(None if frac is None else [frac], 1)
    _check(lib().vd_slerp_rows(ptr(a), ptr(b), arr, ptr(frac_dev), ptr(out), ptr(w_out), n, int(N), stream()), "vd_slerp_rows")


DPS_OPS = {"mask": 0, "down": 1, "gray": 2}


def dps_residual(xt, out, meas, mask, k8, mot, cfg, clip, op, par, dout, dxt, sumsq, x0hat, n, Cc, H, W):
    """r = meas - A g of the guided x0 prediction g, sumsq[b] = sum r^2 and the cotangents of (1/2)||r||^2: dout (the shape of out) for the
    network's VJP, dxt for the direct path (vd_dps_residual).  op: DPS_OPS; par = the mask's channel count (1 or C) / the down-sampling
    factor / unused; mask only for op 0; x0hat (optional) receives g.  k8: sample_step's 8 host floats"""
    arr = _host_floats(k8, 8)
    _check(lib().vd_dps_residual(ptr(xt), ptr(out), ptr(meas), ptr(mask), arr, mot, int(cfg), int(clip), int(op), int(par), ptr(dout),
                                 ptr(dxt), ptr(sumsq), ptr(x0hat), n, Cc, H, W, stream()), "vd_dps_residual")


BLUR_KMAX, BLUR_PLANE_MAX = 33, 4096         # VDX_BLUR_KMAX, VDX_BLUR_PLANE_MAX of include/vdiff_blur.h (tests/test_blur_cpu.py holds them together)


def dps_residual_blur(xt, out, meas, taps, k8, mot, cfg, clip, dout, dxt, sumsq, x0hat, n, Cc, H, W):
    """dps_residual for the blur operator (vdx_dps_residual_blur): taps = the (kh, kw) kernel on the device, fp32 contiguous, one for every
    sample and channel; cross-correlation, reflect boundary; meas of the image's shape.  The outputs are dps_residual's"""
    arr = _host_floats(k8, 8)
    _check(lib().vdx_dps_residual_blur(ptr(xt), ptr(out), ptr(meas), ptr(taps), arr, mot, int(cfg), int(clip), int(taps.shape[0]),
                                       int(taps.shape[1]), ptr(dout), ptr(dxt), ptr(sumsq), ptr(x0hat), n, Cc, H, W, stream()),
           "vdx_dps_residual_blur")


def blur_planes(x, taps, adjoint, y, planes, H, W):
    """y = A x, or A^T x with ``adjoint``, of ``planes`` planes of H x W floats under the blur operator of ``taps`` (vdx_blur_planes)"""
    _check(lib().vdx_blur_planes(ptr(x), ptr(taps), int(taps.shape[0]), int(taps.shape[1]), int(bool(adjoint)), ptr(y), planes, H, W, stream()),
           "vdx_blur_planes")


def dps_step(xt, out, noise, dxin, dxt, sumsq, k8, zeta, mot, cfg, last, clip, xn, xdup, n, Cc, HW):
    """sample_step, then xn -= zeta / sqrt(sumsq[b]) * (dxt[b] + the rows of dxin of sample b); the term is selected: zeta = 0 or
    sumsq[b] = 0 leaves sample_step's row (vd_dps_step).  xn may alias xt"""
    arr = _host_floats(k8, 8)
    _check(lib().vd_dps_step(ptr(xt), ptr(out), ptr(noise), ptr(dxin), ptr(dxt), ptr(sumsq), arr, float(zeta), mot, int(cfg), int(last),
                             int(clip), ptr(xn), ptr(xdup), n, Cc, HW, stream()), "vd_dps_step")


def ddnm_step(xt, out, noise, meas, mask, k8, lam, mot, cfg, last, clip, op, par, xn, xdup, sumsq, n, Cc, H, W):
    """sample_step, then xn += cw * A^+(meas - A g) on every preimage, g the guided x0 prediction and cw = lam on the last step, else
    c2 * lam (vd_ddnm_step).  Selected: lam = 0 leaves sample_step's row, a mask element 0 has no measurement.  op, par, mask, meas:
    dps_residual's; sumsq (optional, n floats) receives sum r^2 over the measured elements of each sample.  xn may alias xt"""
    arr = _host_floats(k8, 8)
    _check(lib().vd_ddnm_step(ptr(xt), ptr(out), ptr(noise), ptr(meas), ptr(mask), arr, float(lam), mot, int(cfg), int(last), int(clip),
                              int(op), int(par), ptr(xn), ptr(xdup), ptr(sumsq), n, Cc, H, W, stream()), "vd_ddnm_step")


def lsm_draw(hist, count, u, cdf, t_out, idx_out, w_out, T, K, B, uniform_prob):
    """B timesteps from B fp64 uniforms in proportion to the root mean square of each timestep's loss history (vd_lsm_draw): t_out fp64,
    idx_out int32, w_out fp32 = 1 / (T q_idx); cdf (T fp64) receives the distribution drawn from"""
    _check(lib().vd_lsm_draw(ptr(hist), ptr(count), ptr(u), ptr(cdf), ptr(t_out), ptr(idx_out), ptr(w_out), T, K, B, float(uniform_prob),
                             stream()), "vd_lsm_draw")


def lsm_update(hist, count, pos, idx, loss, n, T, K):
    """n rows (idx int32, loss fp32) enter the per-timestep rings in row order (vd_lsm_update); n = 0 is a no-op"""
    _check(lib().vd_lsm_update(ptr(hist), ptr(count), ptr(pos), ptr(idx), ptr(loss), n, T, K, stream()), "vd_lsm_update")


def sumsq(g, out1):
    ws = workspace(lib().vd_sumsq_ws_bytes(g.numel()), g.device, "sumsq")
    _check(lib().vd_sumsq(ptr(g), g.numel(), ptr(out1), ws.data_ptr(), ws.numel() * 4, stream()), "vd_sumsq")


def adamw_ema(p, g, m, v, ema, gnorm_sq, max_norm, lr, b1, b2, eps, wd, bc1, bc2, ema_decay, r_lo=0, r_hi=0, r_mode=0, r_bc1=1.0,
              r_bc2=1.0):
    """r_*: an index range treated apart this step, see vd_adamw_ema (1 = no gradient this step, 2 = own bias corrections)"""
    _check(lib().vd_adamw_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), ptr(gnorm_sq), max_norm, lr, b1, b2, eps,
                              wd, bc1, bc2, ema_decay, int(r_lo), int(r_hi), int(r_mode), r_bc1, r_bc2, stream()), "vd_adamw_ema")


def adamw_ema_flagged(p, g, m, v, ema, gnorm_sq, max_norm, lr, b1, b2, eps, wd, bc1, bc2, ema_decay, r_lo, r_hi, r_flag, r_steps):
    """the update with the [r_lo, r_hi) decision made on the device (vd_adamw_ema_flagged): r_flag = device float[1], r_steps = device
    int32[1] (advanced by the call when the flag is set)"""
    assert r_flag.dtype == torch.float32 and r_steps.dtype == torch.int32
    _check(lib().vd_adamw_ema_flagged(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), ptr(gnorm_sq), max_norm, lr, b1, b2, eps,
                                      wd, bc1, bc2, ema_decay, int(r_lo), int(r_hi), ptr(r_flag), ptr(r_steps), float(b1), float(b2),
                                      stream()), "vd_adamw_ema_flagged")


def adamw_emas(p, g, m, v, ema, gnorm_sq, max_norm, lr, b1, b2, eps, wd, bc1, bc2, ema_decay, pema, pema_rate, r_lo=0, r_hi=0, r_mode=0,
               r_bc1=1.0, r_bc2=1.0, r_flag=None, r_steps=None, n_pema=None):
    """adamw_ema (r_flag None) or adamw_ema_flagged (r_flag, r_steps given) with the power-function EMA shadows ``pema`` (1..4 flat
    tensors; an entry None is passed as NULL and refused) updated in the same pass at the rates ``pema_rate`` (the doubles 1 - beta_t of
    phema.power_ema_rate): vd_adamw_emas.  ``n_pema`` defaults to len(pema)"""
    if r_flag is not None:
        assert r_flag.dtype == torch.float32 and r_steps is not None and r_steps.dtype == torch.int32
    k = len(pema)
    shadows = (_vp * max(k, 1))(*[ptr(e) for e in pema])
    rates = (C.c_double * max(k, 1))(*[float(r) for r in pema_rate])
    _check(lib().vd_adamw_emas(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), ptr(gnorm_sq), max_norm, lr, b1, b2, eps, wd, bc1, bc2,
                               ema_decay, int(r_lo), int(r_hi), int(r_mode), r_bc1, r_bc2, ptr(r_flag), ptr(r_steps), float(b1), float(b2),
                               shadows, rates, k if n_pema is None else int(n_pema), stream()), "vd_adamw_emas")


def ema_combine(out, acc, src, w):
    """out (fp32, or None) = (float) s and acc (fp64, or None) = s with s = acc + sum_j w[j] src[j] in fp64, one fma per source in
    order (vd_ema_combine).  ``src``: up to 32 flat fp32 tensors of one length (None allowed where w[j] == 0: such a source is not read)"""
    k = len(src)
    n = (out if out is not None else acc if acc is not None else src[0]).numel()
    assert len(w) == k and all(s is None or (s.dtype == torch.float32 and s.numel() == n and s.is_contiguous()) for s in src)
    assert out is None or (out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n)
    assert acc is None or (acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() == n)
    srcs = (_vp * max(k, 1))(*[ptr(s) for s in src])
    ws = (C.c_double * max(k, 1))(*[float(x) for x in w])
    _check(lib().vd_ema_combine(ptr(out), ptr(acc), srcs, ws, k, n, stream()), "vd_ema_combine")


# ----------------------------------------------------------------------------------------------- k-NN precision / recall (metrics.hip)
KNN_K_STEP = 64                # feature length granule of the distance kernels (zero padding changes no distance)


def features_f16(x):
    """[n, d] fp16 device features as the distance kernels take them: contiguous, 16-byte aligned, d zero-padded to a multiple of
    KNN_K_STEP (a copy only when one of those does not hold already)"""
    if not x.is_cuda:
        raise HipError(_CPU_TENSOR)
    if x.dtype != torch.float16 or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise HipError(f"features must be a non-empty [n, d] float16 tensor, got {x.dtype} {tuple(x.shape)}")
    pad = -x.shape[1] % KNN_K_STEP
    if pad or not x.is_contiguous() or x.data_ptr() % 16:
        x = torch.nn.functional.pad(x, (0, pad)).contiguous()
    return x


def _dev_f16(x):
    if not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 2 and x.is_contiguous() and x.data_ptr() % 16 == 0
            and x.shape[1] % KNN_K_STEP == 0):
        raise HipError("distance kernels take features prepared by features_f16 (device fp16, contiguous, aligned, padded d)")
    return x.data_ptr()


def _dev_f32(x, n):
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == n):
        raise HipError(f"expected a contiguous device float32 tensor of {n} elements")
    return x.data_ptr()


def rows_sqnorm_f16(x):
    """fp32 squared norms of the rows of prepared features x (features_f16)"""
    n, d = x.shape
    sq = torch.empty(n, dtype=torch.float32, device=x.device)
    _check(lib().vd_rows_sqnorm_f16(_dev_f16(x), n, d, sq.data_ptr(), stream()), "vd_rows_sqnorm_f16")
    return sq


def knn_kth_f16(q, q_sq, c, c_sq, kth):
    """fp32 [nq]: kth-th smallest distance from each row of q to the rows of c (with multiplicity), prepared features + their norms"""
    nq, d = q.shape
    nc = c.shape[0]
    if c.shape[1] != d:
        raise HipError(f"feature lengths differ: {d} vs {c.shape[1]}")
    out = torch.empty(nq, dtype=torch.float32, device=q.device)
    nb = lib().vd_knn_kth_ws_bytes(nq, nc, kth)
    ws = workspace(nb, q.device, "knn")
    _check(lib().vd_knn_kth_f16(_dev_f16(q), _dev_f32(q_sq, nq), nq, _dev_f16(c), _dev_f32(c_sq, nc), nc, d, kth, out.data_ptr(),
                                ws.data_ptr(), ws.numel() * 4, stream()), "vd_knn_kth_f16")
    return out


def manifold_hits_f16(q, q_sq, s, s_sq, radius):
    """uint8 [nq]: 1 where a row of q lies within radius[j] (fp32) of some support row s_j, else 0"""
    nq, d = q.shape
    ns = s.shape[0]
    if s.shape[1] != d:
        raise HipError(f"feature lengths differ: {d} vs {s.shape[1]}")
    hit = torch.empty(nq, dtype=torch.uint8, device=q.device)
    ws = workspace(lib().vd_manifold_hits_ws_bytes(ns), q.device, "knn_hits")
    _check(lib().vd_manifold_hits_f16(_dev_f16(q), _dev_f32(q_sq, nq), nq, _dev_f16(s), _dev_f32(s_sq, ns), _dev_f32(radius, ns), ns, d,
                                      hit.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream()), "vd_manifold_hits_f16")
    return hit


# ----------------------------------------------------------------------------------------------- FID statistics / products (fid.hip)
def _dev_rows(x, dtype, what):
    """a 2-D device tensor of `dtype` whose rows are contiguous (any row pitch): (pointer, rows, columns, pitch)"""
    if not x.is_cuda:
        raise HipError(_CPU_TENSOR)
    if x.dtype != dtype or x.dim() != 2 or x.shape[0] < 1 or x.stride(1) != 1:
        raise HipError(f"{what} must be a non-empty 2-D {dtype} tensor with contiguous rows, got {x.dtype} {tuple(x.shape)} "
                       f"strides {tuple(x.stride())}")
    return x.data_ptr(), x.shape[0], x.shape[1], x.stride(0)


def _dev_f64(x, shape):
    if not (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and tuple(x.shape) == tuple(shape)):
        raise HipError(f"expected a contiguous device float64 tensor of shape {tuple(shape)}")
    return x.data_ptr()


def fid_shift(x, shift):
    """shift[d] (fp64) = the fp32-rounded column means of the fp32 batch x[n, d]: the centre the running sums of fid_accum refer to"""
    px, n, d, ldx = _dev_rows(x, torch.float32, "features")
    _check(lib().vd_fid_shift(px, n, d, ldx, _dev_f64(shift, (d,)), stream()), "vd_fid_shift")


def fid_accum(x, shift, sum_, outer):
    """sum_[d] += sum_i (x_i - shift), outer[d, d] += sum_i (x_i - shift)(x_i - shift)^T in fp64 for the fp32 batch x[n, d]; outer
    holds the lower triangle of 64 x 64 tiles only (include/vdiff_hip.h)"""
    px, n, d, ldx = _dev_rows(x, torch.float32, "features")
    _check(lib().vd_fid_accum(px, n, d, ldx, _dev_f64(shift, (d,)), _dev_f64(sum_, (d,)), _dev_f64(outer, (d, d)), stream()),
           "vd_fid_accum")


def atb_f64(A, B):
    """fp64 [m, n] = A^T B for fp64 device matrices A[k, m], B[k, n]"""
    pa, k, m, lda = _dev_rows(A, torch.float64, "A")
    pb, kb, n, ldb = _dev_rows(B, torch.float64, "B")
    if kb != k or A.device != B.device:
        raise HipError(f"A^T B needs operands with the same number of rows on one device: {tuple(A.shape)} vs {tuple(B.shape)}")
    Cm = torch.empty(m, n, dtype=torch.float64, device=A.device)
    _check(lib().vd_atb_f64(pa, pb, Cm.data_ptr(), k, m, n, lda, ldb, n, stream()), "vd_atb_f64")
    return Cm


# ----------------------------------------------------------------------------------------------- KID sums / Inception Score (kid.hip)
def kid_indices(idx, n, what="indices"):
    """a host index array as kid_sums takes it: a numpy int32 array [subsets, m] with every value in [0, n).  Raises ValueError
    otherwise; touches no device.  The kernels gather rows through these values unchecked (include/vdiff_hip.h), so this check is
    the only thing between a bad index and an out-of-bounds read."""
    if not isinstance(idx, np.ndarray) or idx.dtype != np.int32 or idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"{what} must be a numpy int32 array of shape [subsets, subset_size], got "
                         f"{getattr(idx, 'dtype', type(idx).__name__)} {getattr(idx, 'shape', ())}")
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= n:
        raise ValueError(f"{what} must lie in [0, {n}): found {lo if lo < 0 else hi}")
    return np.ascontiguousarray(idx)


def kid_sums(x, y, ix=None, iy=None, degree=3, gamma=None, coef0=1.0):
    """fp64 device tensor [subsets, 3]: per subset the polynomial-kernel sums (XX over positions i != j, YY likewise, XY over all
    pairs) of the rows x[ix[s]] and y[iy[s]] of the fp32 device features x[nx, d], y[ny, d] (include/vdiff_hip.h).  ix, iy: host
    int32 numpy arrays [subsets, m], or None for all rows of that set in order (then the other side is None or has one subset).
    Their shape and range are checked here, on the host, and the device copies are made here: there is no other way to hand
    indices to the kernel.  gamma=None means 1 / d."""
    px, nx, d, ldx = _dev_rows(x, torch.float32, "features")
    py, ny, dy, ldy = _dev_rows(y, torch.float32, "features")
    if dy != d or x.device != y.device:
        raise HipError(f"the two feature sets need one feature length and one device: {tuple(x.shape)} vs {tuple(y.shape)}")
    if ix is not None:
        ix = kid_indices(ix, nx, "ix")
    if iy is not None:
        iy = kid_indices(iy, ny, "iy")
    subsets = ix.shape[0] if ix is not None else (iy.shape[0] if iy is not None else 1)
    if iy is not None and iy.shape[0] != subsets:
        raise ValueError(f"ix and iy hold different numbers of subsets: {subsets} vs {iy.shape[0]}")
    mx = ix.shape[1] if ix is not None else nx
    my = iy.shape[1] if iy is not None else ny
    dix = torch.from_numpy(ix).to(x.device) if ix is not None else None
    diy = torch.from_numpy(iy).to(x.device) if iy is not None else None
    out = torch.empty(subsets, 3, dtype=torch.float64, device=x.device)
    ws = workspace(lib().vd_kid_ws_bytes(subsets, mx, my), x.device, "kid")
    _check(lib().vd_kid_sums(px, nx, ldx, py, ny, ldy, d, ptr(dix), ptr(diy), subsets, mx, my, 1.0 / d if gamma is None else float(gamma),
                             float(coef0), int(degree), out.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream()), "vd_kid_sums")
    return out


def is_scores(logits, splits):
    """fp64 device tensor [splits]: the Inception Score of each split of the fp32 device logits [n, classes] (include/vdiff_hip.h)"""
    pl, n, classes, ld = _dev_rows(logits, torch.float32, "logits")
    scores = torch.empty(max(int(splits), 1), dtype=torch.float64, device=logits.device)
    ws = workspace(lib().vd_is_ws_bytes(n, classes, int(splits)), logits.device, "is")
    _check(lib().vd_is_scores(pl, n, classes, ld, int(splits), scores.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream()), "vd_is_scores")
    return scores
