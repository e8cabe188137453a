/* vdiff_hip.h -- C ABI of libvdiff_hip.so: the MI355X (gfx950) kernels behind the
 * v-diffusion hot path (UNet forward/backward inside the diffusion train step + the DDIM/CFG
 * sampling loop of tqch/v-diffusion-torch).
 *
 * The reference has no FFI layer: its hot path bottoms out in ATen calls.  Each entry point
 * below replaces one of those call sites (cited as reference file:line) and is what a binding
 * of this path has to import -- see INTEGRATION.md for the ctypes stub.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch types.  All tensors are fp32 unless stated.
 *  - activations are NHWC: [image][y][x][channel] with an explicit per-pixel stride `ld`
 *    (in floats, multiple of 4, base 16-byte aligned) so channel slices of a wider buffer
 *    (the "virtual concat" of reference unet.py:315) can be read/written in place.
 *  - the library never allocates, frees or retains device memory; scratch comes in through
 *    `ws` arguments (size from the matching *_ws_bytes query).  Every launch goes to the
 *    `stream` argument (a hipStream_t passed as void*).  No host synchronisation anywhere,
 *    so every call is HIP-graph capturable.
 *  - return value: 0 on success, non-zero on error; vd_last_error() gives the message of
 *    the calling thread's last failure.
 */
#ifndef VDIFF_HIP_H
#define VDIFF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VD_VERSION 100

int         vd_version(void);
const char* vd_last_error(void);

/* Compute units the PERSISTENT convolution launches (vd_conv3x3_wino, vd_conv3x3_dgrad_wino43: one workgroup per CU holding all of its
 * LDS and registers for the whole launch, 0.1-1.5 ms) leave free: their grids are sized CUs - n.  A data-parallel rank sets it so that
 * the RCCL kernels of a gradient bucket launched from inside backward (reference DDP overlap, train.py:141-148) find a free CU at once
 * instead of waiting for a persistent launch to tail off.  Process-wide, default 0 or the VD_RESERVE_CUS environment variable;
 * 0 <= n <= CUs - 8; multiples of 8 keep the XCD-aware item order of those kernels.  Returns the previous value, or -1 if refused. */
int         vd_set_reserved_cus(int32_t n);
int         vd_reserved_cus(void);

/* Calibration loop for bench.py (no reference counterpart: a measurement aid): `blocks` workgroups of 8 waves run `iters` x 16
 * register-only v_mfma_f32_16x16x4_f32 per wave (2048 FLOP each per wave) on operands hashed from `seed`; lane 0 of workgroup b writes
 * stamps[2b] = shader cycles (s_memtime) and stamps[2b + 1] = 100 MHz ticks (s_memrealtime) the loop took: the in-kernel clock is their
 * quotient x 100 MHz.  sink: one float, never written in practice. */
int         vd_mfma_calibrate(float* sink, unsigned long long* stamps, int32_t blocks, int32_t iters, uint32_t seed, void* stream);

/* ------------------------------------------------------------------ dense contractions (MFMA fp32)
 * One tile engine (v_mfma_f32_32x32x2_f32, LDS-staged, double buffered) behind every
 * matmul-shaped op of the path.  C[z][m][n] = alpha * sum_k A(z,m,k) * B(z,n,k) (+bias[n]) (+R[z][m][n]) (+C) */
enum { VD_ROW = 0,      /* operand stored [rows][k], k contiguous                                  */
       VD_COL = 1,      /* operand stored [k][rows], rows contiguous                               */
       VD_IM2COL = 2 }; /* A: 3x3 patches of an NHWC image, k = (tap, channel)  (conv forward/dgrad)
                           B: 3x3 patches, k = pixel, n = (tap, channel)         (conv wgrad)       */

typedef struct vd_gemm_desc {
    const float* A; const float* B; float* C;
    const float* bias;          /* [N] or NULL                                                      */
    const float* R;             /* residual, same indexing as C with ldr / sR*, or NULL             */
    int32_t M, N, K;
    int32_t a_kind, b_kind;
    int64_t lda, ldb, ldc, ldr;
    int32_t batch, nh;          /* z in [0,batch): zb = z / nh, zh = z % nh (nh >= 1)               */
    int64_t sAb, sAh, sBb, sBh, sCb, sCh, sRb, sRh;
    float   alpha;
    int32_t accumulate;         /* C += result                                                      */
    int32_t H, W, Cin;          /* image geometry for VD_IM2COL                                     */
    int32_t splitk;             /* >1: K is split over `splitk` slabs in ws, then reduced into C    */
    float*  ws; int64_t ws_bytes;
    int32_t tile;               /* 0 = auto; 128, 64, 12864 (128x64), 64128 (64x128) force the block tile;  */
                                /*   128256: the 128x256 split-operand form (N % 256 == 0, no split-K)     */
    float*  colsum;             /* optional, VD_COL A only: colsum[m] (+)= sum_k A[k][m] (bias gradient of a */
    int32_t colsum_accumulate;  /*   weight-gradient GEMM, computed from the tiles already staged); batch = 1  */
    float*  stats;              /* optional, forward launches: GroupNorm partials of the OUTPUT rows, laid out  */
    int32_t stats_hw;           /*   [image][chunk][2][N] with chunk = BM/2 rows (BM from vd_gemm_last_tile);    */
                                /*   stats_hw = rows (pixels) per image; finalize: vd_gn_stats_from_partials     */
    int64_t sBias;              /* batched launches: bias of entry z is bias + (z / nh) * sBias (0 = one shared bias) */
} vd_gemm_desc;

/* replaces F.linear (modules.py:79-80), 1x1 F.conv2d (modules.py:141-144 <- unet.py:70,71,134), the two
 * einsum contractions of attention (unet.py:57,61-63) and all of their autograd backward GEMMs */
int vd_gemm(const vd_gemm_desc* d, void* stream);
/* ((F*100 + KT)*1000 + BM)*1000 + BN of the calling thread's last vd_gemm / vd_conv3x3* launch (profiling aid: names the
 * kernel instantiation gemm_dma_kernel<BM,BN,a_kind,b_kind,splitk,KT,TR> the launch went to; F bit 0 = TR, transposed-accumulator
 * epilogue (launches without output statistics); F >= 2: split-operand form, below; KT = 0 means the register-staged fallback
 * gemm_kernel<BM,BN,a_kind,b_kind,splitk>).
 * Environment, read once per process: VD_GEMM_SPLIT (default 1 since round 5; 0 = fp32 MFMA everywhere, the A/B form) sends the 128-row tiles of vd_gemm and
 * every vd_gemm_grouped_wgrad launch to the split-operand forms (gemm_split_kernel<...>): each fp32 operand value is split exactly into three bf16 pieces in registers and the six piece
 * products that reach 2^-24 of a.b run on the 16-bit matrix cores with fp32 accumulation.  Same results to fp32 rounding (error against
 * fp64 0.6-0.9 of the fp32 MFMA chain's: tests/test_kernels_gpu.py::test_split_operand_gemm_forms_in_subprocess), 15-26 % shorter
 * launches (in-kernel clock 1.88 GHz instead of 2.28: the 16-bit pipes ARE power-limited on random data), -2.3 % on a train step of either
 * workload (profiles/r05_split_step_ab.txt); vd_gemm_split_forms() tells which form is in effect.  DOMAIN of the split forms: finite operands of
 * magnitude <= the largest bf16 (3.39e38); a larger or infinite operand yields NaN where the fp32 MFMA yields a finite value or Inf
 * (bf16(x) rounds to Inf, the residual x - Inf poisons the products); pieces below the smallest normal bf16 are flushed. */
int vd_gemm_last_tile(void);
int vd_gemm_split_forms(void);   /* 1: the split-operand forms are in effect for this process (VD_GEMM_SPLIT, default 1), 0: fp32 MFMA everywhere */
/* The 128x256 split-operand form gemm_split_kernel<128,256,a_kind,b_kind,false,16,TR> (code ..16128256): plain and batched ROW/ROW launches
 * that would run the 128x128 KT = 16 split form take it when N % 256 == 0 and ceil(M/128) * (N/256) * batch is at least two workgroups per CU.
 * Same row tile, same statistics chunks, bit-identical results.  tile = 128 keeps the 128x128 form, tile = 128256 forces the wide one at any
 * N % 256 == 0 for ROW/ROW, ROW/COL and COL/COL operands (ROW/COL loses on it per launch and is not dispatched by itself: FINDINGS.md);
 * VD_GEMM_BN256=0 (read once per process) is the A/B switch back to the 128x128 tiles everywhere.
 * vd_gemm_plan_tile: the vd_gemm_last_tile code such a launch WOULD report, from the host plan alone (no device): contiguous aligned operands,
 * no bias / residual; stats != 0: the launch emits GroupNorm partials.  -1 (vd_last_error) where vd_gemm would refuse the request. */
int vd_gemm_plan_tile(int32_t M, int32_t N, int32_t K, int32_t a_kind, int32_t b_kind, int32_t batch, int32_t tile, int32_t stats);
/* `count` (<= 36) same-shape weight-gradient GEMMs in ONE launch -- the 1x1-convolution / linear weight gradients of the blocks of one
 * UNet level (autograd of modules.py:79-80,141-144 w.r.t. the weight), whose operands live in unrelated buffers:
 *   C[e][M][N] (pitch ldc) = A[e]^T B[e],  A[e] = dY [K][M] (pitch lda), B[e] = X [K][N] (pitch ldb)   (= vd_gemm with COL / COL kinds)
 *   colsum[e][m] = sum_k A[e][k][m]   (the bias gradient; colsum may be NULL)
 * split-K over `splitk` slabs per entry through ws (vd_gemm_grouped_wgrad_ws_bytes), reduced in a fixed order: bitwise reproducible.
 * A, B, C, colsum are HOST arrays of device pointers (they travel in the kernel arguments). */
size_t vd_gemm_grouped_wgrad_ws_bytes(int32_t count, int32_t M, int32_t N, int32_t splitk);
/* slab count in [min_slabs, max_slabs] that fills whole residency rounds of the device best (>= 8 K tiles per slab) */
int vd_gemm_grouped_wgrad_auto_split(int32_t count, int32_t M, int32_t N, int32_t K, int32_t min_slabs, int32_t max_slabs);
int vd_gemm_grouped_wgrad(const float* const* A, const float* const* B, float* const* C, float* const* colsum, int32_t count,
                          int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t splitk, float* ws, size_t ws_bytes,
                          void* stream);

/* 3x3 / stride 1 / pad 1 convolution, NHWC (replaces F.conv2d at modules.py:141-144 <- unet.py:121,125,217,232).
 *   y[b,y,x,co] = bias[co] + res[b,y,x,co] + sum_{tap,ci} xin[b,y+dy,x+dx,ci] * wpack[co][tap][ci]
 * wpack comes from vd_pack_conv3x3 ("forward" pack for the forward pass, "dgrad" pack for the input gradient).
 * Cin must be a multiple of 4 (pad 3 -> 4); only co < Cout is written. */
int vd_conv3x3(const float* xin, int64_t ldx, const float* wpack, const float* bias,
               const float* res, int64_t ldres, float* y, int64_t ldy,
               int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t accumulate,
               float* stats_part /* optional: GroupNorm partials of y, see vd_gemm_desc.stats */, void* stream);

/* The same convolution as Winograd F(2x2,3x3) on the fp32 matrix cores (csrc/wino.hip): 2.25x fewer MFMA cycles, exact fp32
 * arithmetic, input/output transforms fused into the tile loads / the epilogue (nothing but x, U, y touches HBM).
 *   U = vd_wino_pack(w): uf[16][Cout][Cin] for the forward pass, ud[16][Cin][Cout] (rotated kernel) for the input gradient
 *   (the input gradient of modules.py:141-144 is the same call with xin = dy, U = ud, Cin <-> Cout).
 * vd_conv3x3_wino_supported: 1 when the geometry is served (H, W even powers of two with 4 <= W/2 <= 64, H*W/4 >= 16 tiles per
 * image, Cin % 16 == 0, Cout % 4 == 0, tensors < 2 GiB); otherwise call vd_conv3x3.  stats_part as in vd_conv3x3 with 64-pixel
 * chunks ([img][H*W/64][2][Cout]); vd_gemm_last_tile() reports BM = 128 for it so chunk = BM/2 holds for both paths. */
int vd_conv3x3_wino_supported(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int64_t ldx, int64_t ldy, int64_t ldres);
int vd_conv3x3_wino(const float* xin, int64_t ldx, const float* U, const float* bias, const float* res, int64_t ldres,
                    float* y, int64_t ldy, int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                    float* stats_part, void* stream);
/* weight gradient of the same convolution in the Winograd domain (dU = sum over tiles of (A dY A^T) (.) (B^T d B), dw = G^T dU G):
 * same arguments and result as vd_conv3x3_wgrad (dw in OIHW, optional dbias), 2.25x fewer MFMA cycles; deterministic (split-K
 * slab planes summed in a fixed order).  Geometry as vd_conv3x3_wino_supported but Cin, Cout only need to be multiples of 4. */
int vd_conv3x3_wgrad_wino_supported(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int64_t ldx, int64_t lddy);
size_t vd_conv3x3_wgrad_wino_ws_bytes(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int vd_conv3x3_wgrad_wino(const float* xin, int64_t ldx, const float* dy, int64_t lddy, int32_t nimg, int32_t H, int32_t W,
                          int32_t Cin, int32_t Cout, float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w,
                          int32_t accumulate, float* ws, size_t ws_bytes, void* stream);
/* the two kernels of vd_conv3x3_wgrad_wino as separate calls (per-kernel timing, bench.py): phase 1 = slab planes (wino_wgrad_kernel),
 * phase 2 = their fixed-order reduction into OIHW (wino_wgrad_reduce_kernel) */
int vd_conv3x3_wgrad_wino_phase(const float* xin, int64_t ldx, const float* dy, int64_t lddy, int32_t nimg, int32_t H, int32_t W,
                                int32_t Cin, int32_t Cout, float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w,
                                int32_t accumulate, float* ws, size_t ws_bytes, int32_t phase, void* stream);
/* (TW * 1000 + NS) * 2 + stats of the calling thread's last vd_conv3x3_wino launch: names the instantiation
 * wino_conv_kernel<TW, NS, stats, false, 0>; negated when the launch took the 128-tile form wino_conv_wide_kernel<TW, NS, stats>
 * (profiling aid, like vd_gemm_last_tile) */
int vd_wino_last_kernel(void);
/* (TWS * 1000 + split-K slabs) * 2 + dbias of the calling thread's last vd_conv3x3_wgrad_wino launch: names the instantiation
 * wino_wgrad_kernel<TWS, dbias> (TWS = min(W/2, 16)) and its slab count (profiling / test aid) */
int vd_wino_wgrad_last_kernel(void);
#ifdef VD_PROBES
/* libvdiff_hip_probe.so only (built with -DVD_PROBES for tests/probe/; the product library has no timing-probe or timing-experiment
 * code): per-wave phase timestamps of the next vd_conv3x3_wino / vd_conv3x3_wgrad_wino launches into buf (64 x uint64 per
 * workgroup), NULL = off */
int vd_wino_set_probe(unsigned long long* buf);
/* the same for the F(4x4,3x3) forward and input-gradient launches -- tests/probe/w43_phases.py: 16 x uint64 per (workgroup, wave, item round < 4) */
int vd_wino43_set_probe(unsigned long long* buf);
/* the longest sibling wait (spin iterations, atomicMax) of the SPLIT GroupNorm-backward launches that follow -- tests/test_multigpu_path_gpu.py soak */
int vd_gn_set_spin_probe(unsigned* buf);
#endif
int vd_wino_pack(const float* w_oihw, int32_t Cout, int32_t Cin, float* uf /* or NULL */, float* ud /* or NULL */, void* stream);
/* ---- input gradient of the same convolution as Winograd F(4x4, 3x3) (csrc/wino43.hip): 36 multiplies per 4x4 output tile where
 * F(2x2,3x3) needs 64 -- 1.78x fewer matrix-core cycles; with the classic interpolation points {0, +-1, +-2, inf} used here ~7x the
 * rounding error of a direct fp32 sum, an order of magnitude inside the stated bound on gradients (per-tensor relative L2 <= 1e-4;
 * autograd of modules.py:141-144).
 *   U43 = vd_wino43_pack(w): (G rot180(w[co][ci]) G^T)[36] in the order the kernel's lanes read it, vd_wino43_u_floats(Cout, Cin) floats;
 *   dx[nimg][H][W][:Cin] = vd_conv3x3_dgrad_wino43(dy[nimg][H][W][:Cout], U43)   every element written, no accumulation.
 * _supported: 1 for 32x32 images, 64-wide images with H % 16 == 0 and 16x16 images in multiples of four (four per work item),
 * Cout % 8 == 0, Cin % 32 == 0, 16-byte rows, tensors < 2 GiB;
 * otherwise call vd_conv3x3_wino with the rotated F(2x2,3x3) image.  vd_wino43_last_kernel: tiles per row (4 / 8 / 16) of the calling
 * thread's last launch, negative for vd_conv3x3_wino43_fwd = the instantiation wino43_conv_kernel<TWT, FWD> (profiling / test aid). */
int vd_conv3x3_dgrad_wino43_supported(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int64_t lddy, int64_t lddx);
size_t vd_wino43_u_floats(int32_t Cout, int32_t Cin);
int vd_conv3x3_dgrad_wino43(const float* dy, int64_t lddy, const float* U43, float* dx, int64_t lddx, int32_t nimg, int32_t H, int32_t W,
                            int32_t Cin, int32_t Cout, void* stream);
int vd_wino43_last_kernel(void);
int vd_wino43_pack(const float* w_oihw, int32_t Cout, int32_t Cin, float* U43, void* stream);
/* all tensors in one launch: items_dev = [n][8] int64 {w, U43, fwd, Cout, Cin, 0, 0, first block}; fwd = 0: the input-gradient image,
 * (Cin/32)*(Cout/8) blocks; fwd = 1: the forward image of vd_wino43_pack_fwd, (Cout/32)*(Cin/8) blocks */
int vd_wino43_pack_batched(const int64_t* items_dev, int32_t n, int64_t total_blocks, void* stream);
/* occupancy rule between the two Winograd orders: 1 when the F(4x4,3x3) convolution kernel (forward: N = Cout; input gradient: N = Cin) is
 * expected to beat the F(2x2,3x3) one on this batch -- both run persistent work items in rounds over the CUs, F(2x2,3x3) has four times as
 * many at 3/8 of the time each (measured at B = 128), so with fewer items than CUs (small-batch sampling) the finer items win.  The
 * engine asks this next to the *_supported queries; the kernels themselves serve every supported geometry regardless. */
int vd_conv3x3_wino43_preferred(int32_t nimg, int32_t H, int32_t W, int32_t N);
/* ---- FORWARD pass of the same convolution through F(4x4,3x3) (replaces F.conv2d of modules.py:141-144 for the residual-block
 * convolutions unet.py:121,125 on the 16x16 / 32x32 / 64-wide layers), with the interpolation points {0, +-3/4, +-3/2, inf}: every
 * coefficient of the data and output transforms is a dyadic rational, exact in fp32, and the whole-network output error is ~2x that of
 * the F(2x2,3x3) forward, inside the stated 2e-5 bound (tests/probe/wino_err_sim.py; measured: tests/test_unet_gpu.py).
 *   U43f = vd_wino43_pack_fwd(w): (G w[co][ci] G^T)[36] in the kernel's lane order, vd_wino43_u_floats(Cout, Cin) floats;
 *   y[nimg][H][W][:Cout] = conv3x3(x[..][:Cin], w) + bias (+ res)     bias / res may be NULL; every element written
 *   stats_part (or NULL): GroupNorm partial sums of y as [nimg][chunks][2][Cout] with ONE CHUNK PER (image, work item):
 *   vd_conv3x3_wino43_fwd_chunk_rows(H, W) pixels per chunk (H*W for 16x16 and 32x32 images, 16*W for 64-wide ones).
 * _supported: the geometries of the input gradient (above) with Cin % 8 == 0, Cout % 32 == 0; otherwise call vd_conv3x3_wino. */
int vd_conv3x3_wino43_fwd_supported(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int64_t ldx, int64_t ldy, int64_t ldres);
int vd_wino43_pack_fwd(const float* w_oihw, int32_t Cout, int32_t Cin, float* U43f, void* stream);
int vd_conv3x3_wino43_fwd_chunk_rows(int32_t H, int32_t W);
int vd_conv3x3_wino43_fwd(const float* xin, int64_t ldx, const float* U43f, const float* bias, const float* res, int64_t ldres, float* y,
                          int64_t ldy, int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, float* stats_part, void* stream);
/* weight (and bias) gradient of the same convolution through F(4x4,3x3), UNFUSED: one HBM-bound pass writes dM = A dY A^T and V = B^T d B
 * ([36][tiles][channels], 2.25x the size of dY / x each), the 36 GEMMs over the tile index run as one vd_gemm_grouped_wgrad launch (1.78x fewer
 * MFMA cycles than vd_conv3x3_wgrad_wino), a small kernel folds G^T . G into OIHW; the bias gradient is the column sum of plane (1,1).
 * Same arguments and result as vd_conv3x3_wgrad_wino (accumulate, padded dims, deterministic).  _supported: H, W, Cin, Cout multiples
 * of 4, at least 512 tiles of 4x4 outputs (8x8 images at batch 128).  _phase: 1 = transforms, 2 = GEMMs (+ slab reduction of layers below 147 456 = 384 x 384 weights per plane), 4 = finish (+ slab reduction of wider layers). */
int vd_conv3x3_wgrad_wino43_supported(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int64_t ldx, int64_t lddy);
size_t vd_conv3x3_wgrad_wino43_ws_bytes(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int vd_conv3x3_wgrad_wino43(const float* xin, int64_t ldx, const float* dy, int64_t lddy, int32_t nimg, int32_t H, int32_t W,
                            int32_t Cin, int32_t Cout, float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w,
                            int32_t accumulate, float* ws, size_t ws_bytes, void* stream);
int vd_conv3x3_wgrad_wino43_phase(const float* xin, int64_t ldx, const float* dy, int64_t lddy, int32_t nimg, int32_t H, int32_t W,
                                  int32_t Cin, int32_t Cout, float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w,
                                  int32_t accumulate, float* ws, size_t ws_bytes, int32_t phase, void* stream);
/* split-K slabs per plane of the calling thread's last vd_conv3x3_wgrad_wino43 launch (test / profiling aid) */
int vd_wino43_wgrad_last_kernel(void);

/* Forward 3x3 convolution through PLANES (csrc/wino43.hip): the weight gradient's input transform writes V = B^T d B
 * ([T/16][36][16][Cin], T = nimg (H/4) (W/4) tiles, vd_conv3x3_wino43_v_floats floats), the 36 products M[xi] = V[xi] U[xi]^T run as one
 * batched launch of the split-operand tile engine and an HBM-bound pass writes y = A^T M A + bias (+ res) and the GroupNorm partials of y
 * ([nimg][chunks][2][Cout], vd_conv3x3_wino43_fwd_chunk_rows pixels per chunk; fixed summation order).  w_oihw is the raw kernel
 * [Cout][Cin][3][3]; ws: vd_conv3x3_wino43_fwd_planes_ws_bytes.  phase: 7 = everything, or 1 (pack + V transform), 2 (GEMMs), 4 (output
 * transform) for per-kernel timing.  V is left behind for vd_conv3x3_wgrad_wino43_v: the same weight gradient as vd_conv3x3_wgrad_wino43,
 * bit for bit, without its input transform.
 * vd_conv3x3_fwd_planes_preferred: host rule (occupancy floor + same-box measurement) for where this form beats the fused forward kernel:
 * `training` != 0 counts the weight gradient's saved transform, 0 the forward alone. */
int vd_conv3x3_wino43_fwd_planes_supported(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int64_t ldx, int64_t ldy,
                                           int64_t ldres);
size_t vd_conv3x3_wino43_v_floats(int32_t nimg, int32_t H, int32_t W, int32_t Cin);
size_t vd_conv3x3_wino43_fwd_planes_ws_bytes(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int vd_conv3x3_fwd_planes_preferred(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t training);
int vd_conv3x3_wino43_fwd_planes(const float* xin, int64_t ldx, const float* w_oihw, const float* bias, const float* res, int64_t ldres,
                                 float* y, int64_t ldy, int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, float* stats_part,
                                 float* V, float* ws, size_t ws_bytes, int32_t phase, void* stream);
int vd_conv3x3_wgrad_wino43_v(const float* V, const float* dy, int64_t lddy, int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                              float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w, int32_t accumulate, float* ws, size_t ws_bytes,
                              int32_t phase, void* stream);

/* Input gradient of the 3x3 convolution through PLANES (csrc/wino43.hip), the exact adjoint of vd_conv3x3_wino43_fwd_planes: with
 * dM = A dY A^T ([T/16][36][16][Cout], vd_conv3x3_wino43_dm_floats floats: the image the weight gradient's transform pass makes of dy, written
 * into the caller's buffer by vd_conv3x3_wino43_dy_image -- same device code, same bits), the 36 products dV[xi] = dM[xi] Ut[xi] run as one
 * batched launch of the split-operand tile engine (Ut = the forward's plane image transposed, packed from the raw kernel w_oihw) and an
 * HBM-bound pass overlap-adds the 6x6 patches B dV B^T into dx[nimg][H][W][:Cin] (every element written once, fixed summation order,
 * channels >= Cin of a pitched dx untouched).  32x32 and 16x16 images.  ws: vd_conv3x3_wino43_dgrad_planes_ws_bytes.  phase: 7 = everything,
 * or 1 (pack), 2 (GEMMs), 4 (overlap-add) for per-kernel timing.
 * vd_conv3x3_wgrad_wino43_vm: the weight gradient with BOTH images given (no transform pass; phase 7, 2 or 4), bitwise the result of
 * vd_conv3x3_wgrad_wino43_v -- so a training step transforms dy once for both gradients.
 * vd_conv3x3_dgrad_planes_preferred: host rule (occupancy floor + same-box measurement) for where this form, given dM, beats the fused
 * F(4x4,3x3) input-gradient kernel; training steps only. */
size_t vd_conv3x3_wino43_dm_floats(int32_t nimg, int32_t H, int32_t W, int32_t Cout);
int vd_conv3x3_wino43_dy_image(const float* dy, int64_t lddy, int32_t nimg, int32_t H, int32_t W, int32_t Cout, float* dM, void* stream);
int vd_conv3x3_wgrad_wino43_vm(const float* V, const float* dM, int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                               float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w, int32_t accumulate, float* ws, size_t ws_bytes,
                               int32_t phase, void* stream);
int vd_conv3x3_wino43_dgrad_planes_supported(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int64_t lddx);
size_t vd_conv3x3_wino43_dgrad_planes_ws_bytes(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int vd_conv3x3_dgrad_planes_preferred(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t training);
int vd_conv3x3_wino43_dgrad_planes(const float* dM, const float* w_oihw, float* dx, int64_t lddx, int32_t nimg, int32_t H, int32_t W,
                                   int32_t Cin, int32_t Cout, float* ws, size_t ws_bytes, int32_t phase, void* stream);

/* all 3x3 kernels of a network in one launch: items_dev = [n][8] int64 {w, uf, ud, Cout, Cin, tiled, 0, first 256-thread block};
 * tiled = 1 (Cout, Cin multiples of 16): the tensor takes (Cout/16)*(Cin/16) blocks of one 16x16 tile, else ceil(Cout*Cin/256) */
int vd_wino_pack_batched(const int64_t* items_dev, int32_t n, int64_t total_blocks, void* stream);

/* "thin" 3x3 convolutions (3-4 channels on one side: in_conv unet.py:217, out_conv :232).  The taps are moved to the thin
 * side so that the wide side is a plain vd_gemm instead of an implicit GEMM with a 64-wide tile on 3 useful columns:
 *   thin input :  xc = vd_im2col3x3(x) [pixels][9*C]            then  y = vd_gemm(xc, wpack[Cout][9*C])  (+ its transposes)
 *   thin output:  z  = vd_gemm(a, wpack viewed [9*Cout][Cin])    then  y = vd_tap_gather(z, bias)
 *   gradients  :  dz = vd_tap_spread(dy);  da = vd_gemm(dz, wpack);  vd_gemm(dz^T a) -> vd_thin_wgrad_finish -> OIHW */
int vd_im2col3x3(const float* x, int64_t ldx, float* xc /* [nimg*H*W][9*C] */, int32_t nimg, int32_t H, int32_t W, int32_t C, void* stream);
/* out[p][co] = bias[co] + sum_tap z[p + off(tap)][co*9 + tap]   (zero padding; co < Cout) */
int vd_tap_gather(const float* z, int64_t ldz, const float* bias, float* out, int64_t ldo, int32_t nimg, int32_t H, int32_t W, int32_t Cout, void* stream);
/* dz[q][co*9 + tap] = dy[q - off(tap)][co]; columns [9*Cout, ldz) are zero-filled */
int vd_tap_spread(const float* dy, int64_t lddy, float* dz, int64_t ldz, int32_t nimg, int32_t H, int32_t W, int32_t Cout, void* stream);
/* g[co][tap*Cin + ci] -> dw_oihw[co][ci][tap] (+)= (ci < Cin_w);  dbias[co] (+)= colsum[co*cs_stride + cs_off] (optional) */
int vd_thin_wgrad_finish(const float* g, int32_t Cout_w, int32_t Cin, int32_t Cin_w, float* dw_oihw, int32_t accumulate,
                         const float* colsum, int32_t cs_stride, int32_t cs_off, float* dbias, void* stream);

/* weight (and bias) gradient of the same convolution, summed over the whole batch (autograd of F.conv2d):
 *   dw_oihw[co][ci][tap] (+)= sum_{b,y,x} dy[b,y,x,co] * xin[b,y+dy,x+dx,ci]      co < Cout_w, ci < Cin_w
 *   dbias[co]            (+)= sum_{b,y,x} dy[b,y,x,co]                             (dbias may be NULL)
 * xin has Cin (multiple of 4, >= Cin_w) channels, dy has Cout (multiple of 4, >= Cout_w) channels. */
size_t vd_conv3x3_wgrad_ws_bytes(int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int vd_conv3x3_wgrad(const float* xin, int64_t ldx, const float* dy, int64_t lddy,
                     int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                     float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w, int32_t accumulate,
                     float* ws, size_t ws_bytes, void* stream);
/* the same in two calls, for per-kernel timing (bench.py's live roofline figure): phase 1 = the split-K MFMA kernel into ws,
 * phase 2 = slab reduction + OIHW transposition into dw_oihw/dbias.  Same stream, same thread, phase 1 first. */
int vd_conv3x3_wgrad_phase(const float* xin, int64_t ldx, const float* dy, int64_t lddy,
                           int32_t nimg, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                           float* dw_oihw, float* dbias, int32_t Cin_w, int32_t Cout_w, int32_t accumulate,
                           float* ws, size_t ws_bytes, int32_t phase, void* stream);

/* OIHW (Cout_w, Cin_w, 3, 3) -> wf[Cout_w][9][Cin_p]  (forward)  and/or  wd[Cin_w][9][Cout_p] with the taps
 * mirrored (dgrad).  Either output may be NULL.  Padding channels are zero-filled. */
int vd_pack_conv3x3(const float* w_oihw, int32_t Cout_w, int32_t Cin_w,
                    float* wf, int32_t Cin_p, float* wd, int32_t Cout_p, void* stream);
/* the same for many tensors in one launch.  items_dev: DEVICE table of n x 8 int64 {w_oihw, wf (or 0), wd (or 0), Cout_w,
 * Cin_w, Cin_p, Cout_p, first_block}; tensor i owns blocks [first_block_i, first_block_{i+1}) of 256 elements each, enough
 * for max(Cout_w*9*Cin_p, Cin_w*9*Cout_p); total_blocks = end of the last tensor. */
int vd_pack_conv3x3_batched(const int64_t* items_dev, int32_t n, int64_t total_blocks, void* stream);

/* ------------------------------------------------------------------ GroupNorm(32, C, eps) + SiLU + FiLM + dropout + resample
 * (nn.GroupNorm unet.py:28-30, nn.SiLU unet.py:25, FiLM unet.py:145-146, nn.Dropout unet.py:135,147,
 *  nn.AvgPool2d / nn.Upsample unet.py:127-132) */
enum { VD_RS_NONE = 0, VD_RS_DOWN = 1, VD_RS_UP = 2 };

/* per-(image, group) mean and 1/sqrt(var+eps) of x[nimg][HW][C]; stats = [nimg][G][2] */
size_t vd_gn_ws_bytes(int32_t nimg, int32_t HW, int32_t C);
int vd_gn_stats(const float* x, int64_t ldx, int32_t nimg, int32_t HW, int32_t C, int32_t G, float eps,
                float* stats, float* ws, size_t ws_bytes, void* stream);

/* the same statistics from the partial sums a producer epilogue left behind (vd_gemm_desc.stats / vd_conv3x3 stats_part):
 * the normalised tensor is the channel concatenation [C1 | C2] of up to two produced tensors (C2 = 0: one source) */
int vd_gn_stats_from_partials(const float* part1, int32_t C1, int32_t chunks1, const float* part2, int32_t C2, int32_t chunks2,
                              int32_t nimg, int32_t HW, int32_t G, float eps, float* stats, void* stream);

/* ... or straight to the coefficient table vd_gn_apply works from (then call vd_gn_apply with stats = NULL) */
int vd_gn_coef_from_partials(const float* part1, int32_t C1, int32_t chunks1, const float* part2, int32_t C2, int32_t chunks2,
                             int32_t nimg, int32_t HW, int32_t G, float eps, const float* gamma, const float* beta,
                             const float* film, float* coef, void* stream);

/* y = resample( dropout( act( (1+scale) * GN(x) + shift ) ) )
 * film: [nimg][2C] (shift first, scale second, unet.py:145) or NULL; act: 1 = SiLU, 0 = identity;
 * gamma/beta NULL => plain resample of x (the skip path, unet.py:138).
 * coef: [nimg][4][C] floats, kept for the backward pass; written here from `stats`, or -- with stats = NULL -- already
 * filled by vd_gn_coef_from_partials. */
int vd_gn_apply(const float* x, int64_t ldx, const float* stats, const float* gamma, const float* beta,
                const float* film, int32_t act, float p_drop, uint64_t seed,
                int32_t resample, float* y, int64_t ldy,
                int32_t nimg, int32_t H, int32_t W, int32_t C, int32_t G, float* coef, void* stream);

/* vd_gn_coef_from_partials + vd_gn_apply in ONE launch (reference: the same nn.GroupNorm call sites, unet.py:28-30 <- :52,119,123,230):
 * every workgroup of the apply pass derives the statistics of the groups it touches from the producers' partial sums (part1 / part2:
 * layout of vd_gemm `stats`, channel-concatenated sources) and the workgroups of pixel chunk 0 write the [nimg][4][C] table `coef`
 * (NULL: not needed, e.g. inference) that vd_gn_apply_bwd reads. */
int vd_gn_apply_from_partials(const float* x, int64_t ldx, const float* part1, int32_t C1, int32_t chunks1, const float* part2, int32_t C2,
                              int32_t chunks2, const float* gamma, const float* beta, const float* film, int32_t act, float p_drop,
                              uint64_t seed, int32_t resample, float* y, int64_t ldy, int32_t nimg, int32_t H, int32_t W, int32_t C,
                              int32_t G, float eps, float* coef, void* stream);

/* backward of vd_gn_apply.  dy is at the OUTPUT resolution of the forward op.
 *   dx (+)= d/dx ; dfilm [nimg][2C] (written) ; dgamma/dbeta (+)= (accumulate_params)
 * add: optional tensor (input resolution, ld = ldadd) added into dx (the skip-path gradient). */
int vd_gn_apply_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* coef,
                    const float* gamma, const float* beta, const float* film, int32_t act, float p_drop, uint64_t seed,
                    int32_t resample, const float* add, int64_t ldadd, float* dx, int64_t lddx, int32_t accumulate_dx,
                    float* dfilm, float* dgamma, float* dbeta, int32_t accumulate_params,
                    int32_t nimg, int32_t H, int32_t W, int32_t C, int32_t G,
                    float* ws, size_t ws_bytes, void* stream);
/* NPT * 10000 + TPB (+ 1000000 for the instantiation with non-temporal loads / stores: slabs of whole 128-byte pixel rows) of the calling
 * thread's last vd_gn_apply_bwd launch when it took the single-pass form gn_bwd_fused_kernel<NPT, TPB, NT>,
 * -1 for the two-pass form (chan_reduce_kernel<1> + gn_bwd_finalize_kernel + gn_bwd_apply_kernel), 0 without a norm (plain resample
 * backward: gn_bwd_apply_kernel).  Profiling aid, like vd_gemm_last_tile. */
int vd_gn_bwd_last_kernel(void);
/* vd_gn_apply_bwd with the sum over images of the per-image dgamma / dbeta terms left to the caller: they are written to
 * pgb_keep[nimg][2][C] ({dgamma, dbeta} terms) and ONE vd_gn_param_sums_batched launch sums them for all norms of a backward pass
 * (the per-norm launch is pure latency: 73 per CIFAR train step).  items_dev = [n][8] int64 {pgb, dgamma, dbeta, nimg, C, accumulate, 0,
 * first 256-thread block}; a norm takes ceil(C / 16) blocks. */
int vd_gn_apply_bwd_keep(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* coef, const float* gamma,
                         const float* beta, const float* film, int32_t act, float p_drop, uint64_t seed, int32_t resample,
                         const float* add, int64_t ldadd, float* dx, int64_t lddx, int32_t accumulate_dx, float* dfilm, float* pgb_keep,
                         int32_t nimg, int32_t H, int32_t W, int32_t C, int32_t G, float* ws, size_t ws_bytes, void* stream);
int vd_gn_param_sums_batched(const int64_t* items_dev, int32_t n, int64_t total_blocks, void* stream);

/* ------------------------------------------------------------------ small reductions / elementwise
 * out[n] (+)= sum_m x[m][n]   (bias gradients) */
size_t vd_colsum_ws_bytes(int64_t M, int32_t N);
int vd_colsum(const float* x, int64_t ldx, int64_t M, int32_t N, float* out, int32_t accumulate,
              float* ws, size_t ws_bytes, void* stream);
/* y = alpha*x + beta*y over [rows][C] with strides */
int vd_axpby(const float* x, int64_t ldx, float alpha, float* y, int64_t ldy, float beta, int64_t rows, int32_t C, void* stream);
/* SiLU forward / backward on a dense vector (nn.SiLU on t_emb, unet.py:142,203) */
int vd_silu(const float* x, float* y, int64_t n, void* stream);
int vd_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, int32_t accumulate, void* stream);
/* row softmax in place over [rows][L] (torch.softmax unet.py:58-59) and its backward: ds = alpha * p * (dp - sum(dp*p)) */
int vd_softmax_rows(float* s, int64_t rows, int32_t L, void* stream);
int vd_softmax_rows_bwd(const float* p, float* dp, int64_t rows, int32_t L, float alpha, void* stream);

/* fused scaled-dot-product attention (BaseAttentionBlock.scaled_dot_product, unet.py:55-64, and its autograd): o = softmax(scale q k^T) v
 * per (image b, head h) without the [B, nh, L, L] logits in HBM.  Operands are rows of the qkv projection:
 * x[(b L + l) ld + h hd + d].  Served: L % 64 == 0 and hd in {64, 128, 256} forward, {64, 128} backward (vd_attn_supported);
 * everything else takes vd_gemm -> vd_softmax_rows -> vd_gemm.  lse [B nh L] (forward output, may be NULL when no backward
 * follows) and delta [B nh L] (backward scratch) are opaque to the caller.  Fixed summation order: bitwise reproducible. */
int vd_attn_supported(int32_t L, int32_t hd, int32_t backward);
int vd_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, float* o, int64_t ldo, float* lse, int32_t B,
                int32_t nh, int32_t L, int32_t hd, float scale, void* stream);
int vd_attn_bwd(const float* q, const float* k, const float* v, int64_t ld, const float* o, int64_t ldo, const float* dout,
                int64_t lddo, const float* lse, float* delta, float* dq, float* dk, float* dv, int64_t ldd, int32_t B,
                int32_t nh, int32_t L, int32_t hd, float scale, void* stream);
/* the same in two calls, for per-kernel timing: phase 1 = dQ (and delta), phase 2 = dK, dV (after phase 1) */
int vd_attn_bwd_phase(const float* q, const float* k, const float* v, int64_t ld, const float* o, int64_t ldo, const float* dout,
                      int64_t lddo, const float* lse, float* delta, float* dq, float* dk, float* dv, int64_t ldd, int32_t B,
                      int32_t nh, int32_t L, int32_t hd, float scale, int32_t phase, void* stream);

/* layout changes at the boundary of the NCHW call surface */
int vd_nchw_to_nhwc(const float* x, float* y, int32_t nimg, int32_t C, int32_t H, int32_t W, int64_t ldy, void* stream);
int vd_nhwc_to_nchw(const float* x, int64_t ldx, float* y, int32_t nimg, int32_t C, int32_t H, int32_t W, void* stream);

/* the data formats either side of the path:
 *   out_u8[b][y][x][c] = uint8(clamp(x*127.5+127.5, 0, 255))   generate.py:149 (quantise + NCHW->HWC pack, on device)
 *   out[b][c][y][x]    = (u8[b][y][x'][c]/255 - 0.5)/0.5, x' mirrored where flip[b]   datasets.py:115-120 (flip may be NULL) */
int vd_images_to_uint8_hwc(const float* x_nchw, uint8_t* out_hwc, int32_t n, int32_t C, int32_t HW, void* stream);
int vd_images_from_uint8_hwc(const uint8_t* in_hwc, const uint8_t* flip, float* out_nchw, int32_t n, int32_t C,
                             int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------ embeddings
 * get_timestep_embedding (functions.py:11-29): fp64 arithmetic, fp32 result [n][dim] */
int vd_timestep_embedding(const double* t, float* out, int32_t n, int32_t dim, double scale, void* stream);
/* OneHot(exclude_zero) + Linear (modules.py:184-201, unet.py:209-215,295): temb[b] += W[:, y-1] (y>0) + bias */
int vd_class_embed(const float* y, const float* w, const float* bias, float* temb, int32_t n, int32_t emb, int32_t ncls, void* stream);
int vd_class_embed_bwd(const float* y, const float* dtemb, float* dw, float* dbias, int32_t n, int32_t emb, int32_t ncls,
                       int32_t accumulate, void* stream);
/* multitag normalisation y / sqrt(max(nnz,1)) (unet.py:290-294) */
int vd_multitag_norm(const float* y, float* out, int32_t n, int32_t ncls, void* stream);

/* ------------------------------------------------------------------ diffusion process (diffusion.py)
 * All images NCHW (the reference call surface); the UNet converts to NHWC at its own boundary.
 * model_out_type: 0 = v, 1 = x0, 2 = eps, 3 = both ; reweight: 0 = constant, 1 = snr, 2 = snr_trunc, 3 = snr_1plus
 * Every entry of this section returns 1 before any launch for a model_out_type outside 0..3 or a null buffer it would read or write
 * (buffers called optional may be null), and for n, C or HW < 1 -- except vd_q_sample, vd_loss_bwd, vd_bpd_bwd and vd_sample_step,
 * where an empty batch is a no-op. */
/* q_sample (diffusion.py:242-245): xt = sqrt(sigmoid(l_b)) x0 + sqrt(sigmoid(-l_b)) eps */
int vd_q_sample(const float* x0, const float* eps, const float* logsnr, float* xt, int32_t n, int32_t C, int32_t HW, void* stream);
/* train_loss mse branch (diffusion.py:520-541 with the conversions of :466-490): per-sample loss[n];
 * aux[n][2] keeps the two branch means of snr_trunc (x0-mse, eps-mse) for the backward pass.
 * out has C channels (2C for model_out_type "both"). */
int vd_loss_fwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr,
                int32_t model_out_type, int32_t reweight, float* loss, float* aux, int32_t n, int32_t C, int32_t HW, void* stream);
/* dout = gloss[b] * d loss_b / d out */
int vd_loss_bwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr,
                const float* aux, const float* gloss, int32_t model_out_type, int32_t reweight, float* dout,
                int32_t n, int32_t C, int32_t HW, void* stream);
/* variational-bound terms of one step (loss_type "kl": GaussianDiffusion._loss_term_bpd diffusion.py:446-464 with
 * normal_kl / discretized_gaussian_loglik of functions.py:31-67), per sample and in bits per dimension:
 *   kl[b]  = mean KL( q(x_s|x_t,x_0) || p(x_s|x_t) ) / ln 2 ,  nll[b] = mean -log p(x_0|x_t) / ln 2 (8-bit bins)
 * coef[n][8] (device) = {a0, b0x, b0e, c1, c2, true_logvar, model_logvar, a0 - 1} per sample: x0_hat = clip?(a0*xt + b0x*out
 * (+ b0e*out_eps)), true_mean = c1*xt + c2*x0, model_mean = c1*xt + c2*x0_hat.  pred (x0_hat, NCHW) and mse[n] are optional;
 * mse is taken from (a0 - 1)*xt + (xt - x0) + b0x*out (+ b0e*out_eps), so slot 7 is a0 - 1 rounded on its own, not fl(a0) - 1. */
int vd_bpd_terms(const float* x0, const float* xt, const float* out, const float* coef, int32_t model_out_type, int32_t clip,
                 float* kl, float* nll, float* pred, float* mse, int32_t n, int32_t C, int32_t HW, void* stream);
/* dout = gloss[b] * d (use_kl[b] != 0 ? kl[b] : nll[b]) / d out   (autograd of the "kl" branch of train_loss, :497-515) */
int vd_bpd_bwd(const float* x0, const float* xt, const float* out, const float* coef, const float* use_kl, const float* gloss,
               int32_t model_out_type, int32_t clip, float* dout, int32_t n, int32_t C, int32_t HW, void* stream);
/* one reverse step (p_mean_var + CFG + noise, diffusion.py:317-392) for a batch that shares the step index.
 * out has n*(1+cfg) images, cond/uncond interleaved when cfg (diffusion.py:369-372).
 * k: 8 HOST floats {a0, b0x, b0e, c1, c2, noise_scale, w_guide, c3}:  x0_hat = clip(a0*xt + b0x*out (+ b0e*out_eps)),
 * mean = last_step ? x0_hat : c1*xt + c2*x0_hat + c3*out (c3: weight of the raw output, used when the output itself is eps), guided = mean_c + w (mean_c - mean_u), xn = guided + noise_scale*noise.
 * xdup (optional): the new state duplicated to 2n interleaved images = the next CFG UNet input.
 * Exactly one of k (host) / k_dev (device, same 8 floats) is given: the device form keeps the launch replayable from a
 * captured HIP graph with per-step coefficients.  xn may alias xt (element-wise in-place update). */
int vd_sample_step(const float* xt, const float* out, const float* noise, const float* k, const float* k_dev,
                   int32_t model_out_type, int32_t cfg, int32_t last_step, int32_t clip,
                   float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream);
/* ---- learned variances (model_var_type "learned"; Nichol & Dhariwal 2021, the intent of diffusion.py:320-324 with the tensor intp_frac
 * of logsnr_to_posterior :155).  The network output has Cp + C channels: Cp = C (2C for "both") prediction channels, then C channels nu.
 * Per element frac = sigmoid(nu), logvar = lvmin + frac*delta, with lvmin the fixed_small (= true posterior) log-variance of the step and
 * delta = lvmax - lvmin = logsigmoid(-logsnr_t) - logsigmoid(-logsnr_s) >= 0, both formed on the host in fp64 and rounded once.
 * No atomics in any of the five: the same call gives the same bits. */
/* vd_bpd_terms for such an output: coef[n][8] = {a0, b0x, b0e, c1, c2, lvmin, delta, a0 - 1}; kl, nll, pred, mse as there, with
 * kl_e = 0.5(-1 - d + e^d + (c2 (x0_hat - x0))^2 e^-logvar), d = lvmin - logvar, and exp(-logvar/2) scaling the decoder's CDF arguments */
int vd_bpd_terms_lv(const float* x0, const float* xt, const float* out, const float* coef, int32_t model_out_type, int32_t clip,
                    float* kl, float* nll, float* pred, float* mse, int32_t n, int32_t C, int32_t HW, void* stream);
/* dout [n][Cp + C][HW] = gloss[b] * d (use_kl[b] != 0 ? kl[b] : nll[b]) / d out.  mean_grad = 0 writes exact zeros to the prediction
 * channels (the stop-gradient of the hybrid loss); the nu channels do not depend on mean_grad.  Under clip a clamped pixel passes no
 * gradient to the prediction channels and still passes one to nu. */
int vd_bpd_bwd_lv(const float* x0, const float* xt, const float* out, const float* coef, const float* use_kl, const float* gloss,
                  int32_t model_out_type, int32_t clip, int32_t mean_grad, float* dout, int32_t n, int32_t C, int32_t HW, void* stream);
/* hybrid loss, one launch each way: loss[b] = mse_b + vlb_weight * (use_kl[b] != 0 ? kl_b : nll_b), mse_b = vd_loss_fwd's value on the
 * prediction channels (every reweight), the bound term vd_bpd_terms_lv's without clipping.  aux[n][4] = {the two snr_trunc means, kl_b,
 * nll_b}.  The backward writes all Cp + C channels: the prediction channels take gloss[b] * d mse_b / d out alone (the bound term's mean
 * is a constant), the nu channels vlb_weight * gloss[b] * d term_b / d nu. */
int vd_hybrid_loss_fwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr, const float* coef,
                       const float* use_kl, int32_t model_out_type, int32_t reweight, float vlb_weight, float* loss, float* aux,
                       int32_t n, int32_t C, int32_t HW, void* stream);
int vd_hybrid_loss_bwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr, const float* coef,
                       const float* use_kl, const float* aux, const float* gloss, int32_t model_out_type, int32_t reweight,
                       float vlb_weight, float* dout, int32_t n, int32_t C, int32_t HW, void* stream);
/* vd_sample_step for such an output (n*(1+cfg) rows of Cp + C channels).  k: 10 HOST floats {a0, b0x, b0e, c1, c2, lvmin, w_guide, c3,
 * delta, 0}; the guided mean is vd_sample_step's, and xn = mean + exp(0.5 (lvmin + delta*sigmoid(nu))) * noise with nu of the
 * CONDITIONAL row (diffusion.py:386-387) when noise is given and last_step = 0; noise = null gives vd_sample_step's bits on the
 * prediction channels.  Wide (dwordx4) when C*HW % 4 == 0 and every base is 16-byte aligned, else scalar; the two agree bit for bit. */
int vd_sample_step_lv(const float* xt, const float* out, const float* noise, const float* k, int32_t model_out_type, int32_t cfg,
                      int32_t last_step, int32_t clip, float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream);
/* progressive distillation (Salimans & Ho 2022): a student with N sampling steps regresses, in x-space, on the result of two
 * deterministic DDIM steps of a teacher on the 2N grid, t -> t' = t - 1/(2N) -> t'' = t - 1/N.  Three launches around the two teacher
 * forwards and the student forward.  coef[n][20] (device), per sample, computed on the host in fp64 from the fp32-rounded
 * log-SNRs, every slot rounded once on its own:
 *    0  1  2   a0 b0x b0e of the TEACHER at t :  x_hat  = clip?(a0*z_t  + b0x*out (+ b0e*out_eps))
 *    3  4      c1 c2 of the DDIM step t' <- t :  z_t'   = c1*z_t + c2*x_hat
 *    5  6  7   a0 b0x b0e of the teacher at t':  x_hat' = clip?(a0*z_t' + b0x*out (+ b0e*out_eps))
 *    8  9      w1 w2, w1 + w2 = 1            :  x_tilde = w1*x_hat + w2*x_hat'   (w2 = c2(t''<-t')/c2(t''<-t); (0, 1) where t'' = 0)
 *   10 11 12   a0 b0x b0e of the STUDENT at t :  x_stud = a0*z_t + b0x*out (+ b0e*out_eps)
 *   13         omega, the loss weight of the sample       14  w_guide of the teacher
 *   15         logsnr(t): vd_q_sample's argument, kept beside the weights made from it; no vd_distill_* kernel reads it
 *   16 17 18   a0 - 1 of slots 0, 5, 10                   19  c1 + c2 - 1
 * Slots 16..19 serve the residual x_stud - x_tilde, which is assembled from each prediction's difference from the state it was made
 * from, (a0 - 1)*z + b0x*out (+ b0e*out_eps), never from the predictions themselves: at high log-SNR they all lie within 1e-3..1e-5 of
 * z_t, where one fp32 ulp of a weight near 1 is up to 1e-3 of the residual (cf. slot 7 of vd_bpd_terms).
 * With cfg the teacher outputs have 2n rows, cond/uncond interleaved as in vd_sample_step, and every teacher prediction is
 * guided in x-space after the optional clip: x = x_c + w_guide (x_c - x_u).  Outputs of a "both" network have 2C channels.
 * Any C*HW; 64-bit element offsets.  dwordx4 accesses when C*HW is a multiple of 4 and all bases are 16-byte aligned, scalar otherwise. */
/* x_hat, d_hat = x_hat - z_t (difference form), z_t' (n rows each) and, when zdup is given (cfg only), z_t' duplicated to 2n interleaved
 * rows = the next teacher input */
int vd_distill_mid(const float* zt, const float* teacher_out, const float* coef, int32_t teacher_out_type, int32_t cfg, int32_t clip,
                   float* xhat, float* dhat, float* zmid, float* zdup, int32_t n, int32_t C, int32_t HW, void* stream);
/* teacher_out = the teacher's output at (z_t', t').  loss[n] = omega * mean_{c,h,w}((x_stud - x_tilde)^2), one workgroup per sample,
 * fixed summation order (bitwise reproducible); resid (n, C, HW) = x_stud - x_tilde for the backward pass; xtilde optional (xhat is
 * read only when it is asked for). */
int vd_distill_loss_fwd(const float* xhat, const float* dhat, const float* zmid, const float* teacher_out, const float* zt,
                        const float* student_out, const float* coef, int32_t teacher_out_type, int32_t student_out_type, int32_t cfg,
                        int32_t clip, float* loss, float* resid, float* xtilde, int32_t n, int32_t C, int32_t HW, void* stream);
/* dout = gloss[b] * omega_b * 2/(C*HW) * resid * b0x   (channels C..2C of a "both" student: * b0e) */
int vd_distill_loss_bwd(const float* resid, const float* coef, const float* gloss, int32_t student_out_type, float* dout,
                        int32_t n, int32_t C, int32_t HW, void* stream);
/* consistency distillation (Song et al. 2023; Luo et al. 2023) and consistency training (Song & Dhariwal 2024): the student at
 * (z_t, t = i/N) regresses on a TARGET network at (z_s, s = (i-1)/N), where z_s is one DDIM step of a frozen teacher down from z_t
 * (distillation) or the same x_0, eps noised to s (training).  Launches around the network forwards: vd_consist_mid or vd_consist_pair,
 * vd_consist_loss_fwd / _bwd.  coef[n][24] (device), per sample, computed on the host in fp64 from the fp32-rounded log-SNRs, every
 * slot rounded once on its own:
 *    0  1  2   a0 b0x b0e of the TEACHER at t :  x_hat  = clip?(a0*z_t + b0x*out (+ b0e*out_eps))          (0 in training mode)
 *    3  4      c1 c2 of the DDIM step s <- t  :  z_s    = c1*z_t + c2*x_hat          ((0, 1) where i = 1: z_0 is x_hat itself)
 *    5  6  7   a0 b0x b0e of the TARGET at s  :  x_tgt  = a0*z_s + b0x*out (+ b0e*out_eps)     (the student's parameterisation)
 *    8  9 10   a0 b0x b0e of the STUDENT at t :  x_stud = a0*z_t + b0x*out (+ b0e*out_eps)
 *   11         omega, the loss weight of the sample       12  w_guide of the teacher
 *   13         logsnr(t): vd_q_sample's argument; vd_consist_pair forms z_t from it exactly as vd_q_sample does
 *   14 15 16   a0 - 1 of slots 0, 5, 8                    17  c1 + c2 - 1 (0 where i = 1)
 *   18 19      alpha_s - alpha_t, sigma_s - sigma_t       20 21  alpha_s, sigma_s
 *   22         1 where i = 1 (s = 0), else 0              23  0
 * The residual is assembled from differences, as vd_distill_loss_fwd's and for its reason:
 *   resid = [(a0_stud - 1) z_t + b0x out_stud] - [(a0_tgt - 1) z_s + b0x out_tgt] - dz,   dz = z_s - z_t from slots 17, 4 or 18, 19.
 * Rows with slot 22 set take the boundary condition f(z, 0) = z: the target is z_s itself, SELECTED -- the target network's output is
 * not read on such a row, so nothing in it reaches loss, resid or gradient.  No atomics, no workspace: the same call gives the same
 * bits.  Any C*HW; 64-bit element offsets; dwordx4 accesses when C*HW is a multiple of 4 and all bases are 16-byte aligned, scalar
 * otherwise, and the two agree bit for bit. */
/* distillation mode.  teacher_out: n*(1+cfg) rows, cond/uncond interleaved, guided in x-space after the optional clip as in
 * vd_distill_mid.  Writes z_s, dz = (c1 + c2 - 1) z_t + c2 (x_hat - z_t) and, when asked, x_hat (n rows each). */
int vd_consist_mid(const float* zt, const float* teacher_out, const float* coef, int32_t teacher_out_type, int32_t cfg, int32_t clip,
                   float* zs, float* dz, float* xhat, int32_t n, int32_t C, int32_t HW, void* stream);
/* training mode, one pass: z_t = vd_q_sample's value bit for bit, z_s = alpha_s x_0 + sigma_s eps, dz = (alpha_s - alpha_t) x_0 +
 * (sigma_s - sigma_t) eps */
int vd_consist_pair(const float* x0, const float* eps, const float* coef, float* zt, float* zs, float* dz, int32_t n, int32_t C,
                    int32_t HW, void* stream);
/* student_out, target_out: n rows in the parameterisation out_type.  One workgroup per sample, fixed summation order, S = sum resid^2
 * in fp64, D = C*HW.  metric 0 (l2): loss = omega S/D, aux = 2/D.  metric 1 (pseudo-Huber, huber_c = c > 0): loss = omega (sqrt(S + c^2)
 * - c) evaluated as omega S/(sqrt(S + c^2) + c), aux = 1/sqrt(S + c^2).  resid (n, C, HW) and aux[n] serve the backward; target
 * (optional) = the target image, z_s on rows with i = 1. */
int vd_consist_loss_fwd(const float* zt, const float* zs, const float* dz, const float* student_out, const float* target_out,
                        const float* coef, int32_t out_type, int32_t metric, double huber_c, float* loss, float* resid, float* aux,
                        float* target, int32_t n, int32_t C, int32_t HW, void* stream);
/* dout = gloss[b] * omega_b * aux[b] * resid * b0x   (channels C..2C of a "both" student: * b0e) */
int vd_consist_loss_bwd(const float* resid, const float* coef, const float* gloss, const float* aux, int32_t out_type, float* dout,
                        int32_t n, int32_t C, int32_t HW, void* stream);
/* e <- e + (1 - decay) (p - e) over every tensor of a module in ONE launch.  items_dev = [n][8] int64 {dst e, src p, count, 0, 0, 0, 0,
 * first block}, blocks of 256 elements, total_blocks = the sum of ceil(count/256).  1 - decay is rounded to fp32 once; decay = 0 copies
 * (e <- p, selected), decay = 1 launches nothing. */
int vd_ema_track_batched(const int64_t* items_dev, int32_t n, int64_t total_blocks, double decay, void* stream);
/* one reverse step of DPM-Solver++(2M) (Lu et al. 2022, data-prediction form): the second-order multistep solver of the
 * probability-flow ODE in log-SNR time, for a batch that shares the step.  xt, hist, xn: n images (NCHW); out: n*(1+cfg) images,
 * cond/uncond interleaved when cfg, 2C channels for a "both" network; xdup (optional, cfg only): 2n images.
 * k: 8 floats {a0, b0x, b0e, c1, c2, c2rho, w_guide, 0}, host (k) or device (k_dev), exactly one of the two as in vd_sample_step.
 * c1 = sigma_s/sigma_t and c2 = alpha_s (1 - e^-h) are the DDIM weights of the step t -> s, h = (logsnr_s - logsnr_t)/2, and
 * c2rho = c2 * h/(2 h_prev) is a slot of its own (rounded once from fp64, not fl(c2)*fl(rho)).  Evaluation order, all in fp32,
 * per element:
 *   x_c  = clip?(a0*xt + b0x*out_c (+ b0e*out_c,eps))     and x_u likewise from the odd rows when cfg (clip per branch, then guide)
 *   g    = cfg ? x_c + w_guide*(x_c - x_u) : x_c
 *   xn   = c1*xt + c2*g + c2rho*(g - hist)
 *   hist = g                                              (read, then overwritten in place: the next step's previous prediction)
 *   xdup = xn on rows 2b and 2b+1                         (the next guided network input)
 * There is no first- or last-step flag: c2rho = 0 makes the step DDIM (the first step of a chain, whose hist the host zero-fills, and
 * every step of order 1), and the row (c1, c2, c2rho) = (0, 1, 0) returns g, the guided x0 prediction every sampler here ends on.
 * xn may alias xt; hist is a buffer of its own.  Any C*HW; 64-bit element offsets; dwordx4 accesses when C*HW is a multiple of 4
 * and all bases are 16-byte aligned, scalar otherwise. */
int vd_solver_step(const float* xt, const float* out, float* hist, const float* k, const float* k_dev,
                   int32_t model_out_type, int32_t cfg, int32_t clip,
                   float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream);
/* one node of the UniPC multistep predictor-corrector (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast
 * Sampling of Diffusion Models", data-prediction form, B(h) = h or e^h - 1), for a batch that shares the node, ONE launch.  The
 * network was called at the PREDICTED state xt; its guided x0 prediction g corrects the step that arrived at this node at no further
 * network call, the predictor of the step that leaves starts from the corrected state, and the history of the last three guided
 * predictions shifts by one.  xt, h0, h1, h2, xn, xc_out: n images (NCHW), h0 the newest prediction; out: n*(1+cfg) images,
 * cond/uncond interleaved when cfg, 2C channels for a "both" network; xdup (optional, cfg only): 2n images; xc_out (optional): the
 * corrected state.
 * k: 16 floats {a0, b0x, b0e, w_guide, c1, c2, p1, p2, eg, e1, e2, 0, 0, 0, 0, 0}, host (k) or device (k_dev), exactly one of the two
 * as in vd_solver_step.  c1, c2 are the DDIM weights of the leaving step; with r_k the log-SNR distance of the k-th older prediction in
 * units of the step and rho^p, rho^c the predictor's and the corrector's weights (v_diffusion.unipc_coefs: host fp64, each slot rounded
 * once), p_k = -alpha_next B rho^p_k / r_k of the leaving step and eg = -alpha B rho^c_p, e_k = -alpha B (rho^c_k - rho^p_k) / r_k
 * of the arriving one.  Evaluation order, all in fp32, per element:
 *   x_c, x_u = clip?(a0*xt + b0x*out (+ b0e*out_eps))      per branch, as vd_solver_step (clip per branch, then guide)
 *   g        = cfg ? x_c + w_guide*(x_c - x_u) : x_c
 *   xc       = xt + eg*(g - h0) + e1*(h1 - h0) + e2*(h2 - h0)      the corrector of the step that arrived at this node
 *   xn       = c1*xc + c2*g + p1*(h0 - g) + p2*(h1 - g)            the predictor of the step leaving it
 *   h2 = h1;  h1 = h0;  h0 = g                              (read, then overwritten in place)
 *   xdup     = xn on rows 2b and 2b+1;   xc_out = xc
 * There is no first- or last-node flag: eg = e1 = e2 = 0 leaves xc = xt (the first node of a chain, whose history the host
 * zero-fills, and every node without the corrector), p2 = 0 with p1 = -c2rho is the vd_solver_step update, and (c1, c2, p1, p2) =
 * (0, 1, 0, 0) returns g, the guided x0 prediction every sampler here ends on.  xn may alias xt; h0, h1, h2 and xc_out are buffers of
 * their own.  No workspace, no atomics: HIP-graph capturable.  Any C*HW; 64-bit element offsets; dwordx4 accesses when C*HW is a
 * multiple of 4 and all bases are 16-byte aligned, scalar otherwise. */
int vd_unipc_step(const float* xt, const float* out, float* h0, float* h1, float* h2, const float* k, const float* k_dev,
                  int32_t model_out_type, int32_t cfg, int32_t clip,
                  float* xn, float* xdup, float* xc_out, int32_t n, int32_t C, int32_t HW, void* stream);
/* dynamic thresholding (Saharia et al. 2022, "Imagen", section 2.3; the companion Lu et al. 2022 recommend for the data-prediction
 * solver under guidance).  kth[b] = the element of rank r (0-based, ascending) of |x[b, 0..N)|, for n rows of N floats, 0 <= r < N.
 * Order: the bit pattern of |x| as an unsigned integer -- -0 = +0, denormals order as numbers, +Inf above every finite value, a NaN
 * above +Inf (where numpy.partition puts it).  The result is one of the row's own values, exact and bitwise reproducible: a radix
 * select (four passes of 8 bits, LDS histograms, integer counts, no floating-point atomics).  One workgroup owns one row and waits
 * on no other workgroup.  There is one code path for every N <= VD_KTH_MAX_ROW (no size boundary between forms other than the access
 * width: dwordx4 when N is a multiple of 4 and x is 16-byte aligned, scalar otherwise; one workgroup is 1024 threads, so rows of more
 * than 1024 accesses take more than one trip per pass). */
#define VD_KTH_MAX_ROW 2147483647LL
int vd_abs_kth_rows(const float* x, int32_t n, int64_t N, int64_t r, float* kth, void* stream);
/* vd_solver_step with the guided prediction thresholded dynamically instead of each branch clipped to [-1, 1]: ONE launch, same table
 * row, same aliasing rules, same host-or-device coefficient forms, same access forms.  Per sample, over its N = C*HW elements:
 *   x_c, x_u = a0*xt + b0x*out (+ b0e*out_eps)            per branch, NOT clipped
 *   g        = cfg ? x_c + w_guide*(x_c - x_u) : x_c
 *   s_raw    = the element of rank r of |g|               (vd_abs_kth_rows' order and selection, inside this launch)
 *   s        = min(max(s_raw, 1), s_max)                  s_max >= 1, +Inf for no cap; a NaN s_raw stays a NaN
 *   g'       = min(max(g, -s), s) / s                     IEEE fp32 division
 *   xn       = c1*xt + c2*g' + c2rho*(g' - hist);   hist = g';   xdup = xn on rows 2b and 2b+1
 * r is the caller's: r = min(N-1, ceil(q*(N-1))) for the quantile q in (0, 1], computed once in fp64 on the host
 * (v_diffusion.threshold_rank) -- the "higher" order statistic, a value of the sample itself, where Imagen interpolates a percentile;
 * the two differ by at most the gap between two neighbouring order statistics.  q = 1: s_raw = max|g|, a pure rescale.
 * An s that is NaN or Inf makes that sample's outputs NaN or 0; other samples are unaffected.  A NaN element of g passes through.
 * s_out (optional, n floats) receives s.  One workgroup owns one sample from its first read to its last write (it re-reads the
 * sample's input rows once per selection pass and once more for the update; they stay in L2) and waits on no other workgroup: the
 * launch is HIP-graph capturable and has no workspace.  Every pass evaluates g by the same fused operations, so the element that
 * holds s_raw > 1 maps to exactly +-1; with s_max = 1 and cfg = 0 the result equals vd_solver_step(clip = 1) bit for bit. */
int vd_solver_step_dyn(const float* xt, const float* out, float* hist, const float* k, const float* k_dev,
                       int32_t model_out_type, int32_t cfg, int64_t r, float s_max, float* s_out,
                       float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream);
/* one reverse step of RePaint inpainting (Lugmayr et al. 2022) in log-SNR terms, ONE launch: vd_sample_step for the unknown region, a
 * draw from q(x_s | x_known) for the known region, and their merge by the mask.  xt, noise, known, knoise, xn: n images (NCHW); out:
 * n*(1+cfg) images, cond/uncond interleaved when cfg, 2C channels for a "both" network; mask: n x mask_c x HW floats in [0, 1] with
 * mask_c = 1 (shared by the channels) or C, 1 = keep the known image; xdup (optional, cfg only): 2n images.
 * k: 10 floats, host (k) or device (k_dev), exactly one of the two as in vd_sample_step: k[0..7] = vd_sample_step's
 * {a0, b0x, b0e, c1, c2, noise_scale, w_guide, c3}, k[8], k[9] = {ak, bk}, the alpha and sigma of the state the step lands on ((1, 0) for
 * the last step, which returns a prediction).  Evaluation order, all in fp32, per element:
 *   x0h  = clip?(a0*xt + b0x*out (+ b0e*out_eps))           per branch
 *   mean = last_step ? x0h : c1*xt + c2*x0h + c3*out
 *   v    = cfg ? mean_c + w_guide*(mean_c - mean_u) : mean_c
 *   u    = v + noise_scale*noise                            (u = v when noise is null)   -- vd_sample_step's value, same expressions
 *   kn   = ak*known + bk*knoise                             (kn = ak*known when knoise is null)
 *   xn   = m == 1 ? kn : m == 0 ? u : m*kn + (1 - m)*u
 *   xdup = xn on rows 2b and 2b+1                           (the next guided network input)
 * The two ends of the mask are selections, not products: a NaN or Inf of the branch not chosen does not reach xn.  With the host form,
 * a null noise needs k[5] == 0 and a null knoise k[9] == 0.  xn may alias xt (each thread reads all it needs before it writes).  No
 * workspace, no LDS, no waiting on another workgroup; HIP-graph capturable with k_dev.  Any C*HW; 64-bit element offsets; dwordx4
 * accesses when C*HW is a multiple of 4, all bases are 16-byte aligned and, for mask_c = 1, HW is a multiple of 4 (a vector then
 * straddles neither two samples, nor the two halves of a "both" output, nor two channels of the shared mask), scalar otherwise. */
int vd_inpaint_step(const float* xt, const float* out, const float* noise, const float* known, const float* mask, const float* knoise,
                    const float* k, const float* k_dev, int32_t model_out_type, int32_t cfg, int32_t last_step, int32_t clip,
                    int32_t mask_c, float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream);
/* the forward transition q(x_t | x_s) of any length in one launch: xn = a*x + b*noise over n rows of N floats, k = {a, b} host or k_dev
 * device, exactly one of the two.  For s < t: a = alpha_t/alpha_s, b^2 = sigma_t^2 (1 - e^(logsnr_t - logsnr_s)) (v_diffusion.jump_coefs):
 * a jump of j grid steps is one Gaussian draw, not j.  xdup (optional): xn on rows 2b and 2b+1, the next guided network input.  xn may
 * alias x.  Access forms as above: dwordx4 when N is a multiple of 4 and all bases are 16-byte aligned, scalar otherwise. */
int vd_forward_jump(const float* x, const float* noise, const float* k, const float* k_dev, float* xn, float* xdup, int32_t n, int64_t N,
                    void* stream);
/* one step of DDPM noise-space inversion (Huberman-Spiegelglas et al. 2024, "An Edit Friendly DDPM Noise Space") in log-SNR terms, ONE
 * launch after the step's network call: the next state is drawn from the image itself and the noise map that makes the ordinary
 * reverse step land on it is extracted.  xt (the state x_{i+1} the network saw), x0, eps, xs, z: n images (NCHW); out: n*(1+cfg)
 * images, cond/uncond interleaved when cfg, 2C channels for a "both" network; xdup (optional, cfg only): 2n images.
 * k: vd_inpaint_step's 10 floats, host (k) or device (k_dev), exactly one of the two: k[0..7] = vd_sample_step's
 * {a0, b0x, b0e, c1, c2, noise_scale, w_guide, c3} of the step that lands on index i, k[8], k[9] = {ak, bk} = the alpha and sigma of
 * index i.  Evaluation order, all in fp32, per element:
 *   x0h  = clip?(a0*xt + b0x*out (+ b0e*out_eps))           per branch
 *   mean = last_step ? x0h : c1*xt + c2*x0h + c3*out
 *   v    = cfg ? mean_c + w_guide*(mean_c - mean_u) : mean_c                 -- vd_inpaint_step's expressions, same fused operations
 *   xs   = ak*x0 + bk*eps                                   (xs = ak*x0 when eps is null)   -- vd_inpaint_step's kn, bit for bit
 *   z    = (xs - v) / noise_scale                           one fp32 subtraction, one IEEE fp32 division
 *   xdup = xs on rows 2b and 2b+1                           (the next guided network input)
 * vd_sample_step on (xt, out, noise = z) then returns xs to rounding.  The step to index 0 has no noise of its own: pass last_step = 1,
 * k[5] = 1, (ak, bk) = (1, 0) and a null eps, and z is the residual x0 - x0h.  xs depends on neither xt nor out: a NaN of the network
 * stays in that sample's z.  With the host form k[5] must be finite and non-zero and a null eps needs k[9] == 0.  xs may alias xt (each
 * thread reads all it needs before it writes); z is a buffer of its own.  No workspace, no LDS, no waiting on another workgroup;
 * HIP-graph capturable with k_dev.  Any C*HW; 64-bit element offsets; dwordx4 accesses when C*HW is a multiple of 4 and all bases are
 * 16-byte aligned, scalar otherwise; the two forms give the same bits. */
int vd_noise_extract(const float* xt, const float* out, const float* x0, const float* eps, const float* k, const float* k_dev,
                     int32_t model_out_type, int32_t cfg, int32_t last_step, int32_t clip, float* xs, float* z, float* xdup, int32_t n,
                     int32_t C, int32_t HW, void* stream);
/* spherical interpolation of n pairs of rows of N floats, ONE launch: out[r] = wa*a[r] + wb*b[r].  The fraction f is one host float
 * (frac) for all rows or n device floats (frac_dev), exactly one of the two.  One workgroup (1024 threads) owns one row and waits on no
 * other.  Pass 1: <a,b>, |a|^2, |b|^2 in fp64, thread t adding the products of its accesses t, t + 1024, ... in order, the lanes of a
 * wave by a fixed butterfly, the 16 wave sums in wave order -- no atomics, the same bits on every call.  Then, in fp64 on one thread:
 *   c = <a,b> / (|a| |b|) clamped to [-1, 1],  w = acos(c),  (wa, wb) = (sin((1-f) w), sin(f w)) / sin(w), each rounded to fp32 once;
 *   (wa, wb) = (1 - f, f) when sin(w) < 1e-6 (parallel or antiparallel rows) or a norm is 0.
 * Pass 2 re-reads the rows: out = fma(wb, b, wa*a) in fp32.  A NaN makes its own row NaN and no other.  w_out (optional, n x 2 floats)
 * receives (wa, wb).  out may alias neither input.  Access forms as above: dwordx4 when N is a multiple of 4 and a, b, out are 16-byte
 * aligned, scalar otherwise (the two forms add in different orders and may differ in the last bit of a weight). */
int vd_slerp_rows(const float* a, const float* b, const float* frac, const float* frac_dev, float* out, float* w_out, int32_t n, int64_t N,
                  void* stream);
/* Diffusion Posterior Sampling (Chung et al. 2023, Algorithm 1; csrc/diffusion.hip): the two launches of one reverse step, either side
 * of the network's input gradient.  Conventions of the reverse steps above: images NCHW fp32; k = the 8 host floats of
 * vd_sample_step {a0, b0x, b0e, c1, c2, noise_scale, w_guide, c3}; out = n*(1+cfg) rows, cond and uncond interleaved, of C channels
 * (2C for "both", model_out_type 3).  Both return 1 before any launch on a bad model_out_type or op, a null required buffer or
 * n, C, H, W (HW) < 1.
 *
 * The measurement operator A acts per sample on the guided prediction g (C, H, W):
 *   op 0  mask      A g = M (.) g, M = mask[n][par][H][W] with par = 1 or C channels, values in [0, 1];   A^T r = M (.) r
 *   op 1  box down-sampling by par in {2, 4, 8} (H, W multiples of it, refused otherwise): the mean over par x par blocks,
 *         (C, H/par, W/par);   A^T r = r / par^2 on every element of the block
 *   op 2  grey      the mean over the channels, (1, H, W);   A^T r = r / C on every channel
 *
 * vd_dps_residual: per branch p = a0*xt + b0x*out (+ b0e*out_eps), xhat = clip ? clamp(p, -1, 1) : p, and the pass mask m = 1 where
 *   -1 <= p <= 1 or clip is off (torch.clamp's subgradient, boundary included).  g = xhat_c + w (xhat_c - xhat_u) with cfg, else xhat;
 *   r = meas - A g (meas: n samples of A's image);  sumsq[b] = sum r^2 over the sample, in a fixed order (one workgroup per sample, no
 *   atomics, no workspace: the same call gives the same bits);  u = -A^T r.  Cotangents of (1/2)||r||^2, unnormalised:
 *     dout (the shape of out)  cond rows (1 + w) m_c u, uncond rows -w m_u u (without cfg: m u), times b0x on the first C channels and
 *                              b0e on the second C of "both"
 *     dxt[n][C][H][W]          a0 [(1 + w) m_c - w m_u] u   (a0 m u without cfg)
 *     x0hat (optional)         g
 * vd_dps_step: vd_sample_step's row (same device helpers: prediction, clip, guided mean, last_step, noise), then
 *     xn -= zeta / sqrt(sumsq[b]) * (dxt[b] + dxin[2b] + dxin[2b+1])      (dxt[b] + dxin[b] without cfg)
 *   with dxin (n*(1+cfg) rows of C*HW) the network's input gradient of dout.  The term is selected, not multiplied: with zeta = 0 or
 *   sumsq[b] = 0 row b is vd_sample_step's bit for bit and a NaN in its dxin / dxt reaches nothing; a sumsq[b] that is not finite makes
 *   that row NaN and leaves the others alone.  Writes xn and the optional xdup (rows 2b, 2b+1); xn may alias xt.  dwordx4 accesses when
 *   C*HW is a multiple of 4 and every base is 16-byte aligned, scalar otherwise: the same bits. */
int vd_dps_residual(const float* xt, const float* out, const float* meas, const float* mask, const float* k, int32_t model_out_type,
                    int32_t cfg, int32_t clip, int32_t op, int32_t par, float* dout, float* dxt, float* sumsq, float* x0hat, int32_t n,
                    int32_t C, int32_t H, int32_t W, void* stream);
int vd_dps_step(const float* xt, const float* out, const float* noise, const float* dxin, const float* dxt, const float* sumsq,
                const float* k, float zeta, int32_t model_out_type, int32_t cfg, int32_t last_step, int32_t clip, float* xn, float* xdup,
                int32_t n, int32_t C, int32_t HW, void* stream);
/* Denoising Diffusion Null-space Model (Wang, Yu, Zhang 2023; csrc/diffusion.hip): one reverse step whose x0 prediction takes its
 * range-space part from a measurement meas = A x and keeps the network's null-space part, g_hat = g + lam * A^+(meas - A g) -- ONE launch,
 * no gradient.  Conventions of the reverse steps above and of the DPS entries: images NCHW fp32; k = the 8 host floats of
 * vd_sample_step {a0, b0x, b0e, c1, c2, noise_scale, w_guide, c3}; out = n*(1+cfg) rows, cond and uncond interleaved, of C channels (2C
 * for "both", model_out_type 3); op, par, mask, meas as vd_dps_residual takes them:
 *   op 0  mask      A g = M (.) g, M = mask[n][par][H][W] with par = 1 or C channels, values in [0, 1];   A^+ r = r / M where M > 0
 *   op 1  box down-sampling by par in {2, 4, 8}: the mean over par x par blocks, (C, H/par, W/par);   A^+ r = r on every element of the block
 *   op 2  grey      the mean over the channels, (1, H, W);   A^+ r = r on every channel
 *
 * Per element of the preimage of measurement element j (1, par^2 or C elements; the preimages tile the image):
 *   v  = vd_sample_step's value, the same device helpers: the clipped prediction per branch, the mean c1*xt + c2*x0_hat (x0_hat itself on
 *        the last step), the guided mean, + k[5]*noise when noise is given
 *   g  = the guided clipped prediction (vd_dps_residual's);  A g = the preimage summed in fp64 and rounded once (vd_dps_residual's rule)
 *   r  = meas_j - A g;   d = A^+ r;   xn = fma(cw, d, v) with cw = lam on the last step, else c2*lam rounded once per launch
 * Selected, not multiplied:
 *   lam == 0              the row is vd_sample_step's bit for bit; without sumsq, meas and mask are not read
 *   mask, M == 0          no correction and no share of sumsq: a NaN in meas there reaches nothing
 *   mask, M == 1, last step, lam == 1 and no noise term (noise null or k[5] == 0):  xn = meas bit for bit
 * sumsq (optional, n floats): sumsq[b] = sum of r^2 over the measured elements of sample b (mask: those with M > 0), added in fp64 in a
 * fixed order (one workgroup per sample, no atomics, no workspace: the same call gives the same bits), stored as fp32; null skips it.
 * Writes xn and the optional xdup (rows 2b, 2b+1); xn may alias xt.  dwordx2 / dwordx4 row accesses when every base is 16-byte aligned,
 * scalar otherwise: the same bits, sumsq included.
 * Returns 1 before any launch on what vd_dps_residual refuses -- a bad model_out_type or op, a null required buffer (xt, out, meas, k, xn,
 * the mask of op 0), n, C, H, W < 1, a mask of neither 1 nor C channels, a factor outside {2, 4, 8} or not dividing H and W -- and on
 * noise == null with k[5] != 0, and on a sample whose output row (C*H*W floats, twice that for "both") does not fit 2^31 - 1: offsets
 * inside a sample are 32-bit. */
int vd_ddnm_step(const float* xt, const float* out, const float* noise, const float* meas, const float* mask, const float* k, float lam,
                 int32_t model_out_type, int32_t cfg, int32_t last_step, int32_t clip, int32_t op, int32_t par, float* xn, float* xdup,
                 float* sumsq, int32_t n, int32_t C, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------ loss-aware timestep resampling (resample.hip)
 * Nichol & Dhariwal 2021, section 3.3: timesteps drawn in proportion to sqrt(E[L_t^2]) and the loss reweighted by 1/(T p_t), with the
 * history of the last K losses per timestep resident on the device (no counterpart in the reference; improved-diffusion's
 * LossSecondMomentResampler keeps it in numpy and draws on the host).  State: hist [T][K] fp32, count [T] int32 (entries held, at most
 * K), pos [T] int32 (next ring slot), cdf [T] fp64.  1 <= T <= 65536, K >= 1.
 *
 * the draw of B timesteps from B uniforms u in [0, 1) (fp64), ONE launch of one workgroup (1024 threads) that waits on no other; no
 * atomics, no workspace, a fixed summation order: the same inputs give the same bits on every call; HIP-graph capturable.  All
 * arithmetic in fp64.  The kernel decides on the device whether the history is warmed up (every count[t] == K):
 *   warmed up: m_t = sqrt(sum_k hist[t][k]^2 / K) (k ascending), S = sum_t m_t, q_t = (1 - uniform_prob) m_t / S + uniform_prob / T
 *              (q_t = 1/T when S is 0 or not finite), cdf[i] = sum_{j <= i} q_j; idx = min(T - 1, #{i : cdf[i] <= u}) by binary search,
 *              w = fp32(1 / (T q_idx)) with q_idx re-evaluated from its history row by the same expression;
 *   otherwise: idx = min(T - 1, floor(u T)), w = 1 exactly, cdf[i] = (i + 1) / T.
 *   t = (idx + 1) / T either way, the value of a uniform draw on the discrete grid.
 * S: thread j adds m_j, m_(j + 1024), ... in order, the 64 lanes of a wave by a fixed butterfly, the 16 wave sums in wave order.  The
 * scan runs over chunks of 1024 timesteps: shuffles inside a wave, the totals of the waves in front added in wave order, the chunks in
 * front carried in a register.  cdf differs from a sequential fp64 sum by rounding only (at most T ulps of 1 in the worst case, a few
 * in practice).  The searches read cdf from LDS for T <= 4096 and from memory above that.  A NaN or negative u lands on index 0. */
int vd_lsm_draw(const float* hist, const int32_t* count, const double* u, double* cdf, double* t_out, int32_t* idx_out, float* w_out,
                int32_t T, int32_t K, int32_t B, double uniform_prob, void* stream);
/* n rows (idx[r], loss[r]) enter the history in row order, ONE launch: a row with idx outside [0, T) or a loss that is not finite is
 * skipped; otherwise hist[idx][pos[idx]] = loss, pos[idx] = (pos[idx] + 1) mod K, count[idx] = min(count[idx] + 1, K).  One thread
 * owns one timestep and walks the rows, staged through LDS 1024 at a time, in order: the state afterwards is the sequential loop's bit
 * for bit, also when a timestep occurs many times in one call (T n integer compares: nothing at T = 1000, n <= 8192).  No atomics, no
 * waiting on another workgroup; n = 0 launches nothing. */
int vd_lsm_update(float* hist, int32_t* count, int32_t* pos, const int32_t* idx, const float* loss, int32_t n, int32_t T, int32_t K,
                  void* stream);

/* ------------------------------------------------------------------ optimizer tail (train_utils.py:159-168, utils.py:144-149)
 * sum of squares of a flat buffer (global-norm clip), fused clip + AdamW + EMA over flat fp32 buffers */
size_t vd_sumsq_ws_bytes(int64_t n);
int vd_sumsq(const float* g, int64_t n, float* out1, float* ws, size_t ws_bytes, void* stream);
/* [r_lo, r_hi) with r_mode != 0 is an index range treated apart this step (the class-embedding tensors, unet.py:207-215):
 * r_mode 1 = the range received no gradient (class-conditional net called with y = None; the reference leaves .grad None and
 * torch.optim.AdamW skips it: p, m, v untouched, per-parameter step not advanced; the EMA shadow still follows p);
 * r_mode 2 = the range is updated with its own bias corrections r_bc1, r_bc2 (its step count lags). r_mode 0: ignored.
 * beta1, beta2 and ema_decay are doubles: the rates 1 - beta1, 1 - beta2, 1 - ema_decay are formed in double on the host and rounded
 * to fp32 once, which is what torch.optim.AdamW and utils.py:149 hand to their fp32 operators (1.f - 0.9999f is 1.66e-4 off 1e-4,
 * 1.f - 0.999f is 1.29e-5 off 1e-3; as vd_ema_track_batched's decay). */
int vd_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                 const float* gnorm_sq, float max_norm, float lr, double beta1, double beta2, float eps, float wd,
                 float bc1, float bc2, double ema_decay, int64_t r_lo, int64_t r_hi, int32_t r_mode, float r_bc1, float r_bc2,
                 void* stream);
/* the same update with the decision about [r_lo, r_hi) made ON THE DEVICE: r_flag[0] > 0 (device float: "some rank's micro-batch of
 * this update carried labels" -- one slot behind the flat gradient buffer, summed over ranks by the last gradient bucket's
 * all-reduce) -> the range is updated with the bias corrections of step count r_steps[0] + 1 (1 - r_beta^k, evaluated in double on
 * the device) and r_steps[0] is advanced; else the range is skipped as r_mode 1 does.  No host ever reads the flag: replaces the
 * per-update host all-reduce the reference's DDP + torch.optim.AdamW pair needs no equivalent of (train_utils.py:159-163:
 * optimizer.step() skips parameters whose .grad is None; under DDP that is the same on every rank by construction). */
int vd_adamw_ema_flagged(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                         const float* gnorm_sq, float max_norm, float lr, double beta1, double beta2, float eps, float wd,
                         float bc1, float bc2, double ema_decay, int64_t r_lo, int64_t r_hi, const float* r_flag, int32_t* r_steps,
                         double r_beta1, double r_beta2, void* stream);

/* ------------------------------------------------------------------ k-NN precision / recall (metrics.hip)
 * The improved precision / recall metric (reference v_diffusion/metrics/precision_recall.py) on fp16 feature rows: a tiled fp16
 * distance GEMM (v_mfma_f32_32x32x16_f16, fp32 accumulation) whose output is reduced per row as it is produced -- no distance
 * matrix in memory (the reference materialises it through torch.cdist and copies it to the host, :50-62).
 * Features: [n][d] IEEE binary16 bits, rows contiguous, base 16-byte aligned, d a positive multiple of 64 (pad with zeros: a zero
 * column changes no distance).  Norms: the fp32 squared row norms written by vd_rows_sqnorm_f16 for those rows (the same MFMA
 * chain as the distance products, so identical rows are at distance exactly 0).
 * d2 = max(|x|^2 + |y|^2 - 2 x.y, 0) in fp32, distance = sqrtf(d2) correctly rounded.  Fixed-order, no atomics: bitwise
 * reproducible.  Any n >= 1 on either side; 64-bit row offsets. */
int    vd_rows_sqnorm_f16(const uint16_t* x, int64_t n, int32_t d, float* sq, void* stream);
/* out[i] = the kth-th smallest distance from q_i to the rows of c, counted with multiplicity (torch.kthvalue(kth) of the distance
 * row: for c == q the self-distance 0 is one of them); 1 <= kth <= min(16, nc).  ws: vd_knn_kth_ws_bytes(nq, nc, kth) bytes,
 * 16-byte aligned (partial lists of the column splits, O(nq kth)). */
size_t vd_knn_kth_ws_bytes(int64_t nq, int64_t nc, int32_t kth);
int    vd_knn_kth_f16(const uint16_t* q, const float* q_sq, int64_t nq, const uint16_t* c, const float* c_sq, int64_t nc, int32_t d,
                      int32_t kth, float* out, void* ws, size_t ws_bytes, void* stream);
/* hit[i] = 1 if some j has distance(q_i, s_j) <= radius[j] (fp32 radii), else 0: the coverage test of calc_pr (reference
 * precision_recall.py:177-206).  ws: vd_manifold_hits_ws_bytes(ns) bytes (per-support-row d2 thresholds). */
size_t vd_manifold_hits_ws_bytes(int64_t ns);
int    vd_manifold_hits_f16(const uint16_t* q, const float* q_sq, int64_t nq, const uint16_t* s, const float* s_sq, const float* radius,
                            int64_t ns, int32_t d, uint8_t* hit, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ FID statistics and products (fid.hip)
 * fp64 accumulation on v_mfma_f64_16x16x4_f64; one workgroup owns each 64 x 64 output tile and walks the whole reduction in order:
 * no atomics, the same call sequence gives bitwise identical results.
 * vd_fid_accum: one batch of fp32 activations x[n][d] (row pitch ldx floats) into running fp64 sums about a per-column shift:
 *   sum[c] += sum_i (x[i][c] - shift[c]),  outer[a][b] += sum_i (x[i][a] - shift[a]) (x[i][b] - shift[b])  (x - shift formed in fp64).
 *   outer is [d][d] contiguous and only its LOWER TRIANGLE OF 64 x 64 TILES is updated (tile row >= tile column, diagonal tiles in
 *   full); the caller mirrors it.  With N rows accumulated and delta = sum / N: mean = shift + delta,
 *   cov = (outer - N delta delta^T) / (N - 1).  shift must stay fixed between resets of sum / outer; vd_fid_shift writes the
 *   fp32-rounded column means of a batch (the first one), which makes every x - shift and every product exact for data of one scale.
 *   Domain: n >= 1, d a positive multiple of 16, ldx >= d and a multiple of 4, every pointer 16-byte aligned.
 * vd_atb_f64: C[m][n] = A^T B for fp64 A[k][m], B[k][n] (row-major, pitches lda / ldb / ldc doubles).
 *   Domain: k >= 1, m and n positive multiples of 16, lda >= m, ldb >= n, ldc >= n, lda and ldb even, 16-byte aligned pointers. */
int    vd_fid_shift(const float* x, int64_t n, int32_t d, int64_t ldx, double* shift, void* stream);
int    vd_fid_accum(const float* x, int64_t n, int32_t d, int64_t ldx, const double* shift, double* sum, double* outer, void* stream);
int    vd_atb_f64(const double* A, const double* B, double* C, int64_t k, int32_t m, int32_t n, int64_t lda, int64_t ldb, int64_t ldc,
                  void* stream);

/* ------------------------------------------------------------------ KID polynomial-kernel sums and Inception Score (kid.hip)
 * fp64 from fp32 rows, one fused pass, no n x n buffer, no atomics, every reduction in a fixed order: the same call gives bitwise
 * identical results.
 * vd_kid_sums: for subset s let X_s[i] = x[ix[s mx + i]] (row pitch ldx floats) and Y_s[j] = y[iy[s my + j]]; with
 *   k(a, b) = (gamma <a, b> + coef0)^degree,
 *   out[s][0] = sum over positions i != j of k(X_s[i], X_s[j]),  out[s][1] = the same over Y_s,
 *   out[s][2] = sum over all (i, j) of k(X_s[i], Y_s[j]).
 *   "Diagonal" means equal positions: an index that occurs twice in a subset is legal and its pair is counted.  A null ix (iy)
 *   means the identity and needs subsets == 1 and mx == nx (my == ny).  The features are widened to fp64 and multiplied on
 *   v_mfma_f64_16x16x4_f64, so every product is exact; the dot product accumulates over d in index order, gamma s + coef0 is one
 *   fp64 multiplication and one addition, the power degree - 1 left-to-right multiplications.  One workgroup owns a 64 x 64 tile
 *   of one Gram of one subset across all of d and writes one partial to ws; XX and YY run the lower triangle of tiles and double
 *   the off-diagonal partials; a second kernel adds each Gram's partials in a fixed order.
 *   Domain: d a positive multiple of 16; ldx, ldy >= d and multiples of 4; x, y, out, ws 16-byte aligned; 1 <= subsets <= 65535;
 *   2 <= mx <= nx, 2 <= my <= ny; 1 <= degree <= 8; ws of vd_kid_ws_bytes(subsets, mx, my) bytes (8 per tile; 0 = bad shape).
 *   PRECONDITION the library cannot check: every index in ix lies in [0, nx) and every index in iy in [0, ny) -- they are device
 *   memory, and a row gathered through an index out of range is read out of bounds.  Callers hand over only index arrays whose
 *   range they have checked on the host (the Python binding builds the device array itself from such a host array).
 * vd_is_scores: split k = rows [k n / splits, (k + 1) n / splits) (integer division) of logits[n][classes] (row pitch ld floats);
 *   per row p = softmax in fp64 with the row maximum subtracted; scores[k] = exp(mean_i sum_c p_ic (log p_ic - log pbar_c)), pbar the
 *   split's mean row; 0 log 0 = 0 (a -inf logit, an underflowed probability, a class without mass in the split).  A NaN logit
 *   makes its own split's score NaN and no other.  A workgroup walks a fixed chunk of 64 rows of one split and leaves the chunk's
 *   column sums of p and its sum of p log p in ws; a second kernel adds the chunks in order and finishes each split.
 *   Domain: classes >= 2 (any; no granule), ld >= classes, 1 <= splits <= 65535, splits <= n <= 2^40, logits 4-byte and scores, ws
 *   8-byte aligned, ws of vd_is_ws_bytes(n, classes, splits) bytes (0 = bad shape). */
size_t vd_kid_ws_bytes(int32_t subsets, int32_t mx, int32_t my);
int    vd_kid_sums(const float* x, int64_t nx, int64_t ldx, const float* y, int64_t ny, int64_t ldy, int32_t d, const int32_t* ix,
                   const int32_t* iy, int32_t subsets, int32_t mx, int32_t my, double gamma, double coef0, int32_t degree,
                   double* out /* [subsets][3] */, void* ws, size_t ws_bytes, void* stream);
size_t vd_is_ws_bytes(int64_t n, int32_t classes, int32_t splits);
int    vd_is_scores(const float* logits, int64_t n, int32_t classes, int64_t ld, int32_t splits, double* scores /* [splits] */, void* ws,
                    size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
