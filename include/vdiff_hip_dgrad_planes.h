/* vdiff_hip_dgrad_planes.h -- further entry points of libvdiff_hip.so, same conventions as vdiff_hip.h (which this header extends; the
 * binding v_diffusion/_hip.py reads both, tests/golden/c_abi_dgrad_planes.json pins this one).
 *
 * Input gradient of the 3x3 convolution through PLANES (csrc/wino43.hip), the exact adjoint of vd_conv3x3_wino43_fwd_planes: with
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
#ifndef VDIFF_HIP_DGRAD_PLANES_H
#define VDIFF_HIP_DGRAD_PLANES_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif
