/* vdiff_blur.h -- the blur operator of Diffusion Posterior Sampling in libvdiff_hip.so (csrc/diffusion.hip): the residual launch of a DPS step
 * when the measurement is a blurred image, and the operator and its adjoint on their own.  Same conventions as vdiff_hip.h (plain pointers
 * and sizes, fp32, the library never allocates, every launch goes to `stream`, 0 on success and vd_last_error() otherwise) and the same type
 * rule: v_diffusion/_hip.py binds these declarations exactly as it binds that header's, under the prefix vdx_.  They stand in a header of
 * their own, under a prefix of their own, so that the tables vdiff_hip.h and vdiff_phema.h declare, which tests/golden/c_abi.json and
 * tests/golden/c_abi_phema.json record entry by entry and which together close over the library's vd_* symbols, stay as recorded; this
 * header's table is recorded in tests/golden/c_abi_blur.json and closes over the library's vdx_* symbols. */
#ifndef VDIFF_BLUR_H
#define VDIFF_BLUR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most taps per side of a kernel, and the most elements H*W of a plane (a channel of one sample): the launches stage whole planes in
 * LDS -- two fp32 planes of the bound and the taps as doubles, 41 KB of static LDS whatever the shape.  64 x 64 is at the bound. */
#define VDX_BLUR_KMAX 33
#define VDX_BLUR_PLANE_MAX 4096

/* The operator.  taps[kh][kw] (device, fp32) is ONE kernel for every sample and channel (depthwise), kh and kw odd, Rh = (kh-1)/2 <= H-1,
 * Rw = (kw-1)/2 <= W-1, not necessarily symmetric.  A is the cross-correlation (torch's conv2d) with the REFLECT boundary that does not
 * repeat the edge (F.pad(mode="reflect")): rho_n(p) = -p for p < 0, 2(n-1) - p for p > n-1, p otherwise, and per plane g[H][W]
 *   (A g)[y][x]   = sum_{i<kh} sum_{j<kw} taps[i][j] * g[rho_H(y+i-Rh)][rho_W(x+j-Rw)]                       i, then j, ascending
 *   (A^T r)[y][x] = sum_{p in pre_H(y)} sum_i sum_{q in pre_W(x)} sum_j taps[i][j] * r[p-i+Rh][q-j+Rw]        terms outside the plane absent
 * with pre_n(y) = (y; -y if 1 <= y <= R; 2(n-1)-y if n-1-R <= y <= n-2), the positions of the padded axis that reflect onto y, in that
 * order, i and j ascending.  Each sum is an fp64 fma chain in exactly that order, rounded to fp32 once: the same call gives the same bits.
 * The measurement A g has the image's shape.
 *
 * vdx_dps_residual_blur: vd_dps_residual (vdiff_hip.h) for this operator -- the same arguments with (taps, kh, kw) in the place of
 *   (mask, op, par), the same conventions (images NCHW; k = the 8 host floats of vd_sample_step; out = n*(1+cfg) rows, cond and uncond
 *   interleaved, of C channels, 2C for model_out_type 3), the same device helpers for the prediction, the clip, the guided g, the pass
 *   masks and the cotangent factors.  Reads xt, out, meas[n][C][H][W], taps, k.  Writes, every element once:
 *     sumsq[b]                 sum r^2 over sample b, r = meas - A g: fp64, in a fixed order (one workgroup per sample, no atomics, no
 *                              workspace), stored as fp32
 *     dout (the shape of out)  with u = -A^T r: cond rows (1 + w) m_c u, uncond rows -w m_u u (without cfg: m u), times b0x on the first C
 *                              channels and b0e on the second C of "both"
 *     dxt[n][C][H][W]          a0 [(1 + w) m_c - w m_u] u   (a0 m u without cfg)
 *     x0hat (optional)         g
 *   vd_dps_step takes them as it takes vd_dps_residual's.  No output may overlap an input or another output.
 * vdx_blur_planes: y = A x (adjoint 0) or A^T x (adjoint 1) of `planes` planes x[planes][H][W], one workgroup per plane, by the device
 *   functions the launch above uses.  y may be x itself (a plane is read whole before it is written), not overlap it otherwise.
 * Both return 1 before any launch -- nothing is dereferenced, no output is written -- on a null required pointer (all but x0hat), kh or kw
 * even or outside 1..VDX_BLUR_KMAX, a radius beyond H-1 or W-1, n, C, H, W or planes < 1, H*W > VDX_BLUR_PLANE_MAX, a model_out_type
 * outside 0..3, an adjoint that is neither 0 nor 1. */
int vdx_dps_residual_blur(const float* xt, const float* out, const float* meas, const float* taps, const float* k, int32_t model_out_type,
                          int32_t cfg, int32_t clip, int32_t kh, int32_t kw, float* dout, float* dxt, float* sumsq, float* x0hat, int32_t n,
                          int32_t C, int32_t H, int32_t W, void* stream);
int vdx_blur_planes(const float* x, const float* taps, int32_t kh, int32_t kw, int32_t adjoint, float* y, int32_t planes, int32_t H,
                    int32_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
