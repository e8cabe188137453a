/* vdiff_hip_dps.h -- further entry points of libvdiff_hip.so, same conventions as vdiff_hip.h (which this header extends; the binding
 * v_diffusion/_hip.py reads both, tests/golden/c_abi_dps.json pins this one).
 *
 * Diffusion Posterior Sampling (Chung et al. 2023, Algorithm 1; csrc/diffusion.hip): the two launches of one reverse step, either side
 * of the network's input gradient.  Conventions of the reverse-step section of vdiff_hip.h: images NCHW fp32; k = the 8 host floats of
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
#ifndef VDIFF_HIP_DPS_H
#define VDIFF_HIP_DPS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vd_dps_residual(const float* xt, const float* out, const float* meas, const float* mask, const float* k, int32_t model_out_type,
                    int32_t cfg, int32_t clip, int32_t op, int32_t par, float* dout, float* dxt, float* sumsq, float* x0hat, int32_t n,
                    int32_t C, int32_t H, int32_t W, void* stream);
int vd_dps_step(const float* xt, const float* out, const float* noise, const float* dxin, const float* dxt, const float* sumsq,
                const float* k, float zeta, int32_t model_out_type, int32_t cfg, int32_t last_step, int32_t clip, float* xn, float* xdup,
                int32_t n, int32_t C, int32_t HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif
