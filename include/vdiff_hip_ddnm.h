/* vdiff_hip_ddnm.h -- a further entry point of libvdiff_hip.so, same conventions as vdiff_hip.h (which this header extends; the binding
 * v_diffusion/_hip.py reads it too, tests/golden/c_abi_ddnm.json pins it).
 *
 * Denoising Diffusion Null-space Model (Wang, Yu, Zhang 2023; csrc/diffusion.hip): one reverse step whose x0 prediction takes its
 * range-space part from a measurement meas = A x and keeps the network's null-space part, g_hat = g + lam * A^+(meas - A g) -- ONE launch,
 * no gradient.  Conventions of the reverse-step section of vdiff_hip.h and of vdiff_hip_dps.h: images NCHW fp32; k = the 8 host floats of
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
#ifndef VDIFF_HIP_DDNM_H
#define VDIFF_HIP_DDNM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vd_ddnm_step(const float* xt, const float* out, const float* noise, const float* meas, const float* mask, const float* k, float lam,
                 int32_t model_out_type, int32_t cfg, int32_t last_step, int32_t clip, int32_t op, int32_t par, float* xn, float* xdup,
                 float* sumsq, int32_t n, int32_t C, int32_t H, int32_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
