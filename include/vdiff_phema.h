/* vdiff_phema.h -- the post-hoc EMA entry points of libvdiff_hip.so (csrc/optim.hip): the optimizer tail with power-function EMA shadows and
 * the fp64-accumulated combination of snapshots.  Same conventions as vdiff_hip.h (plain pointers and sizes, fp32 unless stated, the library
 * never allocates, every launch goes to `stream`, 0 on success and vd_last_error() otherwise) and the same type rule: v_diffusion/_hip.py
 * binds these declarations exactly as it binds that header's.  They stand in a header of their own so that the table vdiff_hip.h declares,
 * which tests/golden/c_abi.json records entry by entry, stays as recorded; this header's table is recorded in tests/golden/c_abi_phema.json. */
#ifndef VDIFF_PHEMA_H
#define VDIFF_PHEMA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* post-hoc EMA (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3.5): the same one-pass
 * update with n_pema (1..4) POWER-FUNCTION shadows behind the classic one.  p, m, v and ema (which may be NULL) receive vd_adamw_ema's
 * arithmetic bit for bit -- r_flag non-NULL: vd_adamw_ema_flagged's, r_steps advanced as there and r_mode, r_bc1, r_bc2 ignored; r_flag
 * NULL: r_mode 0 / 1 / 2 as in vd_adamw_ema and r_steps, r_beta1, r_beta2 ignored.  Then for every power shadow k
 *   pema[k][i] += r_k (p_new[i] - pema[k][i]),   r_k = (float) pema_rate[k],
 * pema_rate[k] the DOUBLE 1 - beta_t = 1 - (1 - 1/t)^(gamma_k + 1) of the shadow's t-th update, formed on the host (phema.power_ema_rate:
 * -expm1((gamma + 1) log1p(-1/t)); rounded to fp32 once, here).  A rate of exactly 1 (t = 1) SELECTS p_new: the shadow is not read, so
 * whatever it held -- a NaN too -- is gone after its first update.  In an r_mode 1 range the shadows still follow p, as ema does.
 * pema and pema_rate are HOST arrays (of device pointers / of doubles) and travel in the kernel arguments.  One dword per lane per
 * operand, every operand streamed once: 36 + 8 n_pema bytes per parameter with the classic shadow.
 * Refused before any launch: n_pema outside 1..4, a NULL shadow, a rate outside (0, 1], a shadow that overlaps p, g, m, v, ema or
 * another shadow, a bad range or bias correction as vd_adamw_ema and vd_adamw_ema_flagged (vdiff_hip.h) refuse them.  The rate compared with 1 is
 * the ROUNDED one: a double within 2^-25 of 1 selects too. */
int vd_adamw_emas(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* gnorm_sq, float max_norm,
                  float lr, double beta1, double beta2, float eps, float wd, float bc1, float bc2, double ema_decay,
                  int64_t r_lo, int64_t r_hi, int32_t r_mode, float r_bc1, float r_bc2,
                  const float* r_flag, int32_t* r_steps, double r_beta1, double r_beta2,
                  float* const* pema, const double* pema_rate, int32_t n_pema, void* stream);
/* the combination of snapshots a post-hoc EMA profile is rebuilt with: per element s = acc[i] (0 without acc), then
 * s = fma(w[j], (double) src[j][i], s) for j = 0 .. k - 1 in that order, in fp64; acc[i] = s when acc is given, out[i] = (float) s when
 * out is given (at least one of them).  src (k device pointers to n floats) and w (k doubles) are HOST arrays, 1 <= k <= 32; a weight
 * of exactly 0 skips its source unread (its pointer may be NULL; a NaN there reaches nothing).  Fixed order, no atomics, no workspace:
 * the same call gives the same bits, and k sources in one call or split over calls chained through acc give the same out bit for bit.
 * 16-byte accesses when out, acc and every source read are 16-byte aligned (n & 3 tail elements apart), one element per lane
 * otherwise: the same bits.  No source read may overlap out or acc. */
int vd_ema_combine(float* out, double* acc, const float* const* src, const double* w, int32_t k, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
