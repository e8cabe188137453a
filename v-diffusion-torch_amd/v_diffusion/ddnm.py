"""Denoising Diffusion Null-space Model (Wang, Yu, Zhang 2023, "Zero-Shot Image Restoration Using Denoising Diffusion Null-Space Model")
in this package's continuous log-SNR terms: training-free restoration from a measurement y = A x (+ noise) for the operators whose
pseudo-inverse is a closed form -- the three of ``p_sample_dps``: a mask, box down-sampling, the channel mean.  Every reverse step
x_t -> x_s replaces the range-space part of the step's x0 prediction g by the measurement's and keeps the network's null-space part,

    g_hat = g + lam * A^+ (y - A g) ,

and continues with the ordinary posterior step on g_hat.  Against DPS: one ordinary network forward per step -- no tape, no input
gradient, no step size to tune -- and with a noiseless measurement and lam = 1 the result satisfies A x = y to rounding.

What runs where: coefficients are ``gd._step_coefs``'s host fp64 arithmetic and ``ddnm_rule``'s; per step there is one network call and
ONE launch (vd_ddnm_step in csrc/diffusion.hip: vd_sample_step's arithmetic and the correction c2 * lam * A^+ r on every preimage, lam *
A^+ r on the last step, which returns the prediction).  The paper's "time travel" is ``resampling_schedule``'s: at every resampling point
the chain jumps forward by ``jump_length`` grid steps -- one draw, one launch (vd_forward_jump) -- and denoises again.  MI355X only: CPU
tensors raise.

Noisy measurements (DDNM+), y = A x + n with n ~ N(0, sigma_y^2), under the paper's simplification that A^+ n has variance sigma_y^2 per
element: the correction carries c2 * lam * sigma_y of noise into x_s, so lam shrinks where that exceeds the step's own noise and the
step's noise scale gives up what the correction brought (``ddnm_rule``); the last step, which adds no noise, takes lam = 0.

Random draws, from one ``torch.Generator(device).manual_seed(seed)``, each of the image shape, always drawn: the initial state x_T, then
one per transition of the schedule -- a reverse step's noise, or a jump's.  Without jumps that is ``p_sample``'s order.
"""
import math
import numbers

import torch

from . import _hip
from .chain import refuse_variants
from .diffusion import _need_cuda
from .inpaint import jump_coefs, resampling_schedule
from .restore import NO_PINV, ddnm_pinv, open_chain, parse_operator, per_index      # noqa: F401  (ddnm_pinv: v_diffusion.ddnm.ddnm_pinv)


def ddnm_rule(c2, noise_scale, sigma_y, last, lam=None):
    """``(lam, noise_scale')`` of one reverse step with posterior-mean weight ``c2`` on the x0 prediction and noise scale
    ``noise_scale``, for a measurement noise ``sigma_y``; python floats, fp64.  The correction lam * A^+(y - A g) enters x_s times c2 and
    brings c2 * lam * sigma_y of measurement noise with it.  lam = 1 where the step's own noise covers that (noise_scale >= c2 * sigma_y),
    else noise_scale / (c2 * sigma_y), so that it exactly does; noise_scale' = sqrt(max(0, noise_scale^2 - (c2 * lam * sigma_y)^2)) is
    what the step still has to add.  The last step returns the prediction and adds no noise: lam = 1 for a noiseless measurement, else 0.
    An explicit ``lam`` replaces the rule's; noise_scale' is formed from it all the same."""
    c2, ns, sy = float(c2), float(noise_scale), float(sigma_y)
    if lam is None:
        if last:
            lam = 1.0 if sy == 0.0 else 0.0
        else:
            lam = 1.0 if ns >= c2 * sy else ns / (c2 * sy)
    lam = float(lam)
    carried = c2 * lam * sy
    if carried == 0.0:
        return lam, ns                                             # (the scale itself, not sqrt(ns^2))
    return lam, math.sqrt(max(0.0, ns * ns - carried * carried))


def _check_inputs(gd, measurement, operator, shape, sigma_y, lam, use_ddim, jump_length, resamplings):
    """everything that can be refused before a launch; returns (kind, par, mask, sigma_y, the lams or None, the schedule)"""
    refuse_variants(gd, "p_sample_ddnm")
    kind, par, mask, _ = parse_operator(operator, tuple(shape), measurement, "measurement")
    if kind == "blur":
        raise NotImplementedError(f"p_sample_ddnm: {NO_PINV}")
    if isinstance(sigma_y, bool) or not isinstance(sigma_y, numbers.Real) or not (math.isfinite(sigma_y) and sigma_y >= 0.0):
        raise ValueError(f"sigma_y must be finite and >= 0, got {sigma_y!r}")
    if sigma_y > 0.0 and use_ddim:
        raise ValueError("sigma_y > 0 with use_ddim=True: a DDIM step adds no noise that could absorb the measurement's")
    ls = per_index("lam", lam, gd.sample_timesteps, lambda v: 0.0 <= v <= 1.0, "lie in [0, 1]", allow_none=True)    # (a NaN: outside)
    sched = resampling_schedule(gd.sample_timesteps, jump_length, resamplings)      # validates the two counts
    _need_cuda(measurement, "p_sample_ddnm")
    return kind, par, mask, float(sigma_y), ls, sched


def p_sample_ddnm(gd, denoise_fn, measurement, operator, shape, label=None, device=None, seed=None, sigma_y=0.0, lam=None, use_ddim=False,
                  jump_length=1, resamplings=1, clip_denoised=True, return_residuals=False):
    """the chain of ``GaussianDiffusion.p_sample_ddnm`` (see there); returns the final image batch on the device, and with
    ``return_residuals`` the (reverse steps, B) norms ||y - A g|| too"""
    kind, par, mask, sigma_y, ls, sched = _check_inputs(gd, measurement, operator, shape, sigma_y, lam, use_ddim, jump_length, resamplings)
    T, fn, clip, op = gd.sample_timesteps, gd.logsnr_fn, bool(clip_denoised), _hip.DPS_OPS[kind]
    ctx, draw, meas, m, ch = open_chain(gd, denoise_fn, measurement, mask, par, shape, label, device, seed)
    (B, C, Hh, Ww), device = ch.x.shape, ch.device
    with ctx, torch.no_grad():
        res = torch.zeros((sum(b < a for a, b in zip(sched, sched[1:])), B), dtype=torch.float32, device=device) if return_residuals else None
        n = 0
        with ch.fixed_weights():
            for cur, nxt in zip(sched, sched[1:]):
                noise = draw()
                if nxt < cur:                                                  # reverse step cur -> nxt = cur - 1
                    k8, t_net = gd._step_coefs(nxt, use_ddim, clip)
                    k8 = list(k8)
                    lm, k8[5] = ddnm_rule(k8[4], k8[5], sigma_y, nxt == 0, None if ls is None else ls[nxt])
                    _hip.ddnm_step(ch.x, ch.net(t_net), noise, meas, m, k8, lm, ch.mot, ch.cfg, nxt == 0, clip, op, par, *ch.dst,
                                   None if res is None else res[n], B, C, Hh, Ww)
                    n += 1
                else:                                                          # jump cur -> nxt = cur + jump_length
                    _hip.forward_jump(ch.x, noise, jump_coefs(fn, T, cur, nxt - cur), *ch.dst, B, C * ch.HW)
                ch.advance()
        return (ch.x, res.sqrt_()) if return_residuals else ch.x
