"""RePaint (Lugmayr et al. 2022, "RePaint: Inpainting using Denoising Diffusion Probabilistic Models") in this package's continuous
log-SNR terms, and SDEdit-style image-to-image (Meng et al. 2022) on the same chain.  Both condition an existing unconditional or
class-conditional checkpoint on a given image without training.

Every reverse step t -> s computes the unknown region with the ordinary posterior step, draws the known region from q(x_s | x_known)
= alpha_s x_known + sigma_s eps, and merges the two with the mask (1 = keep the known image): one fused launch (vd_inpaint_step in
csrc/diffusion.hip) after the step's one network call.  To harmonise the two regions the chain repeatedly jumps forward -- re-noises by
``jump_length`` grid steps -- and denoises again (``resampling_schedule``).  A jump s -> t of any length is ONE Gaussian draw,
x_t = a x_s + b eps with a = alpha_t/alpha_s and b^2 = sigma_t^2 (1 - e^(logsnr_t - logsnr_s)) (``jump_coefs``; b^2 is the "fixed_large"
variance of ``logsnr_to_posterior``), and one launch (vd_forward_jump).  The same primitive is the stochastic sampling step of distilled
few-step students (Salimans & Ho 2022): step back two, jump forward one.

What runs where: schedule and coefficients are host arithmetic in fp64 on the fp32-rounded log-SNRs, each value rounded once; everything
per element is the two kernels.  The chain ends on the step to index 0, which returns the x0 prediction: there (ak, bk) = (1, 0) and the
known region is the known image itself.  MI355X only: CPU tensors raise.

Random draws, from one ``torch.Generator(device).manual_seed(seed)``, each of the image shape, always drawn (also where its scale is 0,
as ``p_sample`` does), in this fixed order: first the initial state (x_T, or the eps of x_start = alpha known + sigma eps); then per
transition of the schedule, a reverse step draws ``noise`` (the posterior's) and then ``knoise`` (the known region's), a jump draws one.
"""
import numbers

import torch
import torch.nn.functional as F

from . import _hip
from .chain import chain_length, image_batch
from .diffusion import F64, _need_cuda
from .restore import mask_channels, open_chain


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return int(v)


def resampling_schedule(T, jump_length=1, resamplings=1):
    """the grid indices a RePaint chain visits, from ``T`` to 0.  The chain descends by single reverse steps; each time it ARRIVES at a
    resampling point -- an index i in {j, 2j, ...} with i <= T - j -- that has jumps left (``resamplings`` - 1 each) it jumps up by
    j = ``jump_length`` and descends again.  It never jumps from 0 (the chain ends on the x0 prediction, which is no sample at
    logsnr(0)).  ``resamplings=1`` is the plain descent.  With P = len(range(j, T - j + 1, j)) there are T + (r - 1) j P reverse steps
    (network calls) and (r - 1) P jumps; (T, j, r) = (4, 1, 2) gives [4, 3, 4, 3, 2, 3, 2, 1, 2, 1, 0]."""
    T, j, r = _positive_int("T", T), _positive_int("jump_length", jump_length), _positive_int("resamplings", resamplings)
    left = {i: r - 1 for i in range(j, T - j + 1, j)}
    seq, i = [T], T
    while i > 0:
        i -= 1
        seq.append(i)
        if left.get(i, 0) > 0:
            left[i] -= 1
            i += j
            seq.append(i)
    return seq


def _logsnr32(logsnr_fn, times):
    """the fp32-rounded log-SNRs of the given grid times, as fp64 -- ``_step_coefs``'s ls32 / lt32.  ``logsnr_fn`` sees a fresh tensor:
    a rescaling schedule rewrites its argument."""
    return logsnr_fn(torch.tensor(times, dtype=F64)).float().double()


def _grid_index(name, T, i, lo):
    T = _positive_int("T", T)
    if isinstance(i, bool) or not isinstance(i, numbers.Integral) or not lo <= i <= T:
        raise ValueError(f"{name} must be an integer in [{lo}, {T}], got {i!r}")
    return T, int(i)


def known_coefs(logsnr_fn, T, i):
    """``(ak, bk)`` = (alpha, sigma) of grid index i, alpha = sqrt(sigmoid(l_i)), sigma = sqrt(sigmoid(-l_i)): fp64 from the fp32-rounded
    log-SNR of i/T, each rounded to fp32 once.  The known region of a state at index i is ak known + bk eps.  i = 0 gives (1.0, 0.0): the
    step to index 0 returns a prediction, so the known region is the known image itself."""
    T, i = _grid_index("i", T, i, 0)
    if i == 0:
        return 1.0, 0.0
    l = _logsnr32(logsnr_fn, [i / T])[0]
    return float(torch.sigmoid(l).sqrt().float()), float(torch.sigmoid(-l).sqrt().float())


def jump_coefs(logsnr_fn, T, i, j):
    """``(a, b)`` of the forward transition s = i/T -> t = (i + j)/T, x_t = a x_s + b eps: a = alpha_t/alpha_s =
    exp((logsigmoid(l_t) - logsigmoid(l_s))/2) and b = sqrt(sigmoid(-l_t) (-expm1(l_t - l_s))), fp64 from the fp32-rounded log-SNRs, each
    rounded to fp32 once.  b^2 is the "fixed_large" variance of ``logsnr_to_posterior``.  a alpha_s = alpha_t and
    a^2 sigma_s^2 + b^2 = sigma_t^2, so a jump of j equals j unit jumps in distribution and is applied as one."""
    T, i = _grid_index("i", T, i, 0)
    j = _positive_int("j", j)
    if i + j > T:
        raise ValueError(f"the jump {i} -> {i + j} leaves the grid of {T} steps")
    ls, lt = _logsnr32(logsnr_fn, [i / T, (i + j) / T])
    a = torch.exp(0.5 * (F.logsigmoid(lt) - F.logsigmoid(ls)))
    b = torch.sqrt(torch.sigmoid(-lt) * (-torch.expm1(lt - ls)))
    return float(a.float()), float(b.float())


def _check_inputs(gd, known, mask, jump_length, resamplings, start):
    """everything that can be refused before a launch; returns (T of the chain, the mask's channel count)"""
    if gd.model_var_type == "learned":
        raise NotImplementedError("model_var_type='learned'")
    image_batch("known", known)
    mask_c = mask_channels(mask, tuple(known.shape), "known")
    Tc = chain_length(gd, start)
    resampling_schedule(Tc, jump_length, resamplings)              # validates the two counts
    return Tc, mask_c


def p_sample_inpaint(gd, denoise_fn, known, mask, label=None, device=None, seed=None, use_ddim=False, jump_length=1, resamplings=1,
                     start=None, clip_denoised=True):
    """the chain of ``GaussianDiffusion.p_sample_inpaint`` (see there); returns the final image batch on the device"""
    Tc, mask_c = _check_inputs(gd, known, mask, jump_length, resamplings, start)
    _need_cuda(known, "p_sample_inpaint")
    T, fn, clip = gd.sample_timesteps, gd.logsnr_fn, bool(clip_denoised)
    sched = resampling_schedule(Tc, jump_length, resamplings)
    # (the chain's first state: x_T, or the eps of the noised start; its x_in is filled below)
    ctx, draw, known, m, ch = open_chain(gd, denoise_fn, known, mask, mask_c, known.shape, label, device, seed, dup=False)
    with ctx:
        B, C, HW = ch.B, ch.C, ch.HW
        if start is not None:                                                  # SDEdit: x_start = alpha known + sigma eps, everywhere
            _hip.forward_jump(known, ch.x, known_coefs(fn, T, Tc), *ch.dst, B, C * HW)
            ch.advance()
        elif ch.cfg:
            ch.x_in.copy_(ch.x.repeat_interleave(2, dim=0))
        with ch.fixed_weights():
            for cur, nxt in zip(sched, sched[1:]):
                if nxt < cur:                                                  # reverse step cur -> nxt = cur - 1
                    k8, t_net = gd._step_coefs(nxt, use_ddim, clip)
                    noise, knoise = draw(), draw()
                    _hip.inpaint_step(ch.x, ch.net(t_net), noise, known, m, knoise, list(k8) + list(known_coefs(fn, T, nxt)), ch.mot, ch.cfg,
                                      nxt == 0, clip, mask_c, *ch.dst, B, C, HW)
                else:                                                          # jump cur -> nxt = cur + jump_length: one draw
                    _hip.forward_jump(ch.x, draw(), jump_coefs(fn, T, cur, nxt - cur), *ch.dst, B, C * HW)
                ch.advance()
        return ch.x
