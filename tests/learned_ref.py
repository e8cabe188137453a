"""CPU restatement of learned variances (model_var_type "learned") -- TEST INFRASTRUCTURE, in the dtype of its tensor arguments: the
per-element log-variance, the two bound terms, the hybrid loss and the reverse step, composed from oracle/diffusion_ref.py as the
reference's diffusion.py:320-324 intends (tensor intp_frac through the "fixed_medium" posterior of :155).

The network output has Cp + C channels, Cp = C (2C for "both") prediction channels and then C channels nu;
logvar = lvmin + sigmoid(nu) * delta with lvmin the fixed_small log-variance and delta = logsigmoid(-logsnr_t) - logsigmoid(-logsnr_s),
both fp64 from the given log-SNRs and rounded to fp32 once, as every posterior coefficient of the oracle is."""
import math

import torch
import torch.nn.functional as F

from oracle import diffusion_ref as dref

F64 = torch.float64


def split(out, mot):
    """(prediction channels, nu) of a learned-variance output"""
    C = out.shape[1] // (3 if mot == "both" else 2)
    return out[:, :out.shape[1] - C], out[:, out.shape[1] - C:]


def lv_coefs(ls, lt):
    """(c1, c2, lvmin, delta) of the step logsnr_t -> logsnr_s, fp32"""
    c1, c2, lvmin = dref.ddpm_coefs(ls, lt, "fixed_small")
    delta = (F.logsigmoid(-lt.to(F64)) - F.logsigmoid(-ls.to(F64))).float()
    return c1, c2, lvmin, delta


def logvar(nu, ls, lt):
    _, _, lvmin, delta = lv_coefs(ls, lt)
    return lvmin.to(nu.dtype) + torch.sigmoid(nu) * delta.to(nu.dtype)


def terms(out, x0, xt, ls, lt, mot, clip=False, detach_mean=False):
    """(kl, decoder nll) per sample in bits per dimension, the x0 prediction and the per-element log-variance (diffusion.py:446-464)"""
    dt = out.dtype
    o, nu = split(out, mot)
    c1, c2, lvmin, _ = (v.to(dt) for v in lv_coefs(ls, lt))
    lv = logvar(nu, ls, lt)
    px0 = dref.predictions(mot, xt, o, lt.to(dt))[0]
    if clip:
        px0 = px0.clamp(-1.0, 1.0)
    if detach_mean:
        px0 = px0.detach()
    kl = dref._fmean(dref.normal_kl(c1 * xt + c2 * x0, lvmin, c1 * xt + c2 * px0, lv)) / math.log(2.0)
    nll = dref._fmean(-dref.discretized_gaussian_loglik(x0, px0, 0.5 * lv)) / math.log(2.0)
    return kl, nll, px0, lv


def mse_loss(pred_out, x0, eps, xt, lt, mot, rw):
    """the mse branch of train_loss (oracle train_loss) on given x_t and prediction channels"""
    if rw == "snr_1plus":
        return dref._fmean((dref.v_from_x0eps(x0, eps, lt) - pred_out) ** 2)
    if rw == "constant":
        return dref._fmean((x0 - pred_out) ** 2)
    if rw == "snr":
        return dref._fmean((eps - pred_out) ** 2)
    px0, peps, _ = dref.predictions(mot, xt, pred_out, lt)
    return torch.maximum(dref._fmean((x0 - px0) ** 2), dref._fmean((eps - peps) ** 2))


def hybrid_loss(out, x0, eps, xt, ls, lt, use_kl, mot, rw, vlb_weight):
    """mse on the prediction channels + vlb_weight * where(use_kl, kl, nll) with the mean detached in the bound term"""
    dt = out.dtype
    kl, nll, _, _ = terms(out, x0, xt, ls, lt, mot, clip=False, detach_mean=True)
    return mse_loss(split(out, mot)[0], x0, eps, xt, lt.to(dt), mot, rw) + vlb_weight * torch.where(use_kl, kl, nll)


def p_sample_step(denoise_fn, schedule, xt, step, T, y, noise, *, model_out_type="v", w_guide=0.0, use_ddim=False, clip=True,
                  return_pred=False):
    """oracle p_sample_step for a learned-variance network: the variance from the conditional row (diffusion.py:386-387)"""
    B, dt = xt.shape[0], xt.dtype
    s = torch.full((B,), step / T, dtype=F64)
    t = torch.full((B,), (step + 1) / T, dtype=F64)
    ls, lt = dref._bcast(schedule(s).float(), xt), dref._bcast(schedule(t).float(), xt)
    cfg = w_guide > 0 and y is not None
    rep = (lambda a: a.repeat_interleave(2, dim=0)) if cfg else (lambda a: a)
    x_in, t_in, y_in = rep(xt), rep(t), (rep(y).clone() if y is not None else None)
    if cfg:
        y_in[1::2] = 0
    o, nu = split(denoise_fn(x_in, t_in, y_in), model_out_type)
    px0 = dref.predictions(model_out_type, x_in, o, rep(lt))[0]
    if clip:
        px0 = px0.clamp(-1.0, 1.0)
    c1, c2, _ = dref.ddim_coefs(ls, lt) if use_ddim else dref.ddpm_coefs(ls, lt, "fixed_small")
    mean = px0 if step == 0 else rep(c1.to(dt)) * x_in + rep(c2.to(dt)) * px0
    if cfg:
        mean = mean[0::2] + w_guide * (mean[0::2] - mean[1::2])
        px0 = px0[0::2] + w_guide * (px0[0::2] - px0[1::2])
        nu = nu[0::2]
    x = mean
    if step > 0 and not use_ddim:
        x = mean + torch.exp(0.5 * logvar(nu, ls, lt)) * noise
    return (x, px0) if return_pred else x
