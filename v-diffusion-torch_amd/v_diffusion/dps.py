"""Diffusion Posterior Sampling (Chung et al. 2023, "Diffusion Posterior Sampling for General Noisy Inverse Problems", Algorithm 1) in
this package's continuous log-SNR terms: training-free restoration from a measurement y = A x (+ noise) with an existing unconditional
or class-conditional checkpoint.  Where RePaint (``p_sample_inpaint``) replaces the known pixels, DPS follows every ordinary reverse step
x_t -> x_s by a gradient step on the measurement residual of the step's x0 prediction,

    x_s <- x_s - zeta_s * grad_{x_t} || y - A x0_hat(x_t) ||_2 ,

so it covers noisy measurements and any linear A with an adjoint: here a soft mask (inpainting), box down-sampling (super-resolution)
and the channel mean (colourisation).  The gradient goes through the network: its input gradient with the weights held fixed
(``UNet.forward_vjp``, the engine's input-only backward pass -- none of the weight-gradient work).

What runs where: coefficients are ``gd._step_coefs``'s host fp64 arithmetic; per step there is one network call with tape, one launch
that forms the residual r = y - A g of the guided (clipped) prediction g, its squared norm per sample and the cotangents of (1/2)||r||^2
(vd_dps_residual in csrc/diffusion.hip), the network's VJP of that cotangent, and one launch that is vd_sample_step's arithmetic followed
by the correction -zeta/||r|| (dxt + the VJP rows) (vd_dps_step).  The last step, which returns the x0 prediction, is corrected too, as in
the paper.  A step whose zeta is 0 needs no gradient: its network call keeps no tape and the launch is vd_sample_step's row, so with
``zeta=0`` the chain is ``p_sample`` bit for bit.  MI355X only: CPU tensors raise.

Random draws, from one ``torch.Generator(device).manual_seed(seed)``, each of the image shape, always drawn: the initial state x_T, then
one per step -- ``p_sample``'s order.
"""
import math
import numbers

import torch
import torch.nn.functional as F

from . import _hip
from .chain import Chain, F64, refuse_variants
from .diffusion import _device_ctx, _need_cuda

OPERATORS = ("mask", "down", "gray")
DOWN_FACTORS = (2, 4, 8)


def _operator(operator, shape):
    """``(kind, par, mask or None, the shape of A's image)`` of an operator on images of ``shape`` = (B, C, H, W); everything about it
    that can be refused without a device.  par: the mask's channel count / the down-sampling factor / 0."""
    if not isinstance(operator, (tuple, list)) or not operator or operator[0] not in OPERATORS:
        raise ValueError(f"operator must be ('mask', mask), ('down', f) or ('gray',), got {operator!r}")
    if len(shape) != 4 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 for v in shape):
        raise ValueError(f"shape must be (B, C, H, W) of positive integers, got {tuple(shape)!r}")
    B, C, H, W = (int(v) for v in shape)
    kind = operator[0]
    if len(operator) != (1 if kind == "gray" else 2):
        raise ValueError(f"operator {kind!r} takes {'no argument' if kind == 'gray' else 'one argument'}, got {len(operator) - 1}")
    if kind == "gray":
        return kind, 0, None, (B, 1, H, W)
    if kind == "down":
        f = operator[1]
        if isinstance(f, bool) or not isinstance(f, numbers.Integral) or f not in DOWN_FACTORS:
            raise ValueError(f"the down-sampling factor must be one of {DOWN_FACTORS}, got {f!r}")
        if H % f or W % f:
            raise ValueError(f"the down-sampling factor {f} must divide H = {H} and W = {W}")
        return kind, int(f), None, (B, C, H // f, W // f)
    mask = operator[1]                                                 # p_sample_inpaint's rules
    if not torch.is_tensor(mask) or mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, C) \
            or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f"mask must have shape (B or 1, 1 or C, H, W) for images of shape {(B, C, H, W)}, got "
                         f"{tuple(getattr(mask, 'shape', ()))}")
    if mask.dtype != torch.bool:
        if not mask.dtype.is_floating_point:
            raise ValueError(f"mask must be float or bool, got {mask.dtype}")
        lo, hi = float(mask.min()), float(mask.max())
        if not (lo >= 0.0 and hi <= 1.0):                              # (a NaN fails both)
            raise ValueError(f"mask values must lie in [0, 1], got [{lo}, {hi}]")
    return kind, int(mask.shape[1]), mask, (B, C, H, W)


def dps_measure(x, operator):
    """A x of an image batch ``x`` (B, C, H, W) with plain torch operations on ``x``'s device: M (.) x for ``("mask", mask)``, the mean
    over f x f blocks for ``("down", f)``, the channel mean (B, 1, H, W) for ``("gray",)``.  Not hot path: it makes the measurement a
    caller hands to ``p_sample_dps`` (adding the measurement noise is the caller's)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"x must be a (B, C, H, W) tensor, got shape {tuple(getattr(x, 'shape', ()))}")
    kind, par, mask, _ = _operator(operator, tuple(x.shape))
    if kind == "mask":
        return mask.to(device=x.device, dtype=x.dtype) * x
    if kind == "down":
        return F.avg_pool2d(x, par)
    return x.mean(dim=1, keepdim=True)


def _zetas(zeta, T):
    """the step size of every destination grid index 0 ... T-1 as python floats"""
    if isinstance(zeta, numbers.Real) and not isinstance(zeta, bool):
        zs = [float(zeta)] * T
    else:
        if torch.is_tensor(zeta):
            zeta = zeta.detach().reshape(-1).tolist() if zeta.dim() <= 1 else None
        if not isinstance(zeta, (list, tuple)) or len(zeta) != T or \
                any(isinstance(z, bool) or not isinstance(z, numbers.Real) for z in zeta):
            raise ValueError(f"zeta must be a float or {T} floats (one per destination grid index), got "
                             f"{len(zeta) if isinstance(zeta, (list, tuple)) else zeta!r}")
        zs = [float(z) for z in zeta]
    bad = [z for z in zs if not (math.isfinite(z) and z >= 0.0)]
    if bad:
        raise ValueError(f"zeta must be finite and >= 0, got {bad[0]!r}")
    return zs


def _check_inputs(gd, measurement, operator, shape, zeta):
    """everything that can be refused before a launch; returns (kind, par, mask, the step sizes)"""
    refuse_variants(gd, "p_sample_dps")
    kind, par, mask, mshape = _operator(operator, tuple(shape))
    if not torch.is_tensor(measurement) or tuple(measurement.shape) != mshape:
        raise ValueError(f"measurement must have shape {mshape}, the image of shape {tuple(shape)} under {kind!r}, got "
                         f"{tuple(getattr(measurement, 'shape', ()))}")
    zs = _zetas(zeta, gd.sample_timesteps)
    _need_cuda(measurement, "p_sample_dps")
    return kind, par, mask, zs


def _net_vjp(denoise_fn, x_in, t, y_in):
    """``(out, vjp)`` of the network at ``x_in``: out fp32 contiguous, vjp(dout) = the input gradient with the weights held fixed.  A
    ``v_diffusion.UNet`` (also behind a wrapper's ``.module``) gives it without autograd (``forward_vjp``); any other callable goes
    through ``torch.autograd.grad`` on a detached copy of the input that requires a gradient."""
    from .models.unet import UNet
    net = getattr(denoise_fn, "module", denoise_fn)
    if isinstance(net, UNet):
        out, vjp = net.forward_vjp(x_in, t, y_in)
        return out.to(torch.float32).contiguous(), vjp
    with torch.enable_grad():
        xg = x_in.detach().clone().requires_grad_(True)
        raw = denoise_fn(xg, t, y_in)
    if not raw.requires_grad:
        raise RuntimeError("p_sample_dps: the network's output does not depend on its input through autograd (no input gradient to take)")

    def vjp(dout):
        return torch.autograd.grad(raw, xg, dout.to(raw.dtype).reshape(raw.shape))[0].to(torch.float32).contiguous()
    return raw.detach().to(torch.float32).contiguous(), vjp


def p_sample_dps(gd, denoise_fn, measurement, operator, shape, label=None, device=None, seed=None, zeta=1.0, use_ddim=False,
                 clip_denoised=True):
    """the chain of ``GaussianDiffusion.p_sample_dps`` (see there); returns the final image batch on the device"""
    kind, par, mask, zs = _check_inputs(gd, measurement, operator, shape, zeta)
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    ctx = _device_ctx(device)
    clip, op = bool(clip_denoised), _hip.DPS_OPS[kind]
    shape = tuple(int(v) for v in shape)
    B, C, Hh, Ww = shape
    with ctx, torch.no_grad():
        generator = None if seed is None else torch.Generator(device).manual_seed(seed)
        draw = lambda: torch.randn(shape, device=device, generator=generator)
        meas = measurement.to(device=device, dtype=torch.float32).contiguous()
        m = None if mask is None else mask.to(device=device, dtype=torch.float32).expand(B, par, Hh, Ww).contiguous()
        ch = Chain(gd, denoise_fn, draw(), label, device)
        co = C * (2 if gd.model_out_type == "both" else 1)
        dout = torch.empty((ch.rows, co, Hh, Ww), dtype=torch.float32, device=device)
        dxt = torch.empty(shape, dtype=torch.float32, device=device)
        sumsq = torch.zeros((B,), dtype=torch.float32, device=device)
        with ch.fixed_weights():
            for nxt in reversed(range(gd.sample_timesteps)):
                k8, t_net = gd._step_coefs(nxt, use_ddim, clip)
                noise = draw()
                if zs[nxt] == 0.0:
                    # no gradient to take: the network keeps no tape and the launch forms vd_sample_step's row (dxin / dxt are not read)
                    out, dxin = ch.net(t_net), dxt
                else:
                    t = torch.full((ch.rows,), t_net, dtype=F64, device=device)
                    out, vjp = _net_vjp(denoise_fn, ch.net_in, t, ch.y_in)
                    if tuple(out.shape) != tuple(dout.shape):
                        raise ValueError(f"the network returned shape {tuple(out.shape)}, expected {tuple(dout.shape)}")
                    _hip.dps_residual(ch.x, out, meas, m, k8, ch.mot, ch.cfg, clip, op, par, dout, dxt, sumsq, None, B, C, Hh, Ww)
                    dxin = vjp(dout)
                _hip.dps_step(ch.x, out, noise, dxin, dxt, sumsq, k8, zs[nxt], ch.mot, ch.cfg, nxt == 0, clip, *ch.dst, B, C, ch.HW)
                ch.advance()
        return ch.x
