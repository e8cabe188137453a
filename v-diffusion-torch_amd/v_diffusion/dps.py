"""Diffusion Posterior Sampling (Chung et al. 2023, "Diffusion Posterior Sampling for General Noisy Inverse Problems", Algorithm 1) in
this package's continuous log-SNR terms: training-free restoration from a measurement y = A x (+ noise) with an existing unconditional
or class-conditional checkpoint.  Where RePaint (``p_sample_inpaint``) replaces the known pixels, DPS follows every ordinary reverse step
x_t -> x_s by a gradient step on the measurement residual of the step's x0 prediction,

    x_s <- x_s - zeta_s * grad_{x_t} || y - A x0_hat(x_t) ||_2 ,

so it covers noisy measurements and any linear A with an adjoint: here a soft mask (inpainting), box down-sampling (super-resolution),
the channel mean (colourisation) and a blur -- one kernel of up to 33 x 33 taps for every channel, reflect boundary (Gaussian and motion
deblurring; ``gaussian_kernel``, and ``blur`` for A and A^T on their own).  The gradient goes through the network: its input gradient with the weights held fixed
(``UNet.forward_vjp``, the engine's input-only backward pass -- none of the weight-gradient work).

What runs where: coefficients are ``gd._step_coefs``'s host fp64 arithmetic; per step there is one network call with tape, one launch
that forms the residual r = y - A g of the guided (clipped) prediction g, its squared norm per sample and the cotangents of (1/2)||r||^2
(vd_dps_residual in csrc/diffusion.hip; vdx_dps_residual_blur for a blur, whose preimages overlap: planes staged in LDS), the network's VJP of that cotangent, and one launch that is vd_sample_step's arithmetic followed
by the correction -zeta/||r|| (dxt + the VJP rows) (vd_dps_step).  The last step, which returns the x0 prediction, is corrected too, as in
the paper.  A step whose zeta is 0 needs no gradient: its network call keeps no tape and the launch is vd_sample_step's row, so with
``zeta=0`` the chain is ``p_sample`` bit for bit.  MI355X only: CPU tensors raise.

Random draws, from one ``torch.Generator(device).manual_seed(seed)``, each of the image shape, always drawn: the initial state x_T, then
one per step -- ``p_sample``'s order.
"""
import math

import torch

from . import _hip
from .chain import F64, refuse_variants
from .diffusion import _need_cuda
from .restore import blur_kernel, dps_measure, gaussian_kernel, open_chain, parse_operator, per_index      # noqa: F401  (dps_measure, gaussian_kernel: v_diffusion.dps.*)


def blur(x, kernel, adjoint=False):
    """A x -- or A^T x with ``adjoint`` -- of an image batch ``x`` (B, C, H, W) fp32 on the GPU under the operator ``("blur", kernel)``:
    one launch, one workgroup per plane (vdx_blur_planes), by the device functions of the DPS residual launch.  fp64 accumulation in a
    fixed order, rounded once.  H * W is at most ``_hip.BLUR_PLANE_MAX``.  Returns a new tensor; CPU tensors raise."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"x must be a (B, C, H, W) tensor, got shape {tuple(getattr(x, 'shape', ()))}")
    _need_cuda(x, "blur")
    B, C, H, W = (int(v) for v in x.shape)
    blur_kernel(kernel, H, W)
    if x.dtype != torch.float32:
        raise ValueError(f"x must be float32, got {x.dtype}")
    if B * C == 0:
        return torch.empty_like(x)
    with torch.cuda.device(x.device), torch.no_grad():
        xc = x.detach().contiguous()
        y = torch.empty_like(xc)
        taps = kernel.detach().to(device=x.device, dtype=torch.float32).contiguous()
        _hip.blur_planes(xc, taps, adjoint, y, B * C, H, W)
    return y


def _check_inputs(gd, measurement, operator, shape, zeta):
    """everything that can be refused before a launch; returns (kind, par, mask, the step sizes)"""
    refuse_variants(gd, "p_sample_dps")
    kind, par, mask, _ = parse_operator(operator, tuple(shape), measurement, "measurement")
    if kind == "blur" and int(shape[2]) * int(shape[3]) > _hip.BLUR_PLANE_MAX:
        raise ValueError(f"the 'blur' operator takes planes of at most {_hip.BLUR_PLANE_MAX} pixels (the launch stages them in LDS), got "
                         f"{int(shape[2])} x {int(shape[3])}")
    zs = per_index("zeta", zeta, gd.sample_timesteps, lambda z: math.isfinite(z) and z >= 0.0, "be finite and >= 0")
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
    clip, op = bool(clip_denoised), _hip.DPS_OPS.get(kind)                  # (a blur has no op: a launch of its own)
    ctx, draw, meas, m, ch = open_chain(gd, denoise_fn, measurement, mask, par, shape, label, device, seed)
    shape, device = tuple(ch.x.shape), ch.device
    B, C, Hh, Ww = shape
    with ctx, torch.no_grad():
        co = C * (2 if gd.model_out_type == "both" else 1)
        dout = torch.empty((ch.rows, co, Hh, Ww), dtype=torch.float32, device=device)
        dxt = torch.empty(shape, dtype=torch.float32, device=device)
        sumsq = torch.zeros((B,), dtype=torch.float32, device=device)
        taps = operator[1].detach().to(device=device, dtype=torch.float32).contiguous() if kind == "blur" else None      # once
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
                    if taps is None:
                        _hip.dps_residual(ch.x, out, meas, m, k8, ch.mot, ch.cfg, clip, op, par, dout, dxt, sumsq, None, B, C, Hh, Ww)
                    else:
                        _hip.dps_residual_blur(ch.x, out, meas, taps, k8, ch.mot, ch.cfg, clip, dout, dxt, sumsq, None, B, C, Hh, Ww)
                    dxin = vjp(dout)
                _hip.dps_step(ch.x, out, noise, dxin, dxt, sumsq, k8, zs[nxt], ch.mot, ch.cfg, nxt == 0, clip, *ch.dst, B, C, ch.HW)
                ch.advance()
        return ch.x
