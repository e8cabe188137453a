"""The way back: from a given image to the noise that produces it.  Three things, none of which needs training.

DDPM noise-space inversion (Huberman-Spiegelglas et al. 2024, "An Edit Friendly DDPM Noise Space") in this package's log-SNR terms.
For a chain of Tc steps, draw INDEPENDENT eps_i and set x_i = alpha_i x_0 + sigma_i eps_i for i = Tc ... 1 ((alpha_i, sigma_i) =
``known_coefs``); these x_i are no sample of the forward process -- neighbours are uncorrelated -- and that is the point: the noise map
the ordinary reverse step would need to go from x_{i+1} to x_i,

    z_i = (x_i - mu_i(x_{i+1})) / noise_scale_i,        mu_i the guided posterior mean of ``vd_sample_step``,

carries the image's structure at every scale.  The step to index 0 has no noise; its map is the residual z_0 = x_0 - x0_hat(x_1), with
scale 1.  Replaying the maps through the ordinary reverse chain returns x_0 for ANY network (``p_sample_replay``); replaying them with
another label or guidance weight is the edit.  Per step: one network call and one fused launch (vd_noise_extract in
csrc/diffusion.hip) that forms the next state, the map, and the duplicated rows of the next guided input.  Replay is the existing
vd_sample_step with ``noise = maps[i]``; on the last step its noise-scale slot carries 1.0, so the residual goes through the same launch.

DDIM / DPM-Solver++ encoding: the probability-flow ODE run upwards, tau_i -> tau_{i+1}, with the solver's own update
x_n = c1 x + c2 g + c2rho (g - g_prev) on the ascending rows of ``encode_coefs``: c1 = sigma_n/sigma_t, c2 = alpha_n (1 - e^-h),
h = (l_n - l_t)/2 < 0, rho = h/(2 h_prev).  vd_solver_step runs them as it is.  ``p_sample_solver(noise=latent)`` decodes.

``slerp``: interpolation of two latents on the sphere (DDIM paper, section 5.3), one launch of vd_slerp_rows.

What runs where: tables and coefficients are fp64 host arithmetic on the fp32-rounded log-SNRs, each value rounded once; everything per
element is the kernels.  MI355X only: CPU tensors raise.  A captured-graph path is not built for any of the three chains.
"""
import numbers

import torch
import torch.nn.functional as F

from . import _hip
from .chain import Chain, chain_length, image_batch, refuse_variants
from .diffusion import F64, _device_ctx, _need_cuda, _pred_coefs
from .inpaint import known_coefs
from .solver import C2RHO, _check, _grid


# ------------------------------------------------------------------------------------------------ DDIM / DPM-Solver++ encoding
def encode_coefs(logsnr_fn, steps, order=1, spacing="time", model_out_type="v", w_guide=0.):
    """``(table, t_net)``: the (steps, 8) fp32 table of vd_solver_step for the ASCENDING steps, row i = tau_i -> tau_{i+1} with
    ``solver_coefs``'s columns {a0, b0x, b0e, c1, c2, c2 rho, w_guide, 0}, and the (steps,) fp64 times the network is called with, tau_i as
    ``logsnr_fn`` left it (the state the step starts from).  Pure torch on the CPU; grid and spacing are ``solver_coefs``'s.

    Built like ``solver_coefs``: per row ``logsnr_fn`` sees the pair (tau_i, tau_{i+1}), the log-SNRs l_t (at tau_i) and l_n (at tau_{i+1})
    are rounded to fp32, a0, b0x, b0e come from ``_pred_coefs`` at l_t, and in fp64 from those fp32 values, each slot rounded once,
    c1 = sigma_n/sigma_t = exp((logsigmoid(-l_n) - logsigmoid(-l_t))/2), c2 = alpha_n (1 - e^-h) = -alpha_n expm1(-h) with
    h = (l_n - l_t)/2 < 0 (so c2 < 0), and c2 rho with rho = h/(2 h_prev).  rho = 0 on row 0 (no previous prediction) and on every row of
    order 1.  Row i undoes the DDIM row of the same interval exactly in exact arithmetic: c1_up c1_down = 1 and c2_down + c1_down c2_up = 0."""
    steps = int(steps)
    _check(steps, order)
    tau = _grid(logsnr_fn, steps, spacing)
    rows, times, h_prev = [], [], None
    for i in range(steps):
        st = torch.tensor([tau[i], tau[i + 1]], dtype=F64)
        l = logsnr_fn(st)                                          # may rewrite st in place
        times.append(float(st[0]))
        lt32, ln32 = l[0:1].float(), l[1:2].float()
        a0, b0x, b0e = _pred_coefs(model_out_type, lt32[0])
        lt, ln = lt32.double(), ln32.double()
        h = 0.5 * float(ln - lt)
        c1 = float(torch.exp(0.5 * (F.logsigmoid(-ln) - F.logsigmoid(-lt))))
        c2 = float(-torch.sigmoid(ln).sqrt() * torch.expm1(torch.tensor(-h, dtype=F64)))
        row = [a0, b0x, b0e, c1, c2, 0.0, float(w_guide), 0.0]
        if order == 2 and h_prev is not None:
            row[C2RHO] = c2 * (h / (2.0 * h_prev))
        h_prev = h
        rows.append(torch.tensor(row, dtype=F64).to(torch.float32))
    return torch.stack(rows).contiguous(), torch.tensor(times, dtype=F64)


def p_encode(gd, denoise_fn, x_0, label=None, device=None, steps=None, order=1, spacing="time", clip_denoised=False, stop=None):
    """the chain of ``GaussianDiffusion.p_encode`` (see there); returns the latent on the device"""
    steps = gd.sample_timesteps if steps is None else int(steps)
    _check(steps, order)
    refuse_variants(gd, "the ascending solver")
    image_batch("x_0", x_0)
    if stop is not None and (isinstance(stop, bool) or not isinstance(stop, numbers.Integral) or not 1 <= stop <= steps):
        raise ValueError(f"stop must be an integer in [1, {steps}], got {stop!r}")
    table, t_net = encode_coefs(gd.logsnr_fn, steps, order, spacing, gd.model_out_type, gd.w_guide)      # host only; checks the spacing
    _need_cuda(x_0, "p_encode")
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    with _device_ctx(device):
        ch = Chain(gd, denoise_fn, x_0.to(device=device, dtype=torch.float32).contiguous().clone(), label, device)
        clip = bool(clip_denoised)
        hist = torch.zeros_like(ch.x)
        with ch.fixed_weights():
            for i in range(steps if stop is None else int(stop)):
                _hip.solver_step(ch.x, ch.net(float(t_net[i])), hist, table[i].tolist(), ch.mot, ch.cfg, clip, *ch.dst, ch.B, ch.C, ch.HW)
                ch.advance()
        return ch.x


# ------------------------------------------------------------------------------------------------ DDPM noise-space inversion
def _ddpm_rows(gd, Tc, clip):
    """[(the 8 floats of vd_sample_step, the network time)] of the DDPM steps landing on i = 0 ... Tc - 1, each noisy step's scale checked"""
    rows = [gd._step_coefs(i, False, clip) for i in range(Tc)]
    for i in range(1, Tc):
        s = rows[i][0][5]
        if not (s > 0.0 and s < float("inf")):
            raise ValueError(f"the step landing on index {i} has noise_scale {s}: there is no noise to extract or to replay")
    return rows


def p_invert_noise(gd, denoise_fn, x_0, label=None, device=None, seed=None, start=None, clip_denoised=True):
    """the chain of ``GaussianDiffusion.p_invert_noise`` (see there); returns (x_start, maps) on the device"""
    refuse_variants(gd, "noise-space inversion (that chain expands perturbations ~300x: a replay would not reconstruct)")
    image_batch("x_0", x_0)
    Tc = chain_length(gd, start)
    clip = bool(clip_denoised)
    rows = _ddpm_rows(gd, Tc, clip)
    _need_cuda(x_0, "p_invert_noise")
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    T, fn = gd.sample_timesteps, gd.logsnr_fn
    with _device_ctx(device):
        generator = None if seed is None else torch.Generator(device).manual_seed(seed)
        x_0 = x_0.to(device=device, dtype=torch.float32).contiguous()
        shape = tuple(x_0.shape)
        draw = lambda: torch.randn(shape, device=device, generator=generator)
        maps = torch.empty((Tc,) + shape, dtype=torch.float32, device=device)
        x_start = torch.empty_like(x_0)
        ch = Chain(gd, denoise_fn, x_start, label, device, in_place=True, dup=False)
        B, C, HW = ch.B, ch.C, ch.HW
        _hip.forward_jump(x_0, draw(), known_coefs(fn, T, Tc), *ch.dst, B, C * HW)             # x_Tc = alpha x_0 + sigma eps_Tc
        ch.x = x_start.clone()                                     # the working state is rewritten in place; x_start is returned
        with ch.fixed_weights():
            for i in reversed(range(Tc)):                          # the step landing on i, from the state at i + 1
                k8, t_net = rows[i]
                eps = draw() if i > 0 else None
                out = ch.net(t_net)
                k10 = list(k8) + list(known_coefs(fn, T, i))
                if i == 0:
                    k10[5] = 1.0                                   # the residual x_0 - x0_hat: scale 1, (ak, bk) = (1, 0), no draw
                _hip.noise_extract(ch.x, out, x_0, eps, k10, ch.mot, ch.cfg, i == 0, clip, ch.x, maps[i], ch.x_in if i > 0 else None,
                                   B, C, HW)
        return x_start, maps


def p_sample_replay(gd, denoise_fn, x_start, maps, label=None, device=None, clip_denoised=True):
    """the chain of ``GaussianDiffusion.p_sample_replay`` (see there); returns the final image batch on the device"""
    refuse_variants(gd, "the replay of noise maps")
    image_batch("x_start", x_start)
    T = gd.sample_timesteps
    if not torch.is_tensor(maps) or maps.dim() != 5 or tuple(maps.shape[1:]) != tuple(x_start.shape) or not 1 <= maps.shape[0] <= T:
        raise ValueError(f"maps must have shape (Tc, {', '.join(str(v) for v in x_start.shape)}) with 1 <= Tc <= {T}, got "
                         f"{tuple(getattr(maps, 'shape', ()))}")
    Tc = int(maps.shape[0])
    clip = bool(clip_denoised)
    rows = _ddpm_rows(gd, Tc, clip)
    _need_cuda(x_start, "p_sample_replay")
    _need_cuda(maps, "p_sample_replay")
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    with _device_ctx(device):
        ch = Chain(gd, denoise_fn, x_start.to(device=device, dtype=torch.float32).contiguous().clone(), label, device)
        maps = maps.to(device=device, dtype=torch.float32).contiguous()
        with ch.fixed_weights():
            for i in reversed(range(Tc)):
                k8, t_net = rows[i]
                k8 = list(k8)
                if i == 0:
                    k8[5] = 1.0                                    # vd_sample_step adds k[5]*noise also on the last step: the residual
                _hip.sample_step(ch.x, ch.net(t_net), maps[i], k8, ch.mot, ch.cfg, i == 0, clip, *ch.dst, ch.B, ch.C, ch.HW)
                ch.advance()
        return ch.x


# ------------------------------------------------------------------------------------------------ spherical interpolation
def slerp(a, b, frac, return_weights=False):
    """Spherical interpolation of two (B, ...) fp32 GPU tensors per sample, over all other dimensions: with w the angle between a[i] and
    b[i], out[i] = (sin((1-f) w) a[i] + sin(f w) b[i]) / sin w.  ``frac`` is a python float (all samples) or a (B,) tensor (one per
    sample), used as fp32.  One launch of vd_slerp_rows: dot product and norms in fp64 in a fixed order (the same bits on every call),
    the two weights formed in fp64 and rounded to fp32 once; they are the linear weights (1-f, f) when sin w < 1e-6 (parallel or
    antiparallel inputs) or an input is all zero.  ``return_weights=True`` also returns the (B, 2) weights.  The result is a new
    tensor.  CPU tensors raise."""
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.shape != b.shape or a.dim() < 1 or a.numel() == 0:
        raise ValueError(f"slerp needs two non-empty (B, ...) tensors of one shape, got {tuple(getattr(a, 'shape', ()))} and "
                         f"{tuple(getattr(b, 'shape', ()))}")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"slerp takes fp32, got {a.dtype} and {b.dtype}")
    B = a.shape[0]
    if torch.is_tensor(frac):
        if tuple(frac.shape) != (B,):
            raise ValueError(f"a tensor frac must have shape ({B},), got {tuple(frac.shape)}")
    elif isinstance(frac, bool) or not isinstance(frac, numbers.Real):
        raise ValueError(f"frac must be a float or a ({B},) tensor, got {frac!r}")
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise RuntimeError("slerp: both tensors must live on one MI355X (there is no CPU path)")
    with _device_ctx(a.device):
        ac, bc = a.contiguous(), b.contiguous()
        out = torch.empty_like(ac)
        w = torch.empty((B, 2), dtype=torch.float32, device=a.device) if return_weights else None
        if torch.is_tensor(frac):
            _hip.slerp_rows(ac, bc, None, out, w, B, ac.numel() // B, frac_dev=frac.to(device=a.device, dtype=torch.float32).contiguous())
        else:
            _hip.slerp_rows(ac, bc, float(frac), out, w, B, ac.numel() // B)
        return (out, w) if return_weights else out
