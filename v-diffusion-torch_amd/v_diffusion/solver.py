"""DPM-Solver++(2M) (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", data-prediction
form): a second-order multistep solver of the probability-flow ODE in log-SNR time.  It needs no training and runs any checkpoint the
DDIM sampler runs, with the same one network evaluation per step.

With lambda = logsnr/2 and, for the step t -> s, h = lambda_s - lambda_t > 0, the DDIM weights of ``logsnr_to_posterior_ddim(eta=0)`` are
c1 = sigma_s/sigma_t and c2 = alpha_s (1 - e^-h), and

    order 1 (DDIM):  x_s = c1 x_t + c2 x_hat_t
    order 2 (2M):    x_s = c1 x_t + c2 [x_hat_t + rho (x_hat_t - x_hat_prev)],   rho = h / (2 h_prev)

x_hat_prev is the (guided) x0 prediction of the step before: one more image of state, no further network call.

What runs where: the weights are fp64 host arithmetic on the fp32-rounded log-SNRs, each slot rounded once into a (steps, 8) table
(``solver_coefs``); everything per element is one fused launch per step (vd_solver_step in csrc/diffusion.hip).  The first step of a
chain has no previous prediction: its row carries c2 rho = 0 and the sampler zero-fills the history image, so one kernel -- and one
captured graph -- serves every step.  The last row is (c1, c2, c2 rho) = (0, 1, 0): the chain ends on the guided x0 prediction, as every
sampler of this package does.  MI355X only: CPU tensors raise.

Thresholding.  ``clip_denoised=True`` clips each branch's x0 prediction to [-1, 1] before guidance, so the guided prediction
g = x_c + w (x_c - x_u) still reaches 1 + 2w.  ``clip_denoised="dynamic"`` is Imagen's dynamic thresholding (Saharia et al. 2022, section
2.3) of g itself, the companion Lu et al. recommend for this solver: per sample s = the magnitude of rank r of |g|, raised to at least 1
(and capped at ``dynamic_max``), g' = clamp(g, -s, s) / s, and the update and the history use g'.  r = ``threshold_rank(N, quantile)`` is
the "higher" order statistic -- a value of the sample, found exactly by a radix select inside the step's one launch
(vd_solver_step_dyn) -- where Imagen interpolates a percentile; the two differ by at most the gap between neighbouring order statistics.
"""
import math

import torch
import torch.nn.functional as F

from . import _hip
from .chain import Chain, captured_step, refuse_variants
from .diffusion import F64, _device_ctx, _pred_coefs, logsnr_to_posterior_ddim, stable_log1mexp

# columns of the coefficient table (include/vdiff_hip.h, vd_solver_step)
K = 8
A0, B0X, B0E, C1, C2, C2RHO, W_GUIDE, _PAD = range(K)

BISECTIONS = 64            # halvings of [0, 1]: the bracket is at the fp64 resolution of tau long before the last one
PROBES = 1025              # uniform probe times of the monotonicity check
GRAPH_CACHE_MAX = 4


def _grid(logsnr_fn, steps, spacing):
    """the steps + 1 grid times tau_0 = 0 < ... < tau_steps = 1 as python floats"""
    if spacing == "time":
        return [i / steps for i in range(steps + 1)]               # the grid (and the division) of ``_step_coefs``
    if spacing != "logsnr":
        raise ValueError(f"spacing must be 'time' or 'logsnr', got {spacing!r}")
    f = lambda t: logsnr_fn(t.clone()).to(F64)                     # a rescaling schedule rewrites its argument: probe on clones
    probe = f(torch.linspace(0.0, 1.0, PROBES, dtype=F64))
    if not bool((probe[1:] < probe[:-1]).all()):
        raise ValueError("spacing='logsnr' needs a strictly decreasing logsnr_fn on [0, 1]")
    ends = f(torch.tensor([0.0, 1.0], dtype=F64))
    frac = torch.arange(1, steps, dtype=F64) / steps
    want = ends[0] + (ends[1] - ends[0]) * frac                    # logsnr(tau_i), linear in i
    lo, hi = torch.zeros_like(want), torch.ones_like(want)
    for _ in range(BISECTIONS):
        mid = 0.5 * (lo + hi)
        right = f(mid) > want                                      # decreasing: the root lies to the right of mid
        lo, hi = torch.where(right, mid, lo), torch.where(right, hi, mid)
    tau = [0.0] + (0.5 * (lo + hi)).tolist() + [1.0]
    if steps > 1:
        at = f(torch.tensor(tau, dtype=F64))
        if not (all(a < b for a, b in zip(tau, tau[1:])) and bool((at[1:] < at[:-1]).all())):
            raise ValueError("spacing='logsnr' needs a strictly decreasing logsnr_fn on [0, 1]")
    return tau


def _check(steps, order):
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    if order not in (1, 2):
        raise ValueError(f"order must be 1 (DDIM) or 2 (DPM-Solver++ 2M), got {order!r}")


def _rows(logsnr_fn, tau, order, model_out_type, w_guide):
    """the table rows in the order a chain executes them, i = steps - 1 ... 0: ((8,) fp32 row, network time) one at a time, so that a
    sampler builds row i on the host while the GPU is busy with step i + 1 (a whole table up front is ~0.2 ms of host time per row
    in front of the first launch)"""
    steps = len(tau) - 1
    h_prev = None
    for i in reversed(range(steps)):
        st = torch.tensor([tau[i], tau[i + 1]], dtype=F64)
        l = logsnr_fn(st)                                          # may rewrite st in place
        t_net = float(st[1])
        ls32, lt32 = l[0:1].float(), l[1:2].float()
        c1, c2, _ = logsnr_to_posterior_ddim(ls32, lt32, eta=0.)
        a0, b0x, b0e = _pred_coefs(model_out_type, lt32[0])
        ls, lt = ls32.double(), lt32.double()
        h = 0.5 * float(ls - lt)
        row = [a0, b0x, b0e, float(c1), float(c2), 0.0, float(w_guide), 0.0]
        if i == 0:
            row[C1], row[C2] = 0.0, 1.0
        elif order == 2 and h_prev is not None:
            # c2 before its rounding (the expression of logsnr_to_posterior_ddim) times rho, rounded once below
            row[C2RHO] = float(torch.exp(stable_log1mexp(0.5 * (lt - ls)) + 0.5 * F.logsigmoid(ls))) * (h / (2.0 * h_prev))
        h_prev = h
        yield torch.tensor(row, dtype=F64).to(torch.float32), t_net


def solver_coefs(logsnr_fn, steps, order=2, spacing="time", model_out_type="v", w_guide=0.):
    """``(table, t_net)``: the (steps, 8) fp32 table of vd_solver_step, row i = the step tau_{i+1} -> tau_i with the columns named
    above, and the (steps,) fp64 times the network is called with, tau_{i+1} as ``logsnr_fn`` left it (a rescaling schedule rewrites its
    argument; the rule of ``GaussianDiffusion._step_coefs``).  Pure torch on the CPU.

    ``spacing="time"``: tau_i = i/steps, the grid of every sampler here.  ``spacing="logsnr"``: logsnr(tau_i) linear in i between
    logsnr(0) and logsnr(1) (uniform steps h: the grid the solver's error analysis assumes), tau_i by fp64 bisection, ends exactly 0, 1.

    The arithmetic is ``_step_coefs``'s: per row ``logsnr_fn`` sees the pair (tau_i, tau_{i+1}), the log-SNRs are rounded to fp32 (the image
    dtype), a0, b0x, b0e come from ``_pred_coefs`` and c1, c2 from ``logsnr_to_posterior_ddim(eta=0)`` -- order 1 is bit for bit the DDIM
    sampler's numbers.  h_i = (l_s - l_t)/2 and rho_i = h_i/(2 h_{i+1}) are fp64 from those fp32 values; c2 rho is the fp64 product
    rounded once.  rho = 0 on the first executed row (i = steps - 1), on every row of order 1, and on row 0, which is (0, 1, 0)."""
    steps = int(steps)
    _check(steps, order)
    rows = list(_rows(logsnr_fn, _grid(logsnr_fn, steps, spacing), order, model_out_type, w_guide))[::-1]
    return torch.stack([r for r, _ in rows]).contiguous(), torch.tensor([t for _, t in rows], dtype=F64)


def threshold_rank(N, quantile):
    """the 0-based ascending rank r = min(N - 1, ceil(quantile (N - 1))) of the magnitude dynamic thresholding takes as s, for a sample
    of N elements and a quantile in (0, 1]: the rank ``numpy.quantile(..., method="higher")`` returns.  fp64 host arithmetic, once."""
    N, q = int(N), float(quantile)
    if N < 1:
        raise ValueError(f"N must be >= 1, got {N}")
    if not 0.0 < q <= 1.0:
        raise ValueError(f"quantile must be in (0, 1], got {quantile!r}")
    return min(N - 1, math.ceil(q * (N - 1)))


def _threshold_max(max_value):
    """s_max as the kernels take it: +Inf for no cap"""
    s_max = math.inf if max_value is None else float(max_value)
    if not s_max >= 1.0:
        raise ValueError(f"the cap of the dynamic threshold must be >= 1, got {max_value!r}")
    return s_max


def _clip_mode(clip_denoised, N, dynamic_quantile, dynamic_max):
    """True / False (static clip of each branch, or none: vd_solver_step), or ("dynamic", r, s_max) (vd_solver_step_dyn)"""
    if isinstance(clip_denoised, str):
        if clip_denoised != "dynamic":
            raise ValueError(f"clip_denoised must be True, False or 'dynamic', got {clip_denoised!r}")
        return ("dynamic", threshold_rank(N, dynamic_quantile), _threshold_max(dynamic_max))
    return bool(clip_denoised)


def _step(clip, x, out, hist, k8, mot, cfg, xn, xdup, B, C, HW, k_dev=None):
    """the step's one launch for a clip mode of ``_clip_mode``"""
    if isinstance(clip, tuple):
        _hip.solver_step_dyn(x, out, hist, k8, mot, cfg, clip[1], clip[2], None, xn, xdup, B, C, HW, k_dev=k_dev)
    else:
        _hip.solver_step(x, out, hist, k8, mot, cfg, clip, xn, xdup, B, C, HW, k_dev=k_dev)


def dynamic_threshold(x, quantile=0.995, max_value=None):
    """``(x', s)``: dynamic thresholding of a (B, ...) fp32 tensor on the GPU by the solver's rule, per sample over all other
    dimensions: s = min(max(the magnitude of rank ``threshold_rank(N, quantile)``, 1), max_value), x' = clamp(x, -s, s) / s.  The order
    statistic is vd_abs_kth_rows' (exact); s has shape (B,).  CPU tensors raise."""
    if x.dim() < 1 or x.shape[0] < 1 or x.numel() == 0:
        raise ValueError(f"dynamic_threshold needs a non-empty (B, ...) tensor, got shape {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"dynamic_threshold takes fp32, got {x.dtype}")
    B = x.shape[0]
    N = x.numel() // B
    r, s_max = threshold_rank(N, quantile), _threshold_max(max_value)
    if not x.is_cuda:
        raise RuntimeError("dynamic_threshold: the tensor must live on an MI355X (there is no CPU path)")
    with _device_ctx(x.device):
        xc = x.contiguous()
        s = torch.empty((B,), dtype=torch.float32, device=x.device)
        _hip.abs_kth_rows(xc, B, N, r, s)
        s = s.clamp(min=1.0, max=s_max)                              # (a NaN stays one)
        sb = s.reshape((B,) + (1,) * (x.dim() - 1))
        return torch.maximum(torch.minimum(xc, sb), -sb) / sb, s


def p_sample_solver(gd, denoise_fn, shape, noise=None, label=None, device=None, seed=None, steps=None, order=2, spacing="time",
                    clip_denoised=True, use_graph=False, dynamic_quantile=0.995, dynamic_max=None):
    """the reverse chain of ``GaussianDiffusion.p_sample_solver`` (see there); returns the final image batch on the device"""
    steps = gd.sample_timesteps if steps is None else int(steps)
    _check(steps, order)
    shape = tuple(shape)
    clip = _clip_mode(clip_denoised, int(shape[1]) * int(shape[2]) * int(shape[3]), dynamic_quantile, dynamic_max)
    refuse_variants(gd, "the multistep solver")
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    with _device_ctx(device):
        generator = None if seed is None else torch.Generator(device).manual_seed(seed)
        if noise is None:
            x_t = torch.randn(shape, device=device, generator=generator)      # the only draw: p_sample's x_T for this seed
        else:
            x_t = noise.to(device=device, dtype=torch.float32).contiguous().clone()
        if use_graph:
            # one reverse step -- network forward + the step's launch on device-resident coefficients -- from this object's own small
            # LRU cache.  The rank and the cap of the dynamic threshold are launch arguments, not table data: ``clip`` is part of the key
            def launch(ch, st, out):
                _step(clip, ch.x, out, st["hist"], None, ch.mot, ch.cfg, *ch.dst, ch.B, ch.C, ch.HW, k_dev=st["k"])
            graph, st, _ = captured_step(gd.__dict__.setdefault("_solver_graphs", {}), GRAPH_CACHE_MAX, gd, denoise_fn, shape, label, device,
                                         launch, key=(clip,), bufs=("hist",))
            st["chain"].load(x_t, label)
            st["hist"].zero_()
            table, t_net = solver_coefs(gd.logsnr_fn, steps, order, spacing, gd.model_out_type, gd.w_guide)
            ktab, t_net = table.to(device), t_net.tolist()
            for i in reversed(range(steps)):
                st["t"].fill_(t_net[i])
                st["k"].copy_(ktab[i])
                graph.replay()
            return st["chain"].x.clone()
        ch = Chain(gd, denoise_fn, x_t, label, device)
        hist = torch.zeros_like(x_t)
        tau = _grid(gd.logsnr_fn, steps, spacing)
        with ch.fixed_weights():
            for k8, t_net in _rows(gd.logsnr_fn, tau, order, gd.model_out_type, gd.w_guide):      # solver_coefs' rows, last one first
                _step(clip, ch.x, ch.net(t_net), hist, k8.tolist(), ch.mot, ch.cfg, *ch.dst, ch.B, ch.C, ch.HW)
                ch.advance()
        return ch.x
