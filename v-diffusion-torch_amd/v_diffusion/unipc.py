"""UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models", multistep,
data-prediction form): a predictor of order up to 3 and a corrector that raises the order by one from the network call the next step
makes anyway.  It needs no training and runs any checkpoint ``p_sample_solver`` runs, with the same one network evaluation per step.

With lambda = logsnr/2 and the grid tau_0 = 0 < ... < tau_T = 1 of ``solver_coefs``, the chain visits the nodes T ... 1 and calls the
network once at each, at the PREDICTED state.  For a step lambda_start -> lambda_end of size h > 0 and order p (the requested order, at
most the number of the step: a chain warms up through orders 1, 2, ...):

    hh = -h,  phi_1 = expm1(hh),  B = hh ("bh1") or expm1(hh) ("bh2")
    r_k = (lambda of the k-th older prediction - lambda_start)/h, k = 1 ... p-1;  r_p = 1, the corrector's new point
    b_j = phi_{j+1} j!/B,  R_{j,k} = r_k^(j-1);  rho^p = [] | [1/2] | R[:p-1,:p-1]^-1 b[:p-1];  rho^c = [1/2] | R^-1 b
    D_k = (m_k - m_0)/r_k,  m_0 the prediction at the step's start
    x_bar = (sigma_end/sigma_start) x - alpha_end phi_1 m_0
    x~    = x_bar - alpha_end B sum_{k<p} rho^p_k D_k                                    (predictor)
    x^c   = x_bar - alpha_end B (sum_{k<p} rho^c_k D_k + rho^c_p (m_new - m_0))          (corrector; m_new = the prediction at x~)

The next predictor starts from x^c and keeps m_new.  x~ and x^c share x_bar, so x^c = x~ + differences of predictions: the whole node
-- guided prediction, corrector of the step that arrived, predictor of the step that leaves, shift of the three history images -- is
one fused launch (vd_unipc_step in csrc/diffusion.hip) and no further state image.  What runs where is ``solver.py``'s split: the weights
are fp64 host arithmetic on the fp32-rounded log-SNRs, each slot rounded once into a (steps, 16) table (``unipc_coefs``), the 2x2 and 3x3
solves included.  The first node's row has no corrector and the sampler zero-fills the history, so one kernel -- and one captured
graph -- serves every node; row 0 is (c1, c2, p1, p2) = (0, 1, 0, 0): the chain ends on the guided x0 prediction, as every sampler of
this package does.  ``variant="bh2", order=2, corrector=False`` is DPM-Solver++(2M).  MI355X only: CPU tensors raise."""
import math
import numbers

import torch

from . import _hip
from .chain import Chain, captured_step, refuse_variants
from .diffusion import F64, _device_ctx, _pred_coefs, logsnr_to_posterior_ddim
from .solver import _grid

# columns of the coefficient table (include/vdiff_hip.h, vd_unipc_step)
K = 16
A0, B0X, B0E, W_GUIDE, C1, C2, P1, P2, EG, E1, E2 = range(11)

VARIANTS = ("bh1", "bh2")
GRAPH_CACHE_MAX = 4


def _check(steps, order, variant):
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    if isinstance(order, bool) or not isinstance(order, numbers.Integral) or order not in (1, 2, 3):
        raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
    if variant not in VARIANTS:
        raise ValueError(f"variant must be 'bh1' or 'bh2', got {variant!r}")


def _step_weights(lam_old, lam_start, lam_end, p, variant):
    """``(B, r, rho_p, rho_c)`` of the step lambda_start -> lambda_end at order p: r = [r_1 ... r_{p-1}] from ``lam_old`` (the lambdas of
    the older predictions, nearest first), the p - 1 predictor and the p corrector weights.  Python floats; the solves are fp64."""
    h = lam_end - lam_start
    hh = -h
    phi1 = math.expm1(hh)
    B = hh if variant == "bh1" else phi1
    r = [(lam_old[k] - lam_start) / h for k in range(p - 1)]
    b, h_phi_k, fact = [], phi1 / hh - 1.0, 1.0
    for j in range(1, p + 1):
        b.append(h_phi_k * fact / B)
        fact *= j + 1
        h_phi_k = h_phi_k / hh - 1.0 / fact
    if p == 1:
        return B, r, [], [0.5]
    nodes = torch.tensor(r + [1.0], dtype=F64)
    R = torch.stack([nodes ** j for j in range(p)])
    b = torch.tensor(b, dtype=F64)
    rho_p = [0.5] if p == 2 else torch.linalg.solve(R[:p - 1, :p - 1], b[:p - 1]).tolist()
    return B, r, rho_p, torch.linalg.solve(R, b).tolist()


def _rows(logsnr_fn, tau, order, variant, corrector, model_out_type, w_guide):
    """the table rows in the order a chain executes them, i = steps - 1 ... 0 (row i = node i + 1): ((16,) fp32 row, network time) one at
    a time, so that a sampler builds row i on the host while the GPU is busy with node i + 2 (``solver._rows``)"""
    steps = len(tau) - 1
    alpha = lambda l: math.sqrt(1.0 / (1.0 + math.exp(-l)))
    lams = []                                                      # lambda of the nodes already visited, nearest first
    for i in reversed(range(steps)):
        st = torch.tensor([tau[i], tau[i + 1]], dtype=F64)
        l = logsnr_fn(st)                                          # may rewrite st in place
        t_net = float(st[1])
        ls32, lt32 = l[0:1].float(), l[1:2].float()
        c1, c2, _ = logsnr_to_posterior_ddim(ls32, lt32, eta=0.)
        a0, b0x, b0e = _pred_coefs(model_out_type, lt32[0])
        ls, lt = float(ls32.double()), float(lt32.double())
        row = [0.0] * K
        row[A0], row[B0X], row[B0E], row[W_GUIDE], row[C1], row[C2] = a0, b0x, b0e, float(w_guide), float(c1), float(c2)
        n = steps - 1 - i                                          # the number of the step that arrived at this node
        if corrector and n >= 1:
            p = min(order, n)
            B, r, rho_p, rho_c = _step_weights(lams[1:p], lams[0], 0.5 * lt, p, variant)
            aB = alpha(lt) * B
            row[EG] = -aB * rho_c[p - 1]
            for k in range(p - 1):
                row[E1 + k] = -aB * (rho_c[k] - rho_p[k]) / r[k]
        if i == 0:
            row[C1], row[C2] = 0.0, 1.0
        else:
            p = min(order, n + 1)
            B, r, rho_p, _ = _step_weights(lams[:p - 1], 0.5 * lt, 0.5 * ls, p, variant)
            aB = alpha(ls) * B
            for k in range(p - 1):
                row[P1 + k] = -aB * rho_p[k] / r[k]
        lams.insert(0, 0.5 * lt)
        yield torch.tensor(row, dtype=F64).to(torch.float32), t_net


def unipc_coefs(logsnr_fn, steps, order=3, variant="bh2", corrector=True, spacing="time", model_out_type="v", w_guide=0.):
    """``(table, t_net)``: the (steps, 16) fp32 table of vd_unipc_step, row i = node i + 1 -- the corrector of the step tau_{i+2} ->
    tau_{i+1} and the predictor of the step tau_{i+1} -> tau_i -- with the columns {a0, b0x, b0e, w_guide, c1, c2, p1, p2, eg, e1, e2,
    0...}, and the (steps,) fp64 times the network is called with, tau_{i+1} as ``logsnr_fn`` left it.  Pure torch on the CPU; grid,
    spacing and the slots a0, b0x, b0e, c1, c2 are ``solver_coefs``'s, bit for bit.

    With alpha the signal level of the node, alpha_next of the node the step leaves for, and r_k, rho^p, rho^c, B of the module's
    docstring (fp64 from the fp32-rounded log-SNRs, every slot rounded once): p_k = -alpha_next B rho^p_k / r_k for the leaving step of
    order min(order, n + 1), n = steps - 1 - i; eg = -alpha B rho^c_p and e_k = -alpha B (rho^c_k - rho^p_k) / r_k for the arriving step
    of order min(order, n).  All e slots are 0 on the first executed row (i = steps - 1) and everywhere with ``corrector=False``; row 0
    is (c1, c2, p1, p2) = (0, 1, 0, 0).  ``variant="bh2", order=2, corrector=False``: p1 = -c2 rho of ``solver_coefs(order=2)``."""
    steps = int(steps)
    _check(steps, order, variant)
    rows = list(_rows(logsnr_fn, _grid(logsnr_fn, steps, spacing), order, variant, bool(corrector), model_out_type, w_guide))[::-1]
    return torch.stack([r for r, _ in rows]).contiguous(), torch.tensor([t for _, t in rows], dtype=F64)


def p_sample_unipc(gd, denoise_fn, shape, noise=None, label=None, device=None, seed=None, steps=None, order=3, variant="bh2",
                   corrector=True, spacing="time", clip_denoised=True, use_graph=False):
    """the reverse chain of ``GaussianDiffusion.p_sample_unipc`` (see there); returns the final image batch on the device"""
    steps = gd.sample_timesteps if steps is None else int(steps)
    _check(steps, order, variant)
    if isinstance(clip_denoised, str):
        if clip_denoised != "dynamic":
            raise ValueError(f"clip_denoised must be True or False, got {clip_denoised!r}")
        raise NotImplementedError("clip_denoised='dynamic' with the UniPC sampler (p_sample_solver thresholds dynamically)")
    clip, corrector, shape = bool(clip_denoised), bool(corrector), tuple(shape)
    refuse_variants(gd, "the UniPC sampler")
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    with _device_ctx(device):
        generator = None if seed is None else torch.Generator(device).manual_seed(seed)
        if noise is None:
            x_t = torch.randn(shape, device=device, generator=generator)      # the only draw: p_sample's x_T for this seed
        else:
            x_t = noise.to(device=device, dtype=torch.float32).contiguous().clone()
        if use_graph:
            # one node -- network forward + the node's launch on device-resident coefficients -- from this object's own small LRU cache;
            # steps, order, variant, corrector and spacing are data of the same graph
            def launch(ch, st, out):
                _hip.unipc_step(ch.x, out, st["h0"], st["h1"], st["h2"], None, ch.mot, ch.cfg, clip, *ch.dst, None, ch.B, ch.C, ch.HW,
                                k_dev=st["k"])
            graph, st, _ = captured_step(gd.__dict__.setdefault("_unipc_graphs", {}), GRAPH_CACHE_MAX, gd, denoise_fn, shape, label, device,
                                         launch, key=(clip,), bufs=("h0", "h1", "h2"), kwidth=K)
            st["chain"].load(x_t, label)
            for name in ("h0", "h1", "h2"):
                st[name].zero_()
            table, t_net = unipc_coefs(gd.logsnr_fn, steps, order, variant, corrector, spacing, gd.model_out_type, gd.w_guide)
            ktab, t_net = table.to(device), t_net.tolist()
            for i in reversed(range(steps)):
                st["t"].fill_(t_net[i])
                st["k"].copy_(ktab[i])
                graph.replay()
            return st["chain"].x.clone()
        ch = Chain(gd, denoise_fn, x_t, label, device)
        h0, h1, h2 = (torch.zeros_like(x_t) for _ in range(3))
        tau = _grid(gd.logsnr_fn, steps, spacing)
        with ch.fixed_weights():
            for k16, t_net in _rows(gd.logsnr_fn, tau, order, variant, corrector, gd.model_out_type, gd.w_guide):    # unipc_coefs' rows
                _hip.unipc_step(ch.x, ch.net(t_net), h0, h1, h2, k16.tolist(), ch.mot, ch.cfg, clip, *ch.dst, None, ch.B, ch.C, ch.HW)
                ch.advance()
        return ch.x
