"""float64 restatement of the UniPC multistep predictor-corrector (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for
Fast Sampling of Diffusion Models", data-prediction form, variants B(h) = h ("bh1") and B(h) = e^h - 1 ("bh2")) in plain torch on CPU
tensors: the yardstick of tests/test_unipc_cpu.py and tests/test_unipc_gpu.py.  Written from the PUBLISHED form -- x_bar, the divided
differences D_k and the small linear solves for the weights -- not from the flattened table of v_diffusion/unipc.py:

    lambda = logsnr/2, the step lambda_start -> lambda_end, h = lambda_end - lambda_start > 0, hh = -h, phi_1 = expm1(hh), B = hh | expm1(hh)
    r_k = (lambda of the k-th older prediction - lambda_start)/h  (k = 1 ... p-1),  r_p = 1 (the corrector's new point)
    b_j = phi_{j+1} j!/B,   R_{j,k} = r_k^(j-1),   rho^p: none | [1/2] | R[:p-1,:p-1] rho = b[:p-1],   rho^c: [1/2] | R rho = b
    D_k = (m_k - m_0)/r_k,  m_0 the prediction at the step's start
    x_bar = (sigma_end/sigma_start) x - alpha_end phi_1 m_0
    x~    = x_bar - alpha_end B sum_{k<p} rho^p_k D_k                                   the predictor: where the network is called next
    x^c   = x_bar - alpha_end B (sum_{k<p} rho^c_k D_k + rho^c_p (m_new - m_0))         the corrector, m_new = the prediction at x~

The next predictor starts from x^c and keeps m_new (it is not evaluated again at x^c).  The step that arrives at node i (of T ... 1) is
step number T - i and runs at order min(P, T - i): a chain warms up through orders 1, 2, ..."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from solver_ref import alpha_sigma, gaussian_problem, x0_from_out   # noqa: E402,F401

F64 = torch.float64


def step_weights(lam_old, lam_start, lam_end, p, variant):
    """(phi_1, B, [r_1 ... r_{p-1}], rho^p (p - 1 weights), rho^c (p weights)) of one step of order p; lam_old = the lambdas of the older
    predictions, nearest first.  Python floats (fp64) and ``torch.linalg.solve`` in fp64."""
    if variant not in ("bh1", "bh2"):
        raise ValueError(variant)
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
    R = torch.tensor([[rk ** (j - 1) for rk in r + [1.0]] for j in range(1, p + 1)], dtype=F64)
    b = torch.tensor(b, dtype=F64)
    rho_p = [] if p == 1 else [0.5] if p == 2 else torch.linalg.solve(R[:p - 1, :p - 1], b[:p - 1]).tolist()
    rho_c = [0.5] if p == 1 else torch.linalg.solve(R, b).tolist()
    return phi1, B, r, rho_p, rho_c


def guided_x0(net, x, t, y, l, out_type, w=0.0, cfg=False, clip=False):
    """the guided x0 prediction at log-SNR l: each branch clipped first, then x_c + w (x_c - x_u)"""
    def pred(lab):
        p = x0_from_out(net(x, t, lab).to(F64), x, l, out_type)
        return p.clamp(-1.0, 1.0) if clip else p
    xc = pred(y)
    return xc + w * (xc - pred(torch.zeros_like(y))) if cfg else xc


def chain(net, x, logsnr_fn, tau, order, variant, corrector, y=None, out_type="x0", w=0.0, cfg=False, clip=False, stop=0,
          round_logsnr=True):
    """the chain over the grid tau_0 = 0 < ... < tau_T = 1 from the state x at node T; ``net(x, t, y)`` sees fp64 tensors, t of shape
    (B,), once per node T ... 1.  stop = 0 ends on the guided x0 prediction of node 1 (what every sampler of the package returns),
    stop = 1 on the state at tau_1 -- corrected when ``corrector``, else the predicted one.  ``round_logsnr``: the log-SNRs are rounded
    to fp32 first, as every coefficient table of the package does (the image dtype)."""
    T = len(tau) - 1
    st = torch.tensor([float(v) for v in tau], dtype=F64)
    l = logsnr_fn(st).to(F64)                                  # a rescaling schedule rewrites st: the network sees the rewritten times
    if round_logsnr:
        l = l.float().double()
    lam = (0.5 * l).tolist()
    al, sg = (v.tolist() for v in alpha_sigma(l))
    x = x.to(F64)
    hist = []                                                  # (lambda, prediction), newest first
    arrived = None                                             # the step that produced x: what its corrector needs
    for i in range(T, 0, -1):
        t = torch.full((x.shape[0],), float(st[i]), dtype=F64)
        m = guided_x0(net, x, t, y, l[i], out_type, w, cfg, clip)
        if arrived is not None and corrector:
            x_bar, aB, rho_c, D, m0 = arrived
            res = rho_c[-1] * (m - m0)
            for rc, d in zip(rho_c, D):
                res = res + rc * d
            x = x_bar - aB * res
        hist.insert(0, (lam[i], m))
        if i == 1:
            return m if stop == 0 else x
        p = min(order, T - i + 1)
        phi1, B, r, rho_p, rho_c = step_weights([hl for hl, _ in hist[1:p]], lam[i], lam[i - 1], p, variant)
        D = [(hist[k + 1][1] - m) / r[k] for k in range(p - 1)]
        x_bar = (sg[i - 1] / sg[i]) * x - al[i - 1] * phi1 * m
        arrived = (x_bar, al[i - 1] * B, rho_c, D, m)
        res = torch.zeros_like(x)
        for rp, d in zip(rho_p, D):
            res = res + rp * d
        x = x_bar - al[i - 1] * B * res


class Stub:
    """pointwise, non-linear stand-in network a(t) x + b(t) tanh(x) + g y (the one of tests/test_solver_gpu.py): the same function in
    fp64 on the CPU and in fp32 on the GPU"""

    training = False

    def __init__(self, a=(0.3, -0.5), b=(0.4, 0.3), g=0.07, both=False):
        self.a, self.b, self.g, self.both = a, b, g, both

    def __call__(self, x, t, y):
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        return torch.cat([out, 0.5 * out - 0.25 * x], dim=1) if self.both else out


def node(k, x, out_c, out_u, h0, h1, h2, both=False, cfg=False, clip=False):
    """``(xn, xc, g)``: the arithmetic of one launch as include/vdiff_hip.h states it for vd_unipc_step, in the dtype of its operands:
    k = the 16 slots as python floats, out_c / out_u = the network output of the conditional / unconditional rows"""
    C = x.shape[1]

    def pred(o):
        p = k[0] * x + k[1] * o[:, :C]
        if both:
            p = p + k[2] * o[:, C:]
        return p.clamp(-1.0, 1.0) if clip else p
    g = pred(out_c)
    if cfg:
        xu = pred(out_u)
        g = g + k[3] * (g - xu)
    xc = x + k[8] * (g - h0) + k[9] * (h1 - h0) + k[10] * (h2 - h0)
    xn = k[4] * xc + k[5] * g + k[6] * (h0 - g) + k[7] * (h1 - g)
    return xn, xc, g


def table_chain(net, x, table, t_net, y=None, both=False, cfg=False, clip=False, dtype=F64):
    """``(the chain's end, the corrected state at node 1)``: rows len(table)-1 ... 0 of a GIVEN table of ``unipc_coefs`` through
    ``node``, zero history first, every operation in ``dtype`` on the device of x: in fp64 what a sampler is off this is its own
    rounding, in fp32 it is the composition of the same ordered arithmetic the kernel is measured against"""
    x = x.to(dtype)
    h0, h1, h2 = (torch.zeros_like(x) for _ in range(3))
    xc = x
    for i in reversed(range(len(table))):
        k = table[i].double().tolist()
        t = torch.full((x.shape[0],), float(t_net[i]), dtype=F64, device=x.device)
        yy = None if y is None else y.to(x.device)
        out_c = net(x, t, yy).to(dtype)
        out_u = net(x, t, torch.zeros_like(yy)).to(dtype) if cfg else None
        x, xc, g = node(k, x, out_c, out_u, h0, h1, h2, both, cfg, clip)
        h0, h1, h2 = g, h0, h1
    return x, xc


def gaussian_errors(logsnr_fn, tau, order, variant, corrector, round_logsnr=True):
    """e(T) = |x(tau_1)/exact(tau_1) - 1| of the chain on the exactly solvable problem of ``solver_ref.gaussian_problem`` (s = 2, an
    x0-network), started on the exact curve: the quantity ``solver_ref.convergence_errors`` defines"""
    scale, net = gaussian_problem(logsnr_fn)
    x1 = chain(net, scale(1.0)[2].reshape(1, 1, 1, 1), logsnr_fn, tau, order, variant, corrector, stop=1, round_logsnr=round_logsnr)
    return float((x1 / scale(float(tau[1]))[2] - 1.0).abs().max())


# the errors of the chain on that problem, cosine schedule on [-6, 6], log-SNR-uniform grid: (variant, corrector, order) -> e(8), e(16),
# e(32), e(64)
TABLE = {
    ("bh2", False, 2): (2.084e-2, 7.800e-3, 2.064e-3, 5.227e-4),
    ("bh2", False, 3): (1.591e-2, 1.786e-4, 1.636e-4, 4.533e-5),
    ("bh2", True, 1): (9.041e-2, 2.538e-2, 6.524e-3, 1.642e-3),
    ("bh2", True, 2): (2.201e-2, 4.000e-3, 5.325e-4, 6.767e-5),
    ("bh2", True, 3): (1.759e-2, 5.259e-5, 3.033e-5, 2.698e-6),
    ("bh1", False, 2): (1.381e-1, 3.084e-2, 7.030e-3, 1.682e-3),
    ("bh1", False, 3): (2.112e-2, 1.073e-4, 1.397e-4, 4.288e-5),
    ("bh1", True, 1): (5.025e-2, 1.117e-2, 2.516e-3, 5.934e-4),
    ("bh1", True, 2): (7.746e-2, 9.034e-3, 1.056e-3, 1.270e-4),
    ("bh1", True, 3): (2.053e-2, 1.486e-4, 1.041e-5, 4.672e-7),
}
