"""float64 restatement of dynamic thresholding (Saharia et al. 2022, section 2.3) inside the DPM-Solver++(2M) step: the yardstick of
tests/test_threshold_cpu.py and tests/test_threshold_gpu.py.  Written from the formulas, not from the package; per sample over its N
elements:

    s_raw = the element of rank r (0-based, ascending) of |g|,   r = min(N - 1, ceil(q (N - 1)))      (the "higher" order statistic)
    s     = min(max(s_raw, 1), s_max),   g' = min(max(g, -s), s) / s
    x_s   = c1 x_t + c2 g' + c2rho (g' - hist),   hist <- g'

with g the UNCLIPPED guided x0 prediction of tests/solver_ref.py (``guided_x0(clip=False)``) and the update that file's ``step``."""
import math

import torch

import solver_ref as R

F64 = torch.float64


def rank(N, q):
    """r = min(N - 1, ceil(q (N - 1))) for q in (0, 1]"""
    if not 0.0 < q <= 1.0:
        raise ValueError(q)
    return min(N - 1, math.ceil(q * (N - 1)))


def s_raw(g, r):
    """(B,) rank-r magnitudes of a (B, ...) tensor: full sort per sample"""
    return g.reshape(g.shape[0], -1).abs().sort(dim=1).values[:, r]


def threshold(g, r, s_max=math.inf):
    """(g', s) of a (B, ...) tensor in its own dtype (fp64 for the yardstick), s of shape (B,)"""
    s = s_raw(g, r).clamp(min=1.0).clamp(max=s_max)
    sb = s.reshape((-1,) + (1,) * (g.dim() - 1))
    return torch.maximum(torch.minimum(g, sb), -sb) / sb, s


def step_dyn(k, xt, out, hist, both, cfg, r, s_max=math.inf):
    """(xn, g', s) of one step of table row k from a given network output ``out`` (n*(1+cfg) rows, cond/uncond interleaved), in fp64"""
    oc, ou = (out[0::2], out[1::2]) if cfg else (out, out)
    net = lambda x, t, lab: (oc if bool(lab.any()) else ou).double()
    g = R.guided_x0(net, xt.double(), None, torch.ones(xt.shape[0]), k.double(), both, cfg, clip=False)
    gp, s = threshold(g, r, s_max)
    return R.step(xt.double(), gp, hist.double(), k.double()), gp, s


def chain_dyn(net, x, table, t_net, r, s_max=math.inf, y=None, both=False, cfg=False, stop=0):
    """``solver_ref.chain`` with every guided prediction thresholded before the update and before it becomes the history"""
    x = x.to(F64)
    hist = torch.zeros_like(x)
    for i in reversed(range(stop, len(table))):
        t = torch.full((x.shape[0],), float(t_net[i]), dtype=F64)
        g = R.guided_x0(net, x, t, y, table[i].to(F64), both, cfg, clip=False)
        gp, _ = threshold(g, r, s_max)
        x, hist = R.step(x, gp, hist, table[i].to(F64)), gp
    return x
