"""float64 restatement of the Denoising Diffusion Null-space Model (Wang, Yu, Zhang 2023) in plain torch: the yardstick of
tests/test_ddnm_cpu.py and tests/test_ddnm_gpu.py.  Written from the formulas, not from v_diffusion/ddnm.py:

    pseudo-inverses   mask: y / M where M > 0, 0 elsewhere  |  the two means: every measurement element copied over its preimage
    step              v = the ordinary reverse step (inpaint_ref.unknown is the product sampler's);  g = the guided, clipped x0
                      prediction (dps_ref.guided);  r = meas - A g;  x_s = v + cw A^+ r with cw = lam on the last step, else c2 lam
                      (v holds c2 g).  Selected: lam = 0 leaves v; a mask element 0 has no measurement and no share of sum r^2; on the
                      last step with lam = 1 and no noise term a mask element 1 IS the measurement
    rule (DDNM+)      lam = 1 where the step's noise covers c2 sigma_y, else noise_scale / (c2 sigma_y); the step keeps
                      sqrt(noise_scale^2 - (c2 lam sigma_y)^2) of its noise; the last step: lam = 1 if sigma_y = 0 else 0

``step`` and ``pinv`` take GIVEN coefficients (python floats) and evaluate in the dtype of their tensor arguments: on fp64 CPU tensors they
are the reference, on fp32 GPU tensors the same functions are the composition the kernel is measured against.  ``chain`` runs a whole
schedule over given draws with an arbitrary callable network."""
import math

import torch

import inpaint_ref as IR
from dps_ref import apply_A, branch, guided                       # noqa: F401  (branch: re-exported for the tests' input recipe)

F64 = torch.float64


def pinv(op, y, shape, par=None, mask=None):
    """A^+ y, of ``shape`` = (B, C, H, W)"""
    if op == "mask":
        m = mask.expand(shape)
        return torch.where(m > 0, y / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(y))
    if op == "down":
        return y.repeat_interleave(par, dim=2).repeat_interleave(par, dim=3)
    assert op == "gray"
    return y.expand(shape)


def rule(c2, noise_scale, sigma_y, last, lam=None):
    """(lam, the noise scale left to the step); an explicit lam replaces the rule's"""
    if lam is None:
        if last:
            lam = 1.0 if sigma_y == 0 else 0.0
        else:
            lam = 1.0 if noise_scale >= c2 * sigma_y else noise_scale / (c2 * sigma_y)
    return lam, math.sqrt(max(0.0, noise_scale ** 2 - (c2 * lam * sigma_y) ** 2))


def step(k, xt, out, noise, meas, op, lam, par=None, mask=None, both=False, cfg=False, last=False, clip=False):
    """dict(xn, sumsq, r, g) of one step; k = the 8 weights of ``inpaint_ref.unknown``"""
    shape = tuple(xt.shape)
    v = IR.unknown(k, xt, out, noise, both, cfg, last, clip)
    g = guided(k, xt, out, both, cfg, clip)[0]
    r = meas - apply_A(op, g, par, mask)
    taken = mask.expand(shape) > 0 if op == "mask" else torch.ones_like(r, dtype=torch.bool)
    r = torch.where(taken, r, torch.zeros_like(r))                # (whatever meas holds where nothing was measured)
    sumsq = (r * r).reshape(shape[0], -1).sum(dim=1)
    if float(lam) == 0.0:
        return dict(xn=v, sumsq=sumsq, r=r, g=g)
    cw = float(lam) if last else float(k[4]) * float(lam)
    d = pinv(op, r, shape, par, mask)
    xn = torch.where(taken if op == "mask" else torch.ones_like(v, dtype=torch.bool), v + cw * d, v)
    if op == "mask" and last and float(lam) == 1.0 and (noise is None or float(k[5]) == 0.0):
        xn = torch.where(mask.expand(shape) == 1, meas, xn)
    return dict(xn=xn, sumsq=sumsq, r=r, g=g)


def chain(net, x, meas, op, sched, step_row, jump_row, noises, sigma_y=0.0, lams=None, par=None, mask=None, y=None, both=False, cfg=False,
          clip=True):
    """the schedule ``sched`` (grid indices from T to 0, jumps included) from the state x.  ``step_row(i)`` gives (the 8 weights, the
    network time) of the reverse step that lands on index i, ``jump_row(i, j)`` the (a, b) of the jump i -> i + j, ``noises`` the draws
    after the initial state, one per transition; ``lams`` None (the rule) or one lam per destination index.  Returns (the final state,
    [the sum r^2 of every reverse step])."""
    noises = iter(noises)
    sums = []
    for cur, nxt in zip(sched, sched[1:]):
        noise = next(noises)
        if nxt == cur - 1:
            k, t_net = step_row(nxt)
            k = [float(v) for v in k]
            lam, k[5] = rule(k[4], k[5], float(sigma_y), nxt == 0, None if lams is None else lams[nxt])
            t = torch.full((x.shape[0],), float(t_net), dtype=F64, device=x.device)
            out = IR.net_out(net, x, t, y, cfg).to(x.dtype)
            res = step(k, x, out, noise, meas, op, lam, par, mask, both, cfg, nxt == 0, clip)
            x = res["xn"]
            sums.append(res["sumsq"])
        else:
            x = IR.jump(x, noise, *jump_row(cur, nxt - cur))
    return x, sums
