"""float64 restatement of Diffusion Posterior Sampling (Chung et al. 2023, Algorithm 1) in plain torch: the yardstick of
tests/test_dps_cpu.py and tests/test_dps_gpu.py.  Written from the formulas, not from v_diffusion/dps.py:

    operators         A g = M (.) g  |  the mean over f x f blocks  |  the mean over the channels;   A^T their adjoints
    residual          g = the guided, clipped x0 prediction of the step;  r = meas - A g;  sumsq = sum r^2 per sample;  u = -A^T r
    cotangents        of (1/2)||r||^2:  dout = d/d out,  dxt = d/d x_t with out held fixed (the closed forms at vd_dps_residual in include/vdiff_hip.h)
    step              x_s = [the ordinary reverse step] - zeta / sqrt(sumsq) (dxt + the rows of dxin of the sample),  dxin = the
                      network's VJP of dout;  the term is selected: zeta = 0 or sumsq = 0 leave the ordinary step

Every function takes GIVEN coefficients (python floats) and evaluates in the dtype of its tensor arguments: on fp64 CPU tensors it is the
reference, on fp32 GPU tensors the same function is the composition the kernels are measured against.  ``chain`` runs a whole chain over
given draws with an arbitrary differentiable network, its VJP taken by torch autograd."""
import torch

import inpaint_ref as IR

F64 = torch.float64
OPS = ("mask", "down", "gray")


def apply_A(op, x, par=None, mask=None):
    """A x of (B, C, H, W): op "mask" (mask (B, 1 or C, H, W)), "down" (par = f), "gray" """
    B, C, H, W = x.shape
    if op == "mask":
        return mask.expand_as(x) * x
    if op == "down":
        return x.reshape(B, C, H // par, par, W // par, par).sum(dim=(3, 5)) / float(par * par)
    assert op == "gray"
    return x.sum(dim=1, keepdim=True) / float(C)


def apply_At(op, r, shape, par=None, mask=None):
    """A^T r, of ``shape`` = (B, C, H, W)"""
    B, C, H, W = shape
    if op == "mask":
        return mask.expand(shape) * r
    if op == "down":
        return (r / float(par * par)).repeat_interleave(par, dim=2).repeat_interleave(par, dim=3)
    assert op == "gray"
    return (r / float(C)).expand(shape)


def measurement_shape(op, shape, par=None):
    B, C, H, W = shape
    return {"mask": (B, C, H, W), "down": (B, C, H // (par or 1), W // (par or 1)), "gray": (B, 1, H, W)}[op]


def branch(k, xt, o, both, clip):
    """(the clipped x0 prediction of one branch, the pass mask of the clip: 1 where -1 <= p <= 1 or clip is off)"""
    a0, b0x, b0e = float(k[0]), float(k[1]), float(k[2])
    C = xt.shape[1]
    p = a0 * xt + b0x * o[:, :C]
    if both:
        p = p + b0e * o[:, C:]
    if not clip:
        return p, torch.ones_like(p)
    return p.clamp(-1.0, 1.0), ((p >= -1.0) & (p <= 1.0)).to(p.dtype)


def guided(k, xt, out, both=False, cfg=False, clip=False):
    """(g, m_c, m_u) from a network output of n*(1+cfg) rows (cond, uncond interleaved); m_u None without guidance"""
    w = float(k[6])
    if not cfg:
        g, m = branch(k, xt, out, both, clip)
        return g, m, None
    xc, mc = branch(k, xt, out[0::2], both, clip)
    xu, mu = branch(k, xt, out[1::2], both, clip)
    return xc + w * (xc - xu), mc, mu


def loss(k, xt, out, meas, op, par=None, mask=None, both=False, cfg=False, clip=False):
    """(1/2) ||meas - A g(x_t, out)||^2 per sample: what the cotangents are the gradient of"""
    g = guided(k, xt, out, both, cfg, clip)[0]
    r = meas - apply_A(op, g, par, mask)
    return 0.5 * (r * r).reshape(r.shape[0], -1).sum(dim=1)


def residual(k, xt, out, meas, op, par=None, mask=None, both=False, cfg=False, clip=False):
    """dict(dout, dxt, sumsq, x0hat, r): the outputs of the residual launch, closed form"""
    a0, b0x, b0e, w = float(k[0]), float(k[1]), float(k[2]), float(k[6])
    g, mc, mu = guided(k, xt, out, both, cfg, clip)
    r = meas - apply_A(op, g, par, mask)
    u = -apply_At(op, r, tuple(xt.shape), par, mask)
    halves = lambda c: torch.cat([c * b0x, c * b0e], dim=1) if both else c * b0x
    if cfg:
        cc, cu = (1.0 + w) * mc * u, -w * mu * u
        dout = torch.stack([halves(cc), halves(cu)], dim=1).reshape((2 * xt.shape[0], -1) + tuple(xt.shape[2:]))
        dxt = a0 * (((1.0 + w) * mc - w * mu) * u)
    else:
        dout = halves(mc * u)
        dxt = a0 * (mc * u)
    return dict(dout=dout, dxt=dxt, sumsq=(r * r).reshape(r.shape[0], -1).sum(dim=1), x0hat=g, r=r)


def step(k, xt, out, noise, dxin, dxt, sumsq, zeta, both=False, cfg=False, last=False, clip=False):
    """the ordinary reverse step (inpaint_ref.unknown is the product sampler's step) and the selected correction"""
    v = IR.unknown(k, xt, out, noise, both, cfg, last, clip)
    if float(zeta) == 0.0:
        return v
    d = dxt + dxin[0::2] + dxin[1::2] if cfg else dxt + dxin
    ss = sumsq.reshape(-1, 1, 1, 1)
    sc = torch.where(torch.isfinite(ss), float(zeta) * (1.0 / ss.sqrt()), torch.full_like(ss, float("nan")))
    take = (ss != 0).expand_as(v)
    return torch.where(take, v - sc * torch.where(take, d, torch.zeros_like(d)), v)


def chain(net, x, meas, op, step_row, noises, zetas, par=None, mask=None, y=None, both=False, cfg=False, clip=True):
    """the T = len(zetas) steps of a chain from the state x.  ``step_row(i)`` gives (the 8 weights, the network time) of the step that
    lands on index i, ``noises`` the draws after the initial state (one per step), ``zetas[i]`` the step size of index i.  ``net(x, t, y)``
    sees tensors of x's dtype and device and must be differentiable in x: its VJP is torch autograd's.  With cfg the network sees the
    state twice, rows interleaved (label y, label 0), as the samplers lay it out."""
    noises = iter(noises)
    rep = 2 if cfg else 1
    y_in = None
    if y is not None:
        y_in = y.repeat_interleave(rep, dim=0).clone()
        if cfg:
            y_in[1::2] = 0
    for nxt in reversed(range(len(zetas))):
        k, t_net = step_row(nxt)
        t = torch.full((x.shape[0] * rep,), float(t_net), dtype=F64, device=x.device)
        with torch.enable_grad():
            xi = x.detach().repeat_interleave(rep, dim=0).requires_grad_(True)
            raw = net(xi, t, y_in)
        out = raw.detach().to(x.dtype)
        res = residual(k, x, out, meas, op, par, mask, both, cfg, clip)
        dxin = torch.autograd.grad(raw, xi, res["dout"].to(raw.dtype))[0].to(x.dtype)
        x = step(k, x, out, next(noises), dxin, res["dxt"], res["sumsq"], zetas[nxt], both, cfg, nxt == 0, clip).detach()
    return x
