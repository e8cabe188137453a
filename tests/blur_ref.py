"""float64 restatement of the blur operator of Diffusion Posterior Sampling in plain torch: the yardstick of tests/test_blur_cpu.py and
tests/test_blur_gpu.py.  Written from the formulas, not from v_diffusion or csrc/diffusion.hip:

    A         (A g)[c, y, x] = sum_i sum_j taps[i, j] * g[c, rho_H(y + i - Rh), rho_W(x + j - Rw)], a cross-correlation with the reflect
              boundary that does not repeat the edge: the reflect-padded tensor is gathered by index, and A is the sum of its Kh * Kw
              shifted slices, each times its tap, added in tap order -- no library convolution and no library padding, so on fp32 GPU
              tensors the function is "the same arithmetic as plain fp32 torch ops"
    A^T       torch autograd of that sum: independent of the gather formula of include/vdiff_blur.h
    residual  dps_ref.residual's outputs with this A (built on dps_ref.guided);  chain: dps_ref.chain's loop with it (dps_ref.step)

Every function evaluates in the dtype of its tensor arguments, as dps_ref's do; the taps enter as python floats."""
import torch

import dps_ref as R

F64 = torch.float64


def rho(n, r, device=None):
    """the source index of every position -r ... n - 1 + r of an axis of n elements padded by reflection"""
    p = torch.arange(-r, n + r, device=device).abs()
    return torch.where(p > n - 1, 2 * (n - 1) - p, p)


def apply_A(x, taps):
    """A x of (..., H, W) with the (Kh, Kw) taps"""
    kh, kw = taps.shape
    H, W = x.shape[-2:]
    assert kh % 2 == 1 and kw % 2 == 1 and kh // 2 <= H - 1 and kw // 2 <= W - 1
    xp = x.index_select(-2, rho(H, kh // 2, x.device)).index_select(-1, rho(W, kw // 2, x.device))
    t = taps.detach().cpu().double().tolist()
    acc = None
    for i in range(kh):
        for j in range(kw):
            term = t[i][j] * xp[..., i:i + H, j:j + W]
            acc = term if acc is None else acc + term
    return acc


def apply_At(r, taps):
    """A^T r, by autograd of apply_A (A is linear: the point of linearisation does not matter)"""
    with torch.enable_grad():
        x = torch.zeros_like(r).requires_grad_(True)
        y = apply_A(x, taps)
    return torch.autograd.grad(y, x, r.detach())[0]


def gather_At(r, taps):
    """A^T r of ONE plane (H, W) by the gather formula of include/vdiff_blur.h, explicit loops in python floats (fp64): the sum over the
    preimages pre_H(y) x pre_W(x) and the taps of taps[i][j] * r~[p - i + Rh][q - j + Rw], r~ = r extended by zero"""
    kh, kw = taps.shape
    H, W = r.shape
    rh, rw = kh // 2, kw // 2
    pre = lambda y, n, R_: [y] + ([-y] if 1 <= y <= R_ else []) + ([2 * (n - 1) - y] if n - 1 - R_ <= y <= n - 2 else [])
    t, rr = taps.double().tolist(), r.double().tolist()
    out = torch.zeros((H, W), dtype=F64)
    for y in range(H):
        for x in range(W):
            acc = 0.0
            for p in pre(y, H, rh):
                for q in pre(x, W, rw):
                    for i in range(kh):
                        for j in range(kw):
                            yy, xx = p - i + rh, q - j + rw
                            if 0 <= yy < H and 0 <= xx < W:
                                acc += t[i][j] * rr[yy][xx]
            out[y, x] = acc
    return out


def residual(k, xt, out, meas, taps, both=False, cfg=False, clip=False):
    """dict(dout, dxt, sumsq, x0hat, r): dps_ref.residual's outputs for the blur operator"""
    a0, b0x, b0e, w = float(k[0]), float(k[1]), float(k[2]), float(k[6])
    g, mc, mu = R.guided(k, xt, out, both, cfg, clip)
    r = meas - apply_A(g, taps)
    u = -apply_At(r, taps)
    halves = lambda c: torch.cat([c * b0x, c * b0e], dim=1) if both else c * b0x
    if cfg:
        cc, cu = (1.0 + w) * mc * u, -w * mu * u
        dout = torch.stack([halves(cc), halves(cu)], dim=1).reshape((2 * xt.shape[0], -1) + tuple(xt.shape[2:]))
        dxt = a0 * (((1.0 + w) * mc - w * mu) * u)
    else:
        dout = halves(mc * u)
        dxt = a0 * (mc * u)
    return dict(dout=dout, dxt=dxt, sumsq=(r * r).reshape(r.shape[0], -1).sum(dim=1), x0hat=g, r=r)


def chain(net, x, meas, taps, step_row, noises, zetas, y=None, both=False, cfg=False, clip=True):
    """dps_ref.chain for the blur operator: the T = len(zetas) steps from the state x, the network's VJP by torch autograd"""
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
        res = residual(k, x, out, meas, taps, both, cfg, clip)
        dxin = torch.autograd.grad(raw, xi, res["dout"].to(raw.dtype))[0].to(x.dtype)
        x = R.step(k, x, out, next(noises), dxin, res["dxt"], res["sumsq"], zetas[nxt], both, cfg, nxt == 0, clip).detach()
    return x
