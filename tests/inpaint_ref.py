"""float64 restatement of the RePaint inpainting sampler in plain torch: the yardstick of tests/test_inpaint_cpu.py and
tests/test_inpaint_gpu.py.  Written from the formulas (Lugmayr et al. 2022 in log-SNR terms), not from v_diffusion/inpaint.py:

    reverse step t -> s   u  = mean(x_t, x0_hat) + noise_scale * noise         (the ordinary posterior step, guided when asked)
                          kn = alpha_s known + sigma_s knoise                  (a draw from q(x_s | known))
                          x_s = kn where m == 1, u where m == 0, m kn + (1 - m) u in between
    jump s -> t           x_t = (alpha_t/alpha_s) x_s + sqrt(sigma_t^2 (1 - e^(l_t - l_s))) eps

``step`` / ``merge`` / ``jump`` take GIVEN coefficients (python floats) and evaluate in the stated order in the dtype of their tensor
arguments: on fp64 CPU tensors they are the reference, and on fp32 GPU tensors the same functions are the composition the kernels are
measured against (kernel and composition then differ in FMA contraction only).  ``chain`` runs a whole schedule over a given list of
noises with an arbitrary callable network."""
import torch

F64 = torch.float64


def alpha_sigma(l):
    l = torch.as_tensor(l, dtype=F64)
    return torch.sigmoid(l).sqrt(), torch.sigmoid(-l).sqrt()


def jump_weights(l_s, l_t):
    """(a, b) of the forward transition from log-SNR l_s to l_t < l_s, from the definition: a = alpha_t/alpha_s,
    b^2 = sigma_t^2 - a^2 sigma_s^2"""
    a_s, s_s = alpha_sigma(l_s)
    a_t, s_t = alpha_sigma(l_t)
    a = a_t / a_s
    return float(a), float((s_t * s_t - a * a * s_s * s_s).clamp(min=0.0).sqrt())


def unknown(k, xt, out, noise, both=False, cfg=False, last=False, clip=False):
    """u: the reverse step of the unknown region from a network output of n*(1+cfg) rows (cond, uncond interleaved) and C (2C) channels;
    k = {a0, b0x, b0e, c1, c2, noise_scale, w_guide, c3, ...}"""
    a0, b0x, b0e, c1, c2, nscale, w, c3 = [float(v) for v in k[:8]]
    C = xt.shape[1]

    def mean(o):
        x0h = a0 * xt + b0x * o[:, :C]
        if both:
            x0h = x0h + b0e * o[:, C:]
        if clip:
            x0h = x0h.clamp(-1.0, 1.0)
        return x0h if last else c1 * xt + c2 * x0h + c3 * o[:, :C]
    if cfg:
        mc, mu = mean(out[0::2]), mean(out[1::2])
        v = mc + w * (mc - mu)
    else:
        v = mean(out)
    return v if noise is None else v + nscale * noise


def merge(u, kn, m):
    """the two ends of the mask select"""
    m = m.expand_as(u)
    return torch.where(m == 1, kn, torch.where(m == 0, u, m * kn + (1.0 - m) * u))


def step(k, xt, out, noise, known, mask, knoise, both=False, cfg=False, last=False, clip=False):
    """one masked reverse step; k = the 8 weights of ``unknown`` and (ak, bk)"""
    ak, bk = float(k[8]), float(k[9])
    kn = ak * known if knoise is None else ak * known + bk * knoise
    return merge(unknown(k, xt, out, noise, both, cfg, last, clip), kn, mask)


def jump(x, noise, a, b):
    return float(a) * x + float(b) * noise


def net_out(net, x, t, y, cfg):
    """the network output as the samplers lay it out: with cfg, rows interleaved cond (label y), uncond (label 0)"""
    if not cfg:
        return net(x, t, y)
    oc, ou = net(x, t, y), net(x, t, torch.zeros_like(y))
    return torch.stack([oc, ou], dim=1).reshape((2 * x.shape[0],) + tuple(oc.shape[1:]))


def chain(net, x, known, mask, sched, step_row, jump_row, noises, y=None, both=False, cfg=False, clip=True):
    """the schedule ``sched`` (grid indices, e.g. [4, 3, 4, 3, ...0]) from the state x at sched[0].  ``step_row(i)`` gives (the 10
    weights, the network time) of the reverse step that lands on index i, ``jump_row(i, j)`` the (a, b) of the jump i -> i + j;
    ``noises`` holds the draws after the initial state in the sampler's order: per reverse step noise then knoise, per jump one.
    ``net(x, t, y)`` sees tensors of x's dtype and device, t of shape (B,)."""
    noises = iter(noises)
    for cur, nxt in zip(sched, sched[1:]):
        if nxt == cur - 1:
            k, t_net = step_row(nxt)
            t = torch.full((x.shape[0],), float(t_net), dtype=F64, device=x.device)
            out = net_out(net, x, t, y, cfg).to(x.dtype)
            noise, knoise = next(noises), next(noises)
            x = step(k, x, out, noise, known, mask, knoise, both, cfg, nxt == 0, clip)
        else:
            x = jump(x, next(noises), *jump_row(cur, nxt - cur))
    return x
