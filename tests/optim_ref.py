"""References of the optimizer tail (csrc/optim.hip: vd_sumsq, vd_adamw_ema, vd_adamw_ema_flagged) in plain torch on the CPU:
tests/test_optim_ref_cpu.py proves them against torch.optim.AdamW + clip_grad_norm_ + the restated utils.py EMA, and
tests/test_optim_kernels_gpu.py holds the kernels to them.  Nothing here touches the library.

One update of flat buffers p, m, v, ema with the gradient g (train_utils.py:159-168, utils.py:144-149):

    clip = min(max_norm / (sqrt(gnorm_sq) + 1e-6), 1)      when a norm is given and max_norm > 0, else 1 (nn.utils.clip_grad_norm_)
    g   <- clip g
    p   <- (1 - lr wd) p                                   (decoupled weight decay)
    m   <- beta1 m + (1 - beta1) g,   v <- beta2 v + (1 - beta2) g^2
    p   <- p - lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps),   bc_i = 1 - beta_i^k
    ema <- ema + (1 - decay) (p - ema)

rng = (lo, hi) is an index range treated apart, as vd_adamw_ema's r_mode: rng_mode 1 = the range received no gradient (p, m, v kept, the
shadow still follows p), rng_mode 2 = the range is updated with the bias corrections of its own step count rng_k.

``step64`` is the truth: fp64 tensors, every constant (1 - beta, 1 - decay, 1 - lr wd, the bias corrections, the clip factor) formed in
Python floats, which is what torch.optim.AdamW and utils.py:149 hand to torch.  ``step32_torch`` is the natural-noise yardstick: the same
update on fp32 CPU tensors through torch.optim.AdamW's own operator sequence.  Both return a new state and leave their arguments alone."""
import math

import torch

F64 = torch.float64
KEYS = ("p", "m", "v", "ema")


def sumsq64(g):
    """sum of squares of a flat buffer in fp64 (0-d tensor)"""
    return (g.detach().to(F64) ** 2).sum()


def _segments(n, k, rng, rng_mode, rng_k):
    """[(lo, hi, step count or None = no gradient)] covering [0, n)"""
    if rng is None or rng_mode == 0:
        return [(0, n, k)]
    lo, hi = rng
    assert 0 <= lo <= hi <= n and rng_mode in (1, 2) and (rng_mode == 1 or rng_k is not None)
    return [(0, lo, k), (lo, hi, None if rng_mode == 1 else rng_k), (hi, n, k)]


def step64(state, g, *, lr, betas, eps, wd, max_norm, gnorm_sq, decay, k, rng=None, rng_mode=0, rng_k=None):
    """state: {"p", "m", "v", "ema"} flat tensors (read as fp64); gnorm_sq: a Python float, a one-element tensor or None"""
    p, m, v, ema = (state[key].detach().to(F64).clone() for key in KEYS)
    g = g.detach().to(F64)
    b1, b2 = betas
    clip = 1.0
    if gnorm_sq is not None and max_norm > 0:
        clip = min(max_norm / (math.sqrt(float(gnorm_sq)) + 1e-6), 1.0)
    g = g * clip
    for lo, hi, kk in _segments(p.numel(), k, rng, rng_mode, rng_k):
        if kk is None or hi == lo:
            continue
        s = slice(lo, hi)
        p[s] *= 1 - lr * wd
        m[s] = b1 * m[s] + (1 - b1) * g[s]
        v[s] = b2 * v[s] + (1 - b2) * g[s] * g[s]
        bc1, bc2 = 1 - b1 ** kk, 1 - b2 ** kk
        p[s] -= lr / bc1 * m[s] / (v[s].sqrt() / math.sqrt(bc2) + eps)
    ema = ema + (1 - decay) * (p - ema)
    return {"p": p, "m": m, "v": v, "ema": ema}


def step32_torch(state, g, *, lr, betas, eps, wd, max_norm, gnorm_sq, decay, k, rng=None, rng_mode=0, rng_k=None):
    """the same update on fp32 CPU tensors, operator for operator what clip_grad_norm_ and torch.optim.AdamW (single-tensor form) run:
    mul_, lerp_, mul_().addcmul_(value=1 - beta2), addcdiv_; the shadow as utils.py:149 writes it"""
    f32 = torch.float32
    p, m, v, ema = (state[key].detach().to(f32).clone() for key in KEYS)
    g = g.detach().to(f32).clone()
    b1, b2 = betas
    if gnorm_sq is not None and max_norm > 0:
        total = torch.as_tensor(float(gnorm_sq), dtype=f32).sqrt()
        g.mul_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    for lo, hi, kk in _segments(p.numel(), k, rng, rng_mode, rng_k):
        if kk is None or hi == lo:
            continue
        ps, ms, vs, gs = p[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi]
        ps.mul_(1 - lr * wd)
        ms.lerp_(gs, 1 - b1)
        vs.mul_(b2).addcmul_(gs, gs, value=1 - b2)
        bc1, bc2 = 1 - b1 ** kk, 1 - b2 ** kk
        denom = (vs.sqrt() / math.sqrt(bc2)).add_(eps)
        ps.addcdiv_(ms, denom, value=-(lr / bc1))
    ema += (1 - decay) * (p - ema)
    return {"p": p, "m": m, "v": v, "ema": ema}
