"""float64 restatement of one consistency-distillation / consistency-training step (Song et al. 2023, Algorithms 2 and 3; Song &
Dhariwal 2024 for the pseudo-Huber metric) and of multistep consistency sampling (Song et al. 2023, Algorithm 1) in plain torch on
CPU tensors: the yardstick of tests/test_consistency_cpu.py and tests/test_consistency_gpu.py.  Everything is taken from first
principles -- alpha, sigma from the log-SNR, the DDIM step as "predict x, re-derive eps, re-noise", the residual as the plain
difference of two x0 predictions (safe in fp64) -- and nothing from the package, so the package's difference forms are checked against
an independent statement.  Log-SNRs are arguments: (B,) fp64 tensors holding the fp32-rounded values the package works from."""
import math
from fractions import Fraction

import torch

from distill_ref import F64, alpha_sigma, col, ddim_step, omega, teacher_x0, x0_from_out      # noqa: F401


def snap_up(t, N):
    """the smallest i in 1..N with i/N >= t, per element, by exact rational comparison"""
    out = []
    for v in torch.as_tensor(t, dtype=F64).reshape(-1).tolist():
        i = max(1, min(N, math.ceil(Fraction(v) * N)))
        out.append(i)
    return out


def z_down(teacher, z_t, x_0, eps, times, logsnrs, y, out_type, w_guide=0.0, clip=False, last_is_x0=True):
    """the state one step down, z_s.  ``teacher`` given: one DDIM step of its (clipped, guided) x0 prediction; with ``last_is_x0`` the
    rows with s = 0 take that prediction itself, what the package's samplers return on their last step.  ``teacher=None``
    (consistency training): alpha_s x_0 + sigma_s eps with the same eps."""
    t, s = times
    l, ls = (col(v) for v in logsnrs)
    if teacher is None:
        a_s, s_s = alpha_sigma(ls)
        return a_s * x_0 + s_s * eps
    xh = teacher_x0(teacher, z_t, t, l, y, out_type, w_guide, clip)
    zs = ddim_step(z_t, xh, ls, l)
    return torch.where(col(s) == 0, xh, zs) if last_is_x0 else zs


def target(target_net, z_s, s, l_s, y, out_type):
    """the target network's x0 prediction at (z_s, s), never guided; z_s itself where s = 0 (boundary condition f(z, 0) = z)"""
    pred = x0_from_out(target_net(z_s, s, y), z_s, col(l_s), out_type)
    return torch.where(col(s) == 0, z_s, pred)


def loss(student_out, z_t, tgt, l_t, out_type, reweight_type, metric, huber_c=0.00054):
    """(B,): omega * S/D (l2) or omega * (sqrt(S + c^2) - c), c = huber_c sqrt(D) (pseudo-Huber), S = sum (x_student - target)^2"""
    xs = x0_from_out(student_out, z_t, col(l_t), out_type)
    S = ((xs - tgt) ** 2).flatten(1).sum(1)
    D = xs[0].numel()
    w = omega(reweight_type, l_t.to(F64))
    if metric == "l2":
        return w * S / D
    if metric == "huber":
        c = huber_c * math.sqrt(D)
        return w * (torch.sqrt(S + c * c) - c)
    raise NotImplementedError(metric)


def schedule(T, n):
    """n grid indices, evenly spaced and strictly descending from T: T (n - k)/n rounded half up, by exact rational arithmetic"""
    return [math.floor(Fraction(T * (n - k), n) + Fraction(1, 2)) for k in range(n)]


def sample_rows(logsnrs_t, logsnrs_next, out_type):
    """per step (a0, b0x, b0e, alpha_next, sigma_next) in fp64 from the fp32-rounded log-SNRs; next = None on the last step"""
    rows = []
    for lt, ln in zip(logsnrs_t, logsnrs_next):
        lt = torch.tensor(float(lt), dtype=F64)
        a, s = alpha_sigma(lt)
        pred = {"v": (a, -s, 0.0), "x0": (0.0, 1.0, 0.0), "eps": (1 / a, -s / a, 0.0),
                "both": (a, torch.sigmoid(-lt), -a * s)}[out_type]            # sigma^2 x + alpha^2 (z - sigma e)/alpha
        nxt = (1.0, 0.0) if ln is None else alpha_sigma(torch.tensor(float(ln), dtype=F64))
        rows.append(tuple(float(v) for v in pred + tuple(nxt)))
    return rows


def sample(net, x_T, draws, times, logsnrs, y, out_type, w_guide=0.0, clip=True):
    """multistep consistency sampling: at times[j] (log-SNR logsnrs[j]) predict x (clipped per branch, then guided), re-noise it to
    times[j + 1] with draws[j]; the last prediction is returned.  times: python floats, descending."""
    x = x_T
    B = x.shape[0]
    for j, (t, l) in enumerate(zip(times, logsnrs)):
        tt = torch.full((B,), t, dtype=F64)
        lt = torch.full((B,), float(l), dtype=F64)
        xh = teacher_x0(net, x, tt, col(lt), y, out_type, w_guide, clip)
        if j == len(times) - 1:
            return xh
        a_n, s_n = alpha_sigma(torch.tensor(float(logsnrs[j + 1]), dtype=F64))
        x = a_n * xh + s_n * draws[j]


# ---- Gaussian data x_0 ~ N(0, var0 I): everything is linear in z and known in closed form
def gaussian_std(l, var0=0.25):
    a, s = alpha_sigma(l)
    return torch.sqrt(a * a * var0 + s * s)


def gaussian_denoiser(l, var0=0.25):
    """E[x_0 | z_t] = k z_t"""
    a, s = alpha_sigma(l)
    return a * var0 / (a * a * var0 + s * s)


def gaussian_consistency(l, l0, var0=0.25):
    """the exact consistency function f(z, t) = z std_0 / std_t of the probability-flow ODE: the factor"""
    return gaussian_std(l0, var0) / gaussian_std(l, var0)
