"""float64 restatement of one progressive-distillation step (Salimans & Ho 2022, Algorithm 2) in plain torch on CPU tensors: the
yardstick of tests/test_distill_cpu.py and tests/test_distill_gpu.py.  Everything is taken from first principles -- alpha, sigma from
the log-SNR, the DDIM step as "predict x, re-derive eps, re-noise", the target as the paper's QUOTIENT (safe in fp64) -- and nothing
from the package, so the package's convex form of the target is checked against an independent statement.  Log-SNRs are arguments:
(B,) fp64 tensors holding the fp32-rounded values the package works from."""
import torch

F64 = torch.float64


def col(v):
    return v.to(F64).reshape(-1, 1, 1, 1)


def alpha_sigma(l):
    return torch.sigmoid(l).sqrt(), torch.sigmoid(-l).sqrt()


def x0_from_out(out, z, l, out_type):
    """x0 prediction of a network output; l (B,1,1,1)"""
    a, s = alpha_sigma(l)
    if out_type == "v":
        return a * z - s * out
    if out_type == "x0":
        return out
    if out_type == "eps":
        return (z - s * out) / a
    if out_type == "both":
        x, e = out.chunk(2, dim=1)
        return torch.sigmoid(-l) * x + torch.sigmoid(l) * (z - s * e) / a
    raise NotImplementedError(out_type)


def ddim_step(z, x, l_s, l_t):
    """deterministic DDIM: eps_hat = (z - alpha_t x)/sigma_t, z_s = alpha_s x + sigma_s eps_hat"""
    a_t, s_t = alpha_sigma(l_t)
    a_s, s_s = alpha_sigma(l_s)
    return a_s * x + s_s * (z - a_t * x) / s_t


def c2(l_s, l_t):
    """weight of x in the DDIM step s <- t, written out: alpha_s - alpha_t sigma_s / sigma_t"""
    a_t, s_t = alpha_sigma(l_t)
    a_s, s_s = alpha_sigma(l_s)
    return a_s - a_t * s_s / s_t


def w2_quotient(l_t, l_mid, l_end):
    """weight of the second teacher prediction in the target, from the quotient's two c2"""
    return c2(l_end, l_mid) / c2(l_end, l_t)


def omega(reweight_type, l):
    snr = torch.exp(l)
    return {"constant": torch.ones_like(snr), "snr": snr, "snr_trunc": snr.clamp(min=1.0), "snr_1plus": 1.0 + snr}[reweight_type]


def teacher_x0(teacher, z, t, l, y, out_type, w_guide, clip):
    """(guided) x0 prediction: each prediction clipped first, then x_c + w (x_c - x_u)"""
    fix = (lambda p: p.clamp(-1.0, 1.0)) if clip else (lambda p: p)
    xc = fix(x0_from_out(teacher(z, t, y), z, l, out_type))
    if w_guide > 0 and y is not None:
        xu = fix(x0_from_out(teacher(z, t, torch.zeros_like(y)), z, l, out_type))
        return xc + w_guide * (xc - xu)
    return xc


def two_steps(teacher, z_t, times, logsnrs, y, out_type, w_guide=0.0, clip=False):
    """two DDIM steps of the teacher, t -> t' -> t'': (x_hat, z_t', x_hat', z_t''); where t'' = 0 the last entry is x_hat', the x0
    prediction the package's samplers return at their last step"""
    t, tm, te = times
    l, lm, le = (col(v) for v in logsnrs)
    xh = teacher_x0(teacher, z_t, t, l, y, out_type, w_guide, clip)
    zm = ddim_step(z_t, xh, lm, l)
    xh2 = teacher_x0(teacher, zm, tm, lm, y, out_type, w_guide, clip)
    ze = ddim_step(zm, xh2, le, lm)
    ze = torch.where(col(te) == 0, xh2, ze)
    return xh, zm, xh2, ze


def target(teacher, z_t, times, logsnrs, y, out_type, w_guide=0.0, clip=False):
    """x_tilde = (z_t'' - (sigma_t''/sigma_t) z_t) / (alpha_t'' - (sigma_t''/sigma_t) alpha_t): the x for which ONE DDIM step t -> t''
    from z_t lands on the teacher's z_t''; x_hat' where t'' = 0"""
    l, _, le = (col(v) for v in logsnrs)
    _, _, xh2, ze = two_steps(teacher, z_t, times, logsnrs, y, out_type, w_guide, clip)
    a_t, s_t = alpha_sigma(l)
    a_e, s_e = alpha_sigma(le)
    r = s_e / s_t
    return torch.where(col(times[2]) == 0, xh2, (ze - r * z_t) / (a_e - r * a_t))


def loss(student_out, z_t, x_tilde, l_t, out_type, reweight_type):
    """omega * mean_{c,h,w}((x_student - x_tilde)^2), (B,)"""
    xs = x0_from_out(student_out, z_t, col(l_t), out_type)
    return omega(reweight_type, l_t.to(F64)) * ((xs - x_tilde) ** 2).flatten(1).mean(1)
