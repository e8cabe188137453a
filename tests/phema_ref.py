"""fp64 restatement of post-hoc EMA (Karras et al. 2024, section 3.5 / appendix C), independent of v_diffusion/phema.py: the recurrence of a
power-function profile, the least-squares weights of a reconstruction, and the exact combination of sources.  numpy and the standard
library only."""
import decimal
import fractions
import math

import numpy as np

U = 2.0 ** -24


def gamma_of(sigma_rel):
    """gamma with sigma_rel = sqrt(gamma + 1) / ((gamma + 2) sqrt(gamma + 3)), by bisection (sigma_rel falls as gamma grows)"""
    lo, hi = 0.0, 1e7
    for _ in range(300):
        mid = 0.5 * (lo + hi)
        if math.sqrt(mid + 1) / ((mid + 2) * math.sqrt(mid + 3)) > sigma_rel:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def beta(t, gamma):
    return (1.0 - 1.0 / t) ** (gamma + 1.0)


def rate_decimal(t, gamma, digits=50):
    """1 - (1 - 1/t)^(gamma + 1) in `digits`-digit decimal arithmetic (gamma taken as the double it is)"""
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        if t == 1:
            return decimal.Decimal(1)
        base = 1 - decimal.Decimal(1) / decimal.Decimal(t)
        return 1 - (base.ln() * (decimal.Decimal(gamma) + 1)).exp()


def track(thetas, gamma, t0=0, e0=None):
    """the profile after each update: e_t = beta_t e_{t-1} + (1 - beta_t) theta_t, t = t0 + 1, ...; thetas: [T][...] float64.  Returns [T][...]"""
    out, e = [], None if e0 is None else np.asarray(e0, dtype=np.float64)
    for i, th in enumerate(np.asarray(thetas, dtype=np.float64)):
        t = t0 + i + 1
        b = beta(t, gamma)
        e = th.copy() if t == 1 else b * e + (1.0 - b) * th
        out.append(e)
    return np.stack(out)


def density(tau, t, gamma):
    """p_{t,gamma}(tau) = (gamma + 1) tau^gamma / t^(gamma + 1) on [0, t], 0 beyond"""
    tau = np.asarray(tau, dtype=np.float64)
    return np.where(tau <= t, (gamma + 1.0) * (tau / t) ** gamma / t, 0.0)


def dot_simpson(ta, ga, tb, gb, panels=200000):
    """composite Simpson of p_a p_b over [0, min(ta, tb)]"""
    hi = min(ta, tb)
    x = np.linspace(0.0, hi, 2 * panels + 1)
    f = density(x, ta, ga) * density(x, tb, gb)
    h = hi / (2 * panels)
    return h / 3.0 * (f[0] + f[-1] + 4.0 * f[1:-1:2].sum() + 2.0 * f[2:-1:2].sum())


def dot_closed(ta, ga, tb, gb):
    """int_0^min p_a p_b = (ga+1)(gb+1) / (ta^(ga+1) tb^(gb+1)) min^(ga+gb+1) / (ga+gb+1), written from the integral"""
    lo = min(ta, tb)
    return math.exp(math.log(ga + 1) + math.log(gb + 1) - (ga + 1) * math.log(ta) - (gb + 1) * math.log(tb)
                    + (ga + gb + 1) * math.log(lo)) / (ga + gb + 1)


def weights(snap_t, snap_gamma, t_r, gamma_r):
    """least-squares weights of the reconstruction of (t_r, gamma_r) from the snapshots (minimum-norm solution of the normal equations)"""
    K = len(snap_t)
    A = np.array([[dot_closed(snap_t[i], snap_gamma[i], snap_t[j], snap_gamma[j]) for j in range(K)] for i in range(K)])
    b = np.array([dot_closed(snap_t[i], snap_gamma[i], t_r, gamma_r) for i in range(K)])
    return np.linalg.lstsq(A, b, rcond=None)[0]


def combine_fraction(srcs, w, idx, acc=None):
    """exact sum_j w_j src_j[i] (+ acc[i]) for i in idx, as Fractions of the doubles / floats they are"""
    out = []
    for i in idx:
        s = fractions.Fraction(float(acc[i])) if acc is not None else fractions.Fraction(0)
        for x, wj in zip(srcs, w):
            if wj != 0.0:
                s += fractions.Fraction(float(wj)) * fractions.Fraction(float(x[i]))
        out.append(s)
    return out


def combine_longdouble(srcs, w):
    """sum_j w_j src_j in numpy.longdouble, and sum_j |w_j src_j| (float64) for the error bound; sources of weight 0 are skipped"""
    s = np.zeros(srcs[0].shape, dtype=np.longdouble)
    mag = np.zeros(srcs[0].shape, dtype=np.float64)
    for x, wj in zip(srcs, w):
        if wj != 0.0:
            s += np.longdouble(wj) * x.astype(np.longdouble)
            mag += np.abs(wj * x.astype(np.float64))
    return s, mag


def ulp32(x):
    """spacing of fp32 at |x| (float64 array in, the ulp of the binade of |x|, at least the subnormal spacing)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def shadow_step_bound(r, p_new, e_old, e_new64):
    """the one-step bound of the kernel's e' = e + r (p' - e): 2 [(2u + u^2) r |p' - e| + u |e'_64|] (three roundings, doubled)"""
    return 2.0 * ((2 * U + U * U) * r * np.abs(p_new - e_old) + U * np.abs(e_new64))
