"""float64 restatement of the DPM-Solver++(2M) sampler in plain torch on CPU tensors: the yardstick of tests/test_solver_cpu.py and
tests/test_solver_gpu.py.  Written from the formulas (Lu et al. 2022, data-prediction form), not from v_diffusion/solver.py:

    lambda = logsnr/2,  h = lambda_s - lambda_t,  x_s = (sigma_s/sigma_t) x_t + alpha_s (1 - e^-h) [x_hat_t + rho (x_hat_t - x_hat_prev)]

``chain`` runs a GIVEN coefficient table (rows {a0, b0x, b0e, c1, c2, c2rho, w, 0}, row i = the step tau_{i+1} -> tau_i, executed from the
last row down) with an arbitrary callable network, every operation in fp64: what the kernel and the samplers are off this is their
own rounding, not the table's.  ``weights`` builds one row's c1, c2, rho from log-SNRs, for checking a table."""
import torch

F64 = torch.float64


def alpha_sigma(l):
    l = torch.as_tensor(l, dtype=F64)
    return torch.sigmoid(l).sqrt(), torch.sigmoid(-l).sqrt()


def x0_from_out(out, z, l, out_type):
    """x0 prediction of a network output at log-SNR l"""
    a, s = alpha_sigma(l)
    if out_type == "v":
        return a * z - s * out
    if out_type == "x0":
        return out
    if out_type == "eps":
        return (z - s * out) / a
    if out_type == "both":
        x, e = out.chunk(2, dim=1)
        return s * s * x + a * a * (z - s * e) / a
    raise NotImplementedError(out_type)


def x0_weights(l, out_type):
    """(a0, b0x, b0e) with x0_hat = a0 z + b0x out (+ b0e out_eps): ``x0_from_out`` read off as weights"""
    a, s = (float(v) for v in alpha_sigma(l))
    return {"v": (a, -s, 0.0), "x0": (0.0, 1.0, 0.0), "eps": (1.0 / a, -s / a, 0.0), "both": (a, s * s, -a * s)}[out_type]


def weights(l_s, l_t, l_prev=None):
    """(c1, c2, rho) of the step t -> s; l_prev = the log-SNR the step before started from (None: first step, rho = 0)"""
    a_s, s_s = alpha_sigma(l_s)
    _, s_t = alpha_sigma(l_t)
    h = 0.5 * (torch.as_tensor(l_s, dtype=F64) - torch.as_tensor(l_t, dtype=F64))
    rho = 0.0 if l_prev is None else float(h / (torch.as_tensor(l_t, dtype=F64) - torch.as_tensor(l_prev, dtype=F64)))
    return float(s_s / s_t), float(-a_s * torch.expm1(-h)), rho


def guided_x0(net, x, t, y, k, both=False, cfg=False, clip=False):
    """the guided x0 prediction of table row k: each branch clipped first, then x_c + w (x_c - x_u)"""
    k = [float(v) for v in k]
    C = x.shape[1]

    def pred(lab):
        out = net(x, t, lab).to(F64)
        p = k[0] * x + k[1] * out[:, :C] + (k[2] * out[:, C:] if both else 0.0)
        return p.clamp(-1.0, 1.0) if clip else p
    xc = pred(y)
    return xc + k[6] * (xc - pred(torch.zeros_like(y))) if cfg else xc


def step(x, g, hist, k):
    """one update from the guided prediction g and the previous one"""
    k = [float(v) for v in k]
    return k[3] * x + k[4] * g + k[5] * (g - hist)


def chain(net, x, table, t_net, y=None, both=False, cfg=False, clip=False, stop=0):
    """rows len(table)-1 ... stop of the table from the state x; ``net(x, t, y)`` sees fp64 tensors, t of shape (B,).  stop = 0 ends on
    the last row's guided x0 prediction, stop = 1 on the state at tau_1."""
    x = x.to(F64)
    hist = torch.zeros_like(x)
    for i in reversed(range(stop, len(table))):
        t = torch.full((x.shape[0],), float(t_net[i]), dtype=F64)
        g = guided_x0(net, x, t, y, table[i].to(F64), both, cfg, clip)
        x, hist = step(x, g, hist, table[i].to(F64)), g
    return x


# ---- a problem with a known solution.  Data N(0, s^2) per element: the exact denoiser is alpha s^2 x / (alpha^2 s^2 + sigma^2), and the
# exact solution of the probability-flow ODE is x_t proportional to sqrt(alpha_t^2 s^2 + sigma_t^2).
def gaussian_problem(logsnr_fn, s=2.0):
    """(scale, net): scale(t) = (alpha, sigma, sqrt(alpha^2 s^2 + sigma^2)) at time(s) t, and the exact x0-network ``net(x, t, y)``"""
    def scale(t):
        a, sg = alpha_sigma(logsnr_fn(torch.as_tensor(t, dtype=F64).reshape(-1).clone()))
        return a, sg, (a * a * s * s + sg * sg).sqrt()

    def net(x, t, y):
        a, _, m = scale(t)
        return (a * s * s / (m * m)).reshape(-1, 1, 1, 1) * x
    return scale, net


def convergence_errors(logsnr_fn, coefs, order, run, steps=(16, 32, 64)):
    """e(T) = |x(tau_1)/exact(tau_1) - 1| on log-SNR-uniform grids.  ``coefs`` is the table builder under test, and
    ``run(net, m1, table, t_net, order)`` takes the chain from x(1) = m1 (on the exact curve) and returns its state at tau_1."""
    scale, net = gaussian_problem(logsnr_fn)
    errs = []
    for T in steps:
        table, t_net = coefs(logsnr_fn, T, order=order, spacing="logsnr", model_out_type="x0")
        x1 = run(net, scale(1.0)[2], table, t_net, order)
        errs.append(float((x1 / scale(float(t_net[0]))[2] - 1.0).abs().max()))
    return errs


def check_convergence(e1, e2):
    """second order halves to a quarter, first order to a half, and second order is the better one by 10x at T = 32"""
    print(f"[solver convergence] order 1: {e1[0]:.3e} {e1[1]:.3e} {e1[2]:.3e} (ratios {e1[0] / e1[1]:.2f} {e1[1] / e1[2]:.2f})   "
          f"order 2: {e2[0]:.3e} {e2[1]:.3e} {e2[2]:.3e} (ratios {e2[0] / e2[1]:.2f} {e2[1] / e2[2]:.2f})")
    assert e2[0] / e2[1] >= 3.5 and e2[1] / e2[2] >= 3.5, e2
    assert 1.8 <= e1[0] / e1[1] <= 2.2 and 1.8 <= e1[1] / e1[2] <= 2.2, e1
    assert e2[1] <= e1[1] / 10, (e1, e2)
