"""float64 restatement of image inversion in plain torch: the yardstick of tests/test_invert_cpu.py and tests/test_invert_gpu.py.
Written from the formulas, not from v_diffusion/invert.py:

    noise-space inversion   x_i = alpha_i x_0 + sigma_i eps_i  (independent eps_i),   z_i = (x_i - mu_i(x_{i+1})) / noise_scale_i,
                            z_0 = x_0 - x0_hat(x_1)            (mu, x0_hat: the guided mean / prediction of the ordinary reverse step)
    replay                  x_i = mu_i(x_{i+1}) + noise_scale_i z_i,   and the chain ends on x0_hat(x_1) + z_0
    encoding                x_n = (sigma_n/sigma_t) x_t + alpha_n (1 - e^-h) [g + rho (g - g_prev)],  h = (l_n - l_t)/2 < 0,  rho = h/(2 h_prev)
    slerp                   (sin((1-f) w) a + sin(f w) b) / sin w,  cos w = <a,b>/(|a||b|);  (1-f) a + f b when sin w < 1e-6 or a norm is 0

The functions take GIVEN coefficients (python floats) and evaluate in the stated order in the dtype of their tensor arguments: on fp64
CPU tensors they are the reference, and on fp32 GPU tensors the same functions are the composition the kernels are measured against.
The guided mean is ``inpaint_ref.unknown``."""
import math

import torch

import inpaint_ref as I

F64 = torch.float64
alpha_sigma = I.alpha_sigma


class Stub:
    """the pointwise stand-in network of tests/test_inpaint_gpu.py, a(t) x + b(t) tanh(x) + g y: the same function in fp64 on the CPU and
    in fp32 on the GPU; ``calls`` (optional list) receives the time of every call"""

    training = False

    def __init__(self, a=(0.3, -0.5), b=(0.4, 0.3), g=0.07, both=False, calls=None):
        self.a, self.b, self.g, self.both, self.calls = a, b, g, both, calls

    def __call__(self, x, t, y):
        if self.calls is not None:
            self.calls.append(float(t[0]))
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        return torch.cat([out, 0.5 * out - 0.25 * x], dim=1) if self.both else out


def ddpm_row(vd, gd, i, clip=True):
    """(the 10 fp32 weights as python floats, the network time) of the DDPM step of ``gd`` that lands on grid index i: ``_step_coefs``'s
    eight and ``known_coefs``'s two; for i = 0 slot 5 carries 1 (the residual's scale).  i = sample_timesteps (no such step) gives zeros
    and the (alpha, sigma) of the start."""
    T = gd.sample_timesteps
    ab = list(vd.known_coefs(gd.logsnr_fn, T, i))
    if i == T:
        return [0.0] * 8 + ab, None
    k8, t_net = gd._step_coefs(i, False, clip)
    k8 = list(k8)
    if i == 0:
        k8[5] = 1.0
    return torch.tensor(k8 + ab, dtype=F64).float().tolist(), t_net


def extract(k, xt, out, x0, eps, both=False, cfg=False, last=False, clip=False):
    """(xs, z) of one inversion step; k = the 8 weights of ``inpaint_ref.unknown`` and (ak, bk)"""
    ak, bk, scale = float(k[8]), float(k[9]), float(k[5])
    xs = ak * x0 if eps is None else ak * x0 + bk * eps
    return xs, (xs - I.unknown(k, xt, out, None, both, cfg, last, clip)) / scale


def invert(net, x0, row, Tc, eps, y=None, both=False, cfg=False, clip=True):
    """(x_Tc, [z_0, ..., z_{Tc-1}]) from the draws eps = [eps_Tc, eps_{Tc-1}, ..., eps_1].  ``row(i)`` gives (the 10 weights, the network
    time) of the step that lands on index i -- for i = 0 with slot 5 = 1 and (ak, bk) = (1, 0) -- and ``row(Tc)[0][8:]`` the (alpha,
    sigma) of the start.  ``net(x, t, y)`` sees tensors of x0's dtype and device, t of shape (B,)."""
    a, s = (float(v) for v in row(Tc)[0][8:10])
    x = a * x0 + s * eps[0]
    start, maps = x, [None] * Tc
    for n, i in enumerate(reversed(range(Tc))):
        k, t_net = row(i)
        t = torch.full((x.shape[0],), float(t_net), dtype=F64, device=x.device)
        out = I.net_out(net, x, t, y, cfg).to(x.dtype)
        x, maps[i] = extract(k, x, out, x0, eps[n + 1] if i > 0 else None, both, cfg, i == 0, clip)
    return start, maps


def replay(net, x, row, maps, y=None, both=False, cfg=False, clip=True):
    """the reverse chain from index len(maps) over the given maps; the last step adds maps[0] with ``row(0)``'s slot 5 (1: the residual)"""
    for i in reversed(range(len(maps))):
        k, t_net = row(i)
        t = torch.full((x.shape[0],), float(t_net), dtype=F64, device=x.device)
        out = I.net_out(net, x, t, y, cfg).to(x.dtype)
        x = I.unknown(k, x, out, maps[i], both, cfg, i == 0, clip)
    return x


def encode_weights(l_t, l_n, l_prev=None):
    """(c1, c2, rho) of the ascending step from log-SNR l_t to l_n < l_t; l_prev = the log-SNR the step before started from"""
    _, s_t = alpha_sigma(l_t)
    a_n, s_n = alpha_sigma(l_n)
    h = 0.5 * (float(l_n) - float(l_t))
    rho = 0.0 if l_prev is None else h / (float(l_t) - float(l_prev))
    return float(s_n / s_t), float(a_n) * (1.0 - math.exp(-h)), rho


def guided_x0(k, x, out, both=False, cfg=False, clip=False):
    """the guided x0 prediction of a table row from a network output of n*(1+cfg) interleaved rows, in x's dtype"""
    a0, b0x, b0e, w = float(k[0]), float(k[1]), float(k[2]), float(k[6])
    C = x.shape[1]

    def pred(o):
        p = a0 * x + b0x * o[:, :C]
        if both:
            p = p + b0e * o[:, C:]
        return p.clamp(-1.0, 1.0) if clip else p
    if not cfg:
        return pred(out)
    pc, pu = pred(out[0::2]), pred(out[1::2])
    return pc + w * (pc - pu)


def solver_chain(net, x, table, t_net, order_of_rows, y=None, both=False, cfg=False, clip=False):
    """the solver update x <- c1 x + c2 g + c2rho (g - g_prev) over the given rows of a table, in x's dtype: ascending rows
    range(stop) of an ``encode_coefs`` table encode, descending rows of a ``solver_coefs`` table decode"""
    hist = torch.zeros_like(x)
    for i in order_of_rows:
        k = [float(v) for v in table[i]]
        t = torch.full((x.shape[0],), float(t_net[i]), dtype=F64, device=x.device)
        g = guided_x0(k, x, I.net_out(net, x, t, y, cfg).to(x.dtype), both, cfg, clip)
        x, hist = k[3] * x + k[4] * g + k[5] * (g - hist), g
    return x


def slerp(a, b, f):
    """(out, wa, wb) per sample over all other dimensions, in the dtype of a; f a float or a (B,) tensor"""
    B = a.shape[0]
    f = torch.as_tensor(f, dtype=a.dtype, device=a.device).expand(B) if not torch.is_tensor(f) else f.to(a.dtype)
    af, bf = a.reshape(B, -1), b.reshape(B, -1)
    dot, na, nb = (af * bf).sum(1), (af * af).sum(1).sqrt(), (bf * bf).sum(1).sqrt()
    ok = (na > 0) & (nb > 0)
    w = torch.acos((dot / torch.where(ok, na * nb, torch.ones_like(na))).clamp(-1.0, 1.0))
    s = torch.sin(w)
    lerp = ~ok | (s < 1e-6)
    s1 = torch.where(lerp, torch.ones_like(s), s)
    wa = torch.where(lerp, 1.0 - f, torch.sin((1.0 - f) * w) / s1)
    wb = torch.where(lerp, f, torch.sin(f * w) / s1)
    shape = (B,) + (1,) * (a.dim() - 1)
    return wa.reshape(shape) * a + wb.reshape(shape) * b, wa, wb
