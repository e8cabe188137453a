"""Learned variances (not a test): time of the fused launches beside what they replace, in the same process, on stand-in network
outputs at 128 x 3 x 32 x 32.
  * the hybrid loss: vd_hybrid_loss_fwd + vd_hybrid_loss_bwd (two launches, no copy) against the composed path -- vd_loss_fwd /
    vd_loss_bwd on a sliced copy of the prediction channels, ATen ops under autograd for the bound term with its mean detached
    (KL rows and decoder rows), and a concatenation of the two gradients;
  * the reverse step: vd_sample_step_lv against vd_sample_step on a sliced copy + ATen ops for exp(0.5 (lvmin + delta sigmoid(nu)))
    * noise, with and without guidance.
Both versions of a pair produce the same numbers and are checked against each other before they are timed.  Every figure is taken
ROUNDS times, the versions alternating, and printed as median [min .. max]; times are device events around ITERS back-to-back calls,
so they include launch gaps the way a training step or a chain sees them.  The expectation to check is that the fused launches are
not slower than the composition.
python tests/perf_learned.py [rounds]"""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]
import torch
import v_diffusion
from v_diffusion import _hip as H

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ITERS, T, STEP, B, RES, C = 200, 50, 25, 128, 32, 3
fn = v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0)
shape, HW = (B, C, RES, RES), RES * RES


def timed(f, iters, warm=20):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v, unit, scale=1.0):
    return f"{statistics.median(v) * scale:8.2f} {unit} [{min(v) * scale:.2f} .. {max(v) * scale:.2f}]"


def report(what, a_name, fa, b_name, fb, worst):
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(fa, ITERS))
        tb.append(timed(fb, ITERS))
    print(f"{what}: {a_name} {spread(ta, 'us', 1e3)}   {b_name} {spread(tb, 'us', 1e3)}   ratio of medians "
          f"{statistics.median(ta) / statistics.median(tb):.3f}   (max relative difference {worst:.1e})", flush=True)


# ------------------------------------------------------------------------------------------------ hybrid loss, forward + backward
gd = v_diffusion.GaussianDiffusion(fn, T, "v", "learned", "snr_trunc", "hybrid", w_guide=0.0)
g = torch.Generator(dev).manual_seed(1)
t = (torch.randint(T, (B,), device=dev, generator=g) + 1).double() / T
t[0] = 1.0 / T                                                        # one decoder row
s = (t - 1.0 / T).clamp(min=0.0)
use_kl = (s != 0).float()
lt32, ls32 = fn(t).float().contiguous(), fn(s).float()
x0 = (torch.rand(shape, device=dev, generator=g) * 2 - 1)
eps = torch.randn(shape, device=dev, generator=g)
xt = torch.empty_like(x0)
H.q_sample(x0, eps, lt32, xt, B, C, HW)
out = torch.cat([torch.randn(shape, device=dev, generator=g) * 0.7, torch.randn(shape, device=dev, generator=g) * 3.0], dim=1).contiguous()
coef = gd._bpd_coefs(ls32, lt32)
gloss = torch.full((B,), 1.0 / B, device=dev)
loss, aux, dout = torch.empty(B, device=dev), torch.empty(B, 4, device=dev), torch.empty_like(out)
state = {}


def hybrid_fused():
    H.hybrid_loss_fwd(x0, eps, xt, out, lt32, coef, use_kl, 0, 2, gd.vlb_weight, loss, aux, B, C, HW)
    H.hybrid_loss_bwd(x0, eps, xt, out, lt32, coef, use_kl, aux, gloss, 0, 2, gd.vlb_weight, dout, B, C, HW)


bc = lambda v: v.reshape(-1, 1, 1, 1)
c1, c2, lvmin, delta = bc(coef[:, 3]), bc(coef[:, 4]), bc(coef[:, 5]), bc(coef[:, 6])
a0, b0x = bc(coef[:, 0]), bc(coef[:, 1])
loss_c, aux_c = torch.empty(B, device=dev), torch.empty(B, 2, device=dev)


def hybrid_composed():
    pred_c = out[:, :C].contiguous()
    dpred = torch.empty_like(pred_c)
    H.loss_fwd(x0, eps, xt, pred_c, lt32, 0, 2, loss_c, aux_c, B, C, HW)
    H.loss_bwd(x0, eps, xt, pred_c, lt32, aux_c, gloss, 0, 2, dpred, B, C, HW)
    nu = out[:, C:].detach().requires_grad_(True)
    with torch.enable_grad():
        lv = lvmin + torch.sigmoid(nu) * delta
        x0h = a0 * xt + b0x * pred_c                                   # detached: a constant to the bound term
        kl = 0.5 * (-1.0 - (lvmin - lv) + (c2 * (x0 - x0h)) ** 2 * torch.exp(-lv) + torch.exp(lvmin - lv))
        inv = torch.exp(-0.5 * lv)
        cdf = lambda z: 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))
        cu = torch.where(x0 > 0.999, torch.ones_like(x0), cdf(inv * (x0 - x0h + 1.0 / 255)))
        cl = torch.where(x0 < -0.999, torch.zeros_like(x0), cdf(inv * (x0 - x0h - 1.0 / 255)))
        nll = -torch.log(torch.clamp(cu - cl - 1e-12, min=0) + 1e-12)
        term = torch.where(use_kl != 0, kl.flatten(1).mean(1), nll.flatten(1).mean(1)) / math.log(2.0)
        (gd.vlb_weight * term * gloss).sum().backward()
    state["loss"] = loss_c + gd.vlb_weight * term.detach()
    state["dout"] = torch.cat([dpred, nu.grad], dim=1)


hybrid_fused()
hybrid_composed()
torch.cuda.synchronize()
rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
m = use_kl != 0                                                       # (a decoder row's nu gradient is ill-conditioned in fp32: not compared)
worst = max(rel(loss, state["loss"]), rel(dout[:, :C], state["dout"][:, :C]), rel(dout[m][:, C:], state["dout"][m][:, C:]))
assert worst <= 1e-3, worst
report(f"hybrid loss fwd + bwd {B} x {C} x {RES} x {RES}", "vd_hybrid_loss_fwd + _bwd", hybrid_fused, "vd_loss_* on a copy + ATen bound + cat",
       hybrid_composed, worst)

# ------------------------------------------------------------------------------------------------ reverse step
for cfg in (False, True):
    gd = v_diffusion.GaussianDiffusion(fn, T, "v", "learned", "snr_trunc", "hybrid", w_guide=1.0 if cfg else 0.0)
    k10, _ = gd._step_coefs(STEP, use_ddim=False)
    k8 = list(k10[:8])
    k8[5] = 0.0
    rows = B * (1 + cfg)
    x, noise, xn, xn2 = (torch.randn(shape, device=dev) for _ in range(4))
    out = torch.cat([torch.randn((rows, C, RES, RES), device=dev), torch.randn((rows, C, RES, RES), device=dev) * 3.0], dim=1).contiguous()
    xdup = torch.empty((2 * B,) + shape[1:], device=dev) if cfg else None

    def step_fused():
        H.sample_step_lv(x, out, noise, k10, 0, cfg, False, True, xn, xdup, B, C, HW)

    def step_composed():
        H.sample_step(x, out[:, :C].contiguous(), None, k8, 0, cfg, False, True, xn2, None, B, C, HW)
        nu = out[0::2, C:] if cfg else out[:, C:]
        nxt = xn2 + torch.exp(0.5 * (k10[5] + k10[8] * torch.sigmoid(nu))) * noise
        state["x"] = nxt
        if cfg:
            state["dup"] = nxt.repeat_interleave(2, dim=0)

    step_fused()
    step_composed()
    torch.cuda.synchronize()
    worst = rel(xn, state["x"])
    assert worst <= 1e-5 and (not cfg or torch.equal(xdup[0::2], xn)), worst
    report(f"reverse step {B} x {C} x {RES} x {RES} {'guided' if cfg else 'plain '}", "vd_sample_step_lv", step_fused, "vd_sample_step on a copy + ATen",
           step_composed, worst)
