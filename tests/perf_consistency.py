"""Consistency distillation / training at 128 x 3 x 32 x 32 (not a test): the launches around the network calls -- vd_consist_mid
(distillation) or vd_consist_pair (training), vd_consist_loss_fwd, vd_consist_loss_bwd -- against the fp32 ATen composition of the
same arithmetic with autograd, and vd_ema_track_batched on the CIFAR UNet's parameter set against the same expression as per-tensor
ATen ops and against torch._foreach_lerp_.  The two sides of each comparison alternate inside one run; each figure is the median of
ROUNDS windows of ITERS calls (device events), with the smallest and largest window beside it.
python tests/perf_consistency.py [iters]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]
import torch
import v_diffusion
from v_diffusion import _hip as H, consistency as D
from bench import build_model, CIFAR

dev = torch.device("cuda", 0)
B, RES, N = 128, 32, 1024
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROUNDS = 7
fn = v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0)


def window(f, iters=ITERS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                       # us per call


def compare(label, **sides):
    for f in sides.values():                                      # warm-up: code objects, allocator
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, f in sides.items():                                 # alternate
            us[k].append(window(f))
    print(label + ":  " + "   ".join(f"{k} {statistics.median(v):8.1f} us [{min(v):.1f} .. {max(v):.1f}]" for k, v in us.items()), flush=True)


HW = RES * RES
gl = torch.full((B,), 1.0 / B, device=dev)
x0, eps, so, go = (torch.randn((B, 3, RES, RES), device=dev) for _ in range(4))
for mode, cfg in (("distillation, plain teacher ", False), ("distillation, guided teacher", True), ("training", False)):
    distil = mode != "training"
    rows = B * (1 + cfg)
    t = (torch.randint(N, (B,), device=dev).double() + 1) / N
    coef, _ = D.consistency_coefs(fn, t, N, "v", "v", "snr_trunc", 1.0 if cfg else 0.0, teacher=distil)
    o1 = torch.randn((rows, 3, RES, RES), device=dev)
    zt, zs, dz, resid, dout = (torch.empty_like(x0) for _ in range(5))
    loss, aux = torch.empty(B, device=dev), torch.empty(B, device=dev)
    H.q_sample(x0, eps, coef[:, D.LOGSNR_T].contiguous(), zt, B, 3, HW)
    c = D.HUBER_C * (3 * HW) ** 0.5

    def fused():
        if distil:
            H.consist_mid(zt, o1, coef, 0, cfg, False, zs, dz, None, B, 3, HW)
        else:
            H.consist_pair(x0, eps, coef, zt, zs, dz, B, 3, HW)
        H.consist_loss_fwd(zt, zs, dz, so, go, coef, 0, 1, c, loss, resid, aux, None, B, 3, HW)
        H.consist_loss_bwd(resid, coef, gl, aux, 0, dout, B, 3, HW)

    k = lambda j: coef[:, j].reshape(-1, 1, 1, 1)
    last = k(D.LAST) != 0

    def tensor_ops():
        if distil:
            rep = (lambda v: v.repeat_interleave(2, dim=0)) if cfg else (lambda v: v)
            tail = rep(k(D.T_B0X)) * o1
            p, d = rep(k(D.T_A0)) * rep(zt) + tail, rep(k(D.T_A0M1)) * rep(zt) + tail
            if cfg:
                p, d = p[0::2] + k(D.W_GUIDE) * (p[0::2] - p[1::2]), d[0::2] + k(D.W_GUIDE) * (d[0::2] - d[1::2])
            z_t = zt
            z_s = torch.where(last, p, k(D.C1) * zt + k(D.C2) * p)
            dzz = torch.where(last, d, k(D.C12M1) * zt + k(D.C2) * d)
        else:
            l = k(D.LOGSNR_T)
            z_t = x0 * torch.sigmoid(l).sqrt() + eps * torch.sigmoid(-l).sqrt()
            z_s = k(D.ALPHA_S) * x0 + k(D.SIGMA_S) * eps
            dzz = k(D.D_ALPHA) * x0 + k(D.D_SIGMA) * eps
        dt = torch.where(last, torch.zeros_like(z_s), k(D.G_A0M1) * z_s + k(D.G_B0X) * go)
        s = so.detach().requires_grad_(True)
        S = (((k(D.S_A0M1) * z_t + k(D.S_B0X) * s - dt) - dzz) ** 2).flatten(1).sum(1)
        ls = coef[:, D.OMEGA] * S / (torch.sqrt(S + c * c) + c)
        ls.backward(gl)
        return s.grad

    compare(f"glue, {mode}", fused=fused, tensor_ops=tensor_ops)

# the target network's update over the CIFAR UNet's parameter set
student = build_model(dev, cfg=CIFAR)
cd = v_diffusion.ConsistencyDiffusion(N, logsnr_fn=fn, model_out_type="v", model_var_type="fixed_large", reweight_type="snr_trunc")
target = cd.make_target(student)
es, ps = [e.data for e in target.parameters()], [p.data for p in student.parameters()]
decay = 0.999
numel = sum(p.numel() for p in ps)
print(f"target update: {len(ps)} tensors, {numel} parameters ({numel * 4 / 2 ** 20:.1f} MiB each side)")


def per_tensor():
    for e, p in zip(es, ps):
        e.add_((1 - decay) * (p - e))


compare("target update", batched=lambda: cd.update_target(student, decay, target=target), per_tensor_aten=per_tensor,
        foreach_lerp=lambda: torch._foreach_lerp_(es, ps, 1 - decay))
