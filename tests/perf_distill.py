"""Progressive distillation on the CIFAR config at batch 128 (not a test): ms per distillation step through HotPathTrainer, and the
glue between the three network passes -- vd_distill_mid, vd_distill_loss_fwd, vd_distill_loss_bwd -- against the same arithmetic as
tensor ops with autograd.  The second teacher forward cannot start before vd_distill_mid, so the glue sits on the critical path.
python tests/perf_distill.py [steps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "v-diffusion-torch_amd")]
import torch
import v_diffusion
from v_diffusion import _hip as H, distill as D
from v_diffusion.trainer import HotPathTrainer
from bench import build_model, CIFAR

dev = torch.device("cuda", 0)
B, RES, N = 128, 32, 4
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
fn = v_diffusion.get_logsnr_schedule("cosine", -20.0, 20.0)


def timed(f, iters=ITERS, warm=3):
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


x = torch.rand((B, 3, RES, RES), device=dev) * 2 - 1
lab = torch.randint(1, 11, (B,), device=dev).float()
teacher = build_model(dev, cfg=CIFAR).eval().requires_grad_(False)
for w in (0.0, 1.0):
    student = build_model(dev, cfg=CIFAR).train()
    dd = v_diffusion.DistillationDiffusion(teacher, N, teacher_w_guide=w, logsnr_fn=fn, model_out_type="v", model_var_type="fixed_large",
                                           reweight_type="snr_trunc")
    trainer = HotPathTrainer(student, dd, lr=2e-4, weight_decay=0.001, warmup=1000, timesteps=N)
    ms = timed(lambda: trainer.step(x, lab))
    gd = v_diffusion.GaussianDiffusion(fn, N, "v", "fixed_large", "snr_trunc", "mse", p_uncond=0.0)
    base = HotPathTrainer(build_model(dev, cfg=CIFAR).train(), gd, lr=2e-4, weight_decay=0.001, warmup=1000, timesteps=N)
    ms0 = timed(lambda: base.step(x, lab))
    print(f"distillation step, CIFAR B={B}, teacher w_guide={w}: {ms:8.2f} ms  (plain train step {ms0:.2f} ms)", flush=True)
    del trainer, base, student

# the glue alone, on stand-in network outputs
for cfg in (False, True):
    rows = B * (1 + cfg)
    t = (torch.randint(N, (B,), device=dev).double() + 1) / N
    coef, _ = D.distill_coefs(fn, t, N, "v", "v", "snr_trunc", 1.0 if cfg else 0.0)
    z, o1, o2, so = (torch.randn((n, 3, RES, RES), device=dev) for n in (B, rows, rows, B))
    xhat, dhat, zmid, resid, dout = (torch.empty_like(z) for _ in range(5))
    zdup = torch.empty_like(o1) if cfg else None
    loss, gl = torch.empty(B, device=dev), torch.full((B,), 1.0 / B, device=dev)

    def fused():
        H.distill_mid(z, o1, coef, 0, cfg, False, xhat, dhat, zmid, zdup, B, 3, RES * RES)
        H.distill_loss_fwd(None, dhat, zmid, o2, z, so, coef, 0, 0, cfg, False, loss, resid, None, B, 3, RES * RES)
        H.distill_loss_bwd(resid, coef, gl, 0, dout, B, 3, RES * RES)

    k = lambda j: coef[:, j].reshape(-1, 1, 1, 1)

    def guided(p):
        return p[0::2] + k(D.W_GUIDE) * (p[0::2] - p[1::2]) if cfg else p

    def tensor_ops():
        rep = (lambda v: v.repeat_interleave(2, dim=0)) if cfg else (lambda v: v)
        tail = rep(k(D.T_B0X)) * o1
        xh, dh = guided(rep(k(D.T_A0)) * rep(z) + tail), guided(rep(k(D.T_A0M1)) * rep(z) + tail)
        zm = k(D.C1) * z + k(D.C2) * xh
        zin = rep(zm)                                              # the next teacher input
        dp = guided(rep(k(D.U_A0M1)) * zin + rep(k(D.U_B0X)) * o2)
        dt = k(D.W1) * dh + k(D.W2) * (dp + k(D.C12M1) * z + k(D.C2) * dh)
        s = so.detach().requires_grad_(True)
        ls = coef[:, D.OMEGA] * ((k(D.S_A0M1) * z + k(D.S_B0X) * s - dt) ** 2).flatten(1).mean(1)
        ls.backward(gl)
        return s.grad

    a, b = timed(fused, 50), timed(tensor_ops, 50)
    print(f"glue, {'guided' if cfg else 'plain '} teacher: fused {a * 1e3:7.1f} us (3 launches)   tensor ops {b * 1e3:7.1f} us", flush=True)
