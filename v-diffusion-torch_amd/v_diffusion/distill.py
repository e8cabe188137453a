"""Progressive distillation (Salimans & Ho 2022, "Progressive Distillation for Fast Sampling of Diffusion Models") on the HIP hot
path: a student with N sampling steps is trained to reach, in ONE deterministic DDIM step, where its teacher gets in TWO steps of
the 2N grid; halving repeats (``next_stage``).

For a sample at t = i/N (i = 1..N), with t' = t - 1/(2N), t'' = t - 1/N and the DDIM weights c1(s<-t) = sigma_s/sigma_t,
c2(s<-t) = alpha_s - alpha_t sigma_s/sigma_t of ``logsnr_to_posterior_ddim(eta=0)``:

    z_t   = alpha_t x_0 + sigma_t eps                x_hat  = teacher's x0 prediction at (z_t, t)
    z_t'  = c1(t'<-t) z_t + c2(t'<-t) x_hat          x_hat' = teacher's x0 prediction at (z_t', t')
    x_tilde = w1 x_hat + w2 x_hat',   w2 = c2(t''<-t') / c2(t''<-t),   w1 = 1 - w2
    loss_b  = omega_b * mean((x_student - x_tilde)^2)

The paper states the target as the quotient (z_t'' - (sigma_t''/sigma_t) z_t) / (alpha_t'' - (sigma_t''/sigma_t) alpha_t); its denominator
is c2(t''<-t), about 1e-3 of alpha at N = 1024, under a difference of nearly equal images.  Since c1(t''<-t') c1(t'<-t) = c1(t''<-t) the
z_t terms of that numerator cancel exactly, and since c1(t''<-t') c2(t'<-t) + c2(t''<-t') = c2(t''<-t) what remains is the weighted mean
above: no cancellation.  Where t'' = 0 the samplers of this package return the x0 prediction of the last step, so the target is x_hat'.

The residual x_student - x_tilde is not formed from those predictions either: at small t they all lie within 1e-3 ... 1e-5 of z_t, and
one fp32 ulp of a weight near 1 would be up to 1e-3 of it.  The kernels form every prediction a second time as its difference from
the state it was made from, (a0 - 1) z + b0x out, with a0 - 1 and c1 + c2 - 1 rounded on their own (columns 16..19), and assemble the
residual from the differences.

What runs where: the weights are per-sample fp64 host-side vector arithmetic rounded once into a (B, 20) table (``distill_coefs``);
everything per element is three fused launches (vd_distill_mid, vd_distill_loss_fwd / _bwd in csrc/diffusion.hip) around the two
teacher forwards and the student forward.  MI355X only: CPU tensors raise.
"""
import torch
import torch.nn.functional as F

from . import _hip
from .diffusion import F64, GaussianDiffusion, _need_cuda, _pred_coefs64, logsnr_to_posterior_ddim

# columns of the coefficient table (include/vdiff_hip.h, vd_distill_mid)
K = 20
(T_A0, T_B0X, T_B0E, C1, C2, U_A0, U_B0X, U_B0E, W1, W2, S_A0, S_B0X, S_B0E, OMEGA, W_GUIDE, LOGSNR_T,
 T_A0M1, U_A0M1, S_A0M1, C12M1) = range(K)


def _a0m1(model_out_type, l32):
    """a0 - 1 of ``_pred_coefs64`` without the cancellation: alpha - 1 = expm1(logsigmoid(l)/2) (v, both), 1/alpha - 1 (eps), -1 (x0)"""
    h = 0.5 * F.logsigmoid(l32.double())
    if model_out_type in ("v", "both"):
        return torch.expm1(h)
    if model_out_type == "eps":
        return torch.expm1(-h)
    if model_out_type == "x0":
        return -torch.ones_like(h)
    raise NotImplementedError(model_out_type)


def _omega(reweight_type, lt64):
    snr = torch.exp(lt64)
    if reweight_type == "constant":
        return torch.ones_like(snr)
    if reweight_type == "snr":
        return snr
    if reweight_type == "snr_trunc":
        return snr.clamp(min=1.0)
    if reweight_type == "snr_1plus":
        return 1.0 + snr
    raise NotImplementedError(reweight_type)


def _snap_up(t, N):
    """the (B,) fp64 grid index of ``t`` snapped UP to the N-step grid: the smallest i in 1..N with i/N >= t (t*N may round up past an
    integer: 7/100 * 100 > 7 stays at 7)"""
    tf = torch.as_tensor(t).reshape(-1).to(F64)
    i = torch.ceil(tf * N)
    return torch.where((i - 1) / N >= tf, i - 1, i).clamp(1, N)


def _c12m1(ls64, lt64):
    """c1 + c2 - 1 of the DDIM step s <- t in fp64, without forming c1 + c2: sigma_s/sigma_t - 1 - expm1((l_t - l_s)/2) alpha_s"""
    return torch.exp(0.5 * (F.logsigmoid(-ls64) - F.logsigmoid(-lt64))) - torch.expm1(0.5 * (lt64 - ls64)) * torch.sigmoid(ls64).sqrt() - 1.0


def distill_coefs(logsnr_fn, t, student_steps, student_out_type, teacher_out_type, reweight_type, teacher_w_guide=0.):
    """``(coef, (t, t_mid, t_end))``: the (B, 20) fp32 table of the vd_distill_* kernels (columns: the names above) and the three
    fp64 time tensors t = i/N (``t`` snapped UP to the student grid, i = 1..N), t - 1/(2N), t - 1/N.

    Pure torch on the device of ``t`` (CPU included).  ``logsnr_fn`` is called once on each of the three times, each a tensor of its
    own: a rescaling schedule rewrites its argument in place, and the returned tensors are what it left -- the times the networks are
    called with, as in ``train_loss``.  All weights are fp64 functions of the fp32-rounded log-SNRs (the values the sampler's
    coefficients are made from), rounded to fp32 once; column 15 is that fp32 logsnr(t), q_sample's argument."""
    N = int(student_steps)
    if N < 1:
        raise ValueError(f"student_steps must be >= 1, got {student_steps}")
    i = _snap_up(t, N)
    tt, tm, te = i / N, (2 * i - 1) / (2 * N), (i - 1) / N
    lt, lm, le = (logsnr_fn(v).to(torch.float32).reshape(-1) for v in (tt, tm, te))
    last = i == 1                                                      # t'' = 0: the target is the x0 prediction at t'
    c1, c2, _ = logsnr_to_posterior_ddim(lm, lt, eta=0.)
    l, m, e = lt.double(), lm.double(), le.double()
    # c1 + c2 - 1 of that step in fp64, rounded on its own: z_t' - z_t = (c1 + c2 - 1) z_t + c2 (x_hat - z_t)
    c12m1 = _c12m1(m, l)
    # c2(s<-t) = alpha_s (1 - exp((l_t - l_s)/2)); alpha_t'' divides out of the ratio
    w2 = torch.expm1(0.5 * (m - e)) / torch.expm1(0.5 * (l - e))
    w2 = torch.where(last, torch.ones_like(w2), w2).float()
    w1 = (1.0 - w2.double()).float()                                   # from the ROUNDED w2: the pair sums to 1 (exactly for w2 >= 1/2)
    ta0, tb0x, tb0e = _pred_coefs64(teacher_out_type, lt)
    ua0, ub0x, ub0e = _pred_coefs64(teacher_out_type, lm)
    sa0, sb0x, sb0e = _pred_coefs64(student_out_type, lt)
    cols = [ta0, tb0x, tb0e, c1, c2, ua0, ub0x, ub0e, w1, w2, sa0, sb0x, sb0e, _omega(reweight_type, l),
            torch.full_like(l, float(teacher_w_guide)), lt,
            _a0m1(teacher_out_type, lt), _a0m1(teacher_out_type, lm), _a0m1(student_out_type, lt), c12m1]
    return torch.stack([c.to(torch.float32) for c in cols], dim=1).contiguous(), (tt, tm, te)


class _DistillLoss(torch.autograd.Function):
    """omega * mean((x_student - x_tilde)^2) per sample with its analytic gradient wrt the student's output."""

    @staticmethod
    def forward(ctx, sout, xhat, dhat, zmid, tout, zt, coef, tmot, smot, cfg, clip, keep):
        B, C = zt.shape[:2]
        HW = zt[0, 0].numel()
        sout = sout.contiguous()
        loss = torch.empty((B,), dtype=torch.float32, device=zt.device)
        resid = torch.empty_like(zt)
        xtilde = torch.empty_like(zt) if keep is not None else None
        with torch.cuda.device(zt.device):
            _hip.distill_loss_fwd(xhat, dhat, zmid, tout, zt, sout, coef, tmot, smot, cfg, clip, loss, resid, xtilde, B, C, HW)
        if keep is not None:
            keep.last_target = xtilde
        ctx.save_for_backward(resid, coef)
        ctx.cfg = (smot, tuple(sout.shape), B, C, HW)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        resid, coef = ctx.saved_tensors
        smot, shape, B, C, HW = ctx.cfg
        dout = torch.empty(shape, dtype=torch.float32, device=resid.device)
        with torch.cuda.device(resid.device):
            _hip.distill_loss_bwd(resid, coef, gloss.to(torch.float32).contiguous(), smot, dout, B, C, HW)
        return (dout,) + (None,) * 11


class DistillationDiffusion(GaussianDiffusion):
    """A ``GaussianDiffusion`` whose ``train_loss`` is one progressive-distillation step: ``denoise_fn`` is the student (N =
    ``student_steps`` sampling steps, ``model_out_type`` its parameterisation), ``teacher_fn`` a frozen network sampled on the 2N grid
    (``teacher_out_type``, default the student's).  ``sample_timesteps = student_steps``, so the inherited samplers run the student
    at N steps; the base signature of ``train_loss`` is kept, so ``HotPathTrainer(model, DistillationDiffusion(...), timesteps=N)``,
    ``FusedAdamW`` and ``DDP(model)`` work unchanged.

    ``teacher_w_guide > 0`` (with labels) guides every teacher prediction in x-space, x_c + w (x_c - x_u), on 2B interleaved rows as
    the sampler builds them -- after the clip when ``clip_teacher`` is set, the order of ``vd_sample_step``.  The target then carries
    the guidance, so the student is sampled WITHOUT it: ``w_guide`` of this object is set to 0.  ``p_uncond`` is ignored: there is no
    label drop and ``y`` is not mutated.  The loss is omega * mean((x_student - x_tilde)^2) with omega from ``reweight_type``
    (constant: 1, snr: SNR_t, snr_trunc: max(SNR_t, 1), snr_1plus: 1 + SNR_t); ``loss_type`` is not consulted."""

    def __init__(self, teacher_fn, student_steps, *, teacher_out_type=None, teacher_w_guide=0., clip_teacher=False, **kwargs):
        if "sample_timesteps" in kwargs:
            raise TypeError("DistillationDiffusion: sample_timesteps is student_steps")
        kwargs.setdefault("loss_type", "mse")
        super().__init__(sample_timesteps=int(student_steps), **kwargs)
        if self.model_var_type == "learned":
            raise NotImplementedError("model_var_type='learned'")
        if self.x0eps_coef:
            raise NotImplementedError("x0eps_coef=True with distillation")
        self.teacher_fn = teacher_fn
        self.student_steps = int(student_steps)
        self.teacher_out_type = teacher_out_type or self.model_out_type
        self.teacher_w_guide = float(teacher_w_guide)
        self.clip_teacher = bool(clip_teacher)
        self.keep_target = False          # True: every train_loss leaves x_tilde in ``last_target`` (tests, inspection)
        self.last_target = None
        assert self.reweight_type in _hip.REWEIGHTS
        assert self.model_out_type in _hip.OUT_TYPES and self.teacher_out_type in _hip.OUT_TYPES
        if isinstance(teacher_fn, torch.nn.Module):
            teacher_fn.eval()
        if self.teacher_w_guide > 0:
            self.w_guide = 0.

    def _teacher(self, x, t, y, want):
        out = self.teacher_fn(x, t, y)
        if tuple(out.shape) != want:
            raise RuntimeError(f"the teacher's output {tuple(out.shape)} must have shape {want}")
        return out.to(torch.float32).contiguous()

    def train_loss(self, denoise_fn, x_0, t, y, noise=None):
        """Per-sample distillation loss (B,).  ``t`` is snapped up to the student grid: the smallest i/N >= t.  That is
        the "kl" branch's ceil(t N)/N except where t N rounds up past an integer in fp64 (7/100 * 100 > 7): a grid point stays where it
        is here, while the "kl" branch moves it one step up.
        ``p_uncond`` is ignored and ``y`` is left as it is: a guided teacher already folds guidance into the target."""
        _need_cuda(x_0, "train_loss")
        if getattr(self.teacher_fn, "training", False):
            raise RuntimeError("DistillationDiffusion: the teacher must be in eval mode")
        if noise is None:
            noise = torch.randn_like(x_0)
        x_0 = x_0.to(torch.float32).contiguous()
        noise = noise.to(torch.float32).contiguous()
        B, C = x_0.shape[:2]
        HW = x_0[0, 0].numel()
        coef, (tt, tm, _) = distill_coefs(self.logsnr_fn, t.to(x_0.device), self.student_steps, self.model_out_type,
                                          self.teacher_out_type, self.reweight_type, self.teacher_w_guide)
        tmot, smot = _hip.OUT_TYPES[self.teacher_out_type], _hip.OUT_TYPES[self.model_out_type]
        cfg = self.teacher_w_guide > 0 and y is not None
        z_t, xhat, dhat, zmid = (torch.empty_like(x_0) for _ in range(4))
        with torch.cuda.device(x_0.device):
            _hip.q_sample(x_0, noise, coef[:, LOGSNR_T].contiguous(), z_t, B, C, HW)
            with torch.no_grad():
                if cfg:
                    y_in = y.repeat_interleave(2, dim=0).clone()
                    y_in[1::2] = 0                                  # unconditional rows, as the sampler builds them
                    x_in, t1, t2 = z_t.repeat_interleave(2, dim=0), tt.repeat_interleave(2), tm.repeat_interleave(2)
                    zdup = torch.empty_like(x_in)
                else:
                    y_in, x_in, t1, t2, zdup = y, z_t, tt, tm, None
                twant = (x_in.shape[0], 2 * C if self.teacher_out_type == "both" else C) + tuple(x_0.shape[2:])
                out = self._teacher(x_in, t1, y_in, twant)
                _hip.distill_mid(z_t, out, coef, tmot, cfg, self.clip_teacher, xhat, dhat, zmid, zdup, B, C, HW)
                out = self._teacher(zdup if cfg else zmid, t2, y_in, twant)
        sout = denoise_fn(z_t, tt, y)
        want = (B, 2 * C if self.model_out_type == "both" else C) + tuple(x_0.shape[2:])
        if tuple(sout.shape) != want:
            raise RuntimeError(f"the student's output {tuple(sout.shape)} must have shape {want}")
        return _DistillLoss.apply(sout.to(torch.float32), xhat, dhat, zmid, out, z_t, coef, tmot, smot, cfg, self.clip_teacher,
                                  self if self.keep_target else None)

    def next_stage(self, student, **overrides):
        """The next halving: a ``DistillationDiffusion`` with N/2 steps whose teacher is a frozen copy of ``student`` (eval mode,
        no gradients) in this stage's parameterisation.  Guidance was folded into ``student`` by this stage, so the new teacher runs
        without it.  Odd N cannot be halved.  ``overrides`` replace constructor arguments (e.g. ``model_out_type`` of the new student)."""
        N = self.student_steps
        if N % 2:
            raise ValueError(f"cannot halve an odd number of sampling steps ({N})")
        net = getattr(student, "module", student)
        if hasattr(net, "detached_copy"):
            teacher = net.detached_copy()
        else:
            import copy
            teacher = copy.deepcopy(net)
        teacher.eval().requires_grad_(False)
        kw = dict(logsnr_fn=self.logsnr_fn, model_out_type=self.model_out_type, model_var_type=self.model_var_type,
                  reweight_type=self.reweight_type, loss_type=self.loss_type, intp_frac=self.intp_frac, w_guide=self.w_guide,
                  p_uncond=self.p_uncond, x0eps_coef=self.x0eps_coef, teacher_out_type=self.model_out_type, teacher_w_guide=0.,
                  clip_teacher=self.clip_teacher)
        kw.update(overrides)
        return DistillationDiffusion(teacher, kw.pop("student_steps", N // 2), **kw)
