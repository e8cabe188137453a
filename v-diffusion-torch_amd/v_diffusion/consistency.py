"""Consistency distillation (Song et al. 2023, "Consistency Models"; Luo et al. 2023, LCM) and consistency training (Song & Dhariwal
2024, "Improved Techniques for Training Consistency Models", iCT) on the HIP hot path, and multistep consistency sampling (Song et al.
2023, Algorithm 1).  Where progressive distillation (``distill.py``) halves the step count once per training run, a consistency model
learns f(z_t, t) = x_0 along the whole probability-flow trajectory in ONE run and samples in 1-4 steps.

The consistency function is the network's x0 prediction, f(z, t) = a0(t) z + b0x(t) out (+ b0e(t) out_eps): for every
parameterisation of this package it tends to z as t -> 0, and on the grid's first step the boundary condition f(z, 0) = z is imposed
outright (below).  For a sample at t = i/N (``t`` snapped UP to the grid, ``distill._snap_up``), s = (i - 1)/N:

    z_t = alpha_t x_0 + sigma_t eps
    distillation:  x_hat = the frozen teacher's (clipped, guided) x0 prediction at (z_t, t);  z_s = c1 z_t + c2 x_hat, one DDIM step
    training:      z_s = alpha_s x_0 + sigma_s eps, the SAME eps; no teacher
    target = f_target(z_s, s) under no_grad, never guided;  z_s itself where i = 1 (s = 0), SELECTED: nothing of the target
             network's output on such a row reaches loss, residual or gradient
    r = f_student(z_t, t) - target,  S_b = sum r^2,  D = C H W
    metric "l2":     loss_b = omega_b S_b / D
    metric "huber":  loss_b = omega_b (sqrt(S_b + c^2) - c) = omega_b S_b / (sqrt(S_b + c^2) + c),  c = huber_c sqrt(D)   (iCT's pseudo-Huber)

At N = 1024 and log-SNR 20 the two predictions and the two states lie within 1e-3 ... 1e-5 of each other, so -- as in ``distill.py``
and for the reason given there -- the residual is never a subtraction of nearly equal images.  Every prediction is formed as its
difference from the state it was made from, and the step between the states from weights rounded on their own:

    r = [(a0_stud - 1) z_t + b0x out_stud] - [(a0_tgt - 1) z_s + b0x out_tgt] - dz
    dz = (c1 + c2 - 1) z_t + c2 (x_hat - z_t)                          (distillation)
    dz = (alpha_s - alpha_t) x_0 + (sigma_s - sigma_t) eps             (training)

What runs where: the weights are per-sample fp64 host-side vector arithmetic rounded once into a (B, 24) table
(``consistency_coefs``); everything per element is three fused launches around the network forwards -- vd_consist_mid (distillation)
or vd_consist_pair (training: z_t, z_s and dz in one pass, in place of vd_q_sample), vd_consist_loss_fwd and vd_consist_loss_bwd in
csrc/diffusion.hip.  The target network's update e <- e + (1 - decay)(p - e) over all parameter tensors is ONE launch
(vd_ema_track_batched).  The sampler needs no kernel of its own: each step is the network call and one launch of vd_sample_step with
the row {a0, b0x, b0e, 0, alpha_next, sigma_next, w_guide, 0}, so x_next = alpha_next x_hat + sigma_next eps, and last_step = 1 at the
end.  MI355X only: CPU tensors raise.  Sample quality of consistency-trained students (FID at 1-4 steps) is unmeasured here."""
import numbers

import torch
import torch.nn.functional as F

from . import _hip
from .chain import Chain, refuse_variants
from .diffusion import F64, GaussianDiffusion, _device_ctx, _need_cuda, _pred_coefs, _pred_coefs64, logsnr_to_posterior_ddim
from .distill import _a0m1, _c12m1, _omega, _snap_up

# columns of the coefficient table (include/vdiff_hip.h, vd_consist_mid)
K = 24
(T_A0, T_B0X, T_B0E, C1, C2, G_A0, G_B0X, G_B0E, S_A0, S_B0X, S_B0E, OMEGA, W_GUIDE, LOGSNR_T, T_A0M1, G_A0M1, S_A0M1, C12M1,
 D_ALPHA, D_SIGMA, ALPHA_S, SIGMA_S, LAST, _PAD) = range(K)

METRICS = _hip.CONSIST_METRICS
HUBER_C = 0.00054                  # iCT's constant: c = 0.00054 sqrt(D)


def consistency_coefs(logsnr_fn, t, steps, student_out_type, teacher_out_type, reweight_type, teacher_w_guide=0., teacher=True):
    """``(coef, (t, s))``: the (B, 24) fp32 table of the vd_consist_* kernels (columns: the names above, documented in
    include/vdiff_hip.h) and the two fp64 time tensors t = i/N (``t`` snapped UP to the grid by ``distill_coefs``'s rule, i = 1..N) and
    s = (i - 1)/N.

    Pure torch on the device of ``t`` (CPU included).  ``logsnr_fn`` is called once on each of the two times, each a tensor of its own
    (a rescaling schedule rewrites its argument in place; the returned tensors are what it left, the times the networks are called
    with).  Every slot is an fp64 function of the fp32-rounded log-SNRs, rounded to fp32 once.  Rows with i = 1 carry (c1, c2,
    c1 + c2 - 1) = (0, 1, 0) and LAST = 1.  ``teacher=False`` (consistency training) leaves the teacher's slots 0; the target network has
    the student's parameterisation."""
    N = int(steps)
    if N < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    i = _snap_up(t, N)
    tt, ts = i / N, (i - 1) / N
    lt, ls = (logsnr_fn(v).to(torch.float32).reshape(-1) for v in (tt, ts))
    last = i == 1
    l, m = lt.double(), ls.double()
    zero, one = torch.zeros_like(l), torch.ones_like(l)
    c1, c2, _ = logsnr_to_posterior_ddim(ls, lt, eta=0.)
    c1 = torch.where(last, zero, c1.double())
    c2 = torch.where(last, one, c2.double())
    c12m1 = torch.where(last, zero, _c12m1(m, l))
    # alpha = exp(logsigmoid(l)/2), sigma = exp(logsigmoid(-l)/2): the steps between the two times as alpha_t expm1(.), not as differences
    alpha_t, sigma_t = torch.exp(0.5 * F.logsigmoid(l)), torch.exp(0.5 * F.logsigmoid(-l))
    d_alpha = alpha_t * torch.expm1(0.5 * (F.logsigmoid(m) - F.logsigmoid(l)))
    d_sigma = sigma_t * torch.expm1(0.5 * (F.logsigmoid(-m) - F.logsigmoid(-l)))
    if teacher:
        ta0, tb0x, tb0e = _pred_coefs64(teacher_out_type, lt)
        ta0m1 = _a0m1(teacher_out_type, lt)
    else:
        ta0 = tb0x = tb0e = ta0m1 = zero
    ga0, gb0x, gb0e = _pred_coefs64(student_out_type, ls)
    sa0, sb0x, sb0e = _pred_coefs64(student_out_type, lt)
    cols = [ta0, tb0x, tb0e, c1, c2, ga0, gb0x, gb0e, sa0, sb0x, sb0e, _omega(reweight_type, l),
            torch.full_like(l, float(teacher_w_guide)), lt, ta0m1, _a0m1(student_out_type, ls), _a0m1(student_out_type, lt), c12m1,
            d_alpha, d_sigma, torch.exp(0.5 * F.logsigmoid(m)), torch.exp(0.5 * F.logsigmoid(-m)), last.to(F64), zero]
    return torch.stack([c.to(torch.float32) for c in cols], dim=1).contiguous(), (tt, ts)


class _ConsistLoss(torch.autograd.Function):
    """the per-sample consistency loss with its analytic gradient wrt the student's output"""

    @staticmethod
    def forward(ctx, sout, tout, zt, zs, dz, coef, smot, metric, c, keep):
        B, C = zt.shape[:2]
        HW = zt[0, 0].numel()
        sout = sout.contiguous()
        loss, aux = (torch.empty((B,), dtype=torch.float32, device=zt.device) for _ in range(2))
        resid = torch.empty_like(zt)
        target = torch.empty_like(zt) if keep is not None else None
        with torch.cuda.device(zt.device):
            _hip.consist_loss_fwd(zt, zs, dz, sout, tout, coef, smot, metric, c, loss, resid, aux, target, B, C, HW)
        if keep is not None:
            keep.last_target = target
        ctx.save_for_backward(resid, coef, aux)
        ctx.cfg = (smot, tuple(sout.shape), B, C, HW)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        resid, coef, aux = ctx.saved_tensors
        smot, shape, B, C, HW = ctx.cfg
        dout = torch.empty(shape, dtype=torch.float32, device=resid.device)
        with torch.cuda.device(resid.device):
            _hip.consist_loss_bwd(resid, coef, gloss.to(torch.float32).contiguous(), aux, smot, dout, B, C, HW)
        return (dout,) + (None,) * 9


def _unwrap(net):
    return getattr(net, "module", net)


class ConsistencyDiffusion(GaussianDiffusion):
    """A ``GaussianDiffusion`` whose ``train_loss`` is one consistency step on the N = ``steps`` grid (module docstring): ``denoise_fn``
    is the student, ``teacher_fn`` a frozen network (``teacher_out_type``, default the student's) -- consistency DISTILLATION -- or
    None -- consistency TRAINING, no teacher forward.  ``target_fn`` is the target network: None = the student itself under
    ``no_grad`` and without dropout (decay 0, iCT's finding; a module in training mode is put in eval mode for that one forward and
    restored afterwards), else a separate module in the student's parameterisation, e.g. ``make_target(student)``, which the caller
    moves towards the student with ``update_target(student, decay)`` after each optimizer step.  ``sample_timesteps = steps``, and the
    base signature of ``train_loss`` is kept, so ``HotPathTrainer(model, cd, timesteps=N)``, ``FusedAdamW`` and ``DDP(model)`` work
    unchanged.

    ``teacher_w_guide > 0`` (with labels) guides the teacher's prediction in x-space on 2B interleaved rows, after the clip when
    ``clip_teacher`` is set, as ``DistillationDiffusion`` does; the target then carries the guidance and ``w_guide`` of this object is
    set to 0.  ``p_uncond`` is ignored and ``y`` is not mutated.  ``metric`` = "huber" (pseudo-Huber, c = ``huber_c`` sqrt(C H W),
    ``huber_c=None`` = 0.00054) or "l2"; omega from ``reweight_type``; ``loss_type`` is not consulted."""

    def __init__(self, steps, *, teacher_fn=None, target_fn=None, teacher_out_type=None, teacher_w_guide=0., clip_teacher=False,
                 metric="huber", huber_c=None, **kwargs):
        if "sample_timesteps" in kwargs:
            raise TypeError("ConsistencyDiffusion: sample_timesteps is steps")
        if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or steps < 1:
            raise ValueError(f"steps must be an integer >= 1, got {steps!r}")
        if metric not in METRICS:
            raise ValueError(f"metric must be 'l2' or 'huber', got {metric!r}")
        huber_c = HUBER_C if huber_c is None else float(huber_c)
        if not huber_c > 0:
            raise ValueError(f"huber_c must be > 0, got {huber_c!r}")
        kwargs.setdefault("loss_type", "mse")
        super().__init__(sample_timesteps=int(steps), **kwargs)
        if self.model_var_type == "learned":
            raise NotImplementedError("model_var_type='learned'")
        if self.x0eps_coef:
            raise NotImplementedError("x0eps_coef=True with consistency models")
        self.steps = int(steps)
        self.teacher_fn, self.target_fn = teacher_fn, target_fn
        self.teacher_out_type = teacher_out_type or self.model_out_type
        self.teacher_w_guide = float(teacher_w_guide)
        self.clip_teacher = bool(clip_teacher)
        self.metric, self.huber_c = metric, huber_c
        self.keep_target = False          # True: every train_loss leaves the target image in ``last_target`` (tests, inspection)
        self.last_target = None
        self._ema_tables = {}
        assert self.reweight_type in _hip.REWEIGHTS
        assert self.model_out_type in _hip.OUT_TYPES and self.teacher_out_type in _hip.OUT_TYPES
        if isinstance(teacher_fn, torch.nn.Module):
            teacher_fn.eval()
        if teacher_fn is not None and self.teacher_w_guide > 0:
            self.w_guide = 0.

    @staticmethod
    def _checked(out, want, who):
        if tuple(out.shape) != want:
            raise RuntimeError(f"the {who}'s output {tuple(out.shape)} must have shape {want}")
        return out.to(torch.float32).contiguous()

    def _target(self, denoise_fn, x, t, y, want):
        """the target network's output under no_grad and without dropout"""
        fn = denoise_fn if self.target_fn is None else self.target_fn
        net = _unwrap(fn)
        flip = isinstance(net, torch.nn.Module) and net.training
        with torch.no_grad():
            if flip:
                net.eval()
            try:
                out = (net if flip else fn)(x, t, y)
            finally:
                if flip:
                    net.train()
        return self._checked(out, want, "target network")

    def train_loss(self, denoise_fn, x_0, t, y, noise=None):
        """Per-sample consistency loss (B,).  ``t`` is snapped up to the grid, the smallest i/N >= t, by the rule of
        ``DistillationDiffusion.train_loss``.  ``p_uncond`` is ignored and ``y`` is left as it is."""
        _need_cuda(x_0, "train_loss")
        if getattr(self.teacher_fn, "training", False):
            raise RuntimeError("ConsistencyDiffusion: the teacher must be in eval mode")
        if noise is None:
            noise = torch.randn_like(x_0)
        x_0 = x_0.to(torch.float32).contiguous()
        noise = noise.to(torch.float32).contiguous()
        B, C = x_0.shape[:2]
        HW = x_0[0, 0].numel()
        distil = self.teacher_fn is not None
        coef, (tt, ts) = consistency_coefs(self.logsnr_fn, t.to(x_0.device), self.steps, self.model_out_type, self.teacher_out_type,
                                           self.reweight_type, self.teacher_w_guide, teacher=distil)
        smot = _hip.OUT_TYPES[self.model_out_type]
        want = (B, 2 * C if self.model_out_type == "both" else C) + tuple(x_0.shape[2:])
        z_t, z_s, dz = (torch.empty_like(x_0) for _ in range(3))
        with torch.cuda.device(x_0.device):
            if distil:
                tmot = _hip.OUT_TYPES[self.teacher_out_type]
                cfg = self.teacher_w_guide > 0 and y is not None
                _hip.q_sample(x_0, noise, coef[:, LOGSNR_T].contiguous(), z_t, B, C, HW)
                with torch.no_grad():
                    if cfg:
                        y_in = y.repeat_interleave(2, dim=0).clone()
                        y_in[1::2] = 0                              # unconditional rows, as the sampler builds them
                        x_in, t_in = z_t.repeat_interleave(2, dim=0), tt.repeat_interleave(2)
                    else:
                        y_in, x_in, t_in = y, z_t, tt
                    twant = (x_in.shape[0], 2 * C if self.teacher_out_type == "both" else C) + tuple(x_0.shape[2:])
                    out = self._checked(self.teacher_fn(x_in, t_in, y_in), twant, "teacher")
                    _hip.consist_mid(z_t, out, coef, tmot, cfg, self.clip_teacher, z_s, dz, None, B, C, HW)
            else:
                _hip.consist_pair(x_0, noise, coef, z_t, z_s, dz, B, C, HW)
        tout = self._target(denoise_fn, z_s, ts, y, want)
        sout = self._checked_student(denoise_fn(z_t, tt, y), want)
        c = self.huber_c * float(C * HW) ** 0.5
        return _ConsistLoss.apply(sout, tout, z_t, z_s, dz, coef, smot, METRICS[self.metric], c, self if self.keep_target else None)

    @staticmethod
    def _checked_student(sout, want):
        if tuple(sout.shape) != want:
            raise RuntimeError(f"the student's output {tuple(sout.shape)} must have shape {want}")
        return sout.to(torch.float32)

    def make_target(self, student):
        """a frozen copy of ``student`` (``DDP`` unwrapped) in compact storages of its own, eval mode, no gradients: the ``target_fn``"""
        net = _unwrap(student)
        if hasattr(net, "detached_copy"):
            target = net.detached_copy()
        else:
            import copy
            target = copy.deepcopy(net)
        return target.eval().requires_grad_(False)

    def _ema_table(self, target, student):
        """the device table of vd_ema_track_batched for this (target, student) pair, built once and rebuilt when a data pointer moved (a
        ``FusedAdamW`` flat store re-points ``.data``).  The two modules' Parameter objects are listed once per pair -- walking a UNet's
        module tree costs more host time than the launch takes on the device -- and only their data pointers are read per call."""
        key = (id(target), id(student))
        entry = self._ema_tables.get(key)
        if entry is None:
            es, ps = list(target.parameters()), list(student.parameters())
            if not es or len(es) != len(ps):
                raise ValueError("update_target: target and student must have the same, non-empty parameter list")
            entry = self._ema_tables[key] = [es, ps, None, None, 0]
        es, ps = entry[0], entry[1]
        ptrs = [t.data_ptr() for t in es + ps]
        if entry[2] != ptrs:
            rows, blocks = [], 0
            for e, p in zip(es, ps):
                if e.shape != p.shape or e.dtype != torch.float32 or p.dtype != torch.float32 or not (e.is_cuda and p.is_cuda) or \
                        e.device != p.device or not (e.is_contiguous() and p.is_contiguous()):
                    del self._ema_tables[key]
                    raise ValueError("update_target: parameters must be contiguous fp32 tensors of equal shapes on one MI355X")
                rows.append([e.data_ptr(), p.data_ptr(), e.numel(), 0, 0, 0, 0, blocks])
                blocks += (e.numel() + 255) // 256
            entry[2:] = [ptrs, torch.tensor(rows, dtype=torch.int64).to(es[0].device), blocks]
        return entry

    @torch.no_grad()
    def update_target(self, student, decay, target=None):
        """target <- target + (1 - decay) (student - target) over every parameter, in one launch.  ``target`` defaults to ``target_fn``;
        decay 0 copies, decay 1 leaves the target as it is.  Call it after the optimizer step."""
        target = _unwrap(self.target_fn if target is None else target)
        if not isinstance(target, torch.nn.Module):
            raise ValueError("update_target needs a separate target module (target_fn=None tracks the student by itself)")
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"decay must lie in [0, 1], got {decay!r}")
        net = _unwrap(student)
        es, _, _, table, blocks = self._ema_table(target, net)
        with torch.cuda.device(table.device):
            _hip.ema_track_batched(table, len(es), blocks, decay)


def consistency_schedule(T, n):
    """the n grid indices of an evenly spaced multistep consistency chain on a T-step grid, strictly descending from T:
    round(T (n - k)/n), k = 0..n-1; ``(T, 1)`` -> ``[T]``"""
    for name, v in (("T", T), ("n", n)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    if n > T:
        raise ValueError(f"n must be at most T = {T}, got {n}")
    return [(2 * T * (n - k) + n) // (2 * n) for k in range(n)]       # round-half-up of T (n - k)/n; distinct since T/n >= 1


def _indices(T, steps):
    if isinstance(steps, numbers.Integral) and not isinstance(steps, bool):
        return consistency_schedule(T, int(steps))
    idx = list(steps)
    if not idx or any(isinstance(i, bool) or not isinstance(i, numbers.Integral) for i in idx):
        raise ValueError(f"steps must be an integer or a list of grid indices, got {steps!r}")
    idx = [int(i) for i in idx]
    if idx[0] != T or idx[-1] < 1 or any(a <= b for a, b in zip(idx, idx[1:])):
        raise ValueError(f"steps must descend strictly from T = {T} and stay >= 1, got {idx}")
    return idx


def _rows(logsnr_fn, indices, T, model_out_type, w_guide):
    """the table rows in the order the chain executes them: ((8,) fp32 row, network time) one at a time (``solver._rows``)"""
    for j, i in enumerate(indices):
        nxt = indices[j + 1] if j + 1 < len(indices) else 0
        st = torch.tensor([nxt / T, i / T], dtype=F64)
        l = logsnr_fn(st)                                          # may rewrite st in place
        t_net = float(st[1])
        ls, lt32 = l[0:1].float().double(), l[1:2].float()
        a0, b0x, b0e = _pred_coefs(model_out_type, lt32[0])
        if nxt == 0:
            an, sn = 1.0, 0.0                                      # the last step returns the prediction itself (last_step = 1)
        else:
            an, sn = float(torch.exp(0.5 * F.logsigmoid(ls))), float(torch.exp(0.5 * F.logsigmoid(-ls)))
        yield torch.tensor([a0, b0x, b0e, 0.0, an, sn, float(w_guide), 0.0], dtype=F64).to(torch.float32), t_net


def consistency_sample_coefs(logsnr_fn, indices, T, model_out_type="v", w_guide=0.):
    """``(table, t_net)``: the (n, 8) fp32 rows of vd_sample_step for a multistep consistency chain over the grid indices ``indices``
    (strictly descending from T), in execution order, and the (n,) fp64 times the network is called with, index/T as ``logsnr_fn``
    left it.  Row j = {a0, b0x, b0e, 0, alpha_next, sigma_next, w_guide, 0}: a0, b0x, b0e from ``_pred_coefs`` at the fp32-rounded
    logsnr(indices[j]/T) as in ``solver_coefs``, alpha_next and sigma_next fp64 functions of the fp32-rounded logsnr(indices[j+1]/T)
    rounded once; the last row has (alpha_next, sigma_next) = (1, 0) and runs with last_step = 1.  Pure torch on the CPU."""
    indices = _indices(int(T), indices)
    rows = list(_rows(logsnr_fn, indices, int(T), model_out_type, w_guide))
    return torch.stack([r for r, _ in rows]).contiguous(), torch.tensor([t for _, t in rows], dtype=F64)


def p_sample_consistency(gd, denoise_fn, shape, noise=None, label=None, device=None, seed=None, steps=1, clip_denoised=True):
    """the chain of ``GaussianDiffusion.p_sample_consistency`` (see there); returns the final image batch on the device"""
    indices = _indices(gd.sample_timesteps, steps)
    if isinstance(clip_denoised, str):
        raise ValueError(f"clip_denoised must be True or False, got {clip_denoised!r}")
    clip, shape = bool(clip_denoised), tuple(shape)
    refuse_variants(gd, "the consistency sampler")
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    with _device_ctx(device):
        generator = None if seed is None else torch.Generator(device).manual_seed(seed)
        if noise is None:
            x_t = torch.randn(shape, device=device, generator=generator)      # the first draw: p_sample's x_T for this seed
        else:
            x_t = noise.to(device=device, dtype=torch.float32).contiguous().clone()
        ch = Chain(gd, denoise_fn, x_t, label, device)
        n = len(indices)
        with ch.fixed_weights():
            for j, (k8, t_net) in enumerate(_rows(gd.logsnr_fn, indices, gd.sample_timesteps, gd.model_out_type, gd.w_guide)):
                last = j == n - 1
                out = ch.net(t_net)
                eps = None if last else torch.randn(shape, device=device, generator=generator)    # one draw per non-final step
                _hip.sample_step(ch.x, out, eps, k8.tolist(), ch.mot, ch.cfg, last, clip, *ch.dst, ch.B, ch.C, ch.HW)
                ch.advance()
        return ch.x
