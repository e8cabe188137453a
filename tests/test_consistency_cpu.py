"""Host side of consistency distillation / training and multistep consistency sampling (v_diffusion/consistency.py): the per-sample
coefficient table, the sampler's rows and the index schedule against the float64 restatement of tests/consist_ref.py and against
identities; the order of the objective itself on Gaussian data, where everything is known in closed form; the public names; and
every refusal that needs no GPU.  No kernel is launched here."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consist_ref as R                                           # noqa: E402

STEPS = (1, 2, 4, 1024)
SCHEDULES = ("cosine", "linear")
REWEIGHTS = ("constant", "snr", "snr_trunc", "snr_1plus")
NEW_NAMES = ("ConsistencyDiffusion", "consistency_coefs", "consistency_sample_coefs", "consistency_schedule")


def _ulp32(x):
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _table(schedule, N, reweight="constant", s="v", te="v", w=0.0, rescale=False, teacher=True):
    import v_diffusion as vd
    from v_diffusion import consistency
    fn = vd.get_logsnr_schedule(schedule, -20.0, 20.0, rescale=rescale)
    t = torch.arange(1, N + 1, dtype=torch.float64) / N            # every grid point
    coef, times = consistency.consistency_coefs(fn, t, N, s, te, reweight, w, teacher=teacher)
    return consistency, fn, t, coef, times


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("N", STEPS)
def test_step_weights(schedule, N):
    import v_diffusion as vd
    from v_diffusion.diffusion import logsnr_to_posterior_ddim
    D, _, t, coef, (tt, ts) = _table(schedule, N)
    assert coef.shape == (N, D.K) and coef.dtype == torch.float32
    i = torch.arange(1, N + 1, dtype=torch.float64)
    assert torch.equal(tt, i / N) and torch.equal(ts, (i - 1) / N)
    fn = vd.get_logsnr_schedule(schedule, -20.0, 20.0)
    l, ls = (fn(v.clone()).float().double() for v in (tt, ts))
    assert torch.equal(coef[:, D.LOGSNR_T].double(), l)
    # i = 1: z_0 is the teacher's prediction itself, (c1, c2, c1 + c2 - 1) = (0, 1, 0), and the row is flagged
    assert coef[0, [D.C1, D.C2, D.C12M1]].tolist() == [0.0, 1.0, 0.0]
    assert coef[:, D.LAST].tolist() == [1.0] + [0.0] * (N - 1)
    # elsewhere the DDIM step s <- t is the package's own (what the sampler multiplies with), and agrees with first principles
    c1, c2, _ = logsnr_to_posterior_ddim(ls.float(), l.float(), eta=0.)
    assert torch.equal(coef[1:, D.C1], c1[1:]) and torch.equal(coef[1:, D.C2], c2[1:])
    a_t, s_t = R.alpha_sigma(l)
    a_s, s_s = R.alpha_sigma(ls)
    # c1 + c2 - 1 = z_s - z_t for x_hat = z_t = 1: against the plain fp64 expression, whose cancellation costs ~1e-16 absolute
    ref = s_s / s_t + (a_s - a_t * s_s / s_t) - 1.0
    err = (coef[1:, D.C12M1].double() - ref[1:]).abs()
    assert bool((err <= _ulp32(ref[1:]) + 4e-16).all())
    # the steps of the training mode and the levels at s, each within half an fp32 ulp of first principles (+ the fp64 cancellation)
    for c, want in ((D.D_ALPHA, a_s - a_t), (D.D_SIGMA, s_s - s_t), (D.ALPHA_S, a_s), (D.SIGMA_S, s_s)):
        err = (coef[:, c].double() - want).abs()
        assert bool((err <= _ulp32(want) + 4e-16).all()), c


@pytest.mark.parametrize("teacher", (True, False), ids=("distillation", "training"))
@pytest.mark.parametrize("types", (("v", "v"), ("eps", "v"), ("both", "x0"), ("x0", "eps")))
def test_prediction_slots_are_pred_coefs64(types, teacher):
    """the three prediction triples are ``_pred_coefs64``'s (student at t, target = the student's parameterisation at s, teacher at t),
    their a0 - 1 slots ``distill._a0m1``'s, and they convert an output as the restatement does"""
    from v_diffusion.diffusion import _pred_coefs64
    from v_diffusion.distill import _a0m1
    s, te = types
    N = 4
    D, fn, _, coef, (tt, ts) = _table("cosine", N, s=s, te=te, w=1.5, teacher=teacher)
    assert bool((coef[:, D.W_GUIDE] == 1.5).all())
    l32, ls32 = fn(tt.clone()).float(), fn(ts.clone()).float()
    triples = [(s, l32, (D.S_A0, D.S_B0X, D.S_B0E), D.S_A0M1), (s, ls32, (D.G_A0, D.G_B0X, D.G_B0E), D.G_A0M1)]
    if teacher:
        triples.append((te, l32, (D.T_A0, D.T_B0X, D.T_B0E), D.T_A0M1))
    else:
        assert bool((coef[:, [D.T_A0, D.T_B0X, D.T_B0E, D.T_A0M1]] == 0).all())
    g = torch.Generator().manual_seed(5)
    z = torch.randn(N, 3, 2, 2, generator=g, dtype=torch.float64)
    for mot, lx, cols, m1 in triples:
        for c, want in zip(cols, _pred_coefs64(mot, lx)):
            assert torch.equal(coef[:, c], want.float())
        assert torch.equal(coef[:, m1], _a0m1(mot, lx).float())
        out = torch.randn(N, 6 if mot == "both" else 3, 2, 2, generator=g, dtype=torch.float64)
        a0, b0x, b0e = (R.col(coef[:, c]) for c in cols)
        got = a0 * z + b0x * out[:, :3] + (b0e * out[:, 3:] if mot == "both" else 0.0)
        ref = R.x0_from_out(out, z, R.col(lx.double()), mot)
        scale = (a0.abs() * z.abs() + b0x.abs() * out[:, :3].abs()).amax(dim=(1, 2, 3), keepdim=True)
        assert bool(((got - ref).abs() <= 2 * 2.0 ** -24 * scale).all())
        # the difference form: (a0 - 1) z + b0x out is the prediction minus z
        dif = R.col(coef[:, m1]) * z + b0x * out[:, :3] + (b0e * out[:, 3:] if mot == "both" else 0.0)
        assert bool(((dif - (ref - z)).abs() <= 2 * 2.0 ** -24 * scale).all())


@pytest.mark.parametrize("reweight", REWEIGHTS)
def test_omega_matches_each_reweight_type(reweight):
    for N in STEPS:
        D, _, _, coef, _ = _table("cosine", N, reweight=reweight)
        assert torch.equal(coef[:, D.OMEGA], R.omega(reweight, coef[:, D.LOGSNR_T].double()).float())


@pytest.mark.parametrize("N", STEPS)
def test_snapping_is_distill_coefs_rule(N):
    from v_diffusion import distill
    D, fn, _, _, _ = _table("cosine", N)
    t = torch.tensor([0.0, 1e-9, 0.3, 0.5, 0.999, 1.0], dtype=torch.float64)
    _, (tt, ts) = D.consistency_coefs(fn, t, N, "v", "v", "constant")
    _, (td, _, te) = distill.distill_coefs(fn, t, N, "v", "v", "constant")
    assert torch.equal(tt, td) and torch.equal(ts, te)
    assert (tt * N).round().long().tolist() == R.snap_up(t, N)
    for n in (10, 100, 1000):                                       # (7/100*100 > 7 in fp64: ceil alone would move it to 8/100)
        g = torch.arange(1, n + 1, dtype=torch.float64) / n
        _, (tg, sg) = D.consistency_coefs(fn, g, n, "v", "v", "constant")
        assert torch.equal(tg, g) and torch.equal(sg, (torch.arange(1, n + 1, dtype=torch.float64) - 1) / n)
    _, (t7, _) = D.consistency_coefs(fn, torch.tensor([7 / 100], dtype=torch.float64), 100, "v", "v", "constant")
    assert float(t7) == 7 / 100
    with pytest.raises(ValueError, match="steps"):
        D.consistency_coefs(fn, t, 0, "v", "v", "constant")


def test_rescaling_schedule_hands_the_networks_the_rewritten_times():
    import v_diffusion as vd
    N = 4
    D, fn, t, coef, (tt, ts) = _table("cosine", N, rescale=True)
    i = torch.arange(1, N + 1, dtype=torch.float64)
    for got, grid in ((tt, i / N), (ts, (i - 1) / N)):
        want = grid.clone()
        vd.get_logsnr_schedule("cosine", -20.0, 20.0, rescale=True)(want)          # rewrites ``want`` in place
        assert torch.equal(got, want) and not torch.equal(got, grid)
    assert torch.equal(t, i / N)                                                     # the caller's tensor is not touched
    assert torch.equal(coef, _table("cosine", N)[3])                                 # the weights are those of the grid times


@pytest.mark.parametrize("T,n", ((1024, 1), (1024, 2), (1024, 4), (1000, 3), (7, 7), (7, 5), (5, 1), (1, 1)))
def test_schedule(T, n):
    import v_diffusion as vd
    idx = vd.consistency_schedule(T, n)
    assert idx == R.schedule(T, n)
    assert idx[0] == T and len(idx) == n and all(a > b for a, b in zip(idx, idx[1:])) and idx[-1] >= 1
    if n == 1:
        assert idx == [T]


@pytest.mark.parametrize("out_type", ("v", "eps", "x0", "both"))
def test_sample_rows(out_type):
    import v_diffusion as vd
    from v_diffusion.solver import solver_coefs
    T, idx = 8, [8, 5, 2, 1]
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    table, t_net = vd.consistency_sample_coefs(fn, idx, T, out_type, 1.5)
    assert table.shape == (4, 8) and table.dtype == torch.float32 and t_net.tolist() == [i / T for i in idx]
    lt = [float(fn(torch.tensor([i / T], dtype=torch.float64)).float()) for i in idx]
    rows = R.sample_rows(lt, lt[1:] + [None], out_type)
    for j, row in enumerate(rows):
        got = table[j, [0, 1, 2, 4, 5]].double()
        want = torch.tensor(row, dtype=torch.float64)
        assert bool(((got - want).abs() <= 4 * _ulp32(want)).all()), (j, got, want)        # a0.. are fp32 evaluations (solver_coefs' rule)
        assert table[j, [3, 6, 7]].tolist() == [0.0, 1.5, 0.0]
    assert table[-1, [4, 5]].tolist() == [1.0, 0.0]
    # the prediction slots are solver_coefs' on the same grid, bit for bit
    full, _ = solver_coefs(fn, T, 1, "time", out_type, 1.5)
    for j, i in enumerate(idx):
        assert torch.equal(table[j, :3], full[i - 1, :3])
    # alpha_next, sigma_next: fp64 from the fp32-rounded log-SNR, rounded once
    for j in range(3):
        a, s = R.alpha_sigma(torch.tensor(lt[j + 1], dtype=torch.float64))
        assert table[j, 4] == a.float() and table[j, 5] == s.float()
    # int and list forms
    a, _ = vd.consistency_sample_coefs(fn, 2, T, out_type)
    b, _ = vd.consistency_sample_coefs(fn, [8, 4], T, out_type)
    assert torch.equal(a, b)
    for bad in ([7, 3], [8, 8], [8, 3, 5], [8, 0], [], 9, 0, [8, 2.5]):
        with pytest.raises(ValueError):
            vd.consistency_sample_coefs(fn, bad, T, out_type)


# ---- the objective itself on Gaussian data x_0 ~ N(0, I/4), cosine schedule on [-6, 6]: exact denoiser as teacher, student = target =
# the exact consistency function f(z, t) = z std_0/std_t.  Everything is linear in z_t, so the RMS residual at step i is known in
# closed form: std_t |f_t - (c1 + c2 k_t) f_s|, k_t the exact denoiser's factor.
def _gauss(N):
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -6.0, 6.0)
    i = torch.arange(1, N + 1, dtype=torch.float64)
    l, ls, l0 = fn(i / N).double(), fn((i - 1) / N).double(), fn(torch.zeros(1, dtype=torch.float64)).double()
    return l, ls, l0


def test_distillation_residual_is_second_order_in_the_step():
    """one DDIM step has local error O(h^2): the RMS residual over all i falls by 4 per doubling of N (asserted: a factor in
    [3.5, 4.5], N = 8 ... 128).  The step to s = 0 is the plain DDIM step here: the package's i = 1 convention (z_0 = the teacher's
    prediction, what its samplers return) replaces that one row by a term that does not shrink with N at logsnr_max = 6 -- it is
    alpha_0-dependent, 1e-9 at the package's default logsnr_max = 20 -- and is no part of the order statement (FINDINGS.md)."""
    rms = []
    for N in (8, 16, 32, 64, 128):
        l, ls, l0 = _gauss(N)
        z = torch.ones(N, 1, 1, 1, dtype=torch.float64)                    # unit state: the residual per unit of z_t
        k = R.col(R.gaussian_denoiser(l))
        i = torch.arange(1, N + 1, dtype=torch.float64)
        teacher = lambda x, t, y: k * x                                   # noqa: E731  an x0-network: the exact denoiser
        zs = R.z_down(teacher, z, None, None, (i / N, (i - 1) / N), (l, ls), None, "x0", last_is_x0=False)
        f_t, f_s = R.col(R.gaussian_consistency(l, l0)), R.col(R.gaussian_consistency(ls, l0))
        r = (f_t * z - f_s * zs).reshape(-1) * R.gaussian_std(l)           # times the RMS of z_t
        assert abs(float(f_s[0]) - 1.0) < 1e-15                            # boundary condition: f(z, 0) = z
        rms.append(float((r * r).mean().sqrt()))
    ratios = [a / b for a, b in zip(rms, rms[1:])]
    print("[consistency order] rms", ["%.3e" % v for v in rms], "ratios", ["%.2f" % v for v in ratios])
    assert all(3.5 <= q <= 4.5 for q in ratios), ratios
    assert rms[0] == pytest.approx(1.364e-2, rel=2e-3) and rms[-1] == pytest.approx(5.420e-5, rel=2e-3)


def test_training_residual_is_unbiased_for_the_distillation_residual():
    """consistency training replaces the teacher's step by alpha_s x_0 + sigma_s eps with the same eps: E[z_s | z_t] is the exact
    denoiser's DDIM step, so with the (linear) exact consistency function the training residual minus the distillation residual has
    zero mean given z_t.  Shown by Monte Carlo over M = 200000 draws per step at N = 16: the mean of the difference d and of its
    projection d z_t / std_t are each within 5 standard errors (sd / sqrt(M), sd estimated from the sample) of 0; with 32 checks a
    false alarm has probability < 2e-5.  The difference itself is not small: its sd is asserted to exceed 100 standard errors."""
    N, M = 16, 200000
    l, ls, l0 = _gauss(N)
    g = torch.Generator().manual_seed(17)
    for j in range(N):
        lt, lss = l[j:j + 1], ls[j:j + 1]
        x0 = 0.5 * torch.randn(M, generator=g, dtype=torch.float64)
        eps = torch.randn(M, generator=g, dtype=torch.float64)
        a_t, s_t = R.alpha_sigma(lt)
        z = (a_t * x0 + s_t * eps).reshape(M, 1, 1, 1)
        times = (torch.full((M,), (j + 1) / N, dtype=torch.float64), torch.full((M,), j / N, dtype=torch.float64))
        logs = (lt.expand(M), lss.expand(M))
        k = R.gaussian_denoiser(lt)
        zs_d = R.z_down(lambda x, t, y: k * x, z, None, None, times, logs, None, "x0", last_is_x0=False)
        zs_t = R.z_down(None, z, x0.reshape(M, 1, 1, 1), eps.reshape(M, 1, 1, 1), times, logs, None, "x0")
        f_s = R.gaussian_consistency(lss, l0)
        d = (f_s * (zs_d - zs_t)).reshape(-1)                              # r_train - r_distill: the student's term cancels
        se = float(d.std()) / math.sqrt(M)
        proj = d * z.reshape(-1) / R.gaussian_std(lt)
        assert float(d.std()) > 100 * se
        assert abs(float(d.mean())) <= 5 * se, (j, float(d.mean()), se)
        assert abs(float(proj.mean())) <= 5 * float(proj.std()) / math.sqrt(M), (j, float(proj.mean()))


def test_entry_points_are_declared_and_bound():
    """(declarations and ctypes signatures of the entry points: tests/test_host_cpu.py pins the whole C ABI)"""
    import v_diffusion as vd
    from v_diffusion import _hip
    for fn in ("consist_mid", "consist_pair", "consist_loss_fwd", "consist_loss_bwd", "ema_track_batched"):
        assert callable(getattr(_hip, fn))
    for name in NEW_NAMES:
        assert name in vd.__all__ and hasattr(vd, name)
    assert callable(vd.GaussianDiffusion.p_sample_consistency)
    assert vd.DistillationDiffusion.p_sample_consistency is vd.GaussianDiffusion.p_sample_consistency
    assert issubclass(vd.ConsistencyDiffusion, vd.GaussianDiffusion)


def _kw(**over):
    import v_diffusion as vd
    kw = dict(logsnr_fn=vd.get_logsnr_schedule("cosine", -20.0, 20.0), model_out_type="v", model_var_type="fixed_large",
              reweight_type="snr_trunc")
    kw.update(over)
    return kw


def test_constructor_and_train_loss_refusals():
    import v_diffusion as vd
    teacher = torch.nn.Linear(2, 2)
    cd = vd.ConsistencyDiffusion(4, teacher_fn=teacher, teacher_out_type="eps", teacher_w_guide=2.0, w_guide=0.3, p_uncond=0.2, **_kw())
    assert not teacher.training and cd.w_guide == 0.0 and cd.teacher_w_guide == 2.0    # a guided teacher's student samples unguided
    assert cd.sample_timesteps == cd.steps == 4 and cd.loss_type == "mse" and cd.metric == "huber" and cd.huber_c == 0.00054
    assert cd.keep_target is False and cd.last_target is None
    ct = vd.ConsistencyDiffusion(4, w_guide=0.3, teacher_w_guide=2.0, **_kw())
    assert ct.teacher_fn is None and ct.target_fn is None and ct.w_guide == 0.3        # no teacher: nothing folds guidance in
    with pytest.raises(NotImplementedError, match="learned"):
        vd.ConsistencyDiffusion(4, **_kw(model_var_type="learned"))
    with pytest.raises(NotImplementedError, match="x0eps_coef"):
        vd.ConsistencyDiffusion(4, x0eps_coef=True, **_kw())
    for bad in ("l1", "lpips", None):
        with pytest.raises(ValueError, match="metric"):
            vd.ConsistencyDiffusion(4, metric=bad, **_kw())
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="huber_c"):
            vd.ConsistencyDiffusion(4, huber_c=bad, **_kw())
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="steps"):
            vd.ConsistencyDiffusion(bad, **_kw())
    with pytest.raises(TypeError):
        vd.ConsistencyDiffusion(4, sample_timesteps=8, **_kw())
    t = torch.tensor([0.25, 1.0], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="MI355X"):                                  # no CPU path, like the rest of the package
        ct.train_loss(torch.nn.Identity(), torch.zeros(2, 3, 4, 4), t, None)
    with pytest.raises(ValueError, match="decay"):
        ct.update_target(torch.nn.Linear(2, 2), 1.5, target=torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="target"):
        ct.update_target(torch.nn.Linear(2, 2), 0.5)                                    # target_fn=None: there is nothing to move
    with pytest.raises(ValueError, match="parameter"):
        ct.update_target(torch.nn.Linear(2, 2), 0.5, target=torch.nn.Identity())


def test_make_target_is_a_frozen_compact_copy():
    import v_diffusion as vd
    ct = vd.ConsistencyDiffusion(4, **_kw())
    student = torch.nn.Linear(2, 2)
    wrapped = torch.nn.Sequential()
    wrapped.module = student                                                            # what DDP looks like from outside
    for s in (student, wrapped):
        tgt = ct.make_target(s)
        assert tgt is not student and not tgt.training and all(not p.requires_grad for p in tgt.parameters())
        assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(tgt.parameters(), student.parameters()))
    assert student.training and all(p.requires_grad for p in student.parameters())


def test_sampler_refusals():
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    net = lambda x, t, y: x                                                             # noqa: E731
    shape = (1, 3, 2, 2)
    gd = vd.GaussianDiffusion(fn, 8, "v", "fixed_large", "constant", "mse", w_guide=0.0)
    for bad in (9, 0, [7, 1], [8, 8, 1], [8, 9], [], True, "2", [8, 2.0]):
        with pytest.raises((ValueError, TypeError)):
            gd.p_sample_consistency(net, shape, steps=bad, device="cuda")
    with pytest.raises(ValueError, match="clip_denoised"):
        gd.p_sample_consistency(net, shape, steps=2, clip_denoised="dynamic", device="cuda")
    with pytest.raises(NotImplementedError, match="learned"):
        vd.GaussianDiffusion(fn, 8, "v", "learned", "constant", "mse").p_sample_consistency(net, shape, device="cuda")
    with pytest.raises(NotImplementedError, match="x0eps_coef"):
        vd.GaussianDiffusion(fn, 8, "v", "fixed_large", "constant", "mse", x0eps_coef=True).p_sample_consistency(net, shape, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample_consistency(net, shape, device="cpu")
