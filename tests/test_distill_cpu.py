"""Host side of progressive distillation (v_diffusion/distill.py): the per-sample coefficient table against the float64 restatement of
tests/distill_ref.py, the handling of a rescaling schedule, next_stage's refusal of odd step counts, and the launch wrappers' presence.
No kernel is launched here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distill_ref as R                                           # noqa: E402

STEPS = (1, 2, 4, 1024)
SCHEDULES = ("cosine", "linear")


def _ulp32(x):
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _table(schedule, N, reweight="constant", s="v", te="v", w=0.0, rescale=False):
    import v_diffusion as vd
    from v_diffusion import distill
    fn = vd.get_logsnr_schedule(schedule, -20.0, 20.0, rescale=rescale)
    t = torch.arange(1, N + 1, dtype=torch.float64) / N            # every grid point
    coef, times = distill.distill_coefs(fn, t, N, s, te, reweight, w)
    return distill, fn, t, coef, times


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("N", STEPS)
def test_target_weights(schedule, N):
    import v_diffusion as vd
    D, _, t, coef, (tt, tm, te) = _table(schedule, N)
    assert coef.shape == (N, D.K) and coef.dtype == torch.float32
    i = torch.arange(1, N + 1, dtype=torch.float64)
    assert torch.equal(tt, i / N) and torch.equal(tm, (2 * i - 1) / (2 * N)) and torch.equal(te, (i - 1) / N)
    w1, w2 = coef[:, D.W1].double(), coef[:, D.W2].double()
    assert bool(((w1 + w2 - 1.0).abs() <= _ulp32(torch.ones(()))).all())            # w1 + w2 = 1 to 1 fp32 ulp
    assert float(coef[0, D.W1]) == 0.0 and float(coef[0, D.W2]) == 1.0              # i = 1: the target is x_hat'
    assert bool((w2 > 0).all()) and bool((w2 <= 1).all())
    # the quotient restatement, from the same fp32-rounded log-SNRs (a plain schedule leaves its argument alone)
    fn = vd.get_logsnr_schedule(schedule, -20.0, 20.0)
    l, lm, le = (fn(v.clone()).float().double() for v in (tt, tm, te))
    assert torch.equal(coef[:, D.LOGSNR_T].double(), l)
    ref = R.w2_quotient(l, lm, le)[1:]
    err = (w2[1:] - ref).abs()
    assert bool((err <= 2 * _ulp32(ref)).all()), float((err / _ulp32(ref)).max()) if N > 1 else 0.0
    # the DDIM step t' <- t of the table is the package's own (what the sampler multiplies with), and agrees with first principles
    from v_diffusion.diffusion import logsnr_to_posterior_ddim
    c1, c2, _ = logsnr_to_posterior_ddim(lm.float(), l.float(), eta=0.)
    assert torch.equal(coef[:, D.C1], c1) and torch.equal(coef[:, D.C2], c2)
    assert bool(((coef[:, D.C2].double() - R.c2(lm, l)).abs() <= _ulp32(R.c2(lm, l))).all())


@pytest.mark.parametrize("N", STEPS)
def test_times_are_snapped_up_to_the_student_grid(N):
    D, fn, _, _, _ = _table("cosine", N)
    t = torch.tensor([0.0, 1e-9, 0.3, 0.5, 0.999, 1.0], dtype=torch.float64)
    _, (tt, _, _) = D.distill_coefs(fn, t, N, "v", "v", "constant")
    i = tt * N
    assert torch.equal(i, i.round()) and bool((i >= 1).all()) and bool((i <= N).all())
    assert bool((tt >= t).all()) and bool((((i - 1) / N < t) | (i == 1)).all())           # the smallest such grid point
    grid = torch.arange(1, N + 1, dtype=torch.float64) / N          # a grid point stays where it is, whatever t*N rounds to
    _, (tg, _, _) = D.distill_coefs(fn, grid, N, "v", "v", "constant")
    assert torch.equal(tg, grid)
    for n in (10, 100, 1000):                                       # (7/100*100 > 7 in fp64: ceil alone would move it to 8/100)
        g = torch.arange(1, n + 1, dtype=torch.float64) / n
        _, (tg, _, _) = D.distill_coefs(fn, g, n, "v", "v", "constant")
        assert torch.equal(tg, g)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("reweight", ("constant", "snr", "snr_trunc", "snr_1plus"))
def test_omega_matches_each_reweight_type(schedule, reweight):
    for N in STEPS:
        D, _, _, coef, _ = _table(schedule, N, reweight=reweight)
        l = coef[:, D.LOGSNR_T].double()
        ref = R.omega(reweight, l)
        assert torch.equal(coef[:, D.OMEGA], ref.float())
        if reweight == "snr_trunc":
            assert float(coef[:, D.OMEGA].min()) >= 1.0
        if reweight == "constant":
            assert bool((coef[:, D.OMEGA] == 1).all())


@pytest.mark.parametrize("types", (("v", "v"), ("eps", "v"), ("both", "x0"), ("x0", "eps")))
def test_prediction_weights_match_first_principles(types):
    """x0_hat = a0*z + b0x*out (+ b0e*out_eps) with the table's weights is the restatement's conversion, for student and teacher"""
    s, te = types
    D, _, _, coef, _ = _table("cosine", 4, s=s, te=te, w=1.5)
    assert bool((coef[:, D.W_GUIDE] == 1.5).all())
    fn = __import__("v_diffusion").get_logsnr_schedule("cosine", -20.0, 20.0)
    i = torch.arange(1, 5, dtype=torch.float64)
    l, lm = fn(i / 4).float().double(), fn((2 * i - 1) / 8).float().double()
    g = torch.Generator().manual_seed(5)
    z = torch.randn(4, 3, 2, 2, generator=g, dtype=torch.float64)
    for mot, ls, cols in ((te, l, (D.T_A0, D.T_B0X, D.T_B0E)), (te, lm, (D.U_A0, D.U_B0X, D.U_B0E)), (s, l, (D.S_A0, D.S_B0X, D.S_B0E))):
        out = torch.randn(4, 6 if mot == "both" else 3, 2, 2, generator=g, dtype=torch.float64)
        a0, b0x, b0e = (R.col(coef[:, c]) for c in cols)
        got = a0 * z + b0x * out[:, :3] + (b0e * out[:, 3:] if mot == "both" else 0.0)
        ref = R.x0_from_out(out, z, R.col(ls), mot)
        scale = (a0.abs() * z.abs() + b0x.abs() * out[:, :3].abs()).amax(dim=(1, 2, 3), keepdim=True)
        assert bool(((got - ref).abs() <= 2 * 2.0 ** -24 * scale).all())       # each weight is within half an fp32 ulp


def test_rescaling_schedule_hands_the_networks_the_rewritten_times():
    import v_diffusion as vd
    N = 4
    D, fn, t, coef, (tt, tm, te) = _table("cosine", N, rescale=True)
    plain = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    i = torch.arange(1, N + 1, dtype=torch.float64)
    for got, grid in ((tt, i / N), (tm, (2 * i - 1) / (2 * N)), (te, (i - 1) / N)):
        want = grid.clone()
        vd.get_logsnr_schedule("cosine", -20.0, 20.0, rescale=True)(want)          # rewrites ``want`` in place
        assert torch.equal(got, want) and not torch.equal(got, grid)
    assert torch.equal(t, i / N)                                                     # the caller's tensor is not touched
    # the log-SNRs (hence every weight) are those of the grid times, not of the rewritten ones
    _, _, _, coef_plain, _ = _table("cosine", N)
    assert torch.equal(coef, coef_plain)
    assert torch.equal(coef[:, D.LOGSNR_T], plain(i / N).float())
    dd = vd.DistillationDiffusion(torch.nn.Identity(), N, logsnr_fn=fn, model_out_type="v", model_var_type="fixed_large",
                                  reweight_type="constant")
    assert dd.sample_timesteps == N and dd.teacher_out_type == "v" and dd.loss_type == "mse"
    with pytest.raises(RuntimeError, match="MI355X"):                                # no CPU path, like the rest of the package
        dd.train_loss(torch.nn.Identity(), torch.zeros(N, 3, 4, 4), t, None)
    # (that train_loss hands the networks these tensors is checked on the GPU: test_distill_gpu.py::test_networks_are_called_with_...)


def test_next_stage_halves_and_refuses_odd_step_counts():
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    kw = dict(logsnr_fn=fn, model_out_type="v", model_var_type="fixed_large", reweight_type="snr_trunc")
    teacher = torch.nn.Linear(2, 2)
    dd = vd.DistillationDiffusion(teacher, 4, teacher_out_type="eps", teacher_w_guide=2.0, w_guide=0.3, p_uncond=0.2, **kw)
    assert not teacher.training and dd.w_guide == 0.0 and dd.teacher_w_guide == 2.0     # a guided stage's student samples unguided
    student = torch.nn.Linear(2, 2)
    nxt = dd.next_stage(student)
    assert nxt.student_steps == nxt.sample_timesteps == 2
    assert nxt.teacher_w_guide == 0.0 and nxt.w_guide == 0.0 and nxt.teacher_out_type == "v"
    assert nxt.teacher_fn is not student and not nxt.teacher_fn.training
    assert all(not p.requires_grad for p in nxt.teacher_fn.parameters())
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(nxt.teacher_fn.parameters(), student.parameters()))
    assert student.training and all(p.requires_grad for p in student.parameters())      # the student itself is left alone
    last = nxt.next_stage(student, model_out_type="x0")
    assert last.student_steps == 1 and last.model_out_type == "x0" and last.teacher_out_type == "v"
    with pytest.raises(ValueError, match="odd"):
        last.next_stage(student)
    with pytest.raises(ValueError, match="odd"):
        vd.DistillationDiffusion(teacher, 3, **kw).next_stage(student)
    with pytest.raises(TypeError):
        vd.DistillationDiffusion(teacher, 4, sample_timesteps=8, **kw)


def test_entry_points_are_declared_and_bound():
    """(their declarations and ctypes signatures: tests/test_host_cpu.py pins the whole C ABI)"""
    from v_diffusion import _hip
    assert callable(_hip.distill_mid) and callable(_hip.distill_loss_fwd) and callable(_hip.distill_loss_bwd)
