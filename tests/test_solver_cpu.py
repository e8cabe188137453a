"""Host side of the DPM-Solver++(2M) sampler (v_diffusion/solver.py): the coefficient table against the DDIM numbers of
``GaussianDiffusion._step_coefs`` and against the float64 restatement of tests/solver_ref.py, the log-SNR-uniform grid, the order of
convergence on a problem with a known solution, and the argument checks.  No kernel is launched here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as R                                            # noqa: E402

MOTS = ("v", "x0", "eps", "both")
STEPS = (1, 2, 8, 50)
W = 0.3


def _ulp32(x):
    x = torch.as_tensor(x).float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _gd(fn, T, mot="v", **kw):
    import v_diffusion as vd
    return vd.GaussianDiffusion(fn, T, mot, kw.pop("model_var_type", "fixed_large"), "snr_trunc", "mse", w_guide=W, p_uncond=0.0, **kw)


@pytest.mark.parametrize("rescale", (False, True), ids=("plain", "rescale"))
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("mot", MOTS)
def test_order_one_is_the_ddim_table(mot, T, rescale):
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0, rescale=rescale)
    gd = _gd(fn, T, mot)
    table, t_net = vd.solver_coefs(fn, T, order=1, spacing="time", model_out_type=mot, w_guide=W)
    assert table.shape == (T, 8) and table.dtype == torch.float32 and t_net.shape == (T,) and t_net.dtype == torch.float64
    w32 = float(torch.tensor(W, dtype=torch.float32))
    for i in range(T):
        k8, tn = gd._step_coefs(i, use_ddim=True)
        row = table[i].double().tolist()
        assert float(t_net[i]) == tn                              # the time as the schedule left it
        if i >= 1:
            assert row[:5] == k8[:5], (i, row, k8)
            assert row[5:] == [0.0, w32, 0.0]
        else:
            assert row == k8[:3] + [0.0, 1.0, 0.0, w32, 0.0], (row, k8)
    if not rescale:
        assert t_net.tolist() == [(i + 1) / T for i in range(T)]


@pytest.mark.parametrize("mot", MOTS)
def test_prediction_and_ddim_weights_agree_with_first_principles(mot):
    """slots 3, 4 against alpha, sigma written out, to 1 fp32 ulp: fp64 values rounded once.  So are the prediction weights of "x0" and
    "both"; those of "v" and "eps" are fp32 evaluations as the reference makes them, the DDIM sampler's numbers (test above)."""
    import v_diffusion as vd
    T = 8
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    table, t_net = vd.solver_coefs(fn, T, order=2, model_out_type=mot)
    for i in range(1, T):
        ls, lt = (float(fn(torch.tensor([v], dtype=torch.float64)).float()) for v in (i / T, (i + 1) / T))
        want = list(R.x0_weights(lt, mot)) + list(R.weights(ls, lt)[:2])
        for j, (got, ref) in enumerate(zip(table[i, :5].double().tolist(), want)):
            if j >= 3 or mot in ("x0", "both"):
                assert abs(got - ref) <= float(_ulp32(ref)), (i, j, got, ref)


def _rho_cases():
    import v_diffusion as vd
    return {"sigmoid-time": (vd.get_logsnr_schedule("sigmoid", -20.0, 20.0), "time"),
            "cosine-logsnr": (vd.get_logsnr_schedule("cosine", -20.0, 20.0), "logsnr"),
            "cosine-time": (vd.get_logsnr_schedule("cosine", -20.0, 20.0), "time")}


@pytest.mark.parametrize("T", (1, 2, 8, 50))
@pytest.mark.parametrize("case", ("sigmoid-time", "cosine-logsnr", "cosine-time"))
def test_rho(case, T):
    import v_diffusion as vd
    fn, spacing = _rho_cases()[case]
    table, t_net = vd.solver_coefs(fn, T, order=2, spacing=spacing, model_out_type="v")
    c2, c2rho = table[:, 4].double(), table[:, 5].double()
    assert float(c2rho[T - 1]) == 0.0 and float(c2rho[0]) == 0.0             # first executed row, and the last
    inner = list(range(1, T - 1))
    if case != "cosine-time":                                                # uniform log-SNR steps: rho = 1/2
        for i in inner:
            assert abs(float(c2rho[i] / c2[i]) - 0.5) <= 1e-5, (i, float(c2rho[i] / c2[i]))
    # independent fp64 recomputation from the fp32-rounded log-SNRs of the grid (a plain schedule leaves its argument alone)
    tau = [0.0] + t_net.tolist()
    l = [float(fn(torch.tensor([tau[i], tau[min(i + 1, T)]], dtype=torch.float64))[0].float()) for i in range(T)]
    l.append(float(fn(torch.tensor([tau[T - 1], tau[T]], dtype=torch.float64))[1].float()))
    for i in inner:
        _, c2_ref, rho = R.weights(l[i], l[i + 1], l[i + 2])
        assert abs(float(c2rho[i]) - c2_ref * rho) <= float(_ulp32(c2_ref * rho)), (i, float(c2rho[i]), c2_ref * rho)
    assert all(float(c2rho[i]) > 0 for i in inner)
    first = vd.solver_coefs(fn, T, order=1, spacing=spacing, model_out_type="v")[0]
    assert bool((first[:, 5] == 0).all()) and torch.equal(first[:, :5], table[:, :5])


@pytest.mark.parametrize("T", (1, 2, 16, 50))
@pytest.mark.parametrize("lims", ((-20.0, 20.0), (-6.0, 6.0)))
def test_logsnr_spacing_grid(lims, T):
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", *lims)
    _, t_net = vd.solver_coefs(fn, T, spacing="logsnr")
    tau = torch.tensor([0.0] + t_net.tolist(), dtype=torch.float64)
    assert float(tau[0]) == 0.0 and float(tau[-1]) == 1.0
    assert bool((tau[1:] > tau[:-1]).all())
    l = fn(tau.clone())
    lin = l[0] + (l[-1] - l[0]) * torch.arange(T + 1, dtype=torch.float64) / T
    assert float((l - lin).abs().max()) <= 1e-9, float((l - lin).abs().max())


def test_logsnr_spacing_refuses_a_non_monotone_schedule():
    import v_diffusion as vd
    wavy = lambda t: 10.0 * torch.cos(3.0 * torch.pi * t)          # 10 at 0, -10 at 1, up and down in between
    with pytest.raises(ValueError, match="decreasing"):
        vd.solver_coefs(wavy, 8, spacing="logsnr")
    rising = lambda t: 20.0 * t - 10.0
    with pytest.raises(ValueError, match="decreasing"):
        vd.solver_coefs(rising, 8, spacing="logsnr")
    with pytest.raises(ValueError, match="spacing"):
        vd.solver_coefs(vd.get_logsnr_schedule("cosine"), 8, spacing="karras")


def test_order_of_convergence_on_the_gaussian_problem():
    """cosine schedule on [-6, 6] (with +-20 the end steps are so long that the asymptotic regime starts beyond T = 128), uniform log-SNR
    steps, s = 2, an x0-network, no clip, T = 16, 32, 64.  Measured: order 2 7.80e-3, 2.06e-3, 5.23e-4 (ratios 3.78, 3.95); order 1
    8.86e-2, 4.53e-2, 2.29e-2 (ratios 1.95, 1.98)."""
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -6.0, 6.0)
    run = lambda net, m1, table, t_net, order: R.chain(net, m1.reshape(1, 1, 1, 1), table, t_net, stop=1)
    R.check_convergence(R.convergence_errors(fn, vd.solver_coefs, 1, run), R.convergence_errors(fn, vd.solver_coefs, 2, run))


def test_argument_checks():
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine")
    net = lambda x, t, y: x
    for order in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            vd.solver_coefs(fn, 4, order=order)
        with pytest.raises(ValueError, match="order"):
            _gd(fn, 4).p_sample_solver(net, (1, 3, 4, 4), order=order)
    with pytest.raises(ValueError, match="steps"):
        vd.solver_coefs(fn, 0)
    with pytest.raises(NotImplementedError, match="learned"):
        _gd(fn, 4, model_var_type="learned").p_sample_solver(net, (1, 3, 4, 4))
    with pytest.raises(NotImplementedError, match="x0eps_coef"):
        _gd(fn, 4, x0eps_coef=True).p_sample_solver(net, (1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path, as for the other samplers
        _gd(fn, 4).p_sample_solver(net, (1, 3, 4, 4), device="cpu")
    assert vd.DistillationDiffusion.p_sample_solver is vd.GaussianDiffusion.p_sample_solver
