"""Host side of the UniPC sampler (v_diffusion/unipc.py): the float64 restatement of tests/unipc_ref.py against the errors the scheme
is known to make on a problem with a known solution, the flattened coefficient table against that restatement, its reduction to the
DPM-Solver++(2M) table, and the argument checks.  No kernel is launched here."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unipc_ref as U                                             # noqa: E402

MOTS = ("v", "x0", "eps", "both")
W = 0.3
CASES = [(o, v, c) for o, v, c in itertools.product((1, 2, 3), ("bh1", "bh2"), (False, True))]


def _gd(fn, T, mot="v", **kw):
    import v_diffusion as vd
    return vd.GaussianDiffusion(fn, T, mot, kw.pop("model_var_type", "fixed_large"), "snr_trunc", "mse", w_guide=W, p_uncond=0.0, **kw)


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_reference_reproduces_the_known_errors():
    """the published-form chain on the Gaussian problem (s = 2, cosine schedule on [-6, 6], log-SNR-uniform grid, x0-network, error at
    tau_1): every row of ``unipc_ref.TABLE`` at T = 8, 16, 32 to 3 significant digits (5e-4 relative: half a unit of the third digit
    of a mantissa just below 10).  The grid is ``solver_coefs``'s: nothing of v_diffusion/unipc.py is run here.  The row (bh2, no
    corrector, order 2) is DPM-Solver++(2M): 7.800e-3, 2.064e-3 at T = 16, 32 are the figures of tests/test_solver_cpu.py."""
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -6.0, 6.0)
    tau = {T: [0.0] + vd.solver_coefs(fn, T, order=1, spacing="logsnr", model_out_type="x0")[1].tolist() for T in (8, 16, 32)}
    for (variant, corrector, order), want in U.TABLE.items():
        got = [U.gaussian_errors(fn, tau[T], order, variant, corrector) for T in (8, 16, 32)]
        print(f"[unipc reference {variant} corrector={corrector} order={order}] " + " ".join(f"{g:.4e}" for g in got))
        for g, w in zip(got, want):
            assert abs(g / w - 1.0) <= 5e-4, (variant, corrector, order, got, want)


@pytest.mark.parametrize("spacing", ("time", "logsnr"))
@pytest.mark.parametrize("order,variant,corrector", CASES, ids=[f"{o}-{v}-{'pc' if c else 'p'}" for o, v, c in CASES])
def test_table_through_the_kernel_arithmetic_is_the_published_chain(order, variant, corrector, spacing):
    """``unipc_coefs``'s table through an fp64 loop of the arithmetic the header states for the kernel, against the published-form
    chain on the same grid with a non-linear network, guided, clipped, T = 12 on the cosine +-20 schedule: the two differ by the fp32
    rounding of the table's slots only (the x0 weights of a "v" network are fp32 evaluations), 1e-6 of the result's scale"""
    import v_diffusion as vd
    T = 12
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    table, t_net = vd.unipc_coefs(fn, T, order=order, variant=variant, corrector=corrector, spacing=spacing, model_out_type="v", w_guide=W)
    assert table.shape == (T, 16) and table.dtype == torch.float32 and t_net.shape == (T,) and t_net.dtype == torch.float64
    assert bool((table[:, 11:] == 0).all())
    x, y = _rnd((2, 3, 4, 4), 7), torch.tensor([1.0, 3.0], dtype=torch.float64)
    net = U.Stub()
    tau = [0.0] + t_net.tolist()
    for stop in (0, 1):
        ref = U.chain(net, x, fn, tau, order, variant, corrector, y=y, out_type="v", w=float(torch.tensor(W).float()), cfg=True, clip=True,
                      stop=stop)
        got = U.table_chain(net, x, table, t_net, y, cfg=True, clip=True)[stop]
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"[unipc table vs published form, order {order} {variant} corrector={corrector} {spacing} stop={stop}] {err:.3e}")
        assert err <= 1e-6, err


@pytest.mark.parametrize("spacing", ("time", "logsnr"))
@pytest.mark.parametrize("T", (1, 2, 3, 8, 50))
@pytest.mark.parametrize("mot", MOTS)
def test_bh2_order_two_predictor_is_the_2m_table(mot, T, spacing):
    import v_diffusion as vd
    from v_diffusion import solver as S, unipc as P
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    old, t_old = vd.solver_coefs(fn, T, order=2, spacing=spacing, model_out_type=mot, w_guide=W)
    new, t_new = vd.unipc_coefs(fn, T, order=2, variant="bh2", corrector=False, spacing=spacing, model_out_type=mot, w_guide=W)
    assert torch.equal(t_old, t_new)
    for a, b in ((S.A0, P.A0), (S.B0X, P.B0X), (S.B0E, P.B0E), (S.W_GUIDE, P.W_GUIDE), (S.C1, P.C1), (S.C2, P.C2)):
        assert torch.equal(old[:, a], new[:, b]), (a, b)                      # bit for bit
    c2rho, p1 = old[:, S.C2RHO].double(), new[:, P.P1].double()
    assert bool(((p1 + c2rho).abs() <= 1e-6 * c2rho.abs()).all()), (p1, c2rho)
    assert bool((new[:, P.P2] == 0).all()) and bool((new[:, P.EG:] == 0).all())
    # order 1 with the corrector: nothing to extrapolate from and nothing to correct on the first executed row, and row 0 ends the chain
    one, _ = vd.unipc_coefs(fn, T, order=1, variant="bh2", corrector=True, spacing=spacing, model_out_type=mot, w_guide=W)
    assert bool((one[T - 1, P.P1:] == 0).all())
    assert one[0, P.C1:P.P2 + 1].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert bool((one[:, P.P1:P.P2 + 1] == 0).all()) and bool((one[:, P.E1:] == 0).all())
    if T > 1:
        assert bool((one[:T - 1, P.EG] != 0).all())                           # every later node corrects the step that arrived
    three, _ = vd.unipc_coefs(fn, T, order=3, variant="bh1", corrector=True, spacing=spacing, model_out_type=mot, w_guide=W)
    assert three[0, P.C1:P.P2 + 1].tolist() == [0.0, 1.0, 0.0, 0.0] and bool((three[T - 1, P.P1:] == 0).all())


def test_argument_checks():
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine")

    def net(x, t, y):
        raise AssertionError("the network was called")
    for order in (0, 4, "2", True, 2.0):
        with pytest.raises(ValueError, match="order"):
            vd.unipc_coefs(fn, 4, order=order)
        with pytest.raises(ValueError, match="order"):
            _gd(fn, 4).p_sample_unipc(net, (1, 3, 4, 4), order=order)
    for variant in ("bh3", "BH1", None):
        with pytest.raises(ValueError, match="variant"):
            vd.unipc_coefs(fn, 4, variant=variant)
        with pytest.raises(ValueError, match="variant"):
            _gd(fn, 4).p_sample_unipc(net, (1, 3, 4, 4), variant=variant)
    with pytest.raises(ValueError, match="steps"):
        vd.unipc_coefs(fn, 0)
    with pytest.raises(ValueError, match="spacing"):
        vd.unipc_coefs(fn, 4, spacing="karras")
    with pytest.raises(NotImplementedError, match="dynamic"):
        _gd(fn, 4).p_sample_unipc(net, (1, 3, 4, 4), clip_denoised="dynamic")
    with pytest.raises(ValueError, match="clip_denoised"):
        _gd(fn, 4).p_sample_unipc(net, (1, 3, 4, 4), clip_denoised="static")
    with pytest.raises(NotImplementedError, match="learned"):
        _gd(fn, 4, model_var_type="learned").p_sample_unipc(net, (1, 3, 4, 4))
    with pytest.raises(NotImplementedError, match="x0eps_coef"):
        _gd(fn, 4, x0eps_coef=True).p_sample_unipc(net, (1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path, as for the other samplers
        _gd(fn, 4).p_sample_unipc(net, (1, 3, 4, 4), device="cpu")
    assert vd.DistillationDiffusion.p_sample_unipc is vd.GaussianDiffusion.p_sample_unipc
    for name in ("unipc_coefs", "p_sample_unipc"):
        assert name in vd.__all__ and callable(getattr(vd, name))
