"""Learned variances without a GPU: the CPU restatement (tests/learned_ref.py) against the fixture made from the reference's own
functions (tests/golden/learned_var.npz, tests/make_golden_learned.py), the host coefficient tables against fp64 closed forms, the
constructor and refusal rules, and the wrappers and definitions of the five new entries."""
import math
import os

import numpy as np
import pytest
import torch

import learned_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vd_bpd_terms_lv", "vd_bpd_bwd_lv", "vd_hybrid_loss_fwd", "vd_hybrid_loss_bwd", "vd_sample_step_lv")


def _gd(T=8, mot="v", var="learned", loss="hybrid", **kw):
    import v_diffusion as vd
    return vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T, mot, var, "snr_trunc", loss, **kw)


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "learned_var.npz"), allow_pickle=False)
    return {k: torch.from_numpy(g[k]) for k in g.files}


def test_ref_against_reference_fixture(gold):
    """the fp32 evaluation of learned_ref against the reference's functions composed as diffusion.py:320-324 intends: KL and NLL to
    rtol 1e-6; the log-variance to 4e-6 absolute -- the reference forms the lerp in fp64 and rounds once, learned_ref rounds lvmin and
    delta and forms lvmin + frac*delta in fp32, three roundings of numbers up to 20 (ulp 1.9e-6)"""
    kl, nll, _, lv = lref.terms(gold["out"], gold["x0"], gold["xt"], gold["logsnr_s"], gold["logsnr_t"], "v")
    err = (lv.double() - gold["logvar"].double()).abs().max().item()
    print(f"[learned_ref vs fixture] logvar max abs err {err:.2e}")
    assert float(gold["logvar"].abs().max()) <= 20.0 + 1e-3 and err <= 4e-6
    _, lv_api = _gd().p_mean_var(gold["out"], gold["xt"], gold["logsnr_s"], gold["logsnr_t"], clip_denoised=False, return_pred=False)
    assert torch.allclose(lv_api, lv, rtol=0, atol=4e-6), "the package's tensor API and the restatement disagree on the log-variance"
    use_kl = torch.arange(6) != 0                                # row 0 is the decoder row: its KL is not a loss term
    np.testing.assert_allclose(kl[use_kl].numpy(), gold["kl"][use_kl].numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(nll.numpy(), gold["nll"].numpy(), rtol=1e-6, atol=0)
    # the fixture is what its generator says: one decoder row, both saturation rows, nu = 3 * N(0, 1)
    assert float(gold["logsnr_s"][0]) == pytest.approx(20.0, abs=1e-4) and bool((gold["logsnr_s"][1:] < 19).all())
    assert bool((gold["x0"][0, :, :2] == 1).all()) and bool((gold["x0"][1, :, :2] == -1).all())
    assert 2.5 < float(gold["out"][:, 3:].std()) < 3.5


def test_p_mean_var_tensor_api_against_fixture(gold):
    """the per-sample tensor API splits the output, predicts from the first part and returns the per-element log-variance"""
    gd = _gd()
    mean, lv, pred = gd.p_mean_var(gold["out"], gold["xt"], gold["logsnr_s"], gold["logsnr_t"], clip_denoised=False, return_pred=True)
    _, _, p_ref, _ = lref.terms(gold["out"], gold["x0"], gold["xt"], gold["logsnr_s"], gold["logsnr_t"], "v")
    assert lv.shape == gold["x0"].shape and float((lv.double() - gold["logvar"].double()).abs().max()) <= 4e-6
    np.testing.assert_allclose(pred.numpy(), p_ref.numpy(), rtol=1e-6, atol=1e-6)
    c1, c2, _, _ = lref.lv_coefs(gold["logsnr_s"], gold["logsnr_t"])
    np.testing.assert_allclose(mean.numpy(), (c1 * gold["xt"] + c2 * p_ref).numpy(), rtol=1e-5, atol=1e-6)
    mean_d, lv_d = gd.p_mean_var(gold["out"], gold["xt"], gold["logsnr_s"], gold["logsnr_t"], clip_denoised=True, return_pred=False, use_ddim=True)
    assert mean_d.shape == gold["x0"].shape and float(lv_d) == -math.inf
    with pytest.raises(RuntimeError, match="3 \\+ 3 channels"):
        gd.p_mean_var(gold["out"][:, :5], gold["xt"], gold["logsnr_s"], gold["logsnr_t"], False, False)
    with pytest.raises(RuntimeError, match="6 \\+ 3 channels"):
        _gd(mot="both")._split_learned(gold["out"], 3)


def _closed_forms(ls32, lt32):
    """(lvmin, delta) in fp64 with the math module, from fp32-rounded log-SNRs given as python floats"""
    logsig = lambda x: -math.log1p(math.exp(-x)) if x >= 0 else x - math.log1p(math.exp(x))
    r = lt32 - ls32
    l1mr = math.log1p(-math.exp(r)) if r < -9 else math.log(-math.expm1(r))
    return l1mr + logsig(-ls32), logsig(-lt32) - logsig(-ls32)


@pytest.mark.parametrize("T", [8, 1000])
def test_coefficient_tables_learned_slots(T):
    """slots 5, 6 of _bpd_coefs and 5, 8 of _step_coefs = lvmin and delta, each the fp64 closed form rounded once (half an fp32 ulp),
    with delta >= 0 on every grid step"""
    import v_diffusion as vd
    gd = _gd(T, w_guide=1.5)
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    grid = fn(torch.arange(T + 1, dtype=torch.float64) / T).float()
    ls, lt = grid[:-1], grid[1:]
    coef = gd._bpd_coefs(ls, lt)
    assert coef.shape == (T, 8) and coef.dtype == torch.float32
    plain = _gd(T, var="fixed_small", loss="kl")._bpd_coefs(ls, lt)
    assert torch.equal(coef[:, :6], plain[:, :6]) and torch.equal(coef[:, 7], plain[:, 7])          # only slot 6 changes its meaning
    rnd = lambda v: float(torch.tensor(v, dtype=torch.float64).float())
    for i in (range(T) if T == 8 else list(range(0, T, 7)) + [T - 1]):
        lvmin, delta = _closed_forms(float(ls[i]), float(lt[i]))
        assert float(coef[i, 5]) == pytest.approx(rnd(lvmin), rel=1.2e-7) and float(coef[i, 6]) == pytest.approx(rnd(delta), rel=1.2e-7)
        for ddim in (False, True):
            k, t_net = gd._step_coefs(i, ddim)
            assert len(k) == 10 and t_net == pytest.approx((i + 1) / T)
            assert k[5] == float(coef[i, 5]) and k[8] == float(coef[i, 6]) and k[6] == 1.5 and k[7] == 0.0 and k[9] == 0.0
            k8 = _gd(T, var="fixed_small", loss="kl", w_guide=1.5)._step_coefs(i, ddim)[0]
            assert k[:5] == k8[:5]
    assert bool((coef[:, 6] >= 0).all()) and bool((coef[:, 6] > 0).any())
    if T == 8:
        assert float(coef[0, 5]) == pytest.approx(-20.0, abs=1e-3) and float(coef[0, 6]) == pytest.approx(16.73, abs=5e-3)   # the s = 0 row


class _Net:
    training = False

    def __call__(self, x, t, y):
        raise AssertionError("the network must not be called")


def test_constructor_and_refusal_rules():
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    assert _gd(T=50).vlb_weight == 0.05 and _gd(T=1000).vlb_weight == 1.0 and _gd(vlb_weight=0.25).vlb_weight == 0.25
    assert _gd(var="fixed_large", loss="mse").vlb_weight == 0.008          # the keyword is accepted whatever the loss
    for loss in ("hybrid", "kl", "mse"):
        assert _gd(loss=loss).model_var_type == "learned"
    with pytest.raises(ValueError, match="hybrid"):
        _gd(var="fixed_large", loss="hybrid")
    with pytest.raises(NotImplementedError, match="x0eps_coef"):
        _gd(x0eps_coef=True)
    gd, net, X = _gd(w_guide=0.0), _Net(), torch.zeros((2, 3, 4, 4))
    # what still refuses learned variances, before any launch or network call
    with pytest.raises(NotImplementedError, match="learned"):
        gd.p_sample_solver(net, (1, 3, 4, 4))
    with pytest.raises(NotImplementedError, match="learned"):
        gd.p_sample_inpaint(net, X, torch.zeros((1, 1, 4, 4)), seed=1)
    for call in (lambda: gd.p_invert_noise(net, X, seed=1), lambda: gd.p_sample_replay(net, X, torch.zeros((8,) + tuple(X.shape))),
                 lambda: gd.p_encode(net, X)):
        with pytest.raises(NotImplementedError, match="learned"):
            call()
    with pytest.raises(NotImplementedError, match="learned"):
        vd.DistillationDiffusion(net, 4, logsnr_fn=fn, model_out_type="v", model_var_type="learned", reweight_type="snr_trunc")
    # no CPU path, as for every other loss and sampler
    for loss in ("hybrid", "kl"):
        with pytest.raises(RuntimeError, match="MI355X"):
            _gd(loss=loss).train_loss(net, X, torch.rand(2), None)
    with pytest.raises(RuntimeError, match="MI355X"):
        gd.p_sample(net, (1, 3, 4, 4), device="cpu")


def test_header_exports_and_signatures_agree():
    """every new entry has its launch wrapper and its definition in csrc/diffusion.hip (declarations and ctypes signatures:
    tests/test_host_cpu.py pins the whole C ABI)"""
    from v_diffusion import _hip
    for name in NEW:
        assert callable(getattr(_hip, name[3:]))
    src = open(os.path.join(ROOT, "v-diffusion-torch_amd", "csrc", "diffusion.hip")).read()
    for name in NEW:
        assert f'extern "C" int {name}(' in src
