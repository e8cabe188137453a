"""Device-free checks of DDNM null-space restoration (v_diffusion/ddnm.py):

  * ``ddnm_rule`` against the formulas of DDNM+ -- sigma_y = 0, the switch point noise_scale = c2 sigma_y, the last step, an explicit lam,
    and the variance identity (c2 lam sigma_y)^2 + noise_scale'^2 = noise_scale^2 wherever lam = 1;
  * the pseudo-inverses: A A^+ y = y on the range of A and A^+ A A^+ = A^+ for the three operators, fp64 on CPU tensors, hard masks,
    ``v_diffusion.ddnm_pinv`` against the restatement tests/ddnm_ref.py;
  * every refusal that needs no device, the exported names."""
import ctypes
import math
import os
import sys

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
import ddnm_ref as R                                              # noqa: E402
import dps_ref as DR                                              # noqa: E402
from v_diffusion import _hip                                      # noqa: E402

F64 = torch.float64


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64) * scale


def _gd(T, mot="v", w=0.0, **kw):
    import v_diffusion as vd
    return vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T, mot, "fixed_large", "snr_trunc", "mse", w_guide=w,
                                p_uncond=0.0, **kw)


# ------------------------------------------------------------------------------------------------ 1. the rule
def test_the_rule_is_the_formulas():
    from v_diffusion import ddnm_rule
    # noiseless: lam = 1 on every step and the step's noise scale is returned as it came (the very float, no sqrt of a square)
    for c2, ns in ((0.7, 0.3), (1e-3, 0.9), (0.999, 1e-4), (0.5, 0.0)):
        assert ddnm_rule(c2, ns, 0.0, False) == (1.0, ns) and ddnm_rule(c2, ns, 0.0, True) == (1.0, ns)
    # the step's noise covers the measurement's: lam = 1 and the rest of the variance stays with the step
    c2, ns, sy = 0.6, 0.5, 0.4
    lam, left = ddnm_rule(c2, ns, sy, False)
    assert lam == 1.0 and math.isclose(left, math.sqrt(ns * ns - (c2 * sy) ** 2), rel_tol=1e-15)
    # ... it does not: lam = noise_scale / (c2 sigma_y) carries exactly the step's variance, nothing is left to add
    c2, ns, sy = 0.9, 0.1, 0.5
    lam, left = ddnm_rule(c2, ns, sy, False)
    assert lam == ns / (c2 * sy) and 0.0 < lam < 1.0 and left <= 1e-8         # (the root of a rounding error of 0.01)
    # the switch point noise_scale = c2 sigma_y belongs to lam = 1, with nothing left
    c2, sy = 0.5, 0.25
    assert ddnm_rule(c2, c2 * sy, sy, False) == (1.0, 0.0)
    lam, _ = ddnm_rule(c2, math.nextafter(c2 * sy, 0.0), sy, False)
    assert lam < 1.0
    # the last step adds no noise: a noisy measurement is not put into the result
    assert ddnm_rule(1.0, 0.0, 0.3, True) == (0.0, 0.0) and ddnm_rule(1.0, 0.0, 0.0, True) == (1.0, 0.0)
    # an explicit lam replaces the rule's, and the noise scale left is formed from it (never negative under the root)
    lam, left = ddnm_rule(0.6, 0.5, 0.4, False, lam=0.5)
    assert lam == 0.5 and math.isclose(left, math.sqrt(0.25 - (0.6 * 0.5 * 0.4) ** 2), rel_tol=1e-15)
    assert ddnm_rule(0.9, 0.1, 0.5, False, lam=1.0) == (1.0, 0.0)
    assert ddnm_rule(0.6, 0.5, 0.4, False, lam=0.0) == (0.0, 0.5) and ddnm_rule(0.6, 0.5, 0.4, True, lam=0.25)[0] == 0.25


def test_the_rule_is_the_restatement_s_and_keeps_the_variance():
    from v_diffusion import ddnm_rule
    g = torch.Generator().manual_seed(5)
    ones = 0
    for _ in range(400):
        c2, ns, sy = (float(v) for v in torch.rand(3, generator=g, dtype=F64))
        sy = sy if float(torch.rand(1, generator=g)) > 0.2 else 0.0
        for last in (False, True):
            nsl = 0.0 if last else ns
            lam, left = ddnm_rule(c2, nsl, sy, last)
            rl, rleft = R.rule(c2, nsl, sy, last)
            assert lam == rl and abs(left ** 2 - rleft ** 2) <= 1e-15 and 0.0 <= lam <= 1.0 and 0.0 <= left <= nsl
            if lam == 1.0 and not last:
                ones += 1
                assert abs((c2 * lam * sy) ** 2 + left ** 2 - nsl ** 2) <= 1e-15
            elif not last:
                assert abs(c2 * lam * sy - nsl) <= 1e-15 and left <= 1e-7      # the correction carries all of the step's variance
    assert 50 < ones < 750


# ------------------------------------------------------------------------------------------------ 2. the pseudo-inverses
def operators(shape, seed):
    """[(op, par, mask, the operator argument)] for images of ``shape``: hard masks of both widths (one per sample and one shared), every
    factor that divides the image, grey"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    ops = [("mask", None, (torch.rand((b, c, H, W), generator=g) < 0.6).to(F64)) for b, c in ((B, 1), (B, C), (1, 1))]
    ops += [("down", f, None) for f in (2, 4, 8) if H % f == 0 and W % f == 0]
    ops += [("gray", None, None)]
    return [(op, par, m, {"mask": ("mask", m), "down": ("down", par), "gray": ("gray",)}[op]) for op, par, m in ops]


@pytest.mark.parametrize("shape", [(2, 3, 8, 16), (3, 4, 6, 10), (1, 3, 5, 5)], ids=str)
def test_the_pseudo_inverses(shape):
    from v_diffusion import ddnm_pinv, dps_measure
    for op, par, mask, arg in operators(shape, 3):
        x = rnd(shape, 1)
        y = dps_measure(x, arg)                                   # a measurement in the range of A
        assert torch.equal(y, DR.apply_A(op, x, par, mask)) or torch.allclose(y, DR.apply_A(op, x, par, mask), rtol=0, atol=1e-15)
        p = ddnm_pinv(y, arg, shape)
        assert tuple(p.shape) == shape and p.dtype == F64
        assert torch.equal(p, R.pinv(op, y, shape, par, mask))
        err = float((dps_measure(p, arg) - y).abs().max())
        assert err <= 1e-15 * max(1.0, float(y.abs().max())), (op, par, "A A^+ y = y", err)
        err = float((ddnm_pinv(dps_measure(p, arg), arg, shape) - p).abs().max())
        assert err <= 1e-15 * max(1.0, float(p.abs().max())), (op, par, "A^+ A A^+ = A^+", err)
        # x - A^+ A x lies in the null space of A: the part of a prediction the step keeps
        null = x - ddnm_pinv(dps_measure(x, arg), arg, shape)
        assert float(dps_measure(null, arg).abs().max()) <= 1e-15 * float(x.abs().max()), (op, par)
    # a soft mask: y / M where M > 0, and an element that was not measured takes nothing, whatever y holds there
    m = torch.tensor([0.0, 0.25, 1.0, 0.5], dtype=F64).reshape(1, 1, 1, 4)
    y = torch.tensor([float("nan"), 0.5, -2.0, 1.0], dtype=F64).reshape(1, 1, 1, 4)
    assert ddnm_pinv(y, ("mask", m), (1, 1, 1, 4)).flatten().tolist() == [0.0, 2.0, -2.0, 2.0]
    for bad, msg in (((("blur",), (1, 1, 1, 4)), "operator"), ((("gray",), (1, 3, 1, 4)), None)):
        with pytest.raises(ValueError, match=msg or "shape"):
            ddnm_pinv(torch.zeros(1, 3, 1, 4), *bad)


def test_one_step_of_the_restatement_lands_on_the_measurement():
    """last step, lam = 1, no noise: A xn = meas up to fp64 rounding for the two means, and on the measured elements of a soft mask"""
    shape = (2, 3, 8, 8)
    k = [0.8, -0.6, 0.0, 0.3, 0.7, 0.0, 1.5, 0.0]
    for cfg in (False, True):
        xt, out = rnd(shape, 1), rnd((2 * (1 + cfg), 3, 8, 8), 2)
        soft = torch.rand((2, 1, 8, 8), generator=torch.Generator().manual_seed(4), dtype=F64).round(decimals=1)
        for op, par, mask in (("down", 4, None), ("gray", None, None), ("mask", None, soft)):
            meas = rnd(DR.measurement_shape(op, shape, par), 3)
            res = R.step(k, xt, out, None, meas, op, 1.0, par, mask, False, cfg, True, True)
            back = DR.apply_A(op, res["xn"], par, mask)
            want = meas if mask is None else torch.where(mask.expand(shape) > 0, meas, back)
            assert float((back - want).abs().max()) <= 1e-13, op
            plain = R.step(k, xt, out, None, meas, op, 0.0, par, mask, False, cfg, True, True)
            assert torch.equal(plain["xn"], res["g"]) and torch.equal(plain["sumsq"], res["sumsq"])
            if mask is not None:
                assert torch.equal(res["xn"][mask.expand(shape) == 1], meas[mask.expand(shape) == 1])
                assert torch.equal(res["xn"][mask.expand(shape) == 0], res["g"][mask.expand(shape) == 0])


# ------------------------------------------------------------------------------------------------ 3. refusals without a device
class Stub:
    training = False

    def __call__(self, x, t, y):
        return 0.5 * x


def test_refusals_that_need_no_device():
    import v_diffusion as vd
    shape = (2, 3, 8, 8)
    net = Stub()
    meas = torch.zeros(shape)
    call = lambda gd, *a, **kw: gd.p_sample_ddnm(net, *a, **kw)
    with pytest.raises(NotImplementedError, match="learned"):
        call(vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), 4, "v", "learned", "snr_trunc", "mse"), meas, ("gray",), shape)
    with pytest.raises(NotImplementedError, match="x0eps_coef"):
        call(_gd(4, x0eps_coef=True), meas, ("gray",), shape)
    gd = _gd(4)
    for bad in (("blur", 3), "gray", (), ("gray", 1), ("down",), None):
        with pytest.raises(ValueError, match="operator"):
            call(gd, meas, bad, shape)
    for f in (1, 3, 16, 2.0, True):
        with pytest.raises(ValueError, match="factor"):
            call(gd, meas, ("down", f), shape)
    with pytest.raises(ValueError, match="divide"):
        call(gd, torch.zeros(2, 3, 3, 4), ("down", 2), (2, 3, 6, 9))
    for m in (torch.ones(2, 2, 8, 8), torch.ones(3, 1, 8, 8), torch.ones(2, 1, 8, 4), torch.full((2, 1, 8, 8), 1.5),
              torch.full((2, 1, 8, 8), float("nan")), torch.ones(2, 1, 8, 8, dtype=torch.int32)):
        with pytest.raises(ValueError, match="mask"):
            call(gd, meas, ("mask", m), shape)
    for op, wrong in ((("gray",), shape), (("down", 2), shape), (("down", 4), (2, 3, 4, 4)), (("mask", torch.ones(1, 1, 8, 8)), (2, 1, 8, 8))):
        with pytest.raises(ValueError, match="measurement"):
            call(gd, torch.zeros(wrong), op, shape)
    with pytest.raises(ValueError, match="measurement"):
        call(gd, None, ("gray",), shape)
    gray = torch.zeros(2, 1, 8, 8)
    for s in (-1e-3, float("nan"), float("inf"), "0.1", None, True):
        with pytest.raises(ValueError, match="sigma_y"):
            call(gd, gray, ("gray",), shape, sigma_y=s)
    with pytest.raises(ValueError, match="use_ddim"):
        call(gd, gray, ("gray",), shape, sigma_y=0.1, use_ddim=True)
    for l in (-1e-3, 1.001, float("nan"), float("inf"), [0.1, 0.1, 1.5, 0.1], [0.1, float("nan"), 0.1, 0.1]):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            call(gd, gray, ("gray",), shape, lam=l)
    for l in ([0.1] * 3, [0.1] * 5, [], "1.0", [0.1, 0.1, 0.1, "x"], True):
        with pytest.raises(ValueError, match="lam"):
            call(gd, gray, ("gray",), shape, lam=l)
    for kw in (dict(jump_length=0), dict(jump_length=1.5), dict(resamplings=0), dict(resamplings=True)):
        with pytest.raises(ValueError, match="integer"):
            call(gd, gray, ("gray",), shape, **kw)
    with pytest.raises(RuntimeError, match="MI355X"):                      # CPU tensors, after everything else passed
        call(gd, gray, ("gray",), shape, lam=[0.1] * 4, sigma_y=0.1, jump_length=2, resamplings=2)


def test_the_names_are_exported_and_inherited():
    import v_diffusion as vd
    for name in ("ddnm_rule", "ddnm_pinv"):
        assert name in vd.__all__ and name in vd._HOT and callable(getattr(vd, name))
    assert vd.DistillationDiffusion.p_sample_ddnm is vd.GaussianDiffusion.p_sample_ddnm
    assert callable(_hip.ddnm_step)


# ------------------------------------------------------------------------------------------------ 4. the C entry
def test_the_entry_refuses_before_any_launch():
    """what vd_dps_residual refuses -- a bad model_out_type or op, a null required buffer, n, C, H, W < 1, a mask width that is neither 1
    nor C, a factor outside {2, 4, 8} or not dividing the image -- and a missing noise with a noise scale: 1, with the reason, and
    nothing launched (the addresses are never dereferenced).  noise, xdup, sumsq and, off op 0, the mask are optional"""
    lib = _hip.lib()
    err = lambda: lib.vd_last_error().decode(errors="replace")
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf) // 16 * 16 + 16
    k = (ctypes.c_float * 8)(0.8, -0.6, 0.0, 0.3, 0.7, 0.1, 0.0, 0.0)
    good = dict(xt=a, out=a, noise=a, meas=a, mask=a, k=k, lam=ctypes.c_float(1.0), type=0, cfg=0, last=0, clip=1, op=0, par=1, xn=a,
                xdup=None, sumsq=None, n=1, C=3, H=4, W=4, stream=None)
    def r(**kw):
        return lib.vd_ddnm_step(*{**good, **kw}.values())
    assert r(type=4) == 1 and "model_out_type" in err() and r(type=-1) == 1
    assert r(op=3) == 1 and "bad op" in err() and r(op=-1) == 1
    for name in ("xt", "out", "meas", "mask", "k", "xn"):
        assert r(**{name: None}) == 1 and "null" in err(), name
    for name in ("n", "C", "H", "W"):
        assert r(**{name: 0}) == 1 and "empty" in err(), name
    assert r(par=2) == 1 and "channels" in err()
    for f, H, W in ((3, 6, 6), (16, 16, 16), (1, 4, 4), (2, 5, 4), (4, 8, 6), (8, 8, 12)):
        assert r(op=1, par=f, H=H, W=W) == 1 and "down-sampling" in err(), (f, H, W)
    assert r(noise=None) == 1 and "noise" in err()
