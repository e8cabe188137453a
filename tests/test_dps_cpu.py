"""Device-free checks of Diffusion Posterior Sampling (v_diffusion/dps.py) and of the input-gradient-only backward pass it stands on:

  * the launch trace of ``UNetEngine.backward(tape, dout, None, need_dx=True)`` through the recorder of tests/test_engine_trace_cpu.py:
    none of the weight-gradient, GroupNorm-parameter, FiLM or embedding launches, and the d/dx chain of the full pass launch for launch;
  * the fp64 restatement tests/dps_ref.py against itself: <A x, r> = <x, A^T r>, the closed-form cotangents against torch autograd, and
    a chain that does reduce the measurement residual;
  * every refusal that needs no device, the exported names."""
import collections
import ctypes
import os
import sys

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
import dps_ref as R                                               # noqa: E402
import test_engine_trace_cpu as TR                                # noqa: E402  (the Recorder and the model table: imported, not copied)
from v_diffusion import _hip                                      # noqa: E402

F64 = torch.float64
MOTS = ("v", "eps", "x0", "both")
# the wrappers of the d/dx chain other than the GEMMs (which the weight gradients share): each must run exactly as often as in the full pass
DX_CHAIN = ("gn_apply_bwd", "attn_bwd", "softmax_rows_bwd", "conv3x3_wino43_dgrad_planes", "conv3x3_wino43_dy_image",
            "conv3x3_dgrad_wino43", "conv3x3_wino", "conv3x3", "tap_spread", "nhwc_to_nchw", "pack_conv3x3", "wino_pack")
NEVER = ("gn_param_sums_batched", "class_embed_bwd", "thin_wgrad_finish", "colsum")


# ------------------------------------------------------------------------------------------------ 1. the input-only pass: launches
def _is_dx_gemm(e):
    return e[0] == "gemm" and e[-1].get("colsum") is None and e[-1].get("splitk") in (None, 1)


def _traces(mname):
    """(launch log of the full backward pass -- scenario b of the trace test -- and of the input-only pass) on the same model and inputs"""
    import v_diffusion
    from oracle.cases import make_inputs
    cfg, B, R_, label = TR._configs()[mname]
    torch.manual_seed(0)
    eng = v_diffusion.UNet(**cfg).engine()
    x, t, y = make_inputs(cfg, B, R_, label)
    rec = TR.Recorder(_hip, eng.m)
    try:
        logs = []
        for only in (False, True):
            G = {} if only else eng.new_grads()
            rec.begin(G)
            torch.manual_seed(7)
            out, tape = eng.forward(x, t, y, True, True)
            n0 = len(rec.log)
            dx = eng.backward(tape, torch.zeros_like(out), None if only else G, need_dx=True, progress=None if only else rec.listen)
            assert dx is not None and tuple(dx.shape) == tuple(x.shape) and dx.dtype == torch.float32
            assert eng._wq is None and eng._side is None
            logs.append(rec.log[n0:])
            if only:
                # nothing parameter-shaped was made: every buffer the pass touched is an activation, a packed image or scratch
                assert not rec.grads
        return logs
    finally:
        rec.undo()


@pytest.mark.parametrize("mname", ["tinyA", "tinyC", "cifar"])
def test_the_input_only_pass_launches_the_dx_chain_and_nothing_else(mname):
    assert not [k for k in TR.KNOBS if os.environ.get(k) is not None]
    full, only = _traces(mname)
    assert not [e for e in only if e[0] == "yield"], "the input-only pass reports nothing"
    names = [e[0] for e in only]
    assert not [n for n in names if "wgrad" in n], "a weight-gradient launch"
    assert not [n for n in names if n in NEVER]
    gemms = [e for e in only if e[0] == "gemm"]
    assert gemms and all(_is_dx_gemm(e) for e in gemms), "a GEMM of the input-only pass carries a column sum or a split K"
    cf, co = collections.Counter(e[0] for e in full), collections.Counter(names)
    for w in DX_CHAIN:
        assert co[w] == cf[w], f"{w}: {co[w]} launches, the full pass has {cf[w]}"
    assert co["gn_apply_bwd"] > 0 and co["nhwc_to_nchw"] == 1
    assert set(co) <= set(DX_CHAIN) | {"gemm"}, sorted(set(co) - set(DX_CHAIN) - {"gemm"})
    # the GEMMs of the d/dx chain: those of the full pass up to the input convolution that neither sum columns nor split K
    end = max(i for i, e in enumerate(full) if e[0] == "yield" and e[1] == "in_conv.bias")
    assert len(gemms) == sum(_is_dx_gemm(e) for e in full[:end])
    # ... and the chain is the full pass's, launch for launch: the same wrappers in the same order
    chain_of = lambda log: [e[0] for e in log if e[0] in DX_CHAIN or _is_dx_gemm(e)]
    assert chain_of(only) == chain_of(full[:end]) + [e[0] for e in full[end:] if e[0] in DX_CHAIN]
    # the full pass did run what the input-only pass leaves out (the comparison is not between two empty sets)
    assert any("wgrad" in n for n in cf) and cf["gn_param_sums_batched"] == 1 and cf["colsum"] >= 1


def test_the_input_only_pass_refuses_what_it_cannot_do():
    import v_diffusion
    from oracle.cases import TINY
    eng = v_diffusion.UNet(**TINY["tinyC"]["cfg"]).engine()
    with pytest.raises(ValueError, match="need_dx"):
        eng.backward({}, None, None, need_dx=False)
    with pytest.raises(ValueError, match="progress"):
        eng.backward({}, None, None, need_dx=True, progress=lambda name: None)
    with pytest.raises(ValueError, match="backward_steps"):
        eng.backward_steps({}, None, None, need_dx=True)                 # refused at the call: there is nothing to report
    with pytest.raises(ValueError):
        eng.backward_steps({}, None, None, need_dx=False)


def test_a_saving_forward_inside_fixed_weights_packs_the_dgrad_images_once():
    """a chain runs inside fixed_weights(): a set packed for inference is re-packed, with the input-gradient images, on the FIRST saving
    forward of the context, and every later forward -- saving or not -- uses that set"""
    import v_diffusion
    from oracle.cases import make_inputs
    cfg, B, R_, label = TR._configs()["tinyA"]
    torch.manual_seed(0)
    eng = v_diffusion.UNet(**cfg).engine()
    x, t, y = make_inputs(cfg, B, R_, label)
    rec = TR.Recorder(_hip, eng.m)
    try:
        packs, later = [], []
        with eng.fixed_weights():
            for save in (False, True, True, False, True):
                rec.begin({})
                _, tape = eng.forward(x, t, y, False, save)
                packs.append((eng.packs, sum(e[0] in TR.PACKERS for e in rec.log)))
                if save:
                    assert tape["packs"] is eng.packs
                    rec.begin({})
                    eng.backward(tape, torch.zeros(B, R_, R_, 4), None, need_dx=True)
                    assert not [e for e in rec.log if e[0] in TR.PACKERS or e[0] == "wino_pack"], \
                        "the input gradient packed a residual-block image of its own: the fixed set lacks the dgrad images"
                    later.append(sum(e[0] == "pack_conv3x3" for e in rec.log))
        (p0, n0), (p1, n1), (p2, n2), (p3, n3), (p4, n4) = packs
        assert n0 > 0 and n1 > 0 and p1 is not p0, "the first saving forward packs the set with the input-gradient images"
        assert p2 is p1 and p3 is p1 and p4 is p1 and n2 == n3 == n4 == 0, "packed per step"
        assert later[1:] == [0, 0], "the input convolution's dgrad image is packed once per context too"
    finally:
        rec.undo()


# ------------------------------------------------------------------------------------------------ 2. the restatement, in fp64
def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64) * scale


def operators(shape, seed):
    """[(op, par, mask)] for images of ``shape``: both mask widths, every factor that divides the image, grey"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    ops = [("mask", None, torch.rand((B, c, H, W), generator=g, dtype=F64).round_(decimals=1)) for c in (1, C)]
    ops += [("down", f, None) for f in (2, 4, 8) if H % f == 0 and W % f == 0]
    return ops + [("gray", None, None)]


@pytest.mark.parametrize("shape", [(2, 3, 8, 16), (3, 4, 6, 10), (1, 3, 5, 5)], ids=str)
def test_the_adjoints_are_adjoint(shape):
    for op, par, mask in operators(shape, 3):
        x, r = rnd(shape, 1), rnd(R.measurement_shape(op, shape, par), 2)
        lhs, rhs = (R.apply_A(op, x, par, mask) * r).sum(), (x * R.apply_At(op, r, shape, par, mask)).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs)), (op, par, float(lhs), float(rhs))


K8 = {"v": (0.8, -0.6, 0.0), "eps": (1.25, -0.75, 0.0), "x0": (0.0, 1.0, 0.0), "both": (0.8, 0.36, -0.48)}      # (a0, b0x, b0e)


@pytest.mark.parametrize("clip", (False, True), ids=("noclip", "clip"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
def test_the_closed_form_cotangents_are_autograd_s(mot, cfg, clip):
    shape = (2, 3, 8, 8)
    B, C = shape[:2]
    k = list(K8[mot]) + [0.3, 0.7, 0.1, 1.5 if cfg else 0.0, 0.0]
    for op, par, mask in operators(shape, 11):
        xt = rnd(shape, 5, 1.2).requires_grad_(True)
        out = rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + shape[2:], 6, 1.1).requires_grad_(True)
        meas = rnd(R.measurement_shape(op, shape, par), 7)
        if clip:
            with torch.no_grad():
                p = R.branch(k, xt, out[0::2] if cfg else out, mot == "both", False)[0]
                assert 0.05 < float((p.abs() > 1).double().mean()) < 0.95, "the case saturates some elements and not all"
        res = R.residual(k, xt.detach(), out.detach(), meas, op, par, mask, mot == "both", cfg, clip)
        gx, go = torch.autograd.grad(R.loss(k, xt, out, meas, op, par, mask, mot == "both", cfg, clip).sum(), (xt, out))
        for name, got, want in (("dout", res["dout"], go), ("dxt", res["dxt"], gx)):
            assert tuple(got.shape) == tuple(want.shape)
            err = float((got - want).abs().max())
            assert err <= 1e-12 * max(1.0, float(want.abs().max())), (op, par, name, err)
        r = meas - R.apply_A(op, res["x0hat"], par, mask)
        assert torch.equal(res["sumsq"], (r * r).reshape(B, -1).sum(dim=1))


def test_the_pass_mask_includes_the_boundary():
    """torch.clamp's subgradient: 1 on [-1, 1], ends included"""
    p = torch.tensor([-1.5, -1.0, 0.0, 1.0, 1.5], dtype=F64).reshape(1, 1, 1, 5)
    k = [0.0, 1.0, 0.0, 0, 0, 0, 0.0, 0]
    assert R.branch(k, torch.zeros_like(p), p, False, True)[1].flatten().tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]
    x = p.clone().requires_grad_(True)
    x.clamp(-1.0, 1.0).sum().backward()
    assert x.grad.flatten().tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]


class Stub:
    """the pointwise stand-in network of the chain tests: a(t) x + b(t) tanh(x) + g y"""

    training = False

    def __init__(self, a=(0.3, -0.5), b=(0.4, 0.3), g=0.07, both=False):
        self.a, self.b, self.g, self.both = a, b, g, both

    def __call__(self, x, t, y):
        tc = t.to(x.dtype).reshape(-1, 1, 1, 1)
        out = (self.a[0] + self.a[1] * tc) * x + (self.b[0] + self.b[1] * tc) * torch.tanh(x)
        if y is not None:
            out = out + self.g * y.to(x.dtype).reshape(-1, 1, 1, 1)
        return torch.cat([out, 0.5 * out - 0.25 * x], dim=1) if self.both else out


def _gd(T, mot="v", w=0.0, **kw):
    import v_diffusion as vd
    return vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), T, mot, "fixed_large", "snr_trunc", "mse", w_guide=w,
                                p_uncond=0.0, **kw)


def test_a_chain_with_a_step_size_ends_nearer_the_measurement():
    """on the stand-in network, from the same draws: the mask-operator chain with zeta > 0 ends with a smaller ||meas - A x|| than the
    zeta = 0 chain (the ordinary sampler, which does not know the measurement)"""
    T, shape = 8, (2, 3, 8, 8)
    gd = _gd(T)
    row = lambda i: gd._step_coefs(i, False, True)
    mask = (torch.rand((2, 1, 8, 8), generator=torch.Generator().manual_seed(1)) < 0.5).to(F64)
    meas = mask * rnd(shape, 2, 0.5).clamp(-1, 1)
    x_T, noises = rnd(shape, 3), [rnd(shape, 10 + i) for i in range(T)]
    ends = {}
    for zeta in (0.0, 0.5):
        x = R.chain(Stub(), x_T, meas, "mask", row, noises, [zeta] * T, mask=mask, clip=True)
        ends[zeta] = float((meas - mask * x).norm())
    assert ends[0.5] < 0.9 * ends[0.0], ends


# ------------------------------------------------------------------------------------------------ 3. refusals without a device
def test_refusals_that_need_no_device():
    import v_diffusion as vd
    from v_diffusion.dps import dps_measure
    shape = (2, 3, 8, 8)
    net = Stub()
    meas = torch.zeros(shape)
    call = lambda gd, *a, **kw: gd.p_sample_dps(net, *a, **kw)
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
    with pytest.raises(ValueError, match="divide"):
        call(gd, torch.zeros(2, 3, 1, 1), ("down", 8), (2, 3, 8, 12))
    for m in (torch.ones(2, 2, 8, 8), torch.ones(3, 1, 8, 8), torch.ones(2, 1, 8, 4), torch.ones(1, 8, 8), torch.full((2, 1, 8, 8), 1.5),
              torch.full((2, 1, 8, 8), float("nan")), torch.ones(2, 1, 8, 8, dtype=torch.int32)):
        with pytest.raises(ValueError, match="mask"):
            call(gd, meas, ("mask", m), shape)
    for op, wrong in ((("gray",), shape), (("down", 2), shape), (("down", 4), (2, 3, 4, 4)), (("mask", torch.ones(1, 1, 8, 8)), (2, 1, 8, 8))):
        with pytest.raises(ValueError, match="measurement"):
            call(gd, torch.zeros(wrong), op, shape)
    with pytest.raises(ValueError, match="measurement"):
        call(gd, None, ("gray",), shape)
    gray = torch.zeros(2, 1, 8, 8)
    for z in (-1e-3, float("nan"), float("inf"), [0.1, 0.1, -0.1, 0.1], [0.1, float("inf"), 0.1, 0.1]):
        with pytest.raises(ValueError, match="finite"):
            call(gd, gray, ("gray",), shape, zeta=z)
    for z in ([0.1] * 3, [0.1] * 5, [], "1.0", [0.1, 0.1, 0.1, "x"]):
        with pytest.raises(ValueError, match="zeta"):
            call(gd, gray, ("gray",), shape, zeta=z)
    with pytest.raises(RuntimeError, match="MI355X"):                      # CPU tensors, after everything else passed
        call(gd, gray, ("gray",), shape, zeta=[0.1] * 4)
    # dps_measure: plain torch, the shapes of A's image
    x = rnd(shape, 1)
    assert tuple(dps_measure(x, ("down", 4)).shape) == (2, 3, 2, 2) and tuple(dps_measure(x, ("gray",)).shape) == (2, 1, 8, 8)
    for op, par, mask in operators(shape, 4):
        arg = {"mask": ("mask", mask), "down": ("down", par), "gray": ("gray",)}[op]
        assert torch.allclose(dps_measure(x, arg), R.apply_A(op, x, par, mask), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="operator"):
        dps_measure(x, ("blur",))


def test_the_names_are_exported_and_inherited():
    import v_diffusion as vd
    for name in ("dps_measure", "p_sample_dps"):
        assert name in vd.__all__ and name in vd._HOT and callable(getattr(vd, name))
    assert vd.DistillationDiffusion.p_sample_dps is vd.GaussianDiffusion.p_sample_dps
    assert callable(vd.UNet.forward_vjp)
    assert _hip.DPS_OPS == {"mask": 0, "down": 1, "gray": 2}


# ------------------------------------------------------------------------------------------------ 4. the C entries
def test_the_entries_refuse_before_any_launch():
    """bad model_out_type or op, a null required buffer, n, C, H, W < 1, a mask width that is neither 1 nor C, a factor outside
    {2, 4, 8} or not dividing the image: 1, with the reason, and nothing launched (the addresses are never dereferenced)"""
    lib = _hip.lib()
    err = lambda: lib.vd_last_error().decode(errors="replace")
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf) // 16 * 16 + 16
    k = (ctypes.c_float * 8)(0.8, -0.6, 0.0, 0.3, 0.7, 0.1, 0.0, 0.0)
    res, stp = lib.vd_dps_residual, lib.vd_dps_step
    good = dict(xt=a, out=a, meas=a, mask=a, k=k, type=0, cfg=0, clip=1, op=0, par=1, dout=a, dxt=a, sumsq=a, x0hat=None, n=1, C=3, H=4,
                W=4, stream=None)
    def r(**kw):
        return res(*{**good, **kw}.values())
    assert r(type=4) == 1 and "model_out_type" in err() and r(type=-1) == 1
    assert r(op=3) == 1 and "bad op" in err() and r(op=-1) == 1
    for name in ("xt", "out", "meas", "mask", "k", "dout", "dxt", "sumsq"):
        assert r(**{name: None}) == 1 and "null" in err(), name
    for name in ("n", "C", "H", "W"):
        assert r(**{name: 0}) == 1 and "empty" in err(), name
    assert r(par=2) == 1 and "channels" in err()
    for f, H, W in ((3, 6, 6), (16, 16, 16), (1, 4, 4), (2, 5, 4), (4, 8, 6), (8, 8, 12)):
        assert r(op=1, par=f, H=H, W=W) == 1 and "down-sampling" in err(), (f, H, W)
    gs = dict(xt=a, out=a, noise=a, dxin=a, dxt=a, sumsq=a, k=k, zeta=ctypes.c_float(0.5), type=0, cfg=0, last=0, clip=1, xn=a, xdup=None,
              n=1, C=3, HW=16, stream=None)
    def s(**kw):
        return stp(*{**gs, **kw}.values())
    assert s(type=7) == 1 and "model_out_type" in err()
    for name in ("xt", "out", "dxin", "dxt", "sumsq", "k", "xn"):
        assert s(**{name: None}) == 1 and "null" in err(), name
    for name in ("n", "C", "HW"):
        assert s(**{name: 0}) == 1 and "empty" in err(), name
    assert s(noise=None) == 1 and "noise" in err()
