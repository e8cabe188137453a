"""The forward 3x3 convolution through PLANES (csrc/wino43.hip: V transform -> 36 plane GEMMs on the split-operand tile engine -> output
transform), the weight gradient that takes its V image as given, the engine step that runs both, and the host rule that picks them.

Forward tolerance: the fused F(4x4,3x3) forward kernel's own error against fp64 on the same inputs, measured in the same test, times 1.5
(the split products run at 0.6-0.9 of the fp32 chain's error; the margin covers the different summation order of the output pass)."""
import math

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 7919 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float()


def nhwc(x, ld, fill=3.0):
    """NCHW CPU tensor -> NHWC device tensor with channel pitch ld (padding channels hold `fill`)"""
    n, c, h, w = x.shape
    out = torch.full((n, h, w, ld), fill, device=DEV)
    out[..., :c] = x.permute(0, 2, 3, 1).to(DEV)
    return out


def errs(y_nhwc, C, ref64):
    got = y_nhwc[..., :C].permute(0, 3, 1, 2).double().cpu()
    return ((got - ref64).norm() / ref64.norm()).item(), (got - ref64).abs().max().item()


# (nimg, H, W, Cin, Cout, ldx - Cin): four 16x16 images per fused work item and several row tiles of the plane GEMMs; one 32x32 image per
# statistics chunk; the 64-wide form (W = 64: two chunks of 16 rows per image); a channel-concatenated input (ldx > Cin)
FWD_CASES = [(8, 16, 16, 32, 64, 0), (4, 32, 32, 64, 32, 0), (2, 32, 64, 32, 32, 0), (8, 16, 16, 64, 32, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("full", [True, False], ids=["bias_res_stats", "plain"])
@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_planes_vs_fp64(H, case, full):
    nimg, Hh, Ww, Cin, Cout, ex = case
    HW, ey = Hh * Ww, (8 if full else 0)
    lib = H.lib()
    assert lib.vd_conv3x3_wino43_fwd_planes_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout, Cout + ey) == 1
    assert lib.vd_conv3x3_wino43_fwd_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout, Cout + ey) == 1
    x = rnd(nimg, Cin, Hh, Ww, seed=1)
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    b, res = rnd(Cout, seed=3), rnd(nimg, Cout, Hh, Ww, seed=4)
    ref64 = F.conv2d(x.double(), w.double(), b.double() if full else None, padding=1) + (res.double() if full else 0.0)
    xd, wd = nhwc(x, Cin + ex), w.to(DEV)
    bd = b.to(DEV) if full else None
    rd = nhwc(res, Cout + ey) if full else None
    # the fused kernel on the same inputs: the yardstick
    u43f = torch.empty(lib.vd_wino43_u_floats(Cout, Cin), device=DEV)
    H.wino43_pack_fwd(wd, Cout, Cin, u43f)
    yf = torch.empty(nimg, Hh, Ww, Cout, device=DEV)
    H.conv3x3_wino43_fwd(xd, Cin + ex, u43f, bd, yf, Cout, nimg, Hh, Ww, Cin, Cout, res=rd, ldres=Cout + ey)
    # through planes
    yp = torch.full((nimg, Hh, Ww, Cout + 4), 5.0, device=DEV)
    part = torch.full((H.stats_part_numel(nimg, HW, Cout),), 7.0, device=DEV) if full else None
    v = torch.empty(lib.vd_conv3x3_wino43_v_floats(nimg, Hh, Ww, Cin), device=DEV)
    H.conv3x3_wino43_fwd_planes(xd, Cin + ex, wd, bd, yp, Cout + 4, nimg, Hh, Ww, Cin, Cout, res=rd, ldres=Cout + ey, stats_part=part, v=v)
    yp2 = torch.full_like(yp, 5.0)
    H.conv3x3_wino43_fwd_planes(xd, Cin + ex, wd, bd, yp2, Cout + 4, nimg, Hh, Ww, Cin, Cout, res=rd, ldres=Cout + ey)
    torch.cuda.synchronize()
    assert torch.equal(yp, yp2), "not bitwise reproducible / statistics-free launch differs"
    assert (yp[..., Cout:] == 5.0).all(), "padding channels of y were written"
    rel_f, max_f = errs(yf, Cout, ref64)
    rel_p, max_p = errs(yp, Cout, ref64)
    print(f"planes vs fused {case} full={full}: rel-L2 {rel_p:.3e} / {rel_f:.3e} = {rel_p / rel_f:.2f}, max-abs {max_p:.3e} / {max_f:.3e} = "
          f"{max_p / max_f:.2f}")
    assert math.isfinite(rel_p) and rel_p <= 1.5 * rel_f and max_p <= 1.5 * max_f, (rel_p, rel_f, max_p, max_f)
    if full:
        rows = H.wino43_fwd_chunk_rows(Hh, Ww)
        stats = torch.empty(nimg, 32, 2, device=DEV)
        H.gn_stats_from_partials([(part, Cout, HW // rows)], nimg, HW, stats)
        g = yp[..., :Cout].permute(0, 3, 1, 2).double().cpu().reshape(nimg, 32, -1)          # statistics of what was WRITTEN
        mean, rstd = g.mean(-1), 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-6)
        for got, want, floor, name in ((stats[..., 0], mean, 2e-6, "mean"), (stats[..., 1], rstd, 5e-6, "rstd")):
            err = (got.double().cpu() - want).abs().max().item()
            assert err <= floor * want.abs().max().item(), f"{name}: {err:.3e}"


# nimg 32 at 16x16 = 512 tiles: the floor the F(4x4,3x3) weight gradient serves
@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", [(32, 16, 16, 32, 64), (8, 32, 32, 64, 32)])
def test_weight_gradient_with_v_given_is_bitwise(H, case, accumulate):
    nimg, Hh, Ww, Cin, Cout = case
    lib = H.lib()
    assert H.wgrad43_supported(nimg, Hh, Ww, Cin, Cout, Cin, Cout)
    xd = nhwc(rnd(nimg, Cin, Hh, Ww, seed=1), Cin)
    dyd = nhwc(rnd(nimg, Cout, Hh, Ww, seed=5), Cout)
    wd = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5).to(DEV)
    y = torch.empty(nimg, Hh, Ww, Cout, device=DEV)
    v = torch.empty(lib.vd_conv3x3_wino43_v_floats(nimg, Hh, Ww, Cin), device=DEV)
    H.conv3x3_wino43_fwd_planes(xd, Cin, wd, None, y, Cout, nimg, Hh, Ww, Cin, Cout, v=v)
    init_w, init_b = rnd(Cout, Cin, 3, 3, seed=6).to(DEV), rnd(Cout, seed=7).to(DEV)
    dw0, db0, dw1, db1 = init_w.clone(), init_b.clone(), init_w.clone(), init_b.clone()
    H.conv3x3_wgrad(xd, Cin, dyd, Cout, nimg, Hh, Ww, Cin, Cout, dw0, Cin, Cout, accumulate=accumulate, dbias=db0)
    H.conv3x3_wgrad(None, Cin, dyd, Cout, nimg, Hh, Ww, Cin, Cout, dw1, Cin, Cout, accumulate=accumulate, dbias=db1, v=v)
    torch.cuda.synchronize()
    assert torch.isfinite(dw0).all() and not torch.equal(dw0, init_w)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)


@pytest.mark.gpu
def test_tiny_train_step_through_planes(H):
    """tinyA at B = 32 (512 tiles at 16x16: its four 16x16 convolutions go through planes and keep V under CONV_PLANES = 2) against the same
    step with CONV_PLANES = 0, inside the bound tests/test_unet_gpu.py holds F(4x4,3x3) against F(2x2,3x3) to (output 2e-5; gradients
    L2 <= 1e-4 |ref| + 1e-6 gmax)"""
    import v_diffusion
    from oracle import detrand
    from oracle.cases import TINY, make_inputs, make_weights
    case = TINY["tinyA"]
    cfg, B, R = case["cfg"], 32, case["R"]
    sd = make_weights(cfg)
    x, t, y = make_inputs(cfg, B, R, case["label"])
    gout = detrand.normal("gout", (B, cfg["out_channels"], R, R), 1)
    saved, calls = H.CONV_PLANES, [0]
    real = H.conv3x3_wino43_fwd_planes

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    H.conv3x3_wino43_fwd_planes = spy
    try:
        runs = {}
        for mode in ("0", "2"):
            H.CONV_PLANES = mode
            calls[0] = 0
            model = v_diffusion.UNet(**cfg)
            model.load_state_dict(sd)
            model.to(DEV).train()
            out = model(x.to(DEV), t.to(DEV), y.to(DEV))
            loss = (out * gout.to(DEV)).sum()
            loss.backward()
            torch.cuda.synchronize()
            runs[mode] = (out.detach().cpu(), loss.item(), {k: p.grad.cpu() for k, p in model.named_parameters()}, calls[0])
    finally:
        H.CONV_PLANES, H.conv3x3_wino43_fwd_planes = saved, real
    (o0, l0, g0, n0), (o2, l2, g2, n2) = runs["0"], runs["2"]
    assert n0 == 0 and n2 > 0, (n0, n2)
    assert (o0 - o2).abs().max().item() <= 2e-5
    assert abs(l0 - l2) <= 2e-5 * gout.abs().sum().item()      # (loss = sum(out * gout): what the output bound allows it to move)
    gmax = max(g.norm().item() for g in g0.values())
    for k in g0:
        e = (g0[k].double() - g2[k].double()).norm().item()
        assert e <= 1e-4 * g0[k].double().norm().item() + 1e-6 * gmax, f"{k}: L2 error {e:.3e} vs |grad| {g0[k].norm().item():.3e}"


def test_planes_rule_is_off_at_small_batches_and_on_where_measured():
    """vd_conv3x3_fwd_planes_preferred needs no device: false for every (batch, geometry) of the engine-trace scenarios
    (tests/test_engine_trace_cpu.py: batches 1-3, whose recorded launches must not move), true at the bench shapes that measured faster
    (profiles/r08_conv_planes_geometries.txt)"""
    import v_diffusion
    from v_diffusion import _hip
    from oracle.cases import CIFAR_COND, CELEBA, TINY
    pref = _hip.lib().vd_conv3x3_fwd_planes_preferred
    scen = [(v["cfg"], v["B"], v["R"]) for v in TINY.values()] + [(CIFAR_COND, 2, 32), (CELEBA, 1, 64)]
    for cfg, B, R in scen:
        eng = v_diffusion.UNet(**cfg).engine()
        for _, nb, lh, lw, ci, co in eng._conv_geoms(B, R, R):
            for training in (0, 1):
                assert pref(nb, lh, lw, ci, co, training) == 0, (B, lh, lw, ci, co, training)
    assert _hip.CONV_PLANES == "1", "the suite runs the product default (VD_CONV_PLANES unset)"
    for (nimg, hw, ci, co), want in PLANES_MEASURED.items():
        assert pref(nimg, hw, hw, ci, co, 1) == want, (nimg, hw, ci, co)
    # the B = 64 training step keeps the fused kernel (its launches are counted by tests/test_bench_shapes_gpu.py)
    assert pref(64, 32, 32, 256, 256, 1) == 0 and pref(64, 16, 16, 256, 256, 1) == 0
    # inference forwards stay on the fused kernel (no geometry measured clearly faster alone)
    assert pref(128, 32, 32, 256, 256, 0) == 0 and pref(256, 32, 32, 512, 256, 0) == 0


# (nimg, H = W, Cin, Cout) -> does the training step take the planes path (forward + weight-gradient pair measured faster)?
PLANES_MEASURED = {(128, 32, 256, 256): 1, (128, 32, 512, 256): 1, (128, 16, 256, 256): 0, (128, 16, 512, 256): 0}
