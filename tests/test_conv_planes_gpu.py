"""The forward 3x3 convolution through PLANES (csrc/wino43.hip: V transform -> 36 plane GEMMs on the split-operand tile engine -> output
transform), the weight gradient that takes its V image as given, the engine step that runs both, and the host rule that picks them.

Forward tolerance: the fused F(4x4,3x3) forward kernel's own error against fp64 on the same inputs, measured in the same test, times 1.5
(the split products run at 0.6-0.9 of the fp32 chain's error; the margin covers the different summation order of the output pass).

Which form of the tile engine each shape runs (vd_gemm_plan_tile at M = tiles, N = Cout, K = Cin, batch 36; pinned without a device by
test_plans_of_the_forward_shapes, asserted from vd_gemm_last_tile after every launch of FORM_CASES):
  FWD_CASES (128-256 tiles, Cin, Cout <= 64)    all four: the 64x64 fp32 tile -- they cover the three launches' plumbing, the fused-kernel
                                                yardstick and the image geometries, and NOT the blocked-row A addressing of a 128-row tile
  FORM_CASES                                    gemm_split_kernel, A rows in blocks of 16 (vd_gemm_rowblk), a ragged last row tile:
    (121, 16, 16, 40, 256)                        128x256 KT = 16, one column tile, 16 row tiles (last: 16 rows), K = 16 + 16 + 8
    (57, 16, 16, 24, 512), ldx = Cin + 8          128x256 KT = 16, two column tiles, 8 row tiles (last: 16 rows), K = 16 + 8
    (121, 16, 16, 40, 384)                        128x128 KT = 16 (1728 workgroups), output transform grid.y = 6
    (121, 16, 16, 36, 128), ldx = Cin + 4         128x128 KT = 32 (576 workgroups), K = 32 + 4
    (15, 32, 32, 16, 512)                         128x256 KT = 16, last row tile 64 rows, one image per statistics chunk
    (8, 64, 64, 16, 256)                          128x256 KT = 16, full row tiles, four statistics chunks per image
    (3, 16, 16, 36, 96), ldx = Cin + 4            64x64 fp32 tile; output transform grid.y = 2 with a half-filled second block, 3 images
  Their tolerance is test_kernels_gpu.py::test_conv3x3_wino43_fwd's per-layer bound: 8 x the error torch's own fp32 convolution has against
  fp64 on the same inputs, floor 4e-6 of the largest value.
  test_weight_gradient_with_v_given_is_bitwise: V of its last case is written beside a 128x256 forward, the forwards of the other four run
  the 64x64 tile (the weight gradient reads V, whatever form the forward's GEMMs took)."""
import functools
import math
import os
import subprocess
import sys

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


def close(got, ref64, ref32=None, slack=4.0, floor=2e-6, name=""):           # as in test_kernels_gpu.py
    """|got - ref64| must be within `slack` x the error torch's own fp32 result has (plus a relative floor)."""
    got = got.detach().cpu().double()
    ref64 = ref64.detach().double()
    scale = max(ref64.abs().max().item(), 1e-30)
    err = (got - ref64).abs().max().item()
    nat = 0.0 if ref32 is None else (ref32.detach().double() - ref64).abs().max().item()
    tol = slack * nat + floor * scale
    assert math.isfinite(err) and err <= tol, f"{name}: max err {err:.3e} > tol {tol:.3e} (natural fp32 noise {nat:.3e}, scale {scale:.3e})"
    return err


# ---------------------------------------------------------------------------------------------- the forms of the 36 plane GEMMs
# (split-operand form, K tile, BM, BN) of _hip.tile_fields, without the epilogue flag
WIDE, SPLIT16, SPLIT32, SMALL = (True, 16, 128, 256), (True, 16, 128, 128), (True, 32, 128, 128), (False, 32, 64, 64)
# ((nimg, H, W, Cin, Cout, ldx - Cin), form): the smallest shapes that reach each 128-row form of plan_gemm (csrc/gemm.hip) with a last row
# tile of 16 rows (tiles % 128 == 16) -- see the head of this file.  A = V is addressed in blocks of 16 rows on all of them.
FORM_CASES = [((121, 16, 16, 40, 256, 0), WIDE), ((57, 16, 16, 24, 512, 8), WIDE), ((121, 16, 16, 40, 384, 0), SPLIT16),
              ((121, 16, 16, 36, 128, 4), SPLIT32), ((15, 32, 32, 16, 512, 0), WIDE), ((8, 64, 64, 16, 256, 0), WIDE),
              ((3, 16, 16, 36, 96, 4), SMALL)]
GUARD, GUARD_FILL = 4096, -777.0           # floats in front of and behind V and the workspace, and what they hold


def _inputs(case):
    nimg, Hh, Ww, Cin, Cout, _ = case
    return (rnd(nimg, Cin, Hh, Ww, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=3),
            rnd(nimg, Cout, Hh, Ww, seed=4))


@functools.lru_cache(maxsize=2)
def _conv64(case):
    """fp64 F.conv2d of the case's inputs without bias: computed once, shared by both variants (at most 8.6 GFLOP)"""
    x, w, _, _ = _inputs(case)
    return F.conv2d(x.double(), w.double(), padding=1)


def _guarded(nfloats):
    whole = torch.full((nfloats + 2 * GUARD,), GUARD_FILL, device=DEV)
    return whole, whole[GUARD:GUARD + nfloats]


def _guards_intact(whole):
    return bool((whole[:GUARD] == GUARD_FILL).all()) and bool((whole[-GUARD:] == GUARD_FILL).all())


class _PlanesCall:
    """vd_conv3x3_wino43_fwd_planes called through the C ABI on device copies of the case's inputs, with V and the workspace allocated at
    EXACTLY vd_conv3x3_wino43_v_floats / vd_conv3x3_wino43_fwd_planes_ws_bytes inside guard zones (a row-tile store past M in the last plane,
    or a V store past the last block, lands in one)"""
    def __init__(self, H, case, full):
        nimg, Hh, Ww, Cin, Cout, ex = case
        self.H, self.case, self.lib = H, case, H.lib()
        self.ldres = Cout + 8 if full else 0
        x, w, b, res = _inputs(case)
        self.xd, self.wd = nhwc(x, Cin + ex), w.to(DEV)
        self.bd = b.to(DEV) if full else None
        self.rd = nhwc(res, self.ldres) if full else None
        self.ws_bytes = self.lib.vd_conv3x3_wino43_fwd_planes_ws_bytes(nimg, Hh, Ww, Cin, Cout)
        assert self.ws_bytes % 4 == 0
        self.v_whole, self.v = _guarded(self.lib.vd_conv3x3_wino43_v_floats(nimg, Hh, Ww, Cin))
        self.ws_whole, self.ws = _guarded(self.ws_bytes // 4)

    def launch(self, part=None):
        """-> (y at ldy = Cout + 4, pre-filled with 5; form of the plane GEMMs from vd_gemm_last_tile)"""
        nimg, Hh, Ww, Cin, Cout, ex = self.case
        H = self.H
        y = torch.full((nimg, Hh, Ww, Cout + 4), 5.0, device=DEV)
        rc = self.lib.vd_conv3x3_wino43_fwd_planes(H.ptr(self.xd), Cin + ex, H.ptr(self.wd), H.ptr(self.bd), H.ptr(self.rd), self.ldres, H.ptr(y),
                                                   Cout + 4, nimg, Hh, Ww, Cin, Cout, H.ptr(part), H.ptr(self.v), H.ptr(self.ws), self.ws_bytes,
                                                   7, H.stream())
        assert rc == 0, self.lib.vd_last_error().decode(errors="replace")
        form = H.tile_fields(self.lib.vd_gemm_last_tile())[1:]
        torch.cuda.synchronize()
        return y, form

    def guards_intact(self):
        return _guards_intact(self.v_whole), _guards_intact(self.ws_whole)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [True, False], ids=["bias_res_stats", "plain"])
@pytest.mark.parametrize("case,form", FORM_CASES)
def test_forward_planes_forms_vs_fp64(H, case, form, full):
    """The forward through planes on each form of the tile engine the planner can send the 36 plane GEMMs to, against fp64 F.conv2d
    (+ bias + residual) within test_conv3x3_wino43_fwd's per-layer bound (8 x torch's own fp32 error, floor 4e-6); the form that ran is
    asserted, V and the workspace sit between guard zones, padding channels of y stay, the launch is bitwise reproducible, the GroupNorm
    partials are the statistics of what was written."""
    nimg, Hh, Ww, Cin, Cout, ex = case
    HW = Hh * Ww
    call = _PlanesCall(H, case, full)
    assert call.lib.vd_conv3x3_wino43_fwd_planes_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout + 4, call.ldres) == 1
    x, w, b, res = _inputs(case)
    if full:
        ref64 = _conv64(case) + b.double()[None, :, None, None] + res.double()
        ref32 = F.conv2d(x, w, b, padding=1) + res
    else:
        ref64, ref32 = _conv64(case), F.conv2d(x, w, padding=1)
    chunks = HW // H.wino43_fwd_chunk_rows(Hh, Ww)
    part = torch.full((H.stats_part_numel(nimg, HW, Cout),), 7.0, device=DEV) if full else None
    y, ran = call.launch(part)
    y2, ran2 = call.launch(None)
    assert call.guards_intact() == (True, True), "a store outside V / outside the workspace (V, workspace)"
    assert ran == form and ran2 == form, f"the plane GEMMs ran {ran}, the case is meant for {form}"
    assert torch.equal(y, y2), "not bitwise reproducible / statistics-free launch differs"
    assert (y[..., Cout:] == 5.0).all(), "padding channels of y were written"
    rel, mx = errs(y, Cout, ref64)
    nat = (ref32.double() - ref64).abs().max().item()
    print(f"planes form {ran} code {call.lib.vd_gemm_last_tile()} {case} full={full}: rel-L2 {rel:.3e}, max-abs {mx:.3e} (torch fp32: {nat:.3e})")
    close(y[..., :Cout].permute(0, 3, 1, 2), ref64, ref32, slack=8.0, floor=4e-6, name="planes forward")
    if full:
        used = nimg * chunks * 2 * Cout
        assert (part[used:] == 7.0).all(), "statistics written past [nimg][chunks][2][Cout]"
        stats = torch.empty(nimg, 32, 2, device=DEV)
        H.gn_stats_from_partials([(part, Cout, chunks)], nimg, HW, stats)
        g = y[..., :Cout].permute(0, 3, 1, 2).double().cpu().reshape(nimg, 32, -1)           # statistics of what was WRITTEN
        mean, rstd = g.mean(-1), 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-6)
        for got, want, floor, name in ((stats[..., 0], mean, 2e-6, "mean"), (stats[..., 1], rstd, 5e-6, "rstd")):
            err = (got.double().cpu() - want).abs().max().item()
            assert err <= floor * want.abs().max().item(), f"{name}: {err:.3e}"


def _plain_ys(H):
    """{case: (y of the plain variant on the CPU, form)} of the two 128x256 cases with a 16-row last tile"""
    out = {}
    for case, _ in FORM_CASES[:2]:
        y, form = _PlanesCall(H, case, False).launch()
        out[case] = (y.cpu(), form)
    return out


@pytest.mark.gpu
def test_wide_form_is_bitwise_the_128x128_form(H, tmp_path):
    """csrc/gemm.hip: the 128x256 form runs the same instruction sequence per output element as the 128x128 KT = 16 split form.  One child
    process with VD_GEMM_BN256=0 (read once per process) runs the two wide cases on that form; this process runs them under defaults."""
    out = str(tmp_path / "y128.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, VD_GEMM_BN256="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    child = torch.load(out)
    for case, (y, form) in _plain_ys(H).items():
        assert form == WIDE, (case, form)
        y128 = child[str(case)]
        print(f"wide vs 128x128 {case}: {form} against {SPLIT16}, max |difference| {(y - y128).abs().max().item():.3e}")
        assert torch.equal(y, y128), f"{case}: the 128x256 form differs from the 128x128 KT = 16 form"


def test_plans_of_the_forward_shapes():
    """Without a device: every FORM_CASES shape plans to the form its GPU test asserts (a planner change that moves one shows here first),
    and -- a statement about coverage -- the four FWD_CASES all plan to the 64x64 fp32 tile."""
    from v_diffusion import _hip
    lib = _hip.lib()
    assert not [k for k in ("VD_GEMM_TILE", "VD_GEMM_KT", "VD_GEMM_SPLIT", "VD_GEMM_BN256", "VD_GEMM_LEGACY") if os.environ.get(k) is not None]

    def plan(case):
        nimg, Hh, Ww, Cin, Cout, _ = case
        code = lib.vd_gemm_plan_tile(nimg * (Hh // 4) * (Ww // 4), Cout, Cin, _hip.ROW, _hip.ROW, 36, 0, 0)
        assert code > 0, lib.vd_last_error()
        return _hip.tile_fields(code)[1:]
    for case, form in FORM_CASES:
        assert plan(case) == form, (case, plan(case), form)
        if form[2] == 128:
            assert (case[0] * (case[1] // 4) * (case[2] // 4)) % 128 in (0, 16, 64)      # (full tiles, a 16-row and a 64-row last tile)
    assert {form for _, form in FORM_CASES} == {WIDE, SPLIT16, SPLIT32, SMALL}
    for case in FWD_CASES:
        assert plan(case) == SMALL, (case, plan(case))


# ---------------------------------------------------------------------------------------------- weight gradient with V given
@functools.lru_cache(maxsize=2)
def _wgrad64(case):
    """fp64 autograd of F.conv2d with respect to weight and bias on the case's x and dy"""
    nimg, Hh, Ww, Cin, Cout, _ = case
    x, dy = rnd(nimg, Cin, Hh, Ww, seed=1), rnd(nimg, Cout, Hh, Ww, seed=5)
    w64 = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b64 = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, b64, padding=1).backward(dy.double())
    return w64.grad, b64.grad


# (nimg, H, W, Cin, Cout, ldx - Cin).  nimg 32 at 16x16 = 512 tiles: the floor the F(4x4,3x3) weight gradient serves; V made from a pitched
# input; the 64-wide geometry at that floor; V written beside a 128x256 forward with a 16-row last row tile
@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", [(32, 16, 16, 32, 64, 0), (8, 32, 32, 64, 32, 0), (32, 16, 16, 40, 64, 8), (2, 64, 64, 32, 32, 0),
                                  (121, 16, 16, 40, 256, 0)])
def test_weight_gradient_with_v_given_is_bitwise(H, case, accumulate):
    """bitwise the weight gradient that transforms x itself, and inside test_kernels_gpu.py::test_conv3x3_wgrad_wino43's bounds of fp64
    autograd (dw: relative L2 8e-6, 4e-5 of the largest element; dbias: 2e-5 of the largest element, at least of 1); an accumulating
    run adds exactly that much to what the buffers held, within the same bounds"""
    nimg, Hh, Ww, Cin, Cout, ex = case
    lib = H.lib()
    assert H.wgrad43_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout)
    xd = nhwc(rnd(nimg, Cin, Hh, Ww, seed=1), Cin + ex)
    dyd = nhwc(rnd(nimg, Cout, Hh, Ww, seed=5), Cout)
    wd = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5).to(DEV)
    y = torch.empty(nimg, Hh, Ww, Cout, device=DEV)
    v = torch.empty(lib.vd_conv3x3_wino43_v_floats(nimg, Hh, Ww, Cin), device=DEV)
    H.conv3x3_wino43_fwd_planes(xd, Cin + ex, wd, None, y, Cout, nimg, Hh, Ww, Cin, Cout, v=v)
    if case == FORM_CASES[0][0]:
        assert H.tile_fields(lib.vd_gemm_last_tile())[1:] == WIDE
    init_w, init_b = rnd(Cout, Cin, 3, 3, seed=6).to(DEV), rnd(Cout, seed=7).to(DEV)
    dw0, db0, dw1, db1 = init_w.clone(), init_b.clone(), init_w.clone(), init_b.clone()
    H.conv3x3_wgrad(xd, Cin + ex, dyd, Cout, nimg, Hh, Ww, Cin, Cout, dw0, Cin, Cout, accumulate=accumulate, dbias=db0)
    H.conv3x3_wgrad(None, Cin, dyd, Cout, nimg, Hh, Ww, Cin, Cout, dw1, Cin, Cout, accumulate=accumulate, dbias=db1, v=v)
    torch.cuda.synchronize()
    assert torch.isfinite(dw0).all() and not torch.equal(dw0, init_w)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    ref_w, ref_b = _wgrad64(case)
    if accumulate:          # what the run added = the non-accumulating result; the rest must be what the buffers held
        dwn, dbn = torch.empty_like(dw1), torch.empty_like(db1)
        H.conv3x3_wgrad(None, Cin, dyd, Cout, nimg, Hh, Ww, Cin, Cout, dwn, Cin, Cout, accumulate=False, dbias=dbn, v=v)
        torch.cuda.synchronize()
        got_w, want_w = (dw1.double() - dwn.double()).cpu(), init_w.double().cpu()
        got_b, want_b = (db1.double() - dbn.double()).cpu(), init_b.double().cpu()
    else:
        got_w, want_w, got_b, want_b = dw1.double().cpu(), ref_w, db1.double().cpu(), ref_b
    rel = ((got_w - want_w).norm() / ref_w.norm()).item()
    mx = (got_w - want_w).abs().max().item()
    eb = (got_b - want_b).abs().max().item()
    print(f"wgrad with V given {case} accumulate={accumulate}: dw rel-L2 {rel:.3e}, max-abs {mx:.3e} of {ref_w.abs().max().item():.2f}, "
          f"dbias max-abs {eb:.3e} of {ref_b.abs().max().item():.2f}")
    assert rel <= 8e-6 and mx <= 4e-5 * ref_w.abs().max().item(), (rel, mx)
    assert eb <= 2e-5 * max(ref_b.abs().max().item(), 1.0), eb


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


if __name__ == "__main__":          # the VD_GEMM_BN256=0 child of test_wide_form_is_bitwise_the_128x128_form: argv[1] = where its y go
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "v-diffusion-torch_amd")]
    from v_diffusion import _hip
    assert os.environ.get("VD_GEMM_BN256") == "0" and len(sys.argv) == 2, __doc__
    ys = _plain_ys(_hip)
    for _case, (_y, _form) in ys.items():
        assert _form == SPLIT16, f"{_case}: ran {_form}, not the 128x128 KT = 16 split form"
    torch.save({str(c): y for c, (y, _) in ys.items()}, sys.argv[1])
