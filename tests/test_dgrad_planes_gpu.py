"""The 3x3 input gradient through PLANES (csrc/wino43.hip: dM = A dY A^T, the weight gradient's image of dy -> 36 plane GEMMs on the tile
engine -> overlap-add pass wino43_in_transpose_kernel), the entry that writes dM into a caller's buffer, the weight gradient that takes
both images as given, and the engine step that runs them.

Truth: fp64 autograd of F.conv2d with respect to its input.  Bounds: those of test_kernels_gpu.py::test_conv3x3_dgrad_wino43 (relative L2
<= 1.5e-5, max error <= 6e-5 of the largest element), and -- wherever the fused F(4x4,3x3) input-gradient kernel serves the geometry
(Cin % 32 == 0, Cout % 8 == 0, 16x16 images in fours) -- both errors at most 1.5 x the fused kernel's on the same inputs, the
planes-forward test's margin.

Form of the 36 plane GEMMs (vd_gemm_plan_tile at M = tiles, N = Cin, K = Cout, batch 36; pinned without a device by
tests/test_dgrad_planes_cpu.py, asserted from vd_gemm_last_tile after every launch): the first five cases are too small to fill the chip
twice with 128-row tiles and plan to the 64x64 fp32 tile; the last two are the smallest that reach the 128x256 split-operand form the
training step runs, with A = dM addressed in blocks of 16 rows (vd_gemm_rowblk) and a ragged last row tile."""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
WIDE, SMALL = (True, 16, 128, 256), (False, 32, 64, 64)       # (split-operand form, K tile, BM, BN) of _hip.tile_fields
# ((nimg, H, W, Cin, Cout, lddy - Cout, lddx - Cin), form)
CASES = [((1, 16, 16, 4, 4, 0, 0), SMALL),          # every tile is a border tile, one channel quad
         ((3, 32, 32, 24, 40, 8, 32), SMALL),       # pitched on both sides; a half-filled second channel slice
         ((2, 32, 32, 256, 64, 0, 0), SMALL),       # N = 256, one row tile of 128 tiles
         ((5, 16, 16, 512, 32, 0, 0), SMALL),       # T = 80: a ragged row tile; eight channel slices of 64
         ((4, 32, 32, 96, 256, 0, 0), SMALL),       # six channel slices of 16; Cin no multiple of 64
         ((124, 16, 16, 256, 40, 0, 0), WIDE),      # 128x256, one column tile, 16 row tiles (last: 64 rows), K = 16 + 16 + 8
         ((60, 16, 16, 512, 24, 0, 4), WIDE)]       # 128x256, two column tiles, 8 row tiles (last: 64 rows), K = 16 + 8; pitched dx
GUARD, GUARD_FILL = 4096, -777.0
REL_BOUND, MAX_BOUND, RATIO = 1.5e-5, 6e-5, 1.5


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
    n, c, h, w = x.shape
    out = torch.full((n, h, w, ld), fill, device=DEV)
    out[..., :c] = x.permute(0, 2, 3, 1).to(DEV)
    return out


def _guarded(nfloats, fill=GUARD_FILL):
    whole = torch.full((nfloats + 2 * GUARD,), GUARD_FILL, device=DEV)
    whole[GUARD:GUARD + nfloats] = fill
    return whole, whole[GUARD:GUARD + nfloats]


def _guards_intact(whole):
    return bool((whole[:GUARD] == GUARD_FILL).all()) and bool((whole[-GUARD:] == GUARD_FILL).all())


def _dgrad64(dy, w, Cin):
    """fp64 autograd of F.conv2d with respect to its input"""
    x64 = torch.zeros(dy.shape[0], Cin, dy.shape[2], dy.shape[3], dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w.double(), padding=1).backward(dy.double())
    return x64.grad


@functools.lru_cache(maxsize=2)
def _case_data(case):
    nimg, Hh, Ww, Cin, Cout = case[:5]
    dy, w = rnd(nimg, Cout, Hh, Ww, seed=5), rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    return dy, w, _dgrad64(dy, w, Cin)


class _Call:
    """the three entries through the C ABI; dM, the workspace and dx sit at EXACTLY their sizes between guard zones"""
    def __init__(self, H, geom, dy, w, ey, ex):
        self.H, self.lib, self.geom = H, H.lib(), geom
        nimg, Hh, Ww, Cin, Cout = geom
        self.lddy, self.lddx = Cout + ey, Cin + ex
        self.dyd, self.wd = nhwc(dy, self.lddy), w.to(DEV).contiguous()
        self.ws_bytes = self.lib.vd_conv3x3_wino43_dgrad_planes_ws_bytes(nimg, Hh, Ww, Cin, Cout)
        self.dm_whole, self.dm = _guarded(self.lib.vd_conv3x3_wino43_dm_floats(nimg, Hh, Ww, Cout))
        self.ws_whole, self.ws = _guarded(self.ws_bytes // 4)

    def launch(self):
        """-> (dx [nimg][H][W][lddx] pre-filled with 5, its guarded buffer, form of the plane GEMMs)"""
        nimg, Hh, Ww, Cin, Cout = self.geom
        H, lib = self.H, self.lib
        whole, flat = _guarded(nimg * Hh * Ww * self.lddx, fill=5.0)
        dx = flat.view(nimg, Hh, Ww, self.lddx)
        rc = lib.vd_conv3x3_wino43_dy_image(H.ptr(self.dyd), self.lddy, nimg, Hh, Ww, Cout, H.ptr(self.dm), H.stream())
        assert rc == 0, lib.vd_last_error().decode(errors="replace")
        rc = lib.vd_conv3x3_wino43_dgrad_planes(H.ptr(self.dm), H.ptr(self.wd), H.ptr(dx), self.lddx, nimg, Hh, Ww, Cin, Cout, H.ptr(self.ws),
                                                self.ws_bytes, 7, H.stream())
        assert rc == 0, lib.vd_last_error().decode(errors="replace")
        form = H.tile_fields(lib.vd_gemm_last_tile())[1:]
        torch.cuda.synchronize()
        return dx, whole, form


def _errs(dx, Cin, ref64):
    got = dx[..., :Cin].permute(0, 3, 1, 2).double().cpu()
    return ((got - ref64).norm() / ref64.norm()).item(), (got - ref64).abs().max().item()


def _fused(H, geom, dyd, lddy, w):
    """the fused F(4x4,3x3) input-gradient kernel on the same inputs, or None where it does not serve the geometry"""
    nimg, Hh, Ww, Cin, Cout = geom
    if not H.lib().vd_conv3x3_dgrad_wino43_supported(nimg, Hh, Ww, Cin, Cout, lddy, Cin):
        return None
    u43 = torch.empty(H.lib().vd_wino43_u_floats(Cout, Cin), device=DEV)
    H.wino43_pack(w.to(DEV), Cout, Cin, u43)
    dxf = torch.empty(nimg, Hh, Ww, Cin, device=DEV)
    H.conv3x3_dgrad_wino43(dyd, lddy, u43, dxf, Cin, nimg, Hh, Ww, Cin, Cout)
    torch.cuda.synchronize()
    return dxf


def _check_bounds(H, call, dx, ref64, what):
    Cin = call.geom[3]
    rel, mx = _errs(dx, Cin, ref64)
    big = ref64.abs().max().item()
    dxf = _fused(H, call.geom, call.dyd, call.lddy, call.wd)
    line = f"dgrad planes {what}: rel-L2 {rel:.3e}, max {mx:.3e} of {big:.3f} ({mx / big:.3e})"
    if dxf is not None:
        rel_f, mx_f = _errs(dxf, Cin, ref64)
        line += f"; fused {rel_f:.3e} / {mx_f:.3e}: ratios {rel / rel_f:.2f} / {mx / mx_f:.2f}"
    print(line)
    assert rel <= REL_BOUND and mx <= MAX_BOUND * big, line
    if dxf is not None:
        assert rel <= RATIO * rel_f and mx <= RATIO * mx_f, line


@pytest.mark.gpu
@pytest.mark.parametrize("case,form", CASES)
def test_dgrad_planes_vs_fp64(H, case, form):
    nimg, Hh, Ww, Cin, Cout, ey, ex = case
    dy, w, ref64 = _case_data(case)
    call = _Call(H, case[:5], dy, w, ey, ex)
    assert call.lib.vd_conv3x3_wino43_dgrad_planes_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex) == 1
    dx, whole, ran = call.launch()
    dx2, whole2, ran2 = call.launch()
    assert _guards_intact(call.dm_whole) and _guards_intact(call.ws_whole), "a store outside dM / outside the workspace"
    assert _guards_intact(whole) and _guards_intact(whole2), "a store outside dx"
    assert ran == form and ran2 == form, f"the plane GEMMs ran {ran}, the case is meant for {form}"
    assert torch.equal(dx, dx2), "not bitwise reproducible"
    assert (dx[..., Cin:] == 5.0).all(), "padding channels of dx were written"
    assert torch.isfinite(dx[..., :Cin]).all() and not (dx[..., :Cin] == 5.0).all()
    _check_bounds(H, call, dx, ref64, str(case))


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(4, 32, 32, 32, 16), (4, 16, 16, 64, 8)])
def test_impulse_reaches_every_neighbour_once(H, geom):
    """dy is zero except one pixel per image -- an image corner, the two sides of a tile corner (pixels 3 and 4) and a tile interior --
    so dx is one 3x3 stamp of w per image: a neighbour's share that is missing or added twice is an error of the stamp's own size"""
    nimg, Hh, Ww, Cin, Cout = geom
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    dy = torch.zeros(nimg, Cout, Hh, Ww)
    for img, (py, px) in enumerate([(0, 0), (3, 3), (4, 4), (Hh - 6, 9)]):
        dy[img, :, py, px] = rnd(Cout, seed=10 + img)
    dy[0, :, Hh - 1, Ww - 1] = rnd(Cout, seed=20)
    dy[1, :, 3, 4] = rnd(Cout, seed=21)
    ref64 = _dgrad64(dy, w, Cin)
    call = _Call(H, geom, dy, w, 0, 0)
    dx, whole, _ = call.launch()
    assert _guards_intact(whole) and _guards_intact(call.dm_whole) and _guards_intact(call.ws_whole)
    _check_bounds(H, call, dx, ref64, f"impulses {geom}")
    per_img = (dx.double().cpu().permute(0, 3, 1, 2) - ref64).abs().amax(dim=(1, 2, 3))
    assert (per_img <= MAX_BOUND * ref64.abs().amax(dim=(1, 2, 3))).all(), per_img


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("geom", [(32, 16, 16, 64, 64), (8, 32, 32, 64, 32)])
def test_dy_image_and_weight_gradient_with_both_images_are_bitwise(H, geom, accumulate):
    """vd_conv3x3_wino43_dy_image writes the dM the weight gradient's own transform pass leaves in its workspace, bit for bit, and
    vd_conv3x3_wgrad_wino43_vm on (V, dM) is bitwise vd_conv3x3_wgrad_wino43_v on (V, dy), the accumulating run included"""
    nimg, Hh, Ww, Cin, Cout = geom
    lib = H.lib()
    assert H.wgrad43_supported(nimg, Hh, Ww, Cin, Cout, Cin, Cout)
    xd, dyd = nhwc(rnd(nimg, Cin, Hh, Ww, seed=1), Cin), nhwc(rnd(nimg, Cout, Hh, Ww, seed=5), Cout)
    wd = rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5).to(DEV)
    y = torch.empty(nimg, Hh, Ww, Cout, device=DEV)
    nv, nm = lib.vd_conv3x3_wino43_v_floats(nimg, Hh, Ww, Cin), lib.vd_conv3x3_wino43_dm_floats(nimg, Hh, Ww, Cout)
    v = torch.empty(nv, device=DEV)
    H.conv3x3_wino43_fwd_planes(xd, Cin, wd, None, y, Cout, nimg, Hh, Ww, Cin, Cout, v=v)
    dm_whole, dm = _guarded(nm)
    H.conv3x3_wino43_dy_image(dyd, Cout, nimg, Hh, Ww, Cout, dm)
    init_w, init_b = rnd(Cout, Cin, 3, 3, seed=6).to(DEV), rnd(Cout, seed=7).to(DEV)
    dw0, db0, dw1, db1 = init_w.clone(), init_b.clone(), init_w.clone(), init_b.clone()
    H.conv3x3_wgrad(None, Cin, dyd, Cout, nimg, Hh, Ww, Cin, Cout, dw0, Cin, Cout, accumulate=accumulate, dbias=db0, v=v)
    # (the transform pass of that call left its dM behind V's slot in the "wgrad43" workspace of this stream)
    ws = H.workspace(lib.vd_conv3x3_wgrad_wino43_ws_bytes(nimg, Hh, Ww, Cin, Cout), dyd.device, "wgrad43")
    own = ws[nv:nv + nm].clone()
    H.conv3x3_wgrad_wino43_vm(v, dm, nimg, Hh, Ww, Cin, Cout, dw1, Cin, Cout, accumulate=accumulate, dbias=db1)
    torch.cuda.synchronize()
    assert _guards_intact(dm_whole)
    assert torch.equal(dm, own), "dM differs from the weight gradient's own transform"
    assert torch.isfinite(dw0).all() and not torch.equal(dw0, init_w)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)


def _tiny_grads(B, seed_out=1):
    """parameter gradients of one tinyA backward at batch B"""
    import v_diffusion
    from oracle import detrand
    from oracle.cases import TINY, make_inputs, make_weights
    case = TINY["tinyA"]
    cfg, R = case["cfg"], case["R"]
    x, t, y = make_inputs(cfg, B, R, case["label"])
    gout = detrand.normal("gout", (B, cfg["out_channels"], R, R), seed_out)
    model = v_diffusion.UNet(**cfg)
    model.load_state_dict(make_weights(cfg))
    model.to(DEV).train()
    (model(x.to(DEV), t.to(DEV), y.to(DEV)) * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return {k: p.grad.cpu() for k, p in model.named_parameters()}


def _grads_agree(g0, g1):
    """the per-layer bound tests/test_unet_gpu.py holds F(4x4,3x3) against F(2x2,3x3) to: L2 <= 1e-4 |ref| + 1e-6 gmax"""
    gmax = max(g.norm().item() for g in g0.values())
    for k in g0:
        e = (g0[k].double() - g1[k].double()).norm().item()
        assert e <= 1e-4 * g0[k].double().norm().item() + 1e-6 * gmax, f"{k}: L2 error {e:.3e} vs |grad| {g0[k].norm().item():.3e}"


@pytest.mark.gpu
def test_tiny_train_step_with_input_gradients_through_planes(H):
    """tinyA at B = 32 (512 tiles at 16x16) with forwards AND input gradients through planes wherever supported (CONV_PLANES = DGRAD_PLANES
    = 2: dM written on the main stream, weight gradient on the side stream from (V, dM), input gradient from dM) against the same step
    with the fused input-gradient kernels (DGRAD_PLANES = 0)"""
    saved, calls = (H.CONV_PLANES, H.DGRAD_PLANES), [0]
    real = H.conv3x3_wino43_dgrad_planes

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    H.conv3x3_wino43_dgrad_planes = spy
    try:
        runs = {}
        for mode in ("0", "2"):
            H.CONV_PLANES, H.DGRAD_PLANES = "2", mode
            calls[0] = 0
            runs[mode] = (_tiny_grads(32), calls[0])
    finally:
        (H.CONV_PLANES, H.DGRAD_PLANES), H.conv3x3_wino43_dgrad_planes = saved, real
    (g0, n0), (g2, n2) = runs["0"], runs["2"]
    assert n0 == 0 and n2 > 0, (n0, n2)
    _grads_agree(g0, g2)


@pytest.mark.gpu
def test_switch_off_in_a_child_process(H, tmp_path):
    """VD_DGRAD_PLANES is read once per process: one FRESH child with VD_DGRAD_PLANES=0 runs a B = 4 tinyA backward; its parameter
    gradients agree with this process (the default) within the per-layer bound"""
    out = str(tmp_path / "grads.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, VD_DGRAD_PLANES="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert H.DGRAD_PLANES == os.environ.get("VD_DGRAD_PLANES", H.DGRAD_PLANES)
    _grads_agree(_tiny_grads(4), torch.load(out))


if __name__ == "__main__":          # the VD_DGRAD_PLANES=0 child of test_switch_off_in_a_child_process: argv[1] = where its gradients go
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "v-diffusion-torch_amd")]
    from v_diffusion import _hip
    assert os.environ.get("VD_DGRAD_PLANES") == "0" and _hip.DGRAD_PLANES == "0" and len(sys.argv) == 2, __doc__
    torch.save(_tiny_grads(4), sys.argv[1])
