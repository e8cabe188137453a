"""Device-free checks of the input gradient through planes (csrc/wino43.hip): the host rules vd_conv3x3_wino43_dgrad_planes_supported /
vd_conv3x3_dgrad_planes_preferred, the refusals of the new entry points (every one returns before its first launch), and the form of the
tile engine each case of tests/test_dgrad_planes_gpu.py plans to."""
import ctypes
import importlib.util
import os

import pytest

from v_diffusion import _hip


@pytest.fixture(scope="module")
def lib():
    return _hip.lib()


def _err(lib):
    return lib.vd_last_error().decode(errors="replace")


def test_supported_truth_table(lib):
    f = lib.vd_conv3x3_wino43_dgrad_planes_supported
    assert f(128, 32, 32, 256, 256, 256) == 1 and f(128, 16, 16, 512, 256, 512) == 1
    assert f(1, 16, 16, 4, 4, 4) == 1 and f(3, 32, 32, 24, 40, 56) == 1                   # any image count, channels in fours, pitched dx
    assert f(8, 64, 64, 256, 256, 256) == 0 and f(8, 32, 64, 256, 256, 256) == 0         # 64-wide images: a band needs its neighbours' tile rows
    assert f(8, 8, 8, 256, 256, 256) == 0 and f(8, 32, 16, 256, 256, 256) == 0
    assert f(8, 32, 32, 254, 256, 256) == 0 and f(8, 32, 32, 256, 250, 256) == 0         # channels in fours
    assert f(8, 32, 32, 256, 256, 258) == 0 and f(8, 32, 32, 256, 256, 252) == 0         # dx rows 16-byte aligned, pitch >= Cin
    assert f(0, 32, 32, 256, 256, 256) == 0 and f(65536, 16, 16, 4, 4, 4) == 0           # images ride on grid.y
    assert f(65535, 16, 16, 4, 4, 4) == 1
    assert f(8, 32, 32, 256, 1 << 20, 256) == 0                                          # dM's block pitch outside the GEMM's 32-bit offsets


def test_preferred_truth_table(lib):
    f = lib.vd_conv3x3_dgrad_planes_preferred
    assert not [k for k in ("VD_PLANES_MIN_TILES",) if os.environ.get(k) is not None]
    assert f(128, 32, 32, 256, 256, 1) == 1 and f(128, 32, 32, 512, 256, 1) == 1          # the 16 layers of the B = 128 CIFAR step
    assert f(128, 32, 32, 256, 256, 0) == 0                                              # training steps only (someone has to make dM anyway)
    assert f(64, 32, 32, 256, 256, 1) == 0                                               # 4096 tiles: below the floor
    assert f(128, 16, 16, 256, 256, 1) == 0 and f(128, 16, 16, 512, 256, 1) == 0          # 2048 tiles
    assert f(128, 32, 32, 192, 256, 1) == 0 and f(128, 32, 32, 384, 256, 1) == 0          # Cin = N of the 128 x 256 tile
    assert f(128, 32, 32, 256, 40, 1) == 0                                               # Cout = K in whole K tiles
    assert f(32, 64, 64, 256, 256, 1) == 0                                               # 8192 tiles, but 64-wide: declined by _supported
    assert f(512, 16, 16, 256, 256, 1) == 1                                              # 8192 tiles at 16x16


def test_sizes(lib):
    assert lib.vd_conv3x3_wino43_dm_floats(128, 32, 32, 256) == 36 * 8192 * 256
    assert lib.vd_conv3x3_wino43_dm_floats(3, 8, 8, 8) == 36 * 16 * 8                     # 12 tiles: stored in blocks of 16
    assert lib.vd_conv3x3_wino43_dgrad_planes_ws_bytes(2, 32, 32, 256, 64) == 4 * (36 * 64 * 256 + 36 * 128 * 256)


def test_refusals(lib):
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf) // 16 * 16 + 16                                            # a 16-byte aligned host address: never dereferenced
    big = 1 << 40
    dg = lib.vd_conv3x3_wino43_dgrad_planes
    assert dg(None, a, a, 4, 1, 16, 16, 4, 4, a, big, 7, None) == 1 and "null" in _err(lib)
    assert dg(a, a, a, 4, 1, 16, 16, 4, 4, None, big, 7, None) == 1 and "null" in _err(lib)
    assert dg(a, a, a, 4, 1, 64, 64, 4, 4, a, big, 7, None) == 1 and "unsupported geometry" in _err(lib)
    assert dg(a + 4, a, a, 4, 1, 16, 16, 4, 4, a, big, 7, None) == 1 and "aligned" in _err(lib)
    assert dg(a, a, a + 8, 4, 1, 16, 16, 4, 4, a, big, 7, None) == 1 and "aligned" in _err(lib)
    need = lib.vd_conv3x3_wino43_dgrad_planes_ws_bytes(1, 16, 16, 4, 4)
    assert dg(a, a, a, 4, 1, 16, 16, 4, 4, a, need - 4, 7, None) == 1 and "workspace too small" in _err(lib)
    assert dg(a, a, a, 4, 1, 16, 16, 4, 4, a, need, 3, None) == 1 and "phase" in _err(lib)
    di = lib.vd_conv3x3_wino43_dy_image
    assert di(None, 4, 1, 16, 16, 4, a, None) == 1 and "null" in _err(lib)
    assert di(a, 4, 1, 16, 16, 4, None, None) == 1 and "null" in _err(lib)
    assert di(a, 6, 1, 16, 16, 4, a, None) == 1 and "unsupported geometry" in _err(lib)
    assert di(a, 4, 1, 18, 16, 4, a, None) == 1 and "unsupported geometry" in _err(lib)
    assert di(a + 4, 4, 1, 16, 16, 4, a, None) == 1 and "aligned" in _err(lib)
    vm = lib.vd_conv3x3_wgrad_wino43_vm
    assert vm(None, a, 32, 16, 16, 64, 64, a, a, 64, 64, 0, a, big, 7, None) == 1 and "null" in _err(lib)
    assert vm(a, None, 32, 16, 16, 64, 64, a, a, 64, 64, 0, a, big, 7, None) == 1 and "null" in _err(lib)
    assert vm(a, a, 32, 16, 16, 64, 64, a, a, 64, 64, 0, a, big, 1, None) == 1 and "phase" in _err(lib)
    assert vm(a, a + 4, 32, 16, 16, 64, 64, a, a, 64, 64, 0, a, big, 7, None) == 1 and "aligned" in _err(lib)
    assert vm(a, a, 2, 16, 16, 64, 64, a, a, 64, 64, 0, a, big, 7, None) == 1 and "unsupported geometry" in _err(lib)      # 32 tiles
    need = lib.vd_conv3x3_wgrad_wino43_ws_bytes(32, 16, 16, 64, 64)
    assert vm(a, a, 32, 16, 16, 64, 64, a, a, 64, 64, 0, a, need - 4, 7, None) == 1 and "workspace too small" in _err(lib)


def test_python_rule_follows_the_switch(lib):
    saved = _hip.DGRAD_PLANES
    try:
        for mode, big, small in (("0", False, False), ("1", True, False), ("2", True, True)):
            _hip.DGRAD_PLANES = mode
            assert _hip.dgrad_planes_supported(128, 32, 32, 256, 256, 256, 256) == big
            assert _hip.dgrad_planes_supported(32, 16, 16, 64, 64, 64, 64) == small       # 512 tiles: the weight gradient's floor
            assert not _hip.dgrad_planes_supported(16, 16, 16, 64, 64, 64, 64)            # 256 tiles: no F(4x4,3x3) weight gradient to share dM with
            assert not _hip.dgrad_planes_supported(32, 64, 64, 256, 256, 256, 256)
    finally:
        _hip.DGRAD_PLANES = saved


def test_plans_of_the_gpu_cases(lib):
    """every case of tests/test_dgrad_planes_gpu.py plans to the form its GPU test asserts (a planner change that moves one shows here)"""
    assert not [k for k in ("VD_GEMM_TILE", "VD_GEMM_KT", "VD_GEMM_SPLIT", "VD_GEMM_BN256", "VD_GEMM_LEGACY") if os.environ.get(k) is not None]
    spec = importlib.util.spec_from_file_location("_dgrad_planes_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                     "test_dgrad_planes_gpu.py"))
    gpu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gpu)
    for (nimg, Hh, Ww, Cin, Cout, _, ex), form in gpu.CASES:
        assert lib.vd_conv3x3_wino43_dgrad_planes_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex) == 1
        T = nimg * (Hh // 4) * (Ww // 4)
        code = lib.vd_gemm_plan_tile(T, Cin, Cout, _hip.ROW, _hip.ROW, 36, 0, 0)
        assert code > 0, _err(lib)
        assert _hip.tile_fields(code)[1:] == form, ((nimg, Hh, Ww, Cin, Cout), _hip.tile_fields(code)[1:], form)
        if form == gpu.WIDE:
            assert T % 128 == 64 and T % 16 == 0                                         # a ragged last row tile of whole 16-row blocks
    assert {form for _, form in gpu.CASES} == {gpu.WIDE, gpu.SMALL}
    # the step's own shapes: the 128 x 256 form
    for ci in (256, 512):
        assert _hip.tile_fields(lib.vd_gemm_plan_tile(8192, ci, 256, _hip.ROW, _hip.ROW, 36, 0, 0))[1:] == gpu.WIDE
