"""Host launch plans and the last-launch code, without a device.

The planners of the C ABI (which tile, how many split-K slabs, how much workspace, which geometries a Winograd form serves) are pure
host arithmetic over the shape and the CU count; without a device vd_cu_count() answers 256, the MI355X's own count.  Their answers
over a sweep of shapes are pinned to tests/golden/launch_plans.json, recorded from the library as it stood before the planners were
merged into one (csrc/gemm.hip: plan_grouped; csrc/wino.hip: plan_tiles), so a change of any plan shows here before it shows as a
wrong workspace size on a GPU.

    python tests/test_launch_plans_cpu.py --record      rewrites the table from the library that VDIFF_HIP_LIB names (default: the
                                                        one in the tree) -- only for a change that is MEANT to move a plan
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
for _p in (os.path.join(ROOT, "v-diffusion-torch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

KNOBS = ("VD_GEMM_TILE", "VD_GEMM_SPLIT", "VD_PLANES256", "VD_WINO_WIDE")     # (each would move a plan)


def _geometries():
    """(nimg, H, W, Cin, Cout) of the sweep"""
    from test_bench_shapes_gpu import WINO_ALL          # every 3x3 layer shape of the CIFAR-10 (32x32) and CelebA (64x64) steps at B = 128
    layers = sorted({c[1:5] for c in WINO_ALL})
    out = [(B,) + l for l in layers for B in (128, 1, 8)]
    chans = [(c, c) for c in (4, 20, 192, 576, 1344)] + [(192, 576), (1344, 576), (20, 4)]
    out += [(B, Hh, Ww, ci, co) for (Hh, Ww) in ((4, 4), (8, 8), (8, 16), (128, 128)) for (ci, co) in chans for B in (128, 1, 8)]
    return out


def _sweep(lib):
    """{"nimg,H,W,Cin,Cout": [answers]}: the Winograd planners at the convolution's geometry, the grouped planners at the 1x1 convolution /
    linear layer of the same geometry (M = Cout, N = Cin, K = pixels) and at the 36 planes of its F(4x4,3x3) weight gradient (K = tiles)"""
    table = {}
    for nimg, Hh, Ww, Cin, Cout in _geometries():
        row = [lib.vd_conv3x3_wino_supported(nimg, Hh, Ww, Cin, Cout, Cin, Cout, 0),
               lib.vd_conv3x3_wino_supported(nimg, Hh, Ww, Cin, Cout, Cin + Cout, Cout, Cout),
               lib.vd_conv3x3_wgrad_wino43_supported(nimg, Hh, Ww, Cin, Cout, Cin, Cout),
               lib.vd_conv3x3_wgrad_wino43_ws_bytes(nimg, Hh, Ww, Cin, Cout),
               lib.vd_conv3x3_wgrad_wino_ws_bytes(nimg, Hh, Ww, Cin, Cout)]
        K, T = nimg * Hh * Ww, nimg * (Hh // 4) * (Ww // 4)
        for count in (1, 2, 36):
            for k, lo, hi in ((K, 1, 64), (T, (T + 1535) // 1536, 24)):      # (the engine's call, the F(4x4,3x3) weight gradient's call)
                S = lib.vd_gemm_grouped_wgrad_auto_split(count, Cout, Cin, max(k, 1), lo, hi)
                row += [S, lib.vd_gemm_grouped_wgrad_ws_bytes(count, Cout, Cin, S)]
        table[f"{nimg},{Hh},{Ww},{Cin},{Cout}"] = row
    # the linear layers (time embedding and its per-block projections: hid -> 4 hid -> 4 hid -> C; hid = 256 / 192): K = batch rows
    for Cin, Cout in ((256, 1024), (1024, 1024), (1024, 256), (192, 768), (768, 768), (768, 192), (768, 384), (768, 576)):
        for B in (128, 1, 8):
            row = []
            for count in (1, 2, 36):
                S = lib.vd_gemm_grouped_wgrad_auto_split(count, Cout, Cin, B, 1, 64)
                row += [S, lib.vd_gemm_grouped_wgrad_ws_bytes(count, Cout, Cin, S)]
            table[f"linear,{B},{Cin},{Cout}"] = row
    return table


@pytest.fixture(scope="module")
def hip():
    from v_diffusion import _hip
    return _hip


def test_host_launch_plans_match_the_recorded_table(hip):
    set_knobs = [k for k in KNOBS if os.environ.get(k) is not None]
    assert not set_knobs, f"the recorded plans are the defaults: unset {set_knobs}"
    assert os.path.exists(GOLDEN), f"{GOLDEN} missing"
    want = json.load(open(GOLDEN))
    assert want and len(want) == len(_geometries()) + 24, "recorded table empty or not of this sweep"
    got = _sweep(hip.lib())
    assert got.keys() == want.keys()
    bad = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not bad, f"{len(bad)} of {len(want)} plans moved, e.g. (recorded, now) {list(bad.items())[:3]}"
    # the sweep reaches both answers of every yes/no planner and more than one slab count (it is not a table of zeros)
    cols = list(zip(*[v for k, v in want.items() if not k.startswith("linear")]))
    assert all(set(cols[i]) == {0, 1} for i in (0, 2)) and len(set(cols[5])) > 3 and min(cols[3]) > 0


# last-launch codes of the forms that tests/test_kernels_gpu.py and tests/test_bench_shapes_gpu.py pin, as the integers
# vd_gemm_last_tile returns for them -> (tr, spl, kt, bm, bn)
CODES = {
    16128128: (False, False, 16, 128, 128),      # statistics-emitting KT = 16 128x128 forward convolution (test_conv3x3_stats_at_bench_shapes)
    32128128: (False, False, 32, 128, 128),      # ... its 512-workgroup 16x16 case: KT = 32
    116128128: (True, False, 16, 128, 128),      # input gradient / split-K weight gradient: transposed epilogue, fp32 MFMA (im2col operands)
    316256256: (True, True, 16, 256, 256),       # the 256x256 planes kernel of the F(4x4,3x3) weight gradient
    316128128: (True, True, 16, 128, 128),       # grouped launch on 128x128 tiles, long enough for KT = 16, split-operand form
    332128064: (True, True, 32, 128, 64),        # grouped launch on a rectangular tile
    132064064: (True, False, 32, 64, 64),        # ... with VD_GEMM_SPLIT=0
    232128128: (False, True, 32, 128, 128),      # split-operand GEMM that emits statistics (no transposed epilogue)
    16128032: (False, False, 16, 128, 32),       # both Winograd F(2x2,3x3) forms: 64-pixel statistics chunks = BM / 2
    128128: (False, False, 0, 128, 128),         # VD_GEMM_LEGACY: the register-staged kernel
    64128: (False, False, 0, 64, 128),
}


def test_tile_fields_decodes_the_pinned_codes(hip, monkeypatch):
    for code, (tr, spl, kt, bm, bn) in CODES.items():
        assert hip.tile_fields(code) == (tr, spl, kt, bm, bn), code
        assert ((((tr + 2 * spl) * 100 + kt) * 1000 + bm) * 1000 + bn) == code              # (csrc/common.h: vd_tile_code)
        # what the GPU tests read by hand: flags = code // 10^8 (>= 2: split form), and the GroupNorm chunk size engine._conv derives
        assert (code // 10 ** 6) // 100 == tr + 2 * spl and ((code // 10 ** 6) // 100 >= 2) == spl
        monkeypatch.setattr(hip.lib(), "vd_gemm_last_tile", lambda code=code: code)
        assert hip.last_row_tile() == (code // 1000) % 1000 == bm


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    from v_diffusion import _hip
    tab = _sweep(_hip.lib())
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in tab.items()) + "\n}\n")
    print(f"{len(tab)} geometries from {_hip.LIB_PATH} -> {GOLDEN}")
