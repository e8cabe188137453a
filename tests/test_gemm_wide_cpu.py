"""Which vd_gemm launches take the 128x256 split-operand form: the host plan's own answer (vd_gemm_plan_tile), without a device.

The rule (csrc/gemm.hip: plan_gemm): a plain or batched ROW/ROW launch goes wide when the 128x128 KT = 16 split form would otherwise run,
N % 256 == 0 and ceil(M / 128) * (N / 256) * batch >= 2 * CUs (256 CUs without a device: 512 workgroups).  ROW/COL and COL/COL launches
have the form on request only (tile = 128256): per launch the input-gradient shapes lose on it (FINDINGS.md).
Swept over the plain-GEMM shapes of the CIFAR-10 and CelebA training steps and samplers (1x1 skip convolutions, attention projections and
products, their input gradients) at B = 128, 8 and 1.  What "would otherwise run" is taken from a child process started with
VD_GEMM_BN256=0, the switch that restores the 128x128 dispatch, so the rule is checked against the library's own baseline, not a copy of
its tile menu."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "v-diffusion-torch_amd")
for _p in (PKG, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ROW, COL = 0, 1
WIDE = 128256
KNOBS = ("VD_GEMM_TILE", "VD_GEMM_SPLIT", "VD_GEMM_BN256", "VD_GEMM_KT", "VD_GEMM_LEGACY", "VD_GEMM_TR")        # (each would move a plan)


def _shapes():
    """[(M, N, K, a_kind, b_kind, batch, stats)] of the plain and batched vd_gemm launches of engine.py for both benchmark models"""
    from oracle.cases import CIFAR_COND, CELEBA
    out = []
    for cfg, res in ((CIFAR_COND, 32), (CELEBA, 64)):
        chans = [cfg["hid_channels"] * m for m in cfg["ch_multipliers"]]
        for B in (128, 8, 1):
            for lvl, C in enumerate(chans):
                L = (res >> lvl) ** 2
                M = B * L
                near = {chans[max(lvl - 1, 0)], chans[min(lvl + 1, len(chans) - 1)], C}
                for cin in sorted({c for c in near if c != C} | {C + c for c in near}):       # 1x1 skip convolutions: forward, input gradient
                    out.append((M, C, cin, ROW, ROW, 1, 0))
                    out.append((M, cin, C, ROW, COL, 1, 0))
                if cfg["apply_attn"][lvl]:
                    hd = cfg.get("head_dim") or C // cfg["num_heads"]
                    nh = C // hd
                    out += [(M, 3 * C, C, ROW, ROW, 1, 0), (M, C, C, ROW, ROW, 1, 1),          # proj_in, proj_out (+ statistics)
                            (M, C, C, ROW, COL, 1, 0), (M, C, 3 * C, ROW, COL, 1, 0)]           # their input gradients
                    out += [(L, L, hd, ROW, ROW, B * nh, 0), (L, hd, L, ROW, COL, B * nh, 0),   # Q.K^T, P.V
                            (L, hd, L, COL, COL, B * nh, 0), (L, L, hd, ROW, ROW, B * nh, 0),   # dV, dP
                            (L, hd, L, ROW, COL, B * nh, 0), (L, hd, L, COL, COL, B * nh, 0)]   # dQ, dK
    out += [(131072, 768, 256, ROW, ROW, 1, 0), (131072, 256, 256, ROW, ROW, 1, 0), (131072, 256, 512, ROW, ROW, 1, 0),      # the launches of
            (32768, 768, 256, ROW, ROW, 1, 0), (131072, 256, 768, ROW, COL, 1, 0), (131072, 256, 256, ROW, COL, 1, 0),      # profiles/r06_presplit_price.txt
            (131072, 512, 256, ROW, COL, 1, 0), (32768, 256, 768, ROW, COL, 1, 0), (32768, 512, 256, ROW, COL, 1, 0),
            (32768, 256, 256, ROW, ROW, 1, 1)]
    return sorted(set(out))


def _codes(lib, tile):
    return [lib.vd_gemm_plan_tile(M, N, K, ak, bk, batch, tile, stats) for (M, N, K, ak, bk, batch, stats) in _shapes()]


@pytest.fixture(scope="module")
def hip():
    from v_diffusion import _hip
    set_knobs = [k for k in KNOBS if os.environ.get(k) is not None]
    assert not set_knobs, f"the plans under test are the defaults: unset {set_knobs}"
    return _hip


@pytest.fixture(scope="module")
def baseline(hip):
    """the same sweep in a process with VD_GEMM_BN256=0: today's 128x128 dispatch"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--codes"], env=dict(os.environ, VD_GEMM_BN256="0"), capture_output=True,
                       text=True, timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(line[0][7:])


def test_dispatch_rule_over_the_benchmark_shapes(hip, baseline):
    lib = hip.lib()
    shapes, got = _shapes(), _codes(lib, 0)
    assert len(shapes) == len(baseline) > 100
    wide = []
    for s, code, base in zip(shapes, got, baseline):
        M, N, K, ak, bk, batch, stats = s
        tr, spl, kt, bm, bn = hip.tile_fields(base)
        assert bn != 256, (s, base)                                       # the switch restores the 128x128 dispatch everywhere
        want = (ak, bk) == (ROW, ROW) and spl and kt == 16 and (bm, bn) == (128, 128) and N % 256 == 0 \
            and ((M + 127) // 128) * (N // 256) * batch >= 2 * 256
        if want:
            assert hip.tile_fields(code) == (tr, True, 16, 128, 256), (s, code, base)
            wide.append(s)
        else:
            assert code == base, (s, code, base)                          # every other launch is planned exactly as before
    # both answers occur, plain and batched
    assert any(s[5] > 1 for s in wide) and any(s[5] == 1 for s in wide) and 0 < len(wide) < len(shapes)
    # the pins of the issue
    code = dict(zip(shapes, got))
    assert hip.tile_fields(code[(32768, 256, 256, ROW, ROW, 1, 1)])[3:] == (128, 128)       # 256 workgroups of 128x256: half the chip idle
    assert hip.tile_fields(code[(32768, 256, 768, ROW, COL, 1, 0)])[3:] == (128, 128)
    assert hip.tile_fields(code[(32768, 512, 256, ROW, COL, 1, 0)])[3:] == (128, 128)       # an input gradient (ROW/COL): on request only
    assert hip.tile_fields(code[(131072, 512, 256, ROW, COL, 1, 0)])[3:] == (128, 128)
    assert hip.tile_fields(code[(32768, 768, 256, ROW, ROW, 1, 0)])[3:] == (128, 256)       # 768 workgroups: three per CU
    assert hip.tile_fields(code[(131072, 256, 256, ROW, ROW, 1, 0)]) == (True, True, 16, 128, 256)
    assert code[(131072, 256, 256, ROW, ROW, 1, 0)] == 316128256
    assert hip.tile_fields(code[(1024, 1024, 64, ROW, ROW, 128 * 6, 0)])[3:] == (128, 256)  # CelebA Q.K^T at L = 1024
    assert hip.tile_fields(code[(1024, 64, 1024, ROW, COL, 128 * 6, 0)])[4] != 256          # ... P.V: N = 64


def test_tile_128_always_wins_and_the_wide_request_is_honoured(hip):
    lib = hip.lib()
    for s, code in zip(_shapes(), _codes(lib, 128)):
        assert hip.tile_fields(code)[3:] == (128, 128), (s, code)
    for (M, N, K, ak, bk, batch, stats) in _shapes():
        code = lib.vd_gemm_plan_tile(M, N, K, ak, bk, batch, WIDE, stats)
        if N % 256 == 0:
            assert hip.tile_fields(code)[1:] == (True, 16, 128, 256), (M, N, K, code)      # any size, down to one workgroup
        else:
            assert code == -1 and b"N % 256" in lib.vd_last_error()
    assert hip.tile_fields(lib.vd_gemm_plan_tile(128, 256, 16, ROW, ROW, 1, WIDE, 0))[1:] == (True, 16, 128, 256)
    assert lib.vd_gemm_plan_tile(128, 256, 16, COL, ROW, 1, WIDE, 0) == -1                 # COL/ROW has no 128x256 form
    assert hip.TILE_WIDE == WIDE


if __name__ == "__main__":
    assert sys.argv[1:] == ["--codes"], __doc__
    from v_diffusion import _hip as _H
    print("RESULT " + json.dumps(_codes(_H.lib(), 0)))
