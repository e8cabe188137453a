"""The 128x256 split-operand GEMM form (csrc/gemm.hip: gemm_split_kernel<128, 256, ..., 16, TR>) against the 128x128 form it replaces.

Every case runs the same operands twice -- tile = 128 and the forced wide form (tile = 128256) -- and asserts
  * torch.equal on the output (and on the GroupNorm partials where they are emitted): the wide form runs the same instruction sequence per
    output element (same split8, same six piece products, same k order), so any difference is a bug, not a tolerance question;
  * the wide run's last-tile code: bm = 128, bn = 256, split flag set;
  * the error against an fp64 matmul within the bound of test_kernels_gpu.py::test_split_operand_gemm_forms_in_subprocess:
    rel-L2 <= 1.25 x the fp32 MFMA chain's on the same operands + 1e-9.  The fp32 figures come from ONE child process that runs this
    module's case list with VD_GEMM_SPLIT=0 (the switch is process-wide), shared by every test.
Shapes are the smallest at which the form can go wrong: one / two column tiles, one / several / a ragged row tile, one K tile / prologue +
steady state + tail of the two-stage ring / a ragged K (both forms accept K % 4 == 0), a 16-workgroup launch (from 16 on the XCD remap
is active), and one long launch at natural selection.  Needs an MI355X."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "v-diffusion-torch_amd")
WIDE = 128256
KINDS = {"RR": (0, 0), "RC": (0, 1), "CC": (1, 1)}


def _case(name, kind, M, N, K, *, alpha=1.0, bias=False, res=False, acc=False, pad=0, stats_hw=0, inf_row=None, tile=WIDE):
    return dict(name=name, kind=kind, M=M, N=N, K=K, alpha=alpha, bias=bias, res=res, acc=acc, pad=pad, stats_hw=stats_hw, inf_row=inf_row,
                tile=tile)


def _cases():
    out = []
    # the cross of the issue: N x M x K x kind.  The epilogue alternates with the output pitch: ldc = N and N + 4 take the transposed
    # (dwordx4) epilogue, ldc = N + 2 cannot and takes the plain one; alpha != 1 throughout, bias + residual on every other case
    i = 0
    for kind in KINDS:
        for N in (256, 512):
            for M in (128, 384, 300):
                for K in (16, 48, 40):
                    pad = (0, 4, 2)[i % 3]
                    out.append(_case(f"x_{kind}_{M}_{N}_{K}", kind, M, N, K, alpha=0.5, bias=i % 2 == 0, res=i % 2 == 0, pad=pad))
                    i += 1
    for kind in KINDS:                                   # accumulate into C, both epilogues
        out.append(_case(f"acc_tr_{kind}", kind, 300, 256, 48, alpha=0.75, acc=True, pad=4))
        out.append(_case(f"acc_plain_{kind}", kind, 300, 512, 48, alpha=0.75, acc=True, bias=True, res=True, pad=2))
    for hw in (64, 256):                                 # GroupNorm partials of the output (plain epilogue, ROW/ROW)
        out.append(_case(f"stats_{hw}", "RR", 512, 512, 48, bias=True, res=True, stats_hw=hw))
    out.append(_case("inf_row", "RR", 384, 256, 48, inf_row=131))
    # 16 workgroups and more (the XCD remap is active from 16): 8 row tiles x 2 column tiles
    out.append(_case("remap", "RC", 1024, 512, 48, alpha=0.5, bias=True, res=True))
    # natural selection: 1024 row tiles x 1 column tile >= two workgroups per CU
    out.append(_case("natural", "RR", 131072, 256, 256, bias=True, tile=0))
    return out


CASES = {c["name"]: c for c in _cases()}
BATCHED = dict(name="batched_pv", B=3, nh=2, L=128, hd=256)          # batch 6: the P.V product of _attn_fwd (N = hd = 256)


def _operands(c):
    """deterministic device operands of a case (same in the fp32 child process)"""
    g = torch.Generator(DEV).manual_seed(1000 + sorted(CASES).index(c["name"]))
    M, N, K = c["M"], c["N"], c["K"]
    A = torch.randn((M, K), device=DEV, generator=g)
    B = torch.randn((N, K), device=DEV, generator=g)
    bias = torch.randn((N,), device=DEV, generator=g) if c["bias"] else None
    R = torch.randn((M, N), device=DEV, generator=g) if c["res"] else None
    C0 = torch.randn((M, N + c["pad"]), device=DEV, generator=g)
    if c["inf_row"] is not None:
        A[c["inf_row"], 5] = float("inf")
    return A, B, bias, R, C0


def _reference(c, A, B, bias, R, C0):
    ref = c["alpha"] * (A.double() @ B.double().T)
    if bias is not None:
        ref = ref + bias.double()
    if R is not None:
        ref = ref + R.double()
    if c["acc"]:
        ref = ref + C0[:, :c["N"]].double()
    return ref


def _run(H, c, ops, tile):
    """-> (C with its padding columns, statistics partials or None, last-tile code)"""
    A, B, bias, R, C0 = ops
    ak, bk = KINDS[c["kind"]]
    M, N, K = c["M"], c["N"], c["K"]
    Ad = A if ak == 0 else A.T.contiguous()
    Bd = B if bk == 0 else B.T.contiguous()
    C = C0.clone()
    st = torch.full((M // 64, 2, N), -3.0, device=DEV) if c["stats_hw"] else None
    H.gemm(Ad, Bd, C, M, N, K, a_kind=ak, b_kind=bk, lda=Ad.shape[1], ldb=Bd.shape[1], ldc=N + c["pad"], bias=bias, R=R, ldr=N,
           alpha=c["alpha"], accumulate=c["acc"], tile=tile, stats=st, stats_hw=c["stats_hw"])
    torch.cuda.synchronize()
    return C, st, H.lib().vd_gemm_last_tile()


def _batched_operands():
    b = BATCHED
    g = torch.Generator(DEV).manual_seed(77)
    hid = b["nh"] * b["hd"]
    P = torch.randn((b["B"], b["nh"], b["L"], b["L"]), device=DEV, generator=g)
    qkv = torch.randn((b["B"], b["L"], 3 * hid), device=DEV, generator=g)
    return P, qkv


def _run_batched(H, P, qkv, tile):
    b = BATCHED
    Bz, nh, L, hd = b["B"], b["nh"], b["L"], b["hd"]
    hid, ld = nh * hd, 3 * nh * hd
    O = torch.full((Bz, L, hid), 9.0, device=DEV)
    v = qkv[0, 0, 2 * hid:]
    H.gemm(P, v, O, L, hd, L, a_kind=0, b_kind=1, lda=L, ldb=ld, ldc=hid, batch=Bz * nh, nh=nh, sA=(nh * L * L, L * L),
           sB=(L * ld, hd), sC=(L * hid, hd), tile=tile)
    torch.cuda.synchronize()
    return O, H.lib().vd_gemm_last_tile()


def _batched_reference(P, qkv):
    b = BATCHED
    hid = b["nh"] * b["hd"]
    v = qkv[..., 2 * hid:].reshape(b["B"], b["L"], b["nh"], b["hd"])
    return torch.einsum("bnlm,bmnd->blnd", P.double(), v.double()).reshape(b["B"], b["L"], hid)


def _rel(got, ref, rows=None):
    if rows is not None:
        got, ref = got[rows], ref[rows]
    return ((got.double() - ref).norm() / ref.norm()).item()


def _finite_rows(c):
    return None if c["inf_row"] is None else [r for r in range(c["M"]) if r != c["inf_row"]]


def _child_errors():
    """rel-L2 error against fp64 of every case on the 128x128 tiles of THIS process (the fp32 MFMA chain under VD_GEMM_SPLIT=0)"""
    from v_diffusion import _hip as H
    out = {}
    for name, c in CASES.items():
        ops = _operands(c)
        C, _, code = _run(H, c, ops, 128)
        out[name] = (code, _rel(C[:, :c["N"]], _reference(c, *ops), _finite_rows(c)))
    P, qkv = _batched_operands()
    O, code = _run_batched(H, P, qkv, 128)
    out[BATCHED["name"]] = (code, _rel(O, _batched_reference(P, qkv)))
    print("RESULT " + json.dumps(out))


def _child(env_extra, *args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=dict(os.environ, **env_extra), capture_output=True, text=True,
                       timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(line[0][7:])


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    assert _hip.lib().vd_gemm_split_forms() == 1 and os.environ.get("VD_GEMM_BN256") is None, "run with the default switches"
    return _hip


@pytest.fixture(scope="module")
def fp32_err(H):
    """{case: rel-L2 error of the fp32 MFMA form}: one child process for the whole module"""
    res = _child({"VD_GEMM_SPLIT": "0"}, "--errors")
    for name, (code, _) in res.items():
        assert (code // 10 ** 6) // 100 < 2, f"{name}: the child did not run the fp32 MFMA form ({code})"
    return {k: v[1] for k, v in res.items()}


def _check_wide_code(H, code):
    tr, spl, kt, bm, bn = H.tile_fields(code)
    assert spl and kt == 16 and bm == 128 and bn == 256, code
    return tr


def _both_forms(H, c, fp32_err):
    ops = _operands(c)
    C1, s1, code1 = _run(H, c, ops, 128)
    C2, s2, code2 = _run(H, c, ops, c["tile"])
    tr = _check_wide_code(H, code2)
    t1 = H.tile_fields(code1)
    assert t1[1] and t1[3:] == (128, 128) and t1[0] == tr, (code1, code2)
    N, rows = c["N"], _finite_rows(c)
    assert torch.equal(torch.isnan(C1), torch.isnan(C2)), c["name"]
    assert torch.equal(torch.nan_to_num(C1), torch.nan_to_num(C2)), f"{c['name']}: {(C1 != C2).sum().item()} elements differ"
    if c["pad"]:
        assert torch.equal(C2[:, N:], ops[4][:, N:]), "padding columns touched"
    err = _rel(C2[:, :N], _reference(c, *ops), rows)
    print(f"{c['name']}: code {code2} rel-L2 {err:.3e} (fp32 MFMA {fp32_err[c['name']]:.3e})")
    assert err <= 1.25 * fp32_err[c["name"]] + 1e-9, f"{c['name']}: rel-L2 {err:.3e} vs fp32 MFMA {fp32_err[c['name']]:.3e}"
    return ops, C1, C2, s1, s2, tr


@pytest.mark.parametrize("kind", list(KINDS))
def test_wide_form_equals_128_form_over_the_shape_cross(H, fp32_err, kind):
    seen = set()
    for name, c in CASES.items():
        if name.startswith(f"x_{kind}_") or name in (f"acc_tr_{kind}", f"acc_plain_{kind}") or (name == "remap" and kind == "RC"):
            seen.add(_both_forms(H, c, fp32_err)[5])
    assert seen == {True, False}, "both epilogues must have run"


def test_wide_form_batched_heads(H, fp32_err):
    P, qkv = _batched_operands()
    O1, code1 = _run_batched(H, P, qkv, 128)
    O2, code2 = _run_batched(H, P, qkv, WIDE)
    _check_wide_code(H, code2)
    assert H.tile_fields(code1)[3:] == (128, 128)
    assert torch.equal(O1, O2)
    err = _rel(O2, _batched_reference(P, qkv))
    print(f"batched P.V: code {code2} rel-L2 {err:.3e} (fp32 MFMA {fp32_err[BATCHED['name']]:.3e})")
    assert err <= 1.25 * fp32_err[BATCHED["name"]] + 1e-9


@pytest.mark.parametrize("hw", [64, 256])
def test_wide_form_statistics_partials(H, fp32_err, hw):
    c = CASES[f"stats_{hw}"]
    ops, C1, C2, s1, s2, tr = _both_forms(H, c, fp32_err)
    assert not tr and H.last_row_tile() == 128
    assert torch.equal(s1, s2)
    # and they ARE the per-64-row column sums of the output: [image][chunk][2][N] flattens to [M / 64][2][N] for either stats_hw.
    # fp32 sums of 64 terms: error <= 64 * 2^-24 = 4e-6 of the sum of magnitudes; bound 1e-5
    v = C2.double().reshape(c["M"] // 64, 64, c["N"])
    assert ((s2[:, 0].double() - v.sum(1)).abs() <= 1e-5 * v.abs().sum(1)).all()
    assert ((s2[:, 1].double() - (v * v).sum(1)).abs() <= 1e-5 * (v * v).sum(1)).all()


def test_wide_form_inf_operand_poisons_the_same_rows(H, fp32_err):
    c = CASES["inf_row"]
    ops, C1, C2, *_ = _both_forms(H, c, fp32_err)
    nan_rows = torch.isnan(C2).any(1).nonzero().flatten().tolist()
    assert nan_rows == [c["inf_row"]] and torch.isnan(C2[c["inf_row"]]).all()
    assert torch.isnan(C1).any(1).nonzero().flatten().tolist() == nan_rows


def test_wide_request_is_refused_where_the_form_does_not_exist(H):
    A = torch.zeros((128, 16), device=DEV)
    B = torch.zeros((260, 16), device=DEV)
    C = torch.zeros((128, 260), device=DEV)
    with pytest.raises(H.HipError):
        H.gemm(A, B, C, 128, 260, 16, lda=16, ldb=16, ldc=260, tile=WIDE)          # N % 256 != 0
    with pytest.raises(H.HipError):
        H.gemm(A.T.contiguous(), B[:256], C, 128, 256, 16, a_kind=1, b_kind=0, lda=128, ldb=16, ldc=260, tile=WIDE)      # COL/ROW: not built


def test_wide_form_is_the_natural_choice_of_a_long_n256_launch(H, fp32_err):
    """M = 131 072, N = 256, K = 256 with bias: 1024 workgroups of 128x256 >= two per CU -> bn = 256 with no request; in a process started
    with VD_GEMM_BN256=0 the same launch reports bn = 128"""
    c = CASES["natural"]
    assert c["tile"] == 0
    _both_forms(H, c, fp32_err)
    off = _child({"VD_GEMM_BN256": "0"}, "--natural-code")
    tr, spl, kt, bm, bn = H.tile_fields(off["code"])
    assert spl and kt == 16 and (bm, bn) == (128, 128), off


if __name__ == "__main__":
    for _p in (PKG,):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    if sys.argv[1:] == ["--errors"]:
        _child_errors()
    elif sys.argv[1:] == ["--natural-code"]:
        from v_diffusion import _hip as _H
        _c = CASES["natural"]
        print("RESULT " + json.dumps(dict(code=_run(_H, _c, _operands(_c), 0)[2])))
    else:
        raise SystemExit(__doc__)
