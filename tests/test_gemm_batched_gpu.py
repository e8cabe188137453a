"""The eight batched vd_gemm forms the UNet engine launches (v_diffusion/engine.py: _attn_fwd, _attn_bwd, _film_fwd, _film_bwd), each
against the fp64 einsum of tests/gemm_batched_ref.py:

  1  S  = alpha Q K^T   ROW/ROW   A, B column slices of the packed qkv row          5  dQ = dS K      ROW/COL   C = first third of dqkv
  2  O  = P V           ROW/COL   C a column slice of [B][L][hid]                   6  dK = dS^T Q    COL/COL   C = second third of dqkv
  3  dV = P^T dO        COL/COL   C = third third of the packed dqkv row            7  film[i] = ta W_i^T + b_i   ROW/ROW, sA = (0, 0), sBias
  4  dP = dO V^T        ROW/ROW   lda = hid, ldb = 3 hid                            8  P[i] = dfilm[i] W_i        ROW/COL

Criterion: test_kernels_gpu.close with its defaults (4 x the error of torch's fp32 result of the same expression + 2e-6 x scale), applied
PER BATCH ENTRY; the operands of entry z are scaled by 2^((z % 5) - 2), so an entry computed from another entry's operands cannot pass.
Guard bands: every destination is pre-filled with 7.0, every row pitch is 4 floats wider than the row, 256 rows follow the last image;
after each launch everything outside the entries' own elements -- pad columns, trailing rows, the other heads' thirds of dqkv, and the last
entry's region after a launch over batch - 1 entries -- must equal the pre-fill bit for bit.  Sources carry the same padding as finite junk.
Each form runs as the engine calls it and with accumulate = True, alpha = -0.5 onto a random destination, at every tile request; the
instantiation that ran is asserted from vd_gemm_last_tile.  A `FIG` line per (form, geometry, tile request, mode) records the code, the worst
per-entry error and the fp32 yardstick (both relative to the entry's largest expected magnitude).  Needs an MI355X."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_batched_ref as G                                      # noqa: E402
from test_kernels_gpu import _attn_ref, close, rnd                # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROW, COL = 0, 1
WIDE = 128256
TILES = (0, 64, 128, 12864, 64128)
FORCED = {64: (64, 64), 128: (128, 128), 12864: (128, 64), 64128: (64, 128), WIDE: (128, 256)}
# process-wide switches of csrc/gemm.hip this file is re-run under (test_process_wide_switches); read by the library once per process
LEGACY = os.environ.get("VD_GEMM_LEGACY") is not None

ATTN_GEOMS = [  # B, nh, L, hd
    (3, 2, 64, 64),       # M tail on every 128-row tile, N tail for hd on 128-wide tiles; 6 workgroups at tile 128: no XCD remap
    (2, 3, 192, 32),      # L = 128 + 64, hd below every tile width, nh != B; form 1 at tile 64: 54 workgroups, remap with T % 8 = 6
    (1, 2, 320, 128),     # the L tail of the fused kernels' own tests
    (2, 2, 256, 256),     # the benchmark's head dim; N % 256 == 0 for all six forms
]
FILM_GEOMS = [  # nb, B, E, c2
    (1, 5, 128, 64),
    (3, 64, 256, 384),
    (7, 130, 512, 256),   # M tail 128 + 2; the 128x256 form serves both directions
    (2, 8, 100, 72),      # K no multiple of either K tile, in both directions
    (2, 8, 100, 70),      # forward only: N % 4 != 0 sends the per-entry bias through the column-per-lane epilogue (backward: K % 4 refused)
]
_gid = lambda p, i, g: f"{p}{i}_" + "x".join(map(str, g))
ATTN_PARAMS = [pytest.param(gi, t, id=f"{_gid('g', gi, g)}-t{t}") for gi, g in enumerate(ATTN_GEOMS) for t in TILES + ((WIDE,) if gi == 3 else ())]
FILM_PARAMS = [pytest.param(fi, t, id=f"{_gid('f', fi, g)}-t{t}") for fi, g in enumerate(FILM_GEOMS) for t in TILES + ((WIDE,) if fi == 2 else ())]
RES_PARAMS = [pytest.param(fi, t, id=f"{_gid('f', fi, FILM_GEOMS[fi])}-t{t}") for fi in (2, 4) for t in (0, 128)]
CHILD_GEOMS = 2                                                   # attention geometries the switch rows re-run
CHILD_TESTS = sum(1 for p in ATTN_PARAMS if p.values[0] < CHILD_GEOMS) + CHILD_GEOMS + len(FILM_PARAMS) + len(RES_PARAMS) + 1

SEEN_T = {}               # (geometry, tile request, form) -> workgroups of the launch, from the reported tile


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


def _f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


# ------------------------------------------------------------------------------------------------ one launch, checked
class Dest:
    """a destination layout: how the entries sit in the [rows][pitch] buffer"""

    def __init__(self, rows, pitch, pack, unpack, mask, offset):
        self.rows, self.pitch, self.pack, self.unpack, self.mask, self.offset = rows, pitch, pack, unpack, mask, offset


def _heads_dest(B, nh, L, hd, pitch, col0):
    return Dest(B * L + G.GUARD_ROWS, pitch, lambda x, buf: G.pack_heads(x, pitch, col0, buf),
                lambda buf: G.unpack_heads(buf, B, nh, L, hd, col0), lambda n=None: G.heads_mask(B, nh, L, hd, pitch, col0, n), col0)


def _rows_dest(shape, pitch):
    n = math.prod(shape[:-2])
    R, Cc = shape[-2:]
    return Dest(n * R + G.GUARD_ROWS, pitch, lambda x, buf: G.pack_rows(x, pitch, buf), lambda buf: G.unpack_rows(buf, shape),
                lambda e=None: G.rows_mask(n, R, Cc, pitch, e), 0)


def _tile_checks(H, tile, name):
    """-> (code, bm, bn) of the launch that just ran, after the assertions every launch must meet"""
    code = H.lib().vd_gemm_last_tile()
    tr, spl, kt, bm, bn = H.tile_fields(code)
    assert (kt == 0) == LEGACY, f"{name}: K tile {kt} (0 = the register-staged kernel) with VD_GEMM_LEGACY {'set' if LEGACY else 'unset'} ({code})"
    if tile in FORCED:
        assert (bm, bn) == FORCED[tile], f"{name}: tile request {tile} ran {bm}x{bn} ({code})"
    if bm == 128:
        # the register-staged kernel has no split-operand form: under VD_GEMM_LEGACY the flag is off whatever VD_GEMM_SPLIT says
        assert spl == (bool(H.lib().vd_gemm_split_forms()) and not LEGACY), f"{name}: split flag {spl} ({code})"
    else:
        assert not spl, f"{name}: split flag on a 64-row tile ({code})"
    return code, bm, bn


def _wide_exists(H):
    return bool(H.lib().vd_gemm_split_forms()) and not LEGACY


def _run_form(H, name, key, spec, dest, prod, tile, batch, nh, extra64=None, c0=None, engine_alpha=1.0):
    """One form at one tile request: the engine's call, the accumulate call and the launch over batch - 1 entries, each with its guard bands;
    the numbers per entry.  ``spec``: the gemm() arguments without C / alpha / accumulate / tile / batch; ``extra64``: bias / residual terms
    of the expected value (fp32 tensors broadcastable to the product)."""
    p64, p32 = prod
    M, N = spec["M"], spec["N"]
    lead = p64.shape[:-2]
    full_mask = dest.mask()

    def launch(base_cpu, t, alpha, acc, n):
        out = base_cpu.clone().to(DEV)
        H.gemm(spec["A"], spec["B"], out.view(-1)[dest.offset:], **{k: v for k, v in spec.items() if k not in ("A", "B")},
               alpha=alpha, accumulate=acc, tile=t, batch=n, nh=nh)
        torch.cuda.synchronize()
        return out

    for mode, alpha, acc in (("engine", _f32(engine_alpha), False), ("accumulate", -0.5, True)):
        base = torch.full((dest.rows, dest.pitch), G.SENTINEL)
        if acc:
            dest.pack(c0, base)
        if tile == WIDE and not _wide_exists(H):
            with pytest.raises(H.HipError):                       # the form does not exist in this process: the request is refused
                launch(base, WIDE, alpha, acc, batch)
            continue
        out_d = launch(base, tile, alpha, acc, batch)
        code, bm, bn = _tile_checks(H, tile, name)
        if tile == WIDE:
            ref_d = launch(base, 128, alpha, acc, batch)
            assert H.tile_fields(H.lib().vd_gemm_last_tile())[3:] == (128, 128)
            assert torch.equal(out_d, ref_d), f"{name} [{mode}]: the 128x256 form differs from the 128x128 form in {(out_d != ref_d).sum().item()} elements"
        T = -(-M // bm) * -(-N // bn) * batch
        SEEN_T[key] = T
        out = out_d.cpu()
        assert torch.equal(torch.where(full_mask, base, out), base), \
            f"{name} [{mode}, tile {tile}, code {code}]: {(torch.where(full_mask, base, out) != base).sum().item()} guard elements written"
        got = dest.unpack(out).reshape(-1, M, N)
        terms = [t for t in (extra64 or [])]
        e64 = G.compose(p64, alpha, *terms, c0=c0 if acc else None).reshape(-1, M, N)
        e32 = G.compose(p32, alpha, *terms, c0=c0 if acc else None).reshape(-1, M, N)
        worst, worst_nat = 0.0, 0.0
        for z in range(got.shape[0]):
            err = close(got[z], e64[z], e32[z], name=f"{name} [{mode}, tile {tile}, code {code}] entry {z} of {lead}")
            scale = e64[z].abs().max().item()
            worst = max(worst, err / scale)
            worst_nat = max(worst_nat, (e32[z].double() - e64[z]).abs().max().item() / scale)
        print(f"FIG {name} tile={tile} mode={mode} code={code} T={T} err={worst:.2e} fp32={worst_nat:.2e}")
        if not acc and batch > 1:
            part = launch(base, tile, alpha, False, batch - 1).cpu()
            pm = dest.mask(batch - 1)
            assert torch.equal(torch.where(pm, base, part), base), f"{name} [tile {tile}]: a launch over {batch - 1} of {batch} entries wrote outside them"
            assert not torch.equal(torch.where(pm, part, base), base)                # ... and did write them


def _all_forms(runs):
    """run every form's check; one message per failing form"""
    failed = []
    for name, fn in runs:
        try:
            fn()
        except AssertionError as e:
            failed.append(f"--- {name}: {e}")
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------ attention forms 1-6
@functools.lru_cache(maxsize=None)
def _attn_case(gi):
    """operands, fp64 / fp32 products and the packed device sources of a geometry: built once, never modified"""
    B, nh, L, hd = ATTN_GEOMS[gi]
    hid = nh * hd
    ld, ldo, lds = 3 * hid + G.PAD, hid + G.PAD, L + G.PAD
    d = G.attn_operands(B, nh, L, hd)
    qkv = G.pack_heads(d["q"], ld, 0)
    G.pack_heads(d["k"], ld, hid, qkv)
    G.pack_heads(d["v"], ld, 2 * hid, qkv)
    src = dict(qkv=qkv.to(DEV), dO=G.pack_heads(d["dO"], ldo, 0).to(DEV), P=G.pack_rows(d["P"], lds).to(DEV), dS=G.pack_rows(d["dS"], lds).to(DEV))
    return d, G.attn_products(d), src


def _attn_specs(gi, src):
    """{form: (gemm arguments, destination layout)} -- the launches of engine.py::_attn_fwd / _attn_bwd on the padded buffers"""
    B, nh, L, hd = ATTN_GEOMS[gi]
    hid = nh * hd
    ld, ldo, lds = 3 * hid + G.PAD, hid + G.PAD, L + G.PAD
    flat = src["qkv"].view(-1)
    q, k, v = flat[0:], flat[hid:], flat[2 * hid:]
    sP, sQ, sO = (nh * L * lds, L * lds), (L * ld, hd), (L * ldo, hd)
    maps = _rows_dest((B, nh, L, L), lds)
    third = lambda i: _heads_dest(B, nh, L, hd, ld, i * hid)
    return {
        1: (dict(A=q, B=k, M=L, N=L, K=hd, a_kind=ROW, b_kind=ROW, lda=ld, ldb=ld, ldc=lds, sA=sQ, sB=sQ, sC=sP), maps),
        2: (dict(A=src["P"], B=v, M=L, N=hd, K=L, a_kind=ROW, b_kind=COL, lda=lds, ldb=ld, ldc=ldo, sA=sP, sB=sQ, sC=sO), _heads_dest(B, nh, L, hd, ldo, 0)),
        3: (dict(A=src["P"], B=src["dO"], M=L, N=hd, K=L, a_kind=COL, b_kind=COL, lda=lds, ldb=ldo, ldc=ld, sA=sP, sB=sO, sC=sQ), third(2)),
        4: (dict(A=src["dO"], B=v, M=L, N=L, K=hd, a_kind=ROW, b_kind=ROW, lda=ldo, ldb=ld, ldc=lds, sA=sO, sB=sQ, sC=sP), maps),
        5: (dict(A=src["dS"], B=k, M=L, N=hd, K=L, a_kind=ROW, b_kind=COL, lda=lds, ldb=ld, ldc=ld, sA=sP, sB=sQ, sC=sQ), third(0)),
        6: (dict(A=src["dS"], B=q, M=L, N=hd, K=L, a_kind=COL, b_kind=COL, lda=lds, ldb=ld, ldc=ld, sA=sP, sB=sQ, sC=sQ), third(1)),
    }


@pytest.mark.parametrize("gi,tile", ATTN_PARAMS)
def test_attention_forms(H, gi, tile):
    B, nh, L, hd = ATTN_GEOMS[gi]
    d, prods, src = _attn_case(gi)
    specs = _attn_specs(gi, src)
    runs = []
    for f, (spec, dest) in specs.items():
        c0 = d["c0_map"] if G.ATTN_FORMS[f][3] == "map" else d["c0_head"]
        name = f"form {f} g{gi} {B}x{nh}x{L}x{hd}"
        runs.append((name, functools.partial(_run_form, H, name, ("g", gi, tile, f), spec, dest, prods[f], tile, B * nh, nh, c0=c0,
                                             engine_alpha=1.0 / math.sqrt(hd) if f == 1 else 1.0)))      # (the engine scales the logits only)
    _all_forms(runs)


@pytest.mark.parametrize("gi", [pytest.param(gi, id=_gid("g", gi, g)) for gi, g in enumerate(ATTN_GEOMS)])
def test_attention_chain(H, gi):
    """forms 1 -> softmax_rows -> 2, then 3, 4 -> softmax_rows_bwd -> 5, 6 with exactly the engine's buffers and stride tuples, against
    test_kernels_gpu._attn_ref in fp64 and its autograd under the criterion of test_attn_fused_backward; where the fused kernels serve
    the geometry they run on the same buffers and must meet the same criterion"""
    B, nh, L, hd = ATTN_GEOMS[gi]
    hid, ld = nh * hd, 3 * nh * hd
    qkv = rnd(B, L, 3 * hid, seed=L + hd + 1) * 1.5
    do = rnd(B, L, hid, seed=3)
    g64 = qkv.double().requires_grad_(True)
    o64 = _attn_ref(g64, B, nh, L, hd, torch.float64)
    o64.backward(do.double())
    g32 = qkv.clone().requires_grad_(True)
    o32 = _attn_ref(g32, B, nh, L, hd, torch.float32)
    o32.backward(do)
    qd, dO = qkv.to(DEV), do.to(DEV)
    q, k, v = qd[0, 0, 0:], qd[0, 0, hid:], qd[0, 0, 2 * hid:]
    sP, sQ, sO = (nh * L * L, L * L), (L * ld, hd), (L * hid, hd)
    alpha = 1.0 / math.sqrt(hd)
    S = torch.full((B, nh, L, L), G.SENTINEL, device=DEV)
    O = torch.full((B, L, hid), G.SENTINEL, device=DEV)
    H.gemm(q, k, S, L, L, hd, a_kind=ROW, b_kind=ROW, lda=ld, ldb=ld, ldc=L, batch=B * nh, nh=nh, sA=sQ, sB=sQ, sC=sP, alpha=alpha)
    H.softmax_rows(S, B * nh * L, L)
    H.gemm(S, v, O, L, hd, L, a_kind=ROW, b_kind=COL, lda=L, ldb=ld, ldc=hid, batch=B * nh, nh=nh, sA=sP, sB=sQ, sC=sO)
    dqkv = torch.full((B, L, ld), G.SENTINEL, device=DEV)
    dq, dk, dv = dqkv[0, 0, 0:], dqkv[0, 0, hid:], dqkv[0, 0, 2 * hid:]
    dP = torch.full((B, nh, L, L), G.SENTINEL, device=DEV)
    H.gemm(S, dO, dv, L, hd, L, a_kind=COL, b_kind=COL, lda=L, ldb=hid, ldc=ld, batch=B * nh, nh=nh, sA=sP, sB=sO, sC=sQ)
    H.gemm(dO, v, dP, L, L, hd, a_kind=ROW, b_kind=ROW, lda=hid, ldb=ld, ldc=L, batch=B * nh, nh=nh, sA=sO, sB=sQ, sC=sP)
    H.softmax_rows_bwd(S, dP, B * nh * L, L, alpha)
    H.gemm(dP, k, dq, L, hd, L, a_kind=ROW, b_kind=COL, lda=L, ldb=ld, ldc=ld, batch=B * nh, nh=nh, sA=sP, sB=sQ, sC=sQ)
    H.gemm(dP, q, dk, L, hd, L, a_kind=COL, b_kind=COL, lda=L, ldb=ld, ldc=ld, batch=B * nh, nh=nh, sA=sP, sB=sQ, sC=sQ)
    torch.cuda.synchronize()
    e_fwd = close(O, o64, o32, floor=3e-6, name=f"chain g{gi}: forward")
    e_bwd = close(dqkv, g64.grad, g32.grad, floor=3e-6, name=f"chain g{gi}: backward")
    print(f"FIG chain g{gi} {B}x{nh}x{L}x{hd} three-launch fwd={e_fwd:.2e} bwd={e_bwd:.2e}")
    if H.attn_supported(L, hd, True):
        Of = torch.full((B, L, hid), G.SENTINEL, device=DEV)
        dqkv_f = torch.full((B, L, ld), G.SENTINEL, device=DEV)
        lse, delta = torch.empty(B * nh * L, device=DEV), torch.empty(B * nh * L, device=DEV)
        H.attn_fwd(q, k, v, ld, Of, hid, lse, B, nh, L, hd, alpha)
        H.attn_bwd(q, k, v, ld, Of, hid, dO, hid, lse, delta, dqkv_f[0, 0, 0:], dqkv_f[0, 0, hid:], dqkv_f[0, 0, 2 * hid:], ld, B, nh, L, hd, alpha)
        torch.cuda.synchronize()
        f_fwd = close(Of, o64, o32, floor=3e-6, name=f"chain g{gi}: fused forward")
        f_bwd = close(dqkv_f, g64.grad, g32.grad, floor=3e-6, name=f"chain g{gi}: fused backward")
        print(f"FIG chain g{gi} {B}x{nh}x{L}x{hd} fused fwd={f_fwd:.2e} bwd={f_bwd:.2e}")


def test_both_remap_regimes_are_visited(H):
    """The XCD tile remap of the LDS-DMA kernels moves the batch index too and has two regimes: fewer than 16 workgroups (identity) and
    >= 16 with T % 8 != 0 (unequal XCD shares).  Both must occur among the attention launches of this file: T from the tile the host plan
    reports for every (geometry, tile request, form) -- the same plan vd_gemm launches by, and equal to what the launches of this process
    reported where they have run."""
    regimes = {}
    for gi, (B, nh, L, hd) in enumerate(ATTN_GEOMS):
        for tile in TILES + ((WIDE,) if gi == 3 and _wide_exists(H) else ()):
            for f in G.ATTN_FORMS:
                M, N, K = (L, L, hd) if f in (1, 4) else (L, hd, L)
                ak, bk = {1: (ROW, ROW), 2: (ROW, COL), 3: (COL, COL), 4: (ROW, ROW), 5: (ROW, COL), 6: (COL, COL)}[f]
                code = H.lib().vd_gemm_plan_tile(M, N, K, ak, bk, B * nh, tile, 0)
                assert code > 0, (gi, tile, f)
                bm, bn = H.tile_fields(code)[3:]
                T = -(-M // bm) * -(-N // bn) * B * nh
                if ("g", gi, tile, f) in SEEN_T:
                    assert SEEN_T[("g", gi, tile, f)] == T, (gi, tile, f, T, SEEN_T[("g", gi, tile, f)])
                regimes.setdefault("identity" if T < 16 else ("unequal" if T % 8 else "equal"), []).append((gi, tile, f, T))
    assert regimes.get("identity") and regimes.get("unequal"), {k: len(v) for k, v in regimes.items()}
    assert (0, 128, 1, 6) in regimes["identity"] and (1, 64, 1, 54) in regimes["unequal"]
    print("FIG remap regimes " + ", ".join(f"{k}: {len(v)}" for k, v in sorted(regimes.items())))


# ------------------------------------------------------------------------------------------------ FiLM forms 7, 8
@functools.lru_cache(maxsize=None)
def _film_case(fi):
    nb, B, E, c2 = FILM_GEOMS[fi]
    d = G.film_operands(nb, B, E, c2)
    src = dict(ta=G.pack_rows(d["ta"][None], E + G.PAD).to(DEV), W=G.pack_rows(d["W"], E + G.PAD).to(DEV), bias=d["bias"].to(DEV),
               df=G.pack_rows(d["df"], c2 + G.PAD).to(DEV), R=d["R"].to(DEV))
    return d, G.film_products(d), src


def _film_specs(fi, src, residual=False):
    """the launches of engine.py::_film_fwd / _film_bwd on the padded buffers (bias and residual contiguous, as the engine holds them)"""
    nb, B, E, c2 = FILM_GEOMS[fi]
    lde, ldc2 = E + G.PAD, c2 + G.PAD
    fwd = dict(A=src["ta"], B=src["W"], M=B, N=c2, K=E, a_kind=ROW, b_kind=ROW, lda=lde, ldb=lde, ldc=ldc2, bias=src["bias"], sBias=c2,
               sA=(0, 0), sB=(c2 * lde, 0), sC=(B * ldc2, 0))
    if residual:
        fwd.update(R=src["R"], ldr=c2, sR=(B * c2, 0))
    bwd = dict(A=src["df"], B=src["W"], M=B, N=E, K=c2, a_kind=ROW, b_kind=COL, lda=ldc2, ldb=lde, ldc=lde, sA=(B * ldc2, 0), sB=(c2 * lde, 0),
               sC=(B * lde, 0))
    return {7: (fwd, _rows_dest((nb, B, c2), ldc2)), 8: (bwd, _rows_dest((nb, B, E), lde))}


@pytest.mark.parametrize("fi,tile", FILM_PARAMS)
def test_film_forms(H, fi, tile):
    nb, B, E, c2 = FILM_GEOMS[fi]
    d, prods, src = _film_case(fi)
    specs = _film_specs(fi, src)
    name = lambda f: f"form {f} f{fi} {nb}x{B}x{E}x{c2}"
    runs = [(name(7), functools.partial(_run_form, H, name(7), ("f", fi, tile, 7), *specs[7], prods[7], tile, nb, 1,
                                        extra64=[d["bias"].unsqueeze(1)], c0=d["c0_fwd"]))]
    if c2 % 4 == 0:
        runs.append((name(8), functools.partial(_run_form, H, name(8), ("f", fi, tile, 8), *specs[8], prods[8], tile, nb, 1, c0=d["c0_bwd"])))
    else:
        spec, dest = specs[8]                                     # K % 4 != 0 with a k-contiguous A: refused, nothing launched
        with pytest.raises(H.HipError):
            H.gemm(spec["A"], spec["B"], torch.empty(dest.rows, dest.pitch, device=DEV), **{k: v for k, v in spec.items() if k not in ("A", "B")},
                   batch=nb, tile=tile)
    _all_forms(runs)


@pytest.mark.parametrize("fi,tile", RES_PARAMS)
def test_film_forward_batched_residual(H, fi, tile):
    """form 7 with a residual R[nb][B][c2], sR = (B c2, 0): the batched residual strides through both epilogues (c2 = 256: transposed
    accumulators, c2 = 70: column per lane)"""
    nb, B, E, c2 = FILM_GEOMS[fi]
    d, prods, src = _film_case(fi)
    spec, dest = _film_specs(fi, src, residual=True)[7]
    name = f"form 7+R f{fi} {nb}x{B}x{E}x{c2}"
    _all_forms([(name, functools.partial(_run_form, H, name, ("fr", fi, tile, 7), spec, dest, prods[7], tile, nb, 1,
                                         extra64=[d["bias"].unsqueeze(1), d["R"]], c0=d["c0_fwd"]))])


# ------------------------------------------------------------------------------------------------ process-wide switches
@pytest.mark.parametrize("knobs", [{"VD_GEMM_SPLIT": "0"}, {"VD_GEMM_LEGACY": "1"}, {"VD_GEMM_TR": "0"}, {"VD_GEMM_KT": "16", "VD_GEMM_TILE": "128"}],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_process_wide_switches(H, knobs):
    """The kernels a plain run does not select for these launches -- the fp32-MFMA forms of the 128-row tiles, the register-staged kernel
    with its own batch addressing, the column-per-lane epilogue, the K = 16 tile of the 128x128 forms -- share none of their staging code.
    The switches are read once per process, so each row re-runs this file (first two attention geometries, every FiLM case) in a fresh
    child; the pass count is asserted so that a selection that runs nothing fails."""
    env = dict(os.environ, **knobs)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "--no-header", "-p", "no:cacheprovider", "-k",
                        "not process_wide_switches and not " + " and not ".join(f"g{gi}_" for gi in range(CHILD_GEOMS, len(ATTN_GEOMS)))],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert f"{CHILD_TESTS} passed" in r.stdout and "skipped" not in r.stdout and "failed" not in r.stdout, r.stdout[-500:]
