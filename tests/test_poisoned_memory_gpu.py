"""Every kernel entry that takes pitched operands, a scratch buffer or a non-accumulating destination, run twice: once as its own parity
test runs it (pitch columns 3.0, scratch as the previous launch left it) and checked against fp64 with that test's bound, then again with
NaN in everything the contract of include/vdiff_hip.h says is not read:

  pitch columns of the sources (from the padded channel count up to the pitch), every cached scratch buffer of v_diffusion._hip (whole,
  all streams: tests/poison.py), the real part of every destination of a non-accumulating call, every statistics-partial / colsum side
  output; the pitch columns of destinations hold the finite sentinel -777.

The second run must reproduce the first BIT FOR BIT in the real part of every output, finite, with the sentinels in place: a K tail that
is read and multiplied by zero, a split-K slab summed without having been written, a row of the last 16-tile block of V / dM past T, a
destination accumulated into where it should be overwritten -- each turns a finite leftover into a NaN here.  Every case asserts that the
scratch tag of its entry was among the poisoned ones and that both runs took the same kernel form (the intended one where the entry's own
test names it).

And the memory AROUND the tensors ("Memory a kernel may not read", the write side): every destination and every source is a view
into the middle of a larger allocation (poison.Banded: a band of an image / 256 rows / 64 Ki floats on either side, sentinel around
destinations, the run's pad value -- NaN in the second run -- around sources, so the halo rows above the first image and below the last are
poisoned too), and the second run gets scratch of EXACTLY the bytes asked for, between sentinel bands (poison.ExactWorkspace).  No band
of a destination or of a scratch buffer may change.  Needs an MI355X."""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison as P                                                # noqa: E402
from test_kernels_gpu import close, from_nhwc, ref_gn_block, rnd  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
CLEAN_PAD, CLEAN_FILL = 3.0, 7.0            # what the parity tests put into source pitch columns / destinations


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


@pytest.fixture(autouse=True)
def _drop_bands():
    """the ledger of poison.Banded records keeps their allocations alive: emptied after every test"""
    yield
    P.forget_bands()


def dest(shape, cols=None, poison=False, init=None):
    """a destination: real part (columns [0, cols) of the last axis; cols None: everything) NaN in the poisoned run, CLEAN_FILL in the clean
    one -- or `init` (a CPU tensor of the real part's shape) for an accumulating call --, pitch columns the sentinel; banded: the tensor
    is a view between two sentinel bands of poison.band_elems(shape) floats, which twice() checks after each run"""
    t = P.banded(shape, P.SENTINEL, P.SENTINEL, device=DEV)
    real = t if cols is None else t[..., :cols]
    if init is not None:
        real.copy_(init)
    else:
        real.fill_(NAN if poison else CLEAN_FILL)
    return t


def _sync():
    """device synchronisation; a device fault ends the session here (nothing more is launched on a device that has faulted)"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault, session ended: {e}", returncode=3)


def twice(H, tags, run, verify):
    """run(pad, poison) -> (kernel form, {name: (tensor, real columns or None)}).  Clean run, `verify(outputs)` against fp64, poison, the same
    call again, bitwise comparison.  Returns both forms' common value.

    Memory AROUND the tensors: every destination of dest() and every source of poison.pitched() / pitched_rows() lies between two bands
    (sentinel / the run's pad value), and the poisoned pass runs on poison.ExactWorkspace -- scratch of exactly the bytes the wrapper
    asked for, NaN-filled, between sentinel bands.  After each pass no band of a destination, after the poisoned pass no band of a
    scratch buffer may have changed, and the entry's tag must have been requested."""
    _sync()
    damage = P.bands_damage()                                   # (packed weight images made for this case before it runs)
    assert not damage, f"written outside a destination before the runs: {damage}"
    form_c, clean = run(CLEAN_PAD, False)
    _sync()
    damage = P.bands_damage()
    assert not damage, f"written outside a destination (clean run): {damage}"
    verify(clean)
    found = P.poison_workspaces(H, P.FLOAT_TAGS)
    assert set(tags) <= found, f"scratch of this entry not poisoned: wanted {tags}, cached {sorted(found)}"
    damage = P.bands_damage()                                   # (statistics that verify() finalised into banded tensors)
    assert not damage, f"written outside a destination while verifying: {damage}"
    exact = P.ExactWorkspace()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(H, "workspace", exact)
        form_p, pois = run(NAN, True)
        _sync()
    damage = P.bands_damage()
    assert not damage, f"written outside a destination (poisoned run): {damage}"
    assert exact.intact(), f"written outside the scratch the entry was given {exact.requests}: {exact.damage()}"
    assert set(tags) <= exact.tags(), f"scratch of this entry not requested: wanted {tags}, requested {exact.requests}"
    assert form_c == form_p, f"the two runs took different kernel forms: {form_c} / {form_p}"
    assert clean.keys() == pois.keys()
    for name, (tc, cols) in clean.items():
        tp = pois[name][0]
        rc, rp = (tc, tp) if cols is None else (tc[..., :cols], tp[..., :cols])
        bad = int((~torch.isfinite(rp)).sum())
        assert bad == 0, f"{name}: {bad} of {rp.numel()} elements are not finite after poisoning ({int(torch.isnan(rp).sum())} NaN)"
        if not P.same_bits(rc, rp):
            diff = rc != rp
            raise AssertionError(f"{name}: {int(diff.sum())} of {rc.numel()} elements differ after poisoning, largest difference "
                                 f"{(rc - rp).abs().max().item():.3e}")
        if cols is not None:
            for which, t in (("clean", tc), ("poisoned", tp)):
                assert bool((t[..., cols:] == P.SENTINEL).all()), f"{name}: pitch columns of the destination were written ({which} run)"
    return form_c


def rel_max(got, ref64):
    got, ref64 = got.detach().double().cpu(), ref64.double()
    return ((got - ref64).norm() / ref64.norm()).item(), (got - ref64).abs().max().item()


# ------------------------------------------------------------------------------------------------ vd_gemm
@functools.lru_cache(maxsize=None)
def _gemm_data(M, N, K):
    A, B, bias, R = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3), rnd(M, N, seed=4)
    return A, B, bias, R, 0.5 * (A.double() @ B.double().T) + bias.double() + R.double(), 0.5 * (A @ B.T) + bias + R


@pytest.mark.parametrize("a_kind,b_kind", [(0, 0), (0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K", [(200, 72, 100), (132, 260, 36), (36, 4, 8)])
@pytest.mark.parametrize("tile", [0, 64, 128, 12864, 64128])
def test_gemm_kinds(H, a_kind, b_kind, M, N, K, tile):
    """test_kernels_gpu.py::test_gemm_kinds with EVERY pitch 4 floats above its extent (A, B, residual, C): ragged M, N and K tiles of
    every operand kind on every tile of the menu"""
    A, B, bias, R, ref64, ref32 = _gemm_data(M, N, K)

    def run(pad, poison):
        Ad = P.pitched_rows(A if a_kind == 0 else A.T.contiguous(), (K if a_kind == 0 else M) + 4, pad)
        Bd = P.pitched_rows(B if b_kind == 0 else B.T.contiguous(), (K if b_kind == 0 else N) + 4, pad)
        Rd = P.pitched_rows(R, N + 4, pad)
        Cd = dest((M, N + 4), N, poison)
        H.gemm(Ad, Bd, Cd, M, N, K, a_kind=a_kind, b_kind=b_kind, lda=Ad.shape[1], ldb=Bd.shape[1], ldc=N + 4, bias=P.on_device(bias), R=Rd,
               ldr=N + 4, alpha=0.5, tile=tile)
        return H.lib().vd_gemm_last_tile(), {"C": (Cd, N)}
    twice(H, (), run, lambda o: close(o["C"][0][:, :N], ref64, ref32, name=f"gemm{a_kind}{b_kind}"))


@functools.lru_cache(maxsize=None)
def _wgrad_gemm_data(M, N, K):
    A, B = rnd(K, M, seed=8), rnd(K, N, seed=9)
    return A, B, A.double().T @ B.double(), A.T @ B, A.double().sum(0), A.sum(0)


def _slabs(H, code, K, S):
    """(K tile, K tiles per slab, slabs that hold work) of a split-K launch, from the form that ran (csrc/gemm.hip: run_gemm)"""
    kt = H.tile_fields(code)[2]
    assert kt in (16, 32), code
    kt_total = -(-K // kt)
    per = -(-kt_total // S)
    return kt, per, -(-kt_total // per)


# (12, 260, 1000, 3): the last slab is ragged (its last K tile holds 8 of 32 / 8 of 16 rows); (64, 96, 288, 8): 9 K tiles of 32 at 2 per slab
# fill 5 slabs, 18 of 16 at 3 per slab fill 6 -- the other requested slabs are never written and must not be summed
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,N,K,splitk", [(12, 260, 1000, 3), (64, 96, 288, 8)])
@pytest.mark.parametrize("tile", [0, 128, 64, 12864, 64128])
def test_gemm_splitk_with_colsum(H, M, N, K, splitk, tile, accumulate):
    """test_kernels_gpu.py::test_gemm_colsum_rides_on_wgrad (COL / COL split-K with the bias-gradient rider) on a poisoned "splitk" scratch,
    overwriting (C and colsum NaN beforehand) and accumulating"""
    A, B, c64, c32, s64, s32 = _wgrad_gemm_data(M, N, K)
    c0, s0 = rnd(M, N, seed=11), rnd(M, seed=12)
    seen = {}

    def run(pad, poison):
        Ad, Bd = P.pitched_rows(A, M + 4, pad), P.pitched_rows(B, N + 4, pad)
        Cd = dest((M, N + 4), N, poison, init=c0 if accumulate else None)
        cs = dest((M,), None, poison, init=s0 if accumulate else None)
        H.gemm(Ad, Bd, Cd, M, N, K, a_kind=1, b_kind=1, lda=M + 4, ldb=N + 4, ldc=N + 4, splitk=splitk, tile=tile, colsum=cs,
               accumulate=accumulate, colsum_accumulate=accumulate)
        seen["code"] = H.lib().vd_gemm_last_tile()
        return seen["code"], {"C": (Cd, N), "colsum": (cs, None)}

    def verify(o):
        add_c, add_s = (c0.double(), s0.double()) if accumulate else (0.0, 0.0)
        close(o["C"][0][:, :N], c64 + add_c, c32 + (c0 if accumulate else 0.0), name="wgrad gemm")
        close(o["colsum"][0], s64 + add_s, s32 + (s0 if accumulate else 0.0), name="colsum")
    twice(H, ("splitk",), run, verify)
    kt, per, used = _slabs(H, seen["code"], K, splitk)
    if (M, N, K, splitk) == (64, 96, 288, 8):
        assert used < splitk, f"every requested slab holds work (K tile {kt}): the case no longer has unwritten slabs"
    else:
        assert K % kt != 0 and used == splitk, f"K tile {kt}: the case no longer has a ragged last K tile in its last slab"


@pytest.mark.parametrize("count,M,N,K,splitk,pad", [(3, 64, 96, 1000, 4, 8), (5, 128, 128, 288, 8, 4), (32, 36, 260, 512, 2, 4)])
def test_gemm_grouped_wgrad(H, count, M, N, K, splitk, pad):
    """test_kernels_gpu.py::test_gemm_grouped_wgrad: a ragged last K tile (K = 1000), requested slabs that hold no work (K = 288 at 8
    slabs), 32 entries with ragged M and N tiles"""
    g = torch.Generator(DEV).manual_seed(count * 1000 + M)
    data = [(torch.randn((K, M), device=DEV, generator=g), torch.randn((K, N), device=DEV, generator=g)) for _ in range(count)]
    refs = [(dy.double().T @ x.double(), dy.double().sum(0)) for dy, x in data]

    def run(padv, poison):
        ents = []
        for dy, x in data:
            dyp, xp = (P.banded((K, c + pad), padv, padv, device=DEV, check=False) for c in (M, N))
            dyp[:, :M], xp[:, :N] = dy, x
            ents.append((dyp, xp, dest((M, N + pad), N, poison), dest((M,), None, poison)))
        H.gemm_grouped_wgrad(ents, M, N, K, M + pad, N + pad, N + pad, splitk)
        out = {}
        for e, (_, _, dw, db) in enumerate(ents):
            out[f"dW[{e}]"], out[f"dbias[{e}]"] = (dw, N), (db, None)
        return H.lib().vd_gemm_last_tile(), out

    def verify(o):
        for e, (rw, rb) in enumerate(refs):
            dw, db = o[f"dW[{e}]"][0], o[f"dbias[{e}]"][0]
            assert (dw[:, :N].double() - rw).abs().max().item() <= 2e-6 * rw.abs().max().item() * max(1.0, (K / 1024) ** 0.5), "grouped dW"
            assert (db.double() - rb).abs().max().item() <= 2e-6 * max(rb.abs().max().item(), 1.0) * max(1.0, (K / 1024) ** 0.5), "grouped dbias"
    code = twice(H, ("splitk",), run, verify)
    if K == 288:
        kt = H.tile_fields(code)[2]
        per = -(-(-(-K // kt)) // splitk)
        assert -(-(-(-K // kt)) // per) < splitk, "every requested slab holds work: the case no longer has unwritten slabs"


# ------------------------------------------------------------------------------------------------ 3x3 convolutions: shared data
@functools.lru_cache(maxsize=None)
def _conv_data(nimg, Hh, Ww, Cin, Cout):
    """inputs of a Cin -> Cout convolution and its fp64 / torch-fp32 forward (+ bias + residual) and input gradient"""
    x, w, b = rnd(nimg, Cin, Hh, Ww, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=3)
    res, dy = rnd(nimg, Cout, Hh, Ww, seed=4), rnd(nimg, Cout, Hh, Ww, seed=5)
    y64 = F.conv2d(x.double(), w.double(), b.double(), padding=1) + res.double()
    y32 = F.conv2d(x, w, b, padding=1) + res
    x64 = torch.zeros(nimg, Cin, Hh, Ww, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w.double(), padding=1).backward(dy.double())
    x32 = torch.zeros(nimg, Cin, Hh, Ww, requires_grad=True)
    F.conv2d(x32, w, padding=1).backward(dy)
    return dict(x=x, w=w, b=b, res=res, dy=dy, y64=y64, y32=y32, dx64=x64.grad, dx32=x32.grad)


@functools.lru_cache(maxsize=None)
def _wgrad_data(nimg, Hh, Ww, Cin, Cout, Cin_w, Cout_w):
    """x / dy with zero channels between the real and the padded count (the contract), fp64 / torch-fp32 weight and bias gradients"""
    x = torch.zeros(nimg, Cin, Hh, Ww)
    x[:, :Cin_w] = rnd(nimg, Cin_w, Hh, Ww, seed=1)
    dy = torch.zeros(nimg, Cout, Hh, Ww)
    dy[:, :Cout_w] = rnd(nimg, Cout_w, Hh, Ww, seed=2)
    w64 = torch.zeros(Cout_w, Cin_w, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x[:, :Cin_w].double(), w64, padding=1).backward(dy[:, :Cout_w].double())
    w32 = torch.zeros(Cout_w, Cin_w, 3, 3, requires_grad=True)
    F.conv2d(x[:, :Cin_w], w32, padding=1).backward(dy[:, :Cout_w])
    return dict(x=x, dy=dy, dw64=w64.grad, dw32=w32.grad, db64=dy[:, :Cout_w].double().sum((0, 2, 3)), db32=dy[:, :Cout_w].sum((0, 2, 3)))


def _bound_direct(o, d, add):
    close(o["dw"][0], d["dw64"] + add, d["dw32"] + add, name="conv wgrad")
    close(o["dbias"][0], d["db64"] + add, d["db32"] + add, name="conv dbias")


def _bound_wino(o, d, add):
    close(o["dw"][0], d["dw64"] + add, d["dw32"] + add, slack=8.0, floor=4e-6, name="wino wgrad")
    close(o["dbias"][0], d["db64"] + add, d["db32"] + add, slack=8.0, floor=4e-6, name="wino dbias")


def _bound_wino43(o, d, add):
    """test_kernels_gpu.py::test_conv3x3_wgrad_wino43: relative L2 <= 8e-6, max error <= 4e-5 of the largest element; dbias 2e-5"""
    ref = d["dw64"]
    got = o["dw"][0].double().cpu() - add
    rel, mx = ((got - ref).norm() / ref.norm()).item(), (got - ref).abs().max().item()
    eb = (o["dbias"][0].double().cpu() - add - d["db64"]).abs().max().item()
    print(f"wgrad43: rel-L2 {rel:.3e}, max {mx:.3e} of {ref.abs().max().item():.3f}, dbias max {eb:.3e} of {d['db64'].abs().max().item():.3f}")
    assert rel <= 8e-6 and mx <= 4e-5 * ref.abs().max().item(), f"wgrad43 rel-L2 {rel:.3e}, max {mx:.3e}"
    assert eb <= 2e-5 * max(d["db64"].abs().max().item(), 1.0), f"wgrad43 dbias {eb:.3e}"


def _wgrad_twice(H, case, accumulate, tags, entry, bound, form):
    """weight + bias gradient through `entry(xd, ldx, dyd, lddy, dw, db, accumulate)`; accumulating runs start from ones (as the parity tests)"""
    nimg, Hh, Ww, Cin, Cout, Cin_w, Cout_w, ex, ey = case
    d = _wgrad_data(nimg, Hh, Ww, Cin, Cout, Cin_w, Cout_w)

    def run(pad, poison):
        xd, dyd = P.pitched(d["x"], Cin + ex, pad), P.pitched(d["dy"], Cout + ey, pad)
        dw = dest((Cout_w, Cin_w, 3, 3), None, poison, init=torch.ones(Cout_w, Cin_w, 3, 3) if accumulate else None)
        db = dest((Cout_w,), None, poison, init=torch.ones(Cout_w) if accumulate else None)
        entry(xd, Cin + ex, dyd, Cout + ey, dw, db, accumulate)
        return form(), {"dw": (dw, None), "dbias": (db, None)}
    return twice(H, tags, run, lambda o: bound(o, d, 1.0 if accumulate else 0.0))


# ------------------------------------------------------------------------------------------------ direct 3x3 (implicit GEMM)
DIRECT_CASES = [(3, 16, 16, 64, 32, 32, 64), (5, 8, 8, 36, 68, 4, 4)]       # nimg, H, W, Cin, Cout, ldx - Cin, ldy - Cout
# a single 2x2 image (every tap but the centre is a halo: the rows above and below the tensor are the source's bands); three output
# channels at pitch 4 (forward only: the input gradient's K is a multiple of 4)
DIRECT_SMALL, DIRECT_THIN = (1, 2, 2, 8, 8, 0, 0), (2, 8, 8, 32, 3, 0, 1)


@pytest.mark.parametrize("case", DIRECT_CASES + [DIRECT_SMALL, DIRECT_THIN])
def test_conv3x3_direct_forward(H, case):
    nimg, Hh, Ww, Cin, Cout, ex, ey = case
    d = _conv_data(nimg, Hh, Ww, Cin, Cout)
    wf = dest((Cout, 9, Cin))
    H.pack_conv3x3(P.on_device(d["w"]), Cout, Cin, wf=wf, Cin_p=Cin)

    def run(pad, poison):
        y = dest((nimg, Hh, Ww, Cout + ey), Cout, poison)
        H.conv3x3(P.pitched(d["x"], Cin + ex, pad), Cin + ex, wf, P.on_device(d["b"]), y, Cout + ey, nimg, Hh, Ww, Cin, Cout,
                  res=P.pitched(d["res"], Cout + ey, pad), ldres=Cout + ey)
        return H.lib().vd_gemm_last_tile(), {"y": (y, Cout)}
    twice(H, (), run, lambda o: close(from_nhwc(o["y"][0], Cout), d["y64"], d["y32"], name="conv fwd"))


@pytest.mark.parametrize("case", DIRECT_CASES + [DIRECT_SMALL])
def test_conv3x3_direct_dgrad(H, case):
    nimg, Hh, Ww, Cin, Cout, ex, ey = case
    d = _conv_data(nimg, Hh, Ww, Cin, Cout)
    wd = dest((Cin, 9, Cout))
    H.pack_conv3x3(P.on_device(d["w"]), Cout, Cin, wd=wd, Cout_p=Cout)

    def run(pad, poison):
        dx = dest((nimg, Hh, Ww, Cin + ex), Cin, poison)
        H.conv3x3(P.pitched(d["dy"], Cout + ey, pad), Cout + ey, wd, None, dx, Cin + ex, nimg, Hh, Ww, Cout, Cin)
        return H.lib().vd_gemm_last_tile(), {"dx": (dx, Cin)}
    twice(H, (), run, lambda o: close(from_nhwc(o["dx"][0], Cin), d["dx64"], d["dx32"], name="conv dgrad"))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", DIRECT_CASES)
def test_conv3x3_direct_wgrad(H, case, accumulate):
    nimg, Hh, Ww, Cin, Cout, ex, ey = case

    def entry(xd, ldx, dyd, lddy, dw, db, acc):
        H.conv3x3_wgrad(xd, ldx, dyd, lddy, nimg, Hh, Ww, Cin, Cout, dw, Cin, Cout, accumulate=acc, dbias=db, direct=True)
    _wgrad_twice(H, (nimg, Hh, Ww, Cin, Cout, Cin, Cout, ex, ey), accumulate, ("wgrad",), entry, _bound_direct, H.lib().vd_gemm_last_tile)


# ------------------------------------------------------------------------------------------------ Winograd F(2x2,3x3)
# the pitched rows of WINO_CASES / WINO_WGRAD_CASES: ld > C on both sides with a partial channel block; four images per workgroup (the last
# workgroup holds 1 of 4), Cout % 32 != 0; 64 tiles per row (the largest patch image); 120 work items (a ragged persistent round)
@pytest.mark.parametrize("case", [(3, 16, 16, 32, 96, 32, 64), (5, 8, 8, 48, 36, 0, 4), (1, 8, 128, 16, 20, 0, 0), (10, 32, 32, 32, 96, 0, 0)])
def test_conv3x3_wino_forward_stats_dgrad(H, case):
    nimg, Hh, Ww, Cin, Cout, ex, ey = case
    HW = Hh * Ww
    assert H.lib().vd_conv3x3_wino_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout + ey, Cout + ey) == 1
    d = _conv_data(nimg, Hh, Ww, Cin, Cout)
    uf, ud = dest((16, Cout, Cin)), dest((16, Cin, Cout))
    H.wino_pack(P.on_device(d["w"]), Cout, Cin, uf=uf, ud=ud)
    used = nimg * (HW // 64) * 2 * Cout                        # [img][H*W/64][2][Cout]

    def run(pad, poison):
        y = dest((nimg, Hh, Ww, Cout + ey), Cout, poison)
        part = dest((H.stats_part_numel(nimg, HW, Cout),), used, poison)
        H.conv3x3_wino(P.pitched(d["x"], Cin + ex, pad), Cin + ex, uf, P.on_device(d["b"]), y, Cout + ey, nimg, Hh, Ww, Cin, Cout,
                       res=P.pitched(d["res"], Cout + ey, pad), ldres=Cout + ey, stats_part=part)
        assert H.last_row_tile() == 128
        return H.lib().vd_wino_last_kernel(), {"y": (y, Cout), "stats_part": (part, used)}

    def verify(o):
        close(from_nhwc(o["y"][0], Cout), d["y64"], d["y32"], slack=8.0, floor=4e-6, name="wino fwd")
        if Cout % 32 == 0:
            stats = dest((nimg, 32, 2))
            H.gn_stats_from_partials([(o["stats_part"][0], Cout, HW // 64)], nimg, HW, stats)
            g = d["y64"].reshape(nimg, 32, -1)
            close(stats[..., 0], g.mean(-1), None, floor=4e-6, name="wino stats mean")
            close(stats[..., 1], 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-6), None, floor=1e-5, name="wino stats rstd")
    twice(H, (), run, verify)
    if Cout % 16 == 0:          # input gradient: the same kernel on ud with the channel roles swapped

        def run_d(pad, poison):
            dx = dest((nimg, Hh, Ww, Cin + ex), Cin, poison)
            H.conv3x3_wino(P.pitched(d["dy"], Cout + ey, pad), Cout + ey, ud, None, dx, Cin + ex, nimg, Hh, Ww, Cout, Cin)
            return H.lib().vd_wino_last_kernel(), {"dx": (dx, Cin)}
        twice(H, (), run_d, lambda o: close(from_nhwc(o["dx"][0], Cin), d["dx64"], d["dx32"], slack=8.0, floor=4e-6, name="wino dgrad"))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", [(3, 16, 16, 32, 96, 32, 96, 32, 64), (5, 8, 8, 48, 36, 48, 36, 0, 4)])
def test_conv3x3_wgrad_wino(H, case, accumulate):
    nimg, Hh, Ww, Cin, Cout, _, _, ex, ey = case
    assert H.lib().vd_conv3x3_wgrad_wino_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout + ey) == 1

    def entry(xd, ldx, dyd, lddy, dw, db, acc):
        H.conv3x3_wgrad_wino(xd, ldx, dyd, lddy, nimg, Hh, Ww, Cin, Cout, dw, case[5], case[6], accumulate=acc, dbias=db)
    k = _wgrad_twice(H, case, accumulate, ("wgrad",), entry, _bound_wino, H.lib().vd_wino_wgrad_last_kernel)
    assert k % 2 == 1 and k // 2000 == min(Ww // 2, 16), k          # wino_wgrad_kernel<min(W/2, 16), dbias>


# ------------------------------------------------------------------------------------------------ Winograd F(4x4,3x3), fused kernels
# rows of WINO43_CASES: ld > C on both sides (three images x three channel blocks; three image quads); one quad of 16x16 images in one
# item; a 64-wide image of one 16-row part
W43_CASES = [(3, 32, 32, 96, 24, 8, 32), (12, 16, 16, 96, 40, 8, 32), (4, 16, 16, 32, 8, 0, 0), (1, 16, 64, 32, 16, 0, 0)]


@pytest.mark.parametrize("case", W43_CASES)
def test_conv3x3_wino43_fwd(H, case):
    nimg, Hh, Ww, Cout, Cin, ex, ey = case                     # (as in the parity test: the table's Cin % 32 column is this kernel's Cout)
    HW = Hh * Ww
    assert H.lib().vd_conv3x3_wino43_fwd_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout + ey, Cout + ey) == 1
    d = _conv_data(nimg, Hh, Ww, Cin, Cout)
    u43f = dest((H.lib().vd_wino43_u_floats(Cout, Cin),))
    H.wino43_pack_fwd(P.on_device(d["w"]), Cout, Cin, u43f)
    chunks = HW // H.wino43_fwd_chunk_rows(Hh, Ww)
    used = nimg * chunks * 2 * Cout

    def run(pad, poison):
        y = dest((nimg, Hh, Ww, Cout + ey), Cout, poison)
        part = dest((H.stats_part_numel(nimg, HW, Cout),), used, poison)
        H.conv3x3_wino43_fwd(P.pitched(d["x"], Cin + ex, pad), Cin + ex, u43f, P.on_device(d["b"]), y, Cout + ey, nimg, Hh, Ww, Cin, Cout,
                             res=P.pitched(d["res"], Cout + ey, pad), ldres=Cout + ey, stats_part=part)
        return H.lib().vd_wino43_last_kernel(), {"y": (y, Cout), "stats_part": (part, used)}

    def verify(o):
        y = o["y"][0]
        close(from_nhwc(y, Cout), d["y64"], d["y32"], slack=8.0, floor=4e-6, name="wino43 forward")
        stats = dest((nimg, 32, 2))
        H.gn_stats_from_partials([(o["stats_part"][0], Cout, chunks)], nimg, HW, stats)
        g = from_nhwc(y, Cout).double().reshape(nimg, 32, -1)               # statistics of what was WRITTEN
        close(stats[..., 0], g.mean(-1), None, floor=2e-6, name="mean")
        close(stats[..., 1], 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-6), None, floor=5e-6, name="rstd")
    assert twice(H, (), run, verify) == -(Ww // 4)


@pytest.mark.parametrize("case", W43_CASES)
def test_conv3x3_dgrad_wino43(H, case):
    nimg, Hh, Ww, Cin, Cout, ey, ex = case
    assert H.lib().vd_conv3x3_dgrad_wino43_supported(nimg, Hh, Ww, Cin, Cout, Cout + ey, Cin + ex) == 1
    d = _conv_data(nimg, Hh, Ww, Cin, Cout)
    u43 = dest((H.lib().vd_wino43_u_floats(Cout, Cin),))
    H.wino43_pack(P.on_device(d["w"]), Cout, Cin, u43)

    def run(pad, poison):
        dx = dest((nimg, Hh, Ww, Cin + ex), Cin, poison)
        H.conv3x3_dgrad_wino43(P.pitched(d["dy"], Cout + ey, pad), Cout + ey, u43, dx, Cin + ex, nimg, Hh, Ww, Cin, Cout)
        return H.lib().vd_wino43_last_kernel(), {"dx": (dx, Cin)}

    def verify(o):
        rel, err = rel_max(from_nhwc(o["dx"][0], Cin), d["dx64"])
        assert rel <= 1.5e-5 and err <= 6e-5 * d["dx64"].abs().max().item(), f"wino43 dgrad rel-L2 {rel:.3e}, max err {err:.3e}"
    assert twice(H, (), run, verify) == Ww // 4


# ------------------------------------------------------------------------------------------------ F(4x4,3x3) weight gradient (unfused)
# the pitched row of WGRAD43_CASES, and T % 16 != 0: V / dM are stored in blocks of 16 tiles ([T/16][36][16][C]) and the transform pass
# writes T rows, so the last block keeps 12 / 8 / 4 rows of whatever the scratch held.  T = nimg (H/4) (W/4):
#   (129, 8, 8) T = 516 = 32 * 16 + 4      (130, 8, 8) T = 520, T16 = 528 = 16.5 x 32: a K tile of 32 ends on half a tile
#   (131, 8, 8) T = 524 (12 rows)          (60, 12, 12) T = 540 (12 rows), nine tiles per image: no power of two
WGRAD43_POISON_CASES = [(9, 64, 32, 48, 36, 48, 36, 16, 12), (129, 8, 8, 32, 32, 32, 32, 0, 0), (130, 8, 8, 64, 96, 64, 96, 0, 0),
                        (131, 8, 8, 32, 64, 32, 64, 0, 0), (60, 12, 12, 48, 36, 48, 36, 0, 0)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", WGRAD43_POISON_CASES)
def test_conv3x3_wgrad_wino43(H, case, accumulate):
    nimg, Hh, Ww, Cin, Cout, Cin_w, Cout_w, ex, ey = case
    T = nimg * (Hh // 4) * (Ww // 4)
    assert H.lib().vd_conv3x3_wgrad_wino43_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout + ey) == 1
    assert (T % 16 != 0) == (case != WGRAD43_POISON_CASES[0])

    def entry(xd, ldx, dyd, lddy, dw, db, acc):
        H.conv3x3_wgrad_wino43(xd, ldx, dyd, lddy, nimg, Hh, Ww, Cin, Cout, dw, Cin_w, Cout_w, accumulate=acc, dbias=db)
    form = lambda: (H.lib().vd_wino43_wgrad_last_kernel(), H.lib().vd_gemm_last_tile())
    slabs, code = _wgrad_twice(H, case, accumulate, ("wgrad43",), entry, _bound_wino43, form)
    assert slabs >= 1 and H.tile_fields(code)[2] in (16, 32), (slabs, code)


# ------------------------------------------------------------------------------------------------ planes: forward, (V, dM) weight gradient, input gradient
def _plan(H, T, N, K):
    """form (split-operand, K tile, BM, BN) the planner gives the 36 plane GEMMs of this shape on THIS machine"""
    code = H.lib().vd_gemm_plan_tile(T, N, K, H.ROW, H.ROW, 36, 0, 0)
    assert code > 0, H.lib().vd_last_error()
    return H.tile_fields(code)[1:]


# (nimg, H, W, Cin, Cout, ldx - Cin, ldy - Cout): a pitched y; T = 80 tiles: a ragged last row tile, eight column tiles of 64
@pytest.mark.parametrize("case", [(8, 16, 16, 64, 32, 0, 32), (5, 16, 16, 32, 512, 0, 0)])
def test_forward_planes(H, case):
    """vd_conv3x3_wino43_fwd_planes with bias, residual and statistics, V in the "planes_v" scratch.  Bound: 1.5 x the fused F(4x4,3x3)
    forward kernel's error on the same inputs (test_conv_planes_gpu.py::test_forward_planes_vs_fp64) where that kernel serves the geometry;
    five 16x16 images are not served by it (it takes them in fours): there the bound of test_forward_planes_forms_vs_fp64, 8 x torch's own
    fp32 error with a floor of 4e-6"""
    nimg, Hh, Ww, Cin, Cout, ex, ey = case
    HW, lib = Hh * Ww, H.lib()
    ldres = Cout + 8
    assert lib.vd_conv3x3_wino43_fwd_planes_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout + ey, ldres) == 1
    d = _conv_data(nimg, Hh, Ww, Cin, Cout)
    wd, bd = P.on_device(d["w"]), P.on_device(d["b"])
    chunks = HW // H.wino43_fwd_chunk_rows(Hh, Ww)
    used = nimg * chunks * 2 * Cout

    def run(pad, poison):
        y = dest((nimg, Hh, Ww, Cout + ey), Cout, poison)
        part = dest((H.stats_part_numel(nimg, HW, Cout),), used, poison)
        H.conv3x3_wino43_fwd_planes(P.pitched(d["x"], Cin + ex, pad), Cin + ex, wd, bd, y, Cout + ey, nimg, Hh, Ww, Cin, Cout,
                                    res=P.pitched(d["res"], ldres, pad), ldres=ldres, stats_part=part)
        return H.tile_fields(lib.vd_gemm_last_tile())[1:], {"y": (y, Cout), "stats_part": (part, used)}

    def verify(o):
        y = o["y"][0]
        rel_p, max_p = rel_max(from_nhwc(y, Cout), d["y64"])
        if lib.vd_conv3x3_wino43_fwd_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex, Cout, ldres) == 1:
            u43f = torch.empty(lib.vd_wino43_u_floats(Cout, Cin), device=DEV)
            H.wino43_pack_fwd(wd, Cout, Cin, u43f)
            yf = torch.empty(nimg, Hh, Ww, Cout, device=DEV)
            H.conv3x3_wino43_fwd(P.pitched(d["x"], Cin + ex, CLEAN_PAD), Cin + ex, u43f, bd, yf, Cout, nimg, Hh, Ww, Cin, Cout,
                                 res=P.pitched(d["res"], ldres, CLEAN_PAD), ldres=ldres)
            rel_f, max_f = rel_max(from_nhwc(yf, Cout), d["y64"])
            print(f"planes vs fused {case}: rel-L2 {rel_p:.3e} / {rel_f:.3e}, max-abs {max_p:.3e} / {max_f:.3e}")
            assert math.isfinite(rel_p) and rel_p <= 1.5 * rel_f and max_p <= 1.5 * max_f, (rel_p, rel_f, max_p, max_f)
        else:
            assert nimg % 4 != 0
            close(from_nhwc(y, Cout), d["y64"], d["y32"], slack=8.0, floor=4e-6, name="planes forward")
        stats = dest((nimg, 32, 2))
        H.gn_stats_from_partials([(o["stats_part"][0], Cout, chunks)], nimg, HW, stats)
        g = from_nhwc(y, Cout).double().reshape(nimg, 32, -1)               # statistics of what was WRITTEN
        mean, rstd = g.mean(-1), 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-6)
        for got, want, floor, name in ((stats[..., 0], mean, 2e-6, "mean"), (stats[..., 1], rstd, 5e-6, "rstd")):
            err = (got.double().cpu() - want).abs().max().item()
            assert err <= floor * want.abs().max().item(), f"{name}: {err:.3e}"
    ran = twice(H, ("planes", "planes_v"), run, verify)
    assert ran == _plan(H, nimg * (Hh // 4) * (Ww // 4), Cout, Cin), ran


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("both", [False, True], ids=["v", "vm"])
def test_weight_gradient_from_given_images(H, both, accumulate):
    """vd_conv3x3_wgrad_wino43_v (V given) and _vm (V and dM given) at (32, 16, 16, 64 -> 64): V and dM are INPUTS, written once by the
    forward through planes / vd_conv3x3_wino43_dy_image and left alone; the "wgrad43" scratch and the destinations are poisoned"""
    nimg, Hh, Ww, Cin, Cout = 32, 16, 16, 64, 64
    lib = H.lib()
    assert H.wgrad43_supported(nimg, Hh, Ww, Cin, Cout, Cin, Cout)
    d = _wgrad_data(nimg, Hh, Ww, Cin, Cout, Cin, Cout)
    xd, dyd = P.pitched(d["x"], Cin, CLEAN_PAD), P.pitched(d["dy"], Cout, CLEAN_PAD)
    v = dest((lib.vd_conv3x3_wino43_v_floats(nimg, Hh, Ww, Cin),))
    H.conv3x3_wino43_fwd_planes(xd, Cin, P.on_device(rnd(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)), None,
                                torch.empty(nimg, Hh, Ww, Cout, device=DEV), Cout, nimg, Hh, Ww, Cin, Cout, v=v)
    dm = dest((lib.vd_conv3x3_wino43_dm_floats(nimg, Hh, Ww, Cout),))
    H.conv3x3_wino43_dy_image(dyd, Cout, nimg, Hh, Ww, Cout, dm)

    def run(pad, poison):
        dw = dest((Cout, Cin, 3, 3), None, poison, init=torch.ones(Cout, Cin, 3, 3) if accumulate else None)
        db = dest((Cout,), None, poison, init=torch.ones(Cout) if accumulate else None)
        if both:
            H.conv3x3_wgrad_wino43_vm(v, dm, nimg, Hh, Ww, Cin, Cout, dw, Cin, Cout, accumulate=accumulate, dbias=db)
        else:
            H.conv3x3_wgrad(None, Cin, P.pitched(d["dy"], Cout + 8, pad), Cout + 8, nimg, Hh, Ww, Cin, Cout, dw, Cin, Cout,
                            accumulate=accumulate, dbias=db, v=v)
        return (lib.vd_wino43_wgrad_last_kernel(), lib.vd_gemm_last_tile()), {"dw": (dw, None), "dbias": (db, None)}
    twice(H, ("wgrad43",), run, lambda o: _bound_wino43(o, d, 1.0 if accumulate else 0.0))


# ((nimg, H, W, Cin, Cout, lddy - Cout, lddx - Cin)): rows of test_dgrad_planes_gpu.py::CASES -- pitched on both sides with a half-filled
# channel slice; T = 80: a ragged row tile, eight channel slices of 64
@pytest.mark.parametrize("case", [(3, 32, 32, 24, 40, 8, 32), (5, 16, 16, 512, 32, 0, 0)])
def test_dy_image_and_dgrad_planes(H, case):
    """vd_conv3x3_wino43_dy_image -> vd_conv3x3_wino43_dgrad_planes; bounds of test_dgrad_planes_vs_fp64 (relative L2 <= 1.5e-5, max error
    <= 6e-5 of the largest element; the fused input-gradient kernel serves neither geometry, so its 1.5 x ratio has no yardstick here)"""
    nimg, Hh, Ww, Cin, Cout, ey, ex = case
    lib = H.lib()
    assert lib.vd_conv3x3_wino43_dgrad_planes_supported(nimg, Hh, Ww, Cin, Cout, Cin + ex) == 1
    assert lib.vd_conv3x3_dgrad_wino43_supported(nimg, Hh, Ww, Cin, Cout, Cout + ey, Cin) == 0
    d = _conv_data(nimg, Hh, Ww, Cin, Cout)
    wd = P.on_device(d["w"]).contiguous()
    nm = lib.vd_conv3x3_wino43_dm_floats(nimg, Hh, Ww, Cout)

    def run(pad, poison):
        dm = dest((nm,), None, poison)
        H.conv3x3_wino43_dy_image(P.pitched(d["dy"], Cout + ey, pad), Cout + ey, nimg, Hh, Ww, Cout, dm)
        dx = dest((nimg, Hh, Ww, Cin + ex), Cin, poison)
        H.conv3x3_wino43_dgrad_planes(dm, wd, dx, Cin + ex, nimg, Hh, Ww, Cin, Cout)
        return H.tile_fields(lib.vd_gemm_last_tile())[1:], {"dM": (dm, None), "dx": (dx, Cin)}

    def verify(o):
        rel, mx = rel_max(from_nhwc(o["dx"][0], Cin), d["dx64"])
        print(f"dgrad planes {case}: rel-L2 {rel:.3e}, max {mx:.3e} of {d['dx64'].abs().max().item():.3f}")
        assert rel <= 1.5e-5 and mx <= 6e-5 * d["dx64"].abs().max().item(), (rel, mx)
    T = nimg * (Hh // 4) * (Ww // 4)
    assert T % 16 == 0                                         # (every row of dM is written: the whole buffer is compared)
    ran = twice(H, ("dgrad_planes",), run, verify)
    assert ran == _plan(H, T, Cin, Cout) == (False, 32, 64, 64), ran


# ------------------------------------------------------------------------------------------------ GroupNorm
# nimg, C, H, W, film -> form of the backward (vd_gn_bwd_last_kernel): plain single-pass; two-pass (24-channel slabs: 96-byte rows);
# SPLIT with 4 sibling workgroups per (image, slab)
# act and resample (0 none, 1 down, 2 up: apply and backward index a second resolution) as in GN_CASES
GN_POISON_CASES = [((2, 64, 8, 8, False, True, 0), "plain"), ((3, 96, 8, 8, True, True, 0), "plain"),
                   ((2, 192, 64, 64, False, True, 0), "two-pass"), ((2, 256, 64, 64, False, True, 0), "split4"),
                   ((2, 128, 4, 4, False, False, 0), "any"), ((2, 64, 8, 8, False, True, 1), "any"), ((2, 64, 8, 8, False, True, 2), "any")]


@functools.lru_cache(maxsize=None)
def _gn_data(nimg, Cc, Hh, Ww, use_film, act, rs):
    x = rnd(nimg, Cc, Hh, Ww, seed=1) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * rnd(Cc, seed=2), 0.1 * rnd(Cc, seed=3)
    film = 0.3 * rnd(nimg, 2 * Cc, seed=4) if use_film else None
    Ho, Wo = (Hh // 2, Ww // 2) if rs == 1 else ((Hh * 2, Ww * 2) if rs == 2 else (Hh, Ww))
    dy, add = rnd(nimg, Cc, Ho, Wo, seed=5), rnd(nimg, Cc, Hh, Ww, seed=6)

    def ref(dt):
        xs, g, b_ = x.to(dt).requires_grad_(True), gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
        fl = None if film is None else film.to(dt).requires_grad_(True)
        out = ref_gn_block(xs, g, b_, fl, act, rs)
        out.backward(dy.to(dt))
        return out.detach(), xs.grad + add.to(dt), g.grad, b_.grad, (None if fl is None else fl.grad)
    return dict(x=x, gamma=gamma, beta=beta, film=film, dy=dy, add=add, r64=ref(torch.float64), r32=ref(torch.float32))


@pytest.mark.parametrize("case,form", GN_POISON_CASES)
def test_gn_stats_apply_backward(H, case, form):
    """vd_gn_stats -> vd_gn_apply -> vd_gn_apply_bwd as test_kernels_gpu.py::test_gn_forward_backward runs them, every tensor at pitch C + 8,
    nothing accumulated: statistics, coefficient table, y, dx, dfilm, dgamma, dbeta all start as NaN in the second run"""
    nimg, Cc, Hh, Ww, use_film, act, rs = case
    d = _gn_data(*case)
    ld = Cc + 8
    Ho, Wo = d["dy"].shape[2:]
    gd, bd = P.on_device(d["gamma"]), P.on_device(d["beta"])
    fd = None if d["film"] is None else P.on_device(d["film"])

    def run(pad, poison):
        xd = P.pitched(d["x"], ld, pad)
        stats = dest((nimg, 32, 2), None, poison)
        H.gn_stats(xd, ld, nimg, Hh * Ww, Cc, stats)
        coef, y = dest((nimg, 4, Cc), None, poison), dest((nimg, Ho, Wo, ld), Cc, poison)
        H.gn_apply(xd, ld, stats, gd, bd, fd, act, 0.0, 0, rs, y, ld, nimg, Hh, Ww, Cc, coef)
        dx = dest((nimg, Hh, Ww, ld), Cc, poison)
        dfilm = None if fd is None else dest((nimg, 2 * Cc), None, poison)
        dgam, dbet = dest((Cc,), None, poison), dest((Cc,), None, poison)
        H.gn_apply_bwd(P.pitched(d["dy"], ld, pad), ld, xd, ld, coef, gd, bd, fd, act, 0.0, 0, rs, P.pitched(d["add"], ld, pad), ld, dx, ld,
                       False, dfilm, dgam, dbet, False, nimg, Hh, Ww, Cc)
        out = {"stats": (stats, None), "coef": (coef, None), "y": (y, Cc), "dx": (dx, Cc), "dgamma": (dgam, None), "dbeta": (dbet, None)}
        if dfilm is not None:
            out["dfilm"] = (dfilm, None)
        return H.lib().vd_gn_bwd_last_kernel(), out

    def verify(o):
        (o64, dx64, dg64, db64, df64), (o32, dx32, dg32, db32, df32) = d["r64"], d["r32"]
        close(o["stats"][0][..., 0], d["x"].double().reshape(nimg, 32, -1).mean(-1), None, floor=1e-6, name="gn mean")
        close(from_nhwc(o["y"][0], Cc), o64, o32, name="gn fwd")
        close(from_nhwc(o["dx"][0], Cc), dx64, dx32, slack=6, floor=5e-6, name="gn dx")
        close(o["dgamma"][0], dg64, dg32, slack=6, floor=5e-6, name="dgamma")
        close(o["dbeta"][0], db64, db32, slack=6, floor=5e-6, name="dbeta")
        if use_film:
            close(o["dfilm"][0], df64, df32, slack=6, floor=5e-6, name="dfilm")
    k = twice(H, ("gn",), run, verify)
    if form == "two-pass":
        assert k == -1, k
    elif form == "split4":
        assert k // 100000000 == 4 and k % 10000 == 1024, k
    elif form == "plain":
        assert 0 < k < 100000000, k


def test_gn_apply_from_partials(H):
    """the (3, 8, 8, 64 -> 96) row of test_kernels_gpu.py::test_gn_stats_from_producer_epilogues: vd_conv3x3 leaves GroupNorm partials,
    vd_gn_apply_from_partials finalises and applies them in one launch -- against the statistics of fp64 (floors 2e-6 / 5e-6) and the
    two-launch path on the same buffer (2e-6 of the table, 4e-6 of y), that test's bounds"""
    nimg, Hh, Ww, Cin, C1 = 3, 8, 8, 64, 96
    HW, ldb = Hh * Ww, C1 + 8
    d = _conv_data(nimg, Hh, Ww, Cin, C1)
    wf = dest((C1, 9, Cin))
    H.pack_conv3x3(P.on_device(d["w"]), C1, Cin, wf=wf, Cin_p=Cin)
    gamma, beta, film = P.on_device(rnd(C1, seed=7)), P.on_device(rnd(C1, seed=8)), P.on_device(rnd(nimg, 2 * C1, seed=9) * 0.1)
    npart = H.stats_part_numel(nimg, HW, C1)
    keep = {}

    def run(pad, poison):
        buf = dest((nimg, Hh, Ww, ldb), C1, poison)
        part = P.banded((npart,), NAN if poison else CLEAN_FILL, P.SENTINEL, device=DEV)
        H.conv3x3(P.pitched(d["x"], Cin + 4, pad), Cin + 4, wf, P.on_device(d["b"]), buf, ldb, nimg, Hh, Ww, Cin, C1,
                  res=P.pitched(d["res"], C1 + 4, pad), ldres=C1 + 4, stats_part=part)
        code = H.lib().vd_gemm_last_tile()
        chunks = HW // (H.last_row_tile() // 2)
        used = nimg * chunks * 2 * C1
        torch.cuda.synchronize()
        tail = part[used:]
        assert bool(torch.isnan(tail).all() if poison else (tail == CLEAN_FILL).all()), "statistics written past [nimg][chunks][2][C]"
        assert bool((buf[..., C1:] == P.SENTINEL).all()), "pitch columns of the convolution's output were written"
        y_conv = buf[..., :C1].clone()
        buf[..., C1:] = pad                                    # the destination's pitch columns become a SOURCE's
        y, coef = dest((nimg, Hh, Ww, ldb), C1, poison), dest((nimg, 4, C1), None, poison)
        H.gn_apply_from_partials(buf, ldb, [(part, C1, chunks)], gamma, beta, film, 1, 0.0, 0, H.RS_NONE, y, ldb, nimg, Hh, Ww, C1, coef)
        keep.update(buf=buf, part=part, chunks=chunks)
        return code, {"conv y": (y_conv, None), "stats_part": (part[:used], None), "y": (y, C1), "coef": (coef, None)}

    def verify(o):
        close(from_nhwc(o["conv y"][0], C1), d["y64"], d["y32"], name="conv fwd")
        buf, parts = keep["buf"], [(keep["part"], C1, keep["chunks"])]
        stats = dest((nimg, 32, 2))
        H.gn_stats_from_partials(parts, nimg, HW, stats)
        g = d["y64"].reshape(nimg, 32, -1)
        close(stats[..., 0], g.mean(-1), None, floor=2e-6, name="mean")
        close(stats[..., 1], 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-6), None, floor=5e-6, name="rstd")
        y_a, coef_a = torch.empty(nimg, Hh, Ww, C1, device=DEV), torch.empty(nimg, 4, C1, device=DEV)
        H.gn_apply(buf, ldb, stats, gamma, beta, film, 1, 0.0, 0, H.RS_NONE, y_a, C1, nimg, Hh, Ww, C1, coef_a)
        assert (o["coef"][0] - coef_a).abs().max().item() <= 2e-6 * coef_a.abs().max().item()
        assert (o["y"][0][..., :C1] - y_a).abs().max().item() <= 4e-6 * max(y_a.abs().max().item(), 1.0)
    twice(H, (), run, verify)


# ------------------------------------------------------------------------------------------------ vd_colsum, vd_sumsq
@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum(H, accumulate):
    x = rnd(1000, 72, seed=1)
    o0 = rnd(72, seed=2)

    def run(pad, poison):
        out = dest((72,), None, poison, init=o0 if accumulate else None)
        H.colsum(P.pitched_rows(x, 80, pad), 80, 1000, 72, out, accumulate=accumulate)
        return 0, {"colsum": (out, None)}
    add64, add32 = (o0.double(), o0) if accumulate else (0.0, 0.0)
    twice(H, ("colsum",), run, lambda o: close(o["colsum"][0], x.double().sum(0) + add64, x.sum(0) + add32, name="colsum"))


# 3: the scalar tail alone; 100003: test_sumsq_adamw_ema's size; 4 * 256 * 1024 * 2 + 5: every thread of sumsq_partial_kernel's 1024 x 256
# grid goes round its grid-stride loop twice, five of them a third time, plus a scalar tail
@pytest.mark.parametrize("n", [3, 100003, 4 * 256 * 1024 * 2 + 5])
def test_sumsq(H, n):
    g = rnd(n, seed=2) * 0.1
    ref = (g.double() ** 2).sum().reshape(1)

    def run(pad, poison):
        gd = P.banded_like(g, pad, DEV)                         # what lies before and behind the n floats is not the kernel's to read
        ss = dest((1,), None, poison)
        H.sumsq(gd, ss)
        return 0, {"sumsq": (ss, None)}
    twice(H, ("sumsq",), run, lambda o: close(o["sumsq"][0], ref, None, floor=1e-6, name="sumsq"))
