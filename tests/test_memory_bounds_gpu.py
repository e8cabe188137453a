"""No kernel reads or writes outside its tensors and its scratch ("Memory a kernel may not read", the write side).

tests/test_poisoned_memory_gpu.py holds the GEMM, convolution and GroupNorm entries to that on banded tensors and exact-size scratch.
This file has the rest:

  * the entries that file does not have -- the optimizer tail over flat buffers, the weight packs (single and batched, the batched ones
    into images carved back to back from one buffer as engine.ConvPacks carves them) and the small kernels of csrc/misc.hip --, each as ONE
    call on banded operands (poison.Banded: sentinel bands around destinations, NaN bands around sources) against the plain fp64
    reference of the operation with the bound of the entry's parity test;
  * bases that are only 16-byte aligned: one case per conv / GEMM / GroupNorm entry of the poisoned file with every operand moved 4
    floats off its 512-byte line (the engine passes channel slices of concat buffers): refused before anything is launched, or inside
    the fp64 bound with every band intact;
  * the scratch contracts at their boundary: with exactly the bytes its size function reports an entry succeeds, inside its bound, with
    the scratch bands intact; with one float fewer it is refused before anything is launched.

Nothing here is meant to fault: the bands are memory the test owns, sized (poison.band_elems) so that an overrun of a row, a tile or an
image stays inside them.  Needs an MI355X."""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison as P                                                # noqa: E402
import test_poisoned_memory_gpu as M                              # noqa: E402
from test_kernels_gpu import close, rnd                           # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INT_BAND = 0x5A                    # bands of integer destinations


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


@pytest.fixture(autouse=True)
def _drop_bands():
    yield
    P.forget_bands()


def src(x):
    """a source on the device between NaN bands (integer types: bands of the type's largest value)"""
    return P.on_device(x)


def dst(shape, fill=NAN, init=None, dtype=torch.float32):
    """a destination between sentinel bands: `fill` everywhere (NaN: a non-accumulating call reads nothing of it), or `init`"""
    if not dtype.is_floating_point:
        fill = 0 if fill != fill else fill
    t = P.banded(shape, fill, P.SENTINEL if dtype.is_floating_point else INT_BAND, dtype=dtype, device=DEV)
    if init is not None:
        t.copy_(init)
    return t


def same(got, ref, what):
    """exact equality (copies and single roundings), with a count in the message; NaN left in a destination counts as a difference"""
    got = got.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = int((got != ref).sum())
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ from the reference"


def bands_ok(what):
    M._sync()
    damage = P.bands_damage()
    assert not damage, f"{what}: written outside a destination: {damage}"


# ------------------------------------------------------------------------------------------------ optimizer tail
LR, B1, B2, EPS, WD, DECAY, MAX_NORM = 2e-4, 0.9, 0.999, 1e-8, 0.01, 0.99, 1.0
WRAP = 256 * 8192                  # adamw_ema_kernel's largest grid x block: element WRAP is the first one a thread reaches on its second round


@functools.lru_cache(maxsize=None)
def _adam_data(n):
    p, g, m, ema = rnd(n, seed=1), rnd(n, seed=2) * 0.1, rnd(n, seed=3) * 0.05, rnd(n, seed=5)
    v = (rnd(n, seed=4) * 0.05) ** 2
    gsq = float((g.double() ** 2).sum())
    return p, g, m, v, ema, torch.tensor([gsq], dtype=torch.float32)


def _adam_ref(p, g, m, v, ema, gsq32, lo, hi, mode, r_bc1, r_bc2, step):
    """csrc/optim.hip::adamw_ema_kernel restated in fp64 (torch clip_grad_norm_ + AdamW + EMA); mode 0 / 1 / 2 as vd_adamw_ema"""
    p, g, m, v, ema = (t.double().clone() for t in (p, g, m, v, ema))
    clip = min(MAX_NORM / (math.sqrt(float(gsq32)) + 1e-6), 1.0)
    bc1, bc2 = torch.full_like(p, 1 - B1 ** step), torch.full_like(p, 1 - B2 ** step)
    upd = torch.ones_like(p, dtype=torch.bool)
    if mode == 1:
        upd[lo:hi] = False
    elif mode == 2:
        bc1[lo:hi], bc2[lo:hi] = r_bc1, r_bc2
    gi = g * clip
    mn, vn = B1 * m + (1 - B1) * gi, B2 * v + (1 - B2) * gi * gi
    pn = p * (1 - LR * WD) - (LR / bc1) * mn / (vn.sqrt() / bc2.sqrt() + EPS)
    p, m, v = torch.where(upd, pn, p), torch.where(upd, mn, m), torch.where(upd, vn, v)
    return p, m, v, ema + (1 - DECAY) * (p - ema)


def _range(n):
    """[r_lo, r_hi): odd ends, inside the tensor; at the large size it straddles the grid-stride wrap"""
    return {5: (1, 3), 100003: (777, 50001)}.get(n, (WRAP - 5, WRAP + 2))


@pytest.mark.parametrize("mode", ["all", "skip", "lag", "flag_set", "flag_unset"])
@pytest.mark.parametrize("n", [5, 100003, WRAP + 3])
def test_adamw_ema_stays_inside_its_flat_buffers(H, n, mode):
    """vd_adamw_ema (r_mode 0, 1, 2) and vd_adamw_ema_flagged (flag set / unset) with p, g, m, v, ema, the norm, the flag and the step counter
    all banded; bound of test_kernels_gpu.py::test_sumsq_adamw_ema (2e-6 of the largest element against fp64).  Where the range receives
    no gradient, p, m and v keep their bits inside it."""
    p, g, m, v, ema, gsq = _adam_data(n)
    lo, hi = _range(n)
    step, r_steps0 = 3, 1
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    r_bc1, r_bc2 = 1 - B1 ** (r_steps0 + 1), 1 - B2 ** (r_steps0 + 1)
    pd, md, vd, ed = (dst((n,), init=t) for t in (p, m, v, ema))
    gd, sq = src(g), src(gsq)
    rmode = {"all": 0, "skip": 1, "lag": 2, "flag_set": 2, "flag_unset": 1}[mode]
    if mode.startswith("flag"):
        flag = src(torch.tensor([1.0 if mode == "flag_set" else 0.0]))
        steps = dst((1,), init=torch.tensor([r_steps0], dtype=torch.int32), dtype=torch.int32)
        H.adamw_ema_flagged(pd, gd, md, vd, ed, sq, MAX_NORM, LR, B1, B2, EPS, WD, bc1, bc2, DECAY, lo, hi, flag, steps)
    else:
        H.adamw_ema(pd, gd, md, vd, ed, sq, MAX_NORM, LR, B1, B2, EPS, WD, bc1, bc2, DECAY, r_lo=lo, r_hi=hi, r_mode=rmode,
                    r_bc1=r_bc1 if rmode == 2 else 1.0, r_bc2=r_bc2 if rmode == 2 else 1.0)
    bands_ok(f"adamw_ema {mode} n={n}")
    rp, rm, rv, re = _adam_ref(p, g, m, v, ema, gsq[0], lo, hi, rmode, r_bc1, r_bc2, step)
    for name, got, ref in (("p", pd, rp), ("m", md, rm), ("v", vd, rv), ("ema", ed, re)):
        close(got, ref, None, floor=2e-6, name=f"adamw {name}")
    if rmode == 1:
        for name, got, was in (("p", pd, p), ("m", md, m), ("v", vd, v)):
            assert P.same_bits(got[lo:hi].cpu(), was[lo:hi]), f"{name}[{lo}:{hi}) changed although the range received no gradient"
    if mode.startswith("flag"):
        assert int(steps[0]) == r_steps0 + (mode == "flag_set"), int(steps[0])


def test_ema_track_batched_stays_inside_its_items(H):
    """vd_ema_track_batched over three items of unequal size carved back to back from one banded buffer (the second and third start off
    a 16-byte boundary: the dword path); e + (1 - decay)(p - e) is three roundings from fp64: 5e-7 of the largest element"""
    counts = [1000, 3, 70001]
    e0 = [rnd(c, seed=10 + i) for i, c in enumerate(counts)]
    p0 = [rnd(c, seed=20 + i) for i, c in enumerate(counts)]
    ebuf, pbuf = dst((sum(counts),), init=torch.cat(e0)), src(torch.cat(p0))
    rows, off, blk = [], 0, 0
    for c in counts:
        rows.append([ebuf[off:].data_ptr(), pbuf[off:].data_ptr(), c, 0, 0, 0, 0, blk])
        off, blk = off + c, blk + (c + 255) // 256
    H.ema_track_batched(torch.tensor(rows, dtype=torch.int64).to(DEV), len(counts), blk, 0.9)
    bands_ok("ema_track_batched")
    ref = torch.cat([e.double() + (1 - 0.9) * (p.double() - e.double()) for e, p in zip(e0, p0)])
    close(ebuf, ref, None, floor=5e-7, name="ema track")


# ------------------------------------------------------------------------------------------------ weight packs
PACK_SHAPES = [(32, 8), (96, 40), (36, 48), (64, 64)]            # (Cout, Cin); (36, 48): no 16x16 tiles, the untiled F(2x2,3x3) path
G23 = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
G43_DGRAD = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                          [0, 0, 1]], dtype=torch.float64)
G43_FWD = torch.tensor([[64 / 81, 0, 0], [-128 / 243, -32 / 81, -8 / 27], [-128 / 243, 32 / 81, -8 / 27], [32 / 243, 16 / 81, 8 / 27],
                        [32 / 243, -16 / 81, 8 / 27], [0, 0, 1]], dtype=torch.float64)


def _w(co, ci):
    return rnd(co, ci, 3, 3, seed=2, scale=(9 * ci) ** -0.5)


def _ref_wino(w):
    """(uf [16][Cout][Cin], ud [16][Cin][Cout]) = G k G^T of the kernel / of the rotated kernel with the channel roles swapped, fp64"""
    k = w.double()
    uf = torch.einsum("ai,ocij,bj->aboc", G23, k, G23).reshape(16, *k.shape[:2])
    ud = torch.einsum("ai,ocij,bj->abco", G23, k.flip(-1, -2), G23).reshape(16, k.shape[1], k.shape[0])
    return uf, ud


def _ref_wino43(w, fwd):
    """csrc/wino43.hip::pack43_tile restated: (G k G^T)[36] of GEMM column n and K index k (forward: n = co, k = ci; input gradient: rotated
    kernel, n = ci, k = co) in the order [n / 32][k / 8][xi][(k % 8) / 2][n % 16][(n % 32) / 16][k % 2], fp64"""
    G = G43_FWD if fwd else G43_DGRAD
    k = w.double() if fwd else w.double().flip(-1, -2)
    u = torch.einsum("ai,ocij,bj->ocab", G, k, G).reshape(*k.shape[:2], 36)
    u = u if fwd else u.permute(1, 0, 2)                          # [n][k][xi]
    n, kk = u.shape[:2]
    return u.reshape(n // 32, 2, 16, kk // 8, 4, 2, 36).permute(0, 3, 6, 4, 2, 1, 5).reshape(-1)


def _ref_direct(w, cin_p, cout_p):
    """wf[co][tap][ci_p] = w[co][ci][tap], wd[ci][tap][co_p] = w[co][ci][8 - tap], padding channels zero: copies, exact"""
    co, ci = w.shape[:2]
    wf, wd = torch.zeros(co, 9, cin_p), torch.zeros(ci, 9, cout_p)
    wf[:, :, :ci] = w.reshape(co, ci, 9).permute(0, 2, 1)
    wd[:, :, :co] = w.reshape(co, ci, 9).flip(-1).permute(1, 2, 0)
    return wf, wd


def _carve(buf, sizes):
    """views of `sizes` elements each, back to back from the flat buffer (engine.ConvPacks.carve)"""
    out, off = [], 0
    for n in sizes:
        out.append(buf[off:off + n])
        off += n
    assert off == buf.numel()
    return out


def _table(rows):
    return torch.tensor(rows, dtype=torch.int64).to(DEV)


def test_wino_pack_single_and_batched(H):
    """vd_wino_pack (uf and ud) against G k G^T in fp64 (fp32 transform, halves and three-term sums: 1e-6 of the largest element), and
    vd_wino_pack_batched into two buffers carved back to back: every image bit for bit the single-tensor pack"""
    ws = [src(_w(co, ci)) for co, ci in PACK_SHAPES]
    single = []
    for (co, ci), w in zip(PACK_SHAPES, ws):
        uf, ud = dst((16, co, ci)), dst((16, ci, co))
        H.wino_pack(w, co, ci, uf=uf, ud=ud)
        bands_ok(f"wino_pack {co}x{ci}")
        rf, rd = _ref_wino(_w(co, ci))
        close(uf, rf, None, floor=1e-6, name="uf")
        close(ud, rd, None, floor=1e-6, name="ud")
        only_d = dst((16, ci, co))
        H.wino_pack(w, co, ci, ud=only_d)                       # one image alone
        bands_ok(f"wino_pack ud {co}x{ci}")
        assert P.same_bits(only_d, ud)
        single.append((uf, ud))
    sizes = [16 * co * ci for co, ci in PACK_SHAPES]
    fbuf, dbuf = dst((sum(sizes),)), dst((sum(sizes),))
    rows, blk = [], 0
    for (co, ci), w, f, d in zip(PACK_SHAPES, ws, _carve(fbuf, sizes), _carve(dbuf, sizes)):
        tiled = int(co % 16 == 0 and ci % 16 == 0)
        rows.append([w.data_ptr(), f.data_ptr(), d.data_ptr(), co, ci, tiled, 0, blk])
        blk += (co // 16) * (ci // 16) if tiled else (co * ci + 255) // 256
    assert {r[5] for r in rows} == {0, 1}                           # both block forms
    H.wino_pack_batched(_table(rows), len(rows), blk)
    bands_ok("wino_pack_batched")
    for (co, ci), (uf, ud), f, d in zip(PACK_SHAPES, single, _carve(fbuf, sizes), _carve(dbuf, sizes)):
        assert P.same_bits(f, uf.reshape(-1)) and P.same_bits(d, ud.reshape(-1)), f"batched F(2x2,3x3) image {co}x{ci} differs"


def test_wino43_pack_single_and_batched(H):
    """vd_wino43_pack_fwd / vd_wino43_pack against the fp64 transform in the documented lane order (the kernel evaluates in fp64 and rounds
    once: 2e-7 of the largest element), images of vd_wino43_u_floats floats; vd_wino43_pack_batched into one buffer that holds a forward
    and an input-gradient image per layer back to back, bit for bit the single-tensor packs"""
    lib = H.lib()
    items = []                                                     # (Cout, Cin, forward image?)
    for co, ci in PACK_SHAPES:
        if co % 32 == 0 and ci % 8 == 0:
            items.append((co, ci, 1))
        if ci % 32 == 0 and co % 8 == 0:
            items.append((co, ci, 0))
        elif co % 32 == 0 and ci % 8 == 0:
            items.append((ci, co, 0))                             # (the input gradient of the layer with the channel roles swapped)
    assert sorted(items) == sorted([(32, 8, 1), (8, 32, 0), (96, 40, 1), (40, 96, 0), (64, 64, 1), (64, 64, 0)])
    ws, single = {}, []
    for co, ci, fwd in items:
        w = ws.setdefault((co, ci), src(_w(co, ci)))
        n = lib.vd_wino43_u_floats(co, ci)
        assert n == 36 * co * ci
        u = dst((n,))
        (H.wino43_pack_fwd if fwd else H.wino43_pack)(w, co, ci, u)
        bands_ok(f"wino43_pack{'_fwd' if fwd else ''} {co}x{ci}")
        close(u, _ref_wino43(_w(co, ci), fwd), None, floor=2e-7, name=f"u43{'f' if fwd else ''} {co}x{ci}")
        single.append(u)
    sizes = [lib.vd_wino43_u_floats(co, ci) for co, ci, _ in items]
    buf = dst((sum(sizes),))
    rows, blk = [], 0
    for (co, ci, fwd), img in zip(items, _carve(buf, sizes)):
        rows.append([ws[(co, ci)].data_ptr(), img.data_ptr(), fwd, co, ci, 0, 0, blk])
        blk += (co // 32) * (ci // 8) if fwd else (ci // 32) * (co // 8)
    H.wino43_pack_batched(_table(rows), len(rows), blk)
    bands_ok("wino43_pack_batched")
    for (co, ci, fwd), u, img in zip(items, single, _carve(buf, sizes)):
        assert P.same_bits(img, u), f"batched F(4x4,3x3) image {co}x{ci} fwd={fwd} differs"


def test_pack_conv3x3_single_and_batched(H):
    """vd_pack_conv3x3 (wf and wd, Cin_p / Cout_p four channels above the real counts, zero-filled) is a copy: exact; the batched form into
    two buffers carved back to back, bit for bit"""
    ws = [src(_w(co, ci)) for co, ci in PACK_SHAPES]
    single = []
    for (co, ci), w in zip(PACK_SHAPES, ws):
        wf, wd = dst((co, 9, ci + 4)), dst((ci, 9, co + 4))
        H.pack_conv3x3(w, co, ci, wf=wf, Cin_p=ci + 4, wd=wd, Cout_p=co + 4)
        bands_ok(f"pack_conv3x3 {co}x{ci}")
        rf, rd = _ref_direct(_w(co, ci), ci + 4, co + 4)
        same(wf, rf, f"wf {co}x{ci}")
        same(wd, rd, f"wd {co}x{ci}")
        single.append((wf, wd))
    fs, ds = [co * 9 * (ci + 4) for co, ci in PACK_SHAPES], [ci * 9 * (co + 4) for co, ci in PACK_SHAPES]
    fbuf, dbuf = dst((sum(fs),)), dst((sum(ds),))
    rows, blk = [], 0
    for (co, ci), w, f, d, nf, nd in zip(PACK_SHAPES, ws, _carve(fbuf, fs), _carve(dbuf, ds), fs, ds):
        rows.append([w.data_ptr(), f.data_ptr(), d.data_ptr(), co, ci, ci + 4, co + 4, blk])
        blk += (max(nf, nd) + 255) // 256
    H.pack_conv3x3_batched(_table(rows), len(rows), blk)
    bands_ok("pack_conv3x3_batched")
    for (co, ci), (wf, wd), f, d in zip(PACK_SHAPES, single, _carve(fbuf, fs), _carve(dbuf, ds)):
        assert P.same_bits(f, wf.reshape(-1)) and P.same_bits(d, wd.reshape(-1)), f"batched direct packs {co}x{ci} differ"


# ------------------------------------------------------------------------------------------------ small kernels of csrc/misc.hip
@pytest.mark.parametrize("beta", [2.0, 0.0])
def test_axpby_pitched(H, beta):
    """y = alpha x + beta y over [rows][C] at pitches ldx = C + 8, ldy = C + 4; beta = 0 reads nothing of y (NaN there)"""
    rows, C = 1003, 72
    x, y = rnd(rows, C, seed=1), rnd(rows, C, seed=2)
    yd = dst((rows, C + 4), fill=P.SENTINEL)
    yd[:, :C] = y.to(DEV) if beta else NAN
    H.axpby(P.pitched_rows(x, C + 8, NAN), C + 8, 0.5, yd, C + 4, beta, rows, C)
    bands_ok("axpby")
    close(yd[:, :C], 0.5 * x.double() + beta * y.double(), None, name="axpby")
    assert bool((yd[:, C:] == P.SENTINEL).all()), "pitch columns of y were written"


def test_silu_forward_backward(H):
    n = 5003
    v, g = rnd(n, seed=3) * 3, rnd(n, seed=4)
    vd, od = src(v), dst((n,))
    H.silu(vd, od)
    bands_ok("silu")
    close(od, F.silu(v.double()), F.silu(v), name="silu")
    vs = v.double().requires_grad_(True)
    F.silu(vs).backward(g.double())
    for accumulate in (False, True):
        gd = dst((n,), fill=1.0 if accumulate else NAN)
        H.silu_bwd(vd, src(g), gd, accumulate=accumulate)
        bands_ok("silu_bwd")
        close(gd, vs.grad + (1 if accumulate else 0), None, floor=3e-6, name="silu bwd")


def test_layout_changes(H):
    """vd_nchw_to_nhwc with ldy > C (the pitch columns are part of its contract: zero-filled) and vd_nhwc_to_nchw from a pitched source"""
    nimg, C, Hh, Ww, ld = 5, 3, 7, 9, 8
    x = rnd(nimg, C, Hh, Ww, seed=1)
    y = dst((nimg, Hh, Ww, ld))
    H.nchw_to_nhwc(src(x), y, nimg, C, Hh, Ww, ld)
    bands_ok("nchw_to_nhwc")
    same(y[..., :C], x.permute(0, 2, 3, 1), "nchw_to_nhwc")
    assert bool((y[..., C:] == 0).all()), "nchw_to_nhwc: pitch columns not zero-filled"
    z = dst((nimg, C, Hh, Ww))
    H.nhwc_to_nchw(P.pitched(x, ld, NAN), ld, z, nimg, C, Hh, Ww)
    bands_ok("nhwc_to_nchw")
    same(z, x, "nhwc_to_nchw")


def test_uint8_image_kernels(H):
    """vd_images_to_uint8_hwc and vd_images_from_uint8_hwc with flip, the LAST image among the mirrored ones (a mirrored column index one
    too high reads the band behind the tensor)"""
    n, C, Hh, Ww = 5, 3, 7, 13
    x = rnd(n, C, Hh, Ww, seed=1).clamp(-1.3, 1.3)
    out = dst((n, Hh, Ww, C), fill=7, dtype=torch.uint8)
    H.images_to_uint8_hwc(src(x), out, n, C, Hh * Ww)
    bands_ok("images_to_uint8_hwc")
    same(out, (x * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1), "images_to_uint8_hwc")
    u8 = torch.randint(0, 255, (n, Hh, Ww, C), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)       # (255 is the band)
    flip = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8)
    t = u8.permute(0, 3, 1, 2).float() / 255.0
    t = torch.where(flip.bool()[:, None, None, None], t.flip(-1), t)
    for fl, ref in ((src(flip), (t - 0.5) / 0.5), (None, (u8.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5)):
        got = dst((n, C, Hh, Ww))
        H.images_from_uint8_hwc(src(u8), fl, got, n, C, Hh, Ww)
        bands_ok("images_from_uint8_hwc")
        same(got, ref, f"images_from_uint8_hwc, flip {'given' if fl is not None else 'absent'}")


def test_im2col3x3(H):
    """xc[p][tap C + c] = x[p + off(tap)][c], zero outside the image: a copy, exact.  The halo rows above the first image and below the
    last lie in the source's NaN bands"""
    nimg, Hh, Ww, C, ld = 3, 5, 7, 4, 12
    x = rnd(nimg, C, Hh, Ww, seed=1)
    xc = dst((nimg * Hh * Ww, 9 * C))
    H.im2col3x3(P.pitched(x, ld, NAN), ld, xc, nimg, Hh, Ww, C)
    bands_ok("im2col3x3")
    ref = F.unfold(x, 3, padding=1).reshape(nimg, C, 9, Hh * Ww).permute(0, 3, 2, 1).reshape(nimg * Hh * Ww, 9 * C)
    same(xc, ref, "im2col3x3")


def _taps(t, sign):
    """[n][H][W][...] -> the nine copies shifted by sign * off(tap), zero outside the image, stacked on a new last axis"""
    n, Hh, Ww = t.shape[:3]
    pad = F.pad(t, [0, 0] * (t.ndim - 3) + [1, 1, 1, 1])
    return torch.stack([pad[:, 1 + sign * (tap // 3 - 1):1 + sign * (tap // 3 - 1) + Hh, 1 + sign * (tap % 3 - 1):1 + sign * (tap % 3 - 1) + Ww]
                        for tap in range(9)], -1)


def test_tap_gather_and_spread(H):
    """the thin-output convolution's two tap kernels at ldz = 32 > 9 Cout = 27: vd_tap_gather writes the columns [0, Cout) of its
    destination and nothing else, vd_tap_spread every column of its rows (27 values, five zeros)"""
    nimg, Hh, Ww, Cout, ldz, ldo = 3, 7, 5, 3, 32, 4
    Px = nimg * Hh * Ww
    z, bias, dy = rnd(Px, 9 * Cout, seed=1), rnd(Cout, seed=2), rnd(nimg, Cout, Hh, Ww, seed=3)
    out = dst((nimg, Hh, Ww, ldo), fill=P.SENTINEL)
    out[..., :Cout] = NAN
    H.tap_gather(P.pitched_rows(z, ldz, NAN), ldz, src(bias), out, ldo, nimg, Hh, Ww, Cout)
    bands_ok("tap_gather")

    def gather(dt):        # out[p][co] = bias[co] + sum_tap z[p + off(tap)][co 9 + tap]
        zt = _taps(z.to(dt).reshape(nimg, Hh, Ww, Cout, 9), +1)                   # [..., co, tap of the column, tap of the shift]
        return bias.to(dt) + torch.diagonal(zt, dim1=-2, dim2=-1).sum(-1)
    close(out[..., :Cout], gather(torch.float64), gather(torch.float32), name="tap gather")
    assert bool((out[..., Cout:] == P.SENTINEL).all()), "pitch column of the gathered output was written"
    dz = dst((Px, ldz))
    H.tap_spread(P.pitched(dy, ldo, NAN), ldo, dz, ldz, nimg, Hh, Ww, Cout)
    bands_ok("tap_spread")
    ref = torch.zeros(Px, ldz)
    ref[:, :9 * Cout] = _taps(dy.permute(0, 2, 3, 1), -1).reshape(Px, 9 * Cout)          # dz[q][co 9 + tap] = dy[q - off(tap)][co]
    same(dz, ref, "tap_spread")


@pytest.mark.parametrize("accumulate", [False, True])
def test_thin_wgrad_finish(H, accumulate):
    """g[co][tap Cin + ci] -> dw[co][ci][tap] for ci < Cin_w < Cin, dbias from every ninth column sum: copies / one fp32 addition, exact"""
    Cout_w, Cin, Cin_w = 33, 8, 5
    g, cs = rnd(Cout_w, 9 * Cin, seed=1), rnd(Cout_w * 9, seed=2)
    dw, db = (dst(s, fill=1.0 if accumulate else NAN) for s in ((Cout_w, Cin_w, 3, 3), (Cout_w,)))
    H.thin_wgrad_finish(src(g), Cout_w, Cin, Cin_w, dw, accumulate=accumulate, colsum=src(cs), cs_stride=9, cs_off=4, dbias=db)
    bands_ok("thin_wgrad_finish")
    add = 1.0 if accumulate else 0.0
    rw = g.reshape(Cout_w, 9, Cin)[:, :, :Cin_w].permute(0, 2, 1).reshape(Cout_w, Cin_w, 3, 3)
    same(dw, rw + add, "thin_wgrad_finish dw")
    same(db, cs[4::9] + add, "thin_wgrad_finish dbias")


def test_timestep_embedding_odd_dim(H):
    from oracle.unet_ref import timestep_embedding
    t = torch.tensor([0.0, 1e-3, 0.25, 0.5, 0.999, 1.0, 0.123456789], dtype=torch.float64)
    for dim in (33, 193):
        out = dst((len(t), dim))
        H.timestep_embedding(src(t), out, len(t), dim)
        bands_ok("timestep_embedding")
        assert (out.cpu() - timestep_embedding(t, dim)).abs().max().item() <= 2e-7


def test_class_embed_and_multitag_norm(H):
    n, emb, ncls = 9, 66, 10
    y = torch.tensor([0., 1., 10., 3., 3., 0., 7., 10., 5.])
    w, b, te, g = rnd(emb, ncls, seed=1), rnd(emb, seed=2), rnd(n, emb, seed=3), rnd(n, emb, seed=4)
    oh = F.one_hot((y.long() - 1).clamp(min=0), ncls).double() * (y != 0).double()[:, None]
    ws, bs = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = te.double() + F.linear(oh, ws, bs)
    ref.backward(g.double())
    yd, ted = src(y), dst((n, emb), init=te)
    H.class_embed(yd, src(w), src(b), ted, n, emb, ncls)
    bands_ok("class_embed")
    close(ted, ref.detach(), None, name="class embed")
    dw, db = dst((emb, ncls)), dst((emb,))
    H.class_embed_bwd(yd, src(g), dw, db, n, emb, ncls, accumulate=False)
    bands_ok("class_embed_bwd")
    close(dw, ws.grad, None, name="class dw")
    close(db, bs.grad, None, name="class db")
    tags = (rnd(7, 41, seed=5) > 0.8).float()
    tags[0] = 0
    out = dst((7, 41))
    H.multitag_norm(src(tags), out, 7, 41)
    bands_ok("multitag_norm")
    rt = tags / torch.count_nonzero(tags, dim=1).clamp(min=1.0).sqrt().unsqueeze(1)
    close(out, rt.double(), rt, name="multitag")


# L = 1000: the generic kernel; 256: the register-resident one.  37 rows: the last workgroup holds one row of four
@pytest.mark.parametrize("L", [1000, 256])
def test_softmax_rows_forward_backward(H, L):
    rows = 37
    s, dp = rnd(rows, L, seed=1) * 4, rnd(rows, L, seed=2)
    sd = dst((rows, L), init=s)
    H.softmax_rows(sd, rows, L)
    bands_ok("softmax_rows")
    close(sd, torch.softmax(s.double(), -1), torch.softmax(s, -1), name="softmax")
    ss = s.double().requires_grad_(True)
    torch.softmax(0.25 * ss, -1).backward(dp.double())
    dpd = dst((rows, L), init=dp)
    H.softmax_rows_bwd(src(torch.softmax(0.25 * s.double(), -1).float()), dpd, rows, L, 0.25)
    bands_ok("softmax_rows_bwd")
    close(dpd, ss.grad, None, floor=3e-6, name="softmax bwd")


# ------------------------------------------------------------------------------------------------ the poisoned file's cases, run another way
class _Watch:
    """v_diffusion._hip._check, watched: after every call that succeeded, how many banded tensors had been made (`mark`: the destinations
    of a call that is refused later were made after it); of a refused call, its name and vd_last_error()"""

    def __init__(self, H):
        self.H, self.real, self.mark, self.refused = H, H._check, P.Banded.made, None

    def __call__(self, rc, what):
        if rc == 0:
            self.mark = P.Banded.made
        else:
            self.refused = (what, self.H.lib().vd_last_error().decode(errors="replace"))
        return self.real(rc, what)

    def untouched(self):
        """every destination made since the last successful call holds what dest() put there: NaN (CLEAN_FILL) and sentinels"""
        assert self.refused is not None and self.refused[1], f"refused without a message: {self.refused}"
        M._sync()
        for b in P._ledger:
            if b.check and b.serial > self.mark:
                ok = torch.isnan(b.whole) | (b.whole == P.SENTINEL) | (b.whole == M.CLEAN_FILL)
                assert bool(ok.all()), f"{self.refused[0]} was refused ({self.refused[1]}) after writing {int((~ok).sum())} elements of {tuple(b.real.shape)}"


def _real(t, cols):
    return t if cols is None else t[..., :cols]


def _same_outputs(a, b, what):
    assert a.keys() == b.keys()
    for name, (ta, cols) in a.items():
        assert P.same_bits(_real(ta, cols), _real(b[name][0], cols)), f"{name}: {what}"


def _checked(run, pad, poison, exact, H, what):
    """one run on the scratch `exact`; destination and scratch bands intact afterwards"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(H, "workspace", exact)
        form, out = run(pad, poison)
        M._sync()
    damage = P.bands_damage()
    assert not damage, f"written outside a destination ({what}): {damage}"
    assert exact.intact(), f"written outside the scratch ({what}) {exact.requests}: {exact.damage()}"
    for name, (t, cols) in out.items():
        bad = int((~torch.isfinite(_real(t, cols))).sum())
        assert bad == 0, f"{name}: {bad} elements not finite ({what})"
        if cols is not None:
            assert bool((t[..., cols:] == P.SENTINEL).all()), f"{name}: pitch columns of the destination were written ({what})"
    return form, out


# one case per entry of test_poisoned_memory_gpu.py (its own test function and arguments; every one overwrites its destinations)
G0, W0, W43, WG43 = (3, 96, 8, 8, True, True, 0), (3, 16, 16, 32, 96, 32, 64), M.W43_CASES[1], M.WGRAD43_POISON_CASES
ENTRY_CASES = {
    "gemm_row_row": (M.test_gemm_kinds, (0, 0, 200, 72, 100, 0)), "gemm_row_col": (M.test_gemm_kinds, (0, 1, 200, 72, 100, 0)),
    "gemm_col_col": (M.test_gemm_kinds, (1, 1, 200, 72, 100, 0)), "gemm_col_row": (M.test_gemm_kinds, (1, 0, 200, 72, 100, 0)),
    "gemm_splitk_ragged": (M.test_gemm_splitk_with_colsum, (12, 260, 1000, 3, 0, False)),
    "gemm_splitk_unused_slabs": (M.test_gemm_splitk_with_colsum, (64, 96, 288, 8, 0, False)),
    "gemm_grouped_wgrad": (M.test_gemm_grouped_wgrad, (3, 64, 96, 1000, 4, 8)),
    "direct_forward": (M.test_conv3x3_direct_forward, (M.DIRECT_CASES[1],)), "direct_dgrad": (M.test_conv3x3_direct_dgrad, (M.DIRECT_CASES[1],)),
    "direct_wgrad": (M.test_conv3x3_direct_wgrad, (M.DIRECT_CASES[1], False)),
    "wino_forward_dgrad": (M.test_conv3x3_wino_forward_stats_dgrad, (W0,)),
    "wino_wgrad": (M.test_conv3x3_wgrad_wino, ((5, 8, 8, 48, 36, 48, 36, 0, 4), False)),
    "wino43_forward": (M.test_conv3x3_wino43_fwd, (W43,)), "wino43_dgrad": (M.test_conv3x3_dgrad_wino43, (W43,)),
    "wino43_wgrad": (M.test_conv3x3_wgrad_wino43, (WG43[1], False)), "wino43_wgrad_pitched": (M.test_conv3x3_wgrad_wino43, (WG43[0], False)),
    "planes_forward": (M.test_forward_planes, ((8, 16, 16, 64, 32, 0, 32),)),
    "wgrad_from_v": (M.test_weight_gradient_from_given_images, (False, False)),
    "wgrad_from_v_dm": (M.test_weight_gradient_from_given_images, (True, False)),
    "dy_image_dgrad_planes": (M.test_dy_image_and_dgrad_planes, ((3, 32, 32, 24, 40, 8, 32),)),
    "gn_plain": (M.test_gn_stats_apply_backward, (G0, "plain")),
    "gn_two_pass": (M.test_gn_stats_apply_backward, ((2, 192, 64, 64, False, True, 0), "two-pass")),
    "gn_split4": (M.test_gn_stats_apply_backward, ((2, 256, 64, 64, False, True, 0), "split4")),
    "gn_down": (M.test_gn_stats_apply_backward, ((2, 64, 8, 8, False, True, 1), "any")),
    "gn_apply_from_partials": (M.test_gn_apply_from_partials, ()),
    "colsum": (M.test_colsum, (False,)), "sumsq": (M.test_sumsq, (100003,)),
}


def test_gn_finalisers_and_kept_parameter_terms(H):
    """The GroupNorm entries the chain of the poisoned file does not call: vd_gn_stats_from_partials and vd_gn_coef_from_partials on the
    partial sums a convolution left (bounds of test_kernels_gpu.py::test_gn_stats_from_producer_epilogues: statistics 2e-6 / 5e-6 against
    fp64, the table 2e-6 of the one vd_gn_apply writes), vd_gn_apply_bwd_keep and vd_gn_param_sums_batched over two items whose dgamma /
    dbeta are carved back to back from one buffer, one overwriting, one accumulating (bounds of test_gn_forward_backward)"""
    nimg, Hh, Ww, Cin, C1 = 3, 8, 8, 64, 96
    HW = Hh * Ww
    d = M._conv_data(nimg, Hh, Ww, Cin, C1)
    wf = dst((C1, 9, Cin))
    H.pack_conv3x3(src(d["w"]), C1, Cin, wf=wf, Cin_p=Cin)
    buf, part = dst((nimg, Hh, Ww, C1)), dst((H.stats_part_numel(nimg, HW, C1),))
    H.conv3x3(P.pitched(d["x"], Cin, NAN), Cin, wf, src(d["b"]), buf, C1, nimg, Hh, Ww, Cin, C1, res=P.pitched(d["res"], C1, NAN), ldres=C1,
              stats_part=part)
    parts = [(part, C1, HW // (H.last_row_tile() // 2))]
    gamma, beta, film = src(rnd(C1, seed=7)), src(rnd(C1, seed=8)), src(rnd(nimg, 2 * C1, seed=9) * 0.1)
    stats, coef = dst((nimg, 32, 2)), dst((nimg, 4, C1))
    H.gn_stats_from_partials(parts, nimg, HW, stats)
    H.gn_coef_from_partials(parts, nimg, HW, gamma, beta, film, coef)
    y_a, coef_a = dst((nimg, Hh, Ww, C1)), dst((nimg, 4, C1))
    H.gn_apply(buf, C1, stats, gamma, beta, film, 1, 0.0, 0, H.RS_NONE, y_a, C1, nimg, Hh, Ww, C1, coef_a)
    bands_ok("statistics and coefficient table from partials")
    g = d["y64"].reshape(nimg, 32, -1)
    close(stats[..., 0], g.mean(-1), None, floor=2e-6, name="mean")
    close(stats[..., 1], 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-6), None, floor=5e-6, name="rstd")
    assert (coef - coef_a).abs().max().item() <= 2e-6 * coef_a.abs().max().item(), "coefficient table from partials"

    case = (3, 96, 8, 8, True, True, 0)
    nimg, Cc, Hh, Ww = case[:4]
    n, ld = M._gn_data(*case), Cc + 8
    (_, dx64, dg64, db64, df64), (_, dx32, dg32, db32, df32) = n["r64"], n["r32"]
    gd, bd, fd = src(n["gamma"]), src(n["beta"]), src(n["film"])
    xd, st = P.pitched(n["x"], ld, NAN), dst((nimg, 32, 2))
    H.gn_stats(xd, ld, nimg, Hh * Ww, Cc, st)
    cf, y = dst((nimg, 4, Cc)), M.dest((nimg, Hh, Ww, ld), Cc, True)
    H.gn_apply(xd, ld, st, gd, bd, fd, True, 0.0, 0, 0, y, ld, nimg, Hh, Ww, Cc, cf)
    dx, dfilm, pgb = M.dest((nimg, Hh, Ww, ld), Cc, True), dst((nimg, 2 * Cc)), dst((nimg, 2, Cc))
    H.gn_apply_bwd(P.pitched(n["dy"], ld, NAN), ld, xd, ld, cf, gd, bd, fd, True, 0.0, 0, 0, P.pitched(n["add"], ld, NAN), ld, dx, ld, False, dfilm,
                   None, None, False, nimg, Hh, Ww, Cc, pgb_keep=pgb)
    out = dst((4 * Cc,))
    out[2 * Cc:] = 1.0
    dg0, db0, dg1, db1 = _carve(out, [Cc] * 4)
    blocks = (Cc + 15) // 16
    rows = [[pgb.data_ptr(), dg0.data_ptr(), db0.data_ptr(), nimg, Cc, 0, 0, 0], [pgb.data_ptr(), dg1.data_ptr(), db1.data_ptr(), nimg, Cc, 1, 0, blocks]]
    H.gn_param_sums_batched(_table(rows), 2, 2 * blocks)
    bands_ok("GroupNorm backward with kept parameter terms")
    assert bool((dx[..., Cc:] == P.SENTINEL).all()) and bool((y[..., Cc:] == P.SENTINEL).all()), "pitch columns written"
    close(M.from_nhwc(dx, Cc), dx64, dx32, slack=6, floor=5e-6, name="gn dx")
    close(dfilm, df64, df32, slack=6, floor=5e-6, name="dfilm")
    for got, r64, r32, add in ((dg0, dg64, dg32, 0.0), (db0, db64, db32, 0.0), (dg1, dg64, dg32, 1.0), (db1, db64, db32, 1.0)):
        close(got, r64 + add, r32 + add, slack=6, floor=5e-6, name="summed parameter terms")


# the wrappers reach the *_phase entries (the same kernels as separate calls) when a profile is being recorded
@pytest.mark.parametrize("name", ["direct_wgrad", "wino_wgrad", "wino43_wgrad", "wgrad_from_v", "wgrad_from_v_dm", "planes_forward",
                                  "dy_image_dgrad_planes"])
def test_phase_entries_banded_and_on_exact_scratch(H, name, monkeypatch):
    """vd_conv3x3_wgrad_phase, vd_conv3x3_wgrad_wino_phase, vd_conv3x3_wgrad_wino43_phase and the phases 1 / 2 / 4 of the planes entries: the
    case of the poisoned file as it stands (banded, bit for bit on NaN, exact scratch), with the launches split as bench.py splits them"""
    fn, args = ENTRY_CASES[name]
    profile = []
    monkeypatch.setattr(H, "PROFILE", profile)
    fn(H, *args)
    assert len(profile) >= 4, [r[0] for r in profile]             # two passes of at least two separately timed launches


# ------------------------------------------------------------------------------------------------ bases that are only 16-byte aligned
@pytest.mark.parametrize("name", sorted(ENTRY_CASES))
def test_operands_four_floats_off_their_line(H, name, monkeypatch):
    """The case runs as test_poisoned_memory_gpu.py runs it, but its second pass has every banded operand -- pitched sources, residuals,
    destinations, statistics, biases, weights and their packed images -- 4 floats behind a 512-byte line (16-byte alignment: what a channel
    slice of a concat buffer has), NaN in everything that is not read, on exact-size scratch.  The entry either refuses (non-zero return,
    vd_last_error() set, nothing written) or meets the fp64 bound of its parity test with all bands intact; its bits equal the aligned
    run's when the reported form is the same."""
    fn, args = ENTRY_CASES[name]
    watch = _Watch(H)
    seen = {"runs": 0, "refused": 0}

    def twice(H_, tags, run, verify):
        with P.shifted(0):
            form_a, aligned = _checked(run, M.CLEAN_PAD, False, P.ExactWorkspace(), H, "aligned run")
            verify(aligned)
        bands_ok("aligned run, verified")
        seen["runs"] += 1
        exact = P.ExactWorkspace()
        try:
            form_s, shifted = _checked(run, NAN, True, exact, H, "operands 16 bytes off their line")
        except H.HipError:
            watch.untouched()
            seen["refused"] += 1
            print(f"{name}: refused with operands 16 bytes off their line: {watch.refused}")
            return form_a
        verify(shifted)
        bands_ok("operands 16 bytes off their line, verified")
        assert set(tags) <= exact.tags(), (tags, exact.requests)
        if form_s == form_a:
            _same_outputs(aligned, shifted, "differs from the aligned run although the same kernel form ran")
        else:
            print(f"{name}: form {form_a} aligned, {form_s} with operands 16 bytes off their line")
        return form_a
    monkeypatch.setattr(M, "twice", twice)
    monkeypatch.setattr(H, "_check", watch)
    with P.shifted(4):
        try:
            fn(H, *args)
        except H.HipError:                                       # (a pack or a preparing call refused the shifted weights)
            watch.untouched()
            seen["refused"] += 1
            print(f"{name}: refused before its runs: {watch.refused}")
    assert seen["runs"] or seen["refused"], "the case ran nothing"


# ------------------------------------------------------------------------------------------------ scratch contracts at their boundary
def _gemm_splitk_need(M_, N_, K_, S_):
    """vd_gemm has no size function: the bound of its own entry check, slabs that hold work x (M N + M with colsum) floats"""
    return lambda H, form: M._slabs(H, form, K_, S_)[2] * (M_ * N_ + M_) * 4


def _size(fn, *a):
    return lambda H, form: int(getattr(H.lib(), fn)(*a))


# name of ENTRY_CASES -> (scratch tag, bytes the entry needs, which request of the tag inside one run is cut short, wrapper asks exactly that?)
BOUNDARY = {
    "gemm_splitk_ragged": ("splitk", _gemm_splitk_need(12, 260, 1000, 3), 0, False),
    "gemm_splitk_unused_slabs": ("splitk", _gemm_splitk_need(64, 96, 288, 8), 0, False),
    "gemm_grouped_wgrad": ("splitk", _size("vd_gemm_grouped_wgrad_ws_bytes", 3, 64, 96, 4), 0, True),
    "direct_wgrad": ("wgrad", _size("vd_conv3x3_wgrad_ws_bytes", 5, 8, 8, 36, 68), 0, True),
    "wino_wgrad": ("wgrad", _size("vd_conv3x3_wgrad_wino_ws_bytes", 5, 8, 8, 48, 36), 0, True),
    "wino43_wgrad": ("wgrad43", _size("vd_conv3x3_wgrad_wino43_ws_bytes", *WG43[1][:5]), 0, True),
    "wino43_wgrad_pitched": ("wgrad43", _size("vd_conv3x3_wgrad_wino43_ws_bytes", *WG43[0][:5]), 0, True),
    "wgrad_from_v": ("wgrad43", _size("vd_conv3x3_wgrad_wino43_ws_bytes", 32, 16, 16, 64, 64), 0, True),
    "wgrad_from_v_dm": ("wgrad43", _size("vd_conv3x3_wgrad_wino43_ws_bytes", 32, 16, 16, 64, 64), 0, True),
    "planes_forward": ("planes", _size("vd_conv3x3_wino43_fwd_planes_ws_bytes", 8, 16, 16, 64, 32), 0, True),
    "dy_image_dgrad_planes": ("dgrad_planes", _size("vd_conv3x3_wino43_dgrad_planes_ws_bytes", 3, 32, 32, 24, 40), 0, True),
    "gn_plain": ("gn", _size("vd_gn_ws_bytes", 3, 64, 96), 0, True),                      # vd_gn_stats
    "gn_plain_bwd": ("gn", _size("vd_gn_ws_bytes", 3, 64, 96), 1, True),                  # vd_gn_apply_bwd, single-pass form
    "gn_two_pass_bwd": ("gn", _size("vd_gn_ws_bytes", 2, 4096, 192), 1, True),
    "gn_split4_bwd": ("gn", _size("vd_gn_ws_bytes", 2, 4096, 256), 1, True),
    "colsum": ("colsum", _size("vd_colsum_ws_bytes", 1000, 72), 0, True),
    "sumsq": ("sumsq", _size("vd_sumsq_ws_bytes", 100003), 0, True),
}


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_scratch_of_exactly_the_reported_size_and_one_float_less(H, name, monkeypatch):
    """With scratch of EXACTLY the bytes the entry's size function reports (vd_gemm split-K: the bound of its own entry check) the call
    succeeds inside its fp64 bound, bit for bit what it gives on the roomy scratch, and leaves the scratch bands intact; with 4 bytes
    fewer it is refused before anything is launched: HipError, vd_last_error() set, every destination still NaN."""
    tag, need_of, index, asks_exactly = BOUNDARY[name]
    fn, args = ENTRY_CASES[name[:-4] if name.endswith("_bwd") else name]
    watch = _Watch(H)
    seen = {"runs": 0}

    def twice(H_, tags, run, verify):
        assert tag in tags, (tag, tags)
        form, roomy = run(M.CLEAN_PAD, False)                    # on v_diffusion._hip.workspace: which form runs, and its bits
        M._sync()
        P.forget_bands()
        need = need_of(H, form)
        assert need > 0 and need % 4 == 0, need
        exact = P.ExactWorkspace(force={tag: need}, only={tag: index})
        form_e, out = _checked(run, NAN, True, exact, H, f"{need} bytes of scratch")
        assert form_e == form, (form_e, form)
        verify(out)
        asked = [nb for t, nb in exact.requests if t == tag]
        assert len(asked) > index and asked[index] >= need, f"the wrapper asked for {asked} bytes, the entry needs {need}"
        assert not asks_exactly or asked[index] == need, f"the wrapper asked for {asked} bytes, the size function reports {need}"
        _same_outputs(roomy, out, "differs between roomy and exact scratch")
        short = P.ExactWorkspace(force={tag: need - 4}, only={tag: index})
        watch.refused = None
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(H, "workspace", short)
            with pytest.raises(H.HipError):
                run(NAN, True)
        watch.untouched()
        assert short.intact(), short.damage()
        damage = P.bands_damage()
        assert not damage, damage
        seen["runs"] += 1
        return form
    monkeypatch.setattr(M, "twice", twice)
    monkeypatch.setattr(H, "_check", watch)
    fn(H, *args)
    assert seen["runs"] >= 1
