"""tests/gemm_batched_ref.py against independent formulations: its packing helpers are what turns the logical tensors of the fp64
references into the packed device buffers of tests/test_gemm_batched_gpu.py, so a mistake there would make that file test nothing."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_batched_ref as G                                      # noqa: E402


@pytest.mark.parametrize("B,nh,L,hd", [(3, 2, 64, 64), (2, 3, 192, 32), (1, 2, 5, 4)])
def test_strided_unpacking_of_a_packed_qkv_buffer_is_reshape_permute(B, nh, L, hd):
    hid = nh * hd
    g = torch.Generator().manual_seed(B + L)
    qkv = torch.randn(B, L, 3 * hid, generator=g, dtype=torch.float64)
    pitch = 3 * hid + G.PAD
    buf = torch.full((B * L + G.GUARD_ROWS, pitch), -1.0, dtype=torch.float64)
    buf[:B * L, :3 * hid] = qkv.reshape(B * L, 3 * hid)
    want = qkv.reshape(B, L, 3, nh, hd).permute(2, 0, 3, 1, 4)                # [3][B][nh][L][hd], as test_kernels_gpu._attn_ref splits it
    for third in range(3):
        got = G.unpack_heads_strided(buf, B, nh, L, hd, third * hid)
        assert got.dtype == torch.float64 and torch.equal(got, want[third])
        assert torch.equal(G.unpack_heads(buf, B, nh, L, hd, third * hid), want[third])


def test_pack_roundtrip_masks_and_guards():
    B, nh, L, hd = 2, 3, 8, 4
    hid, pitch = nh * hd, 3 * nh * hd + G.PAD
    d = G.attn_operands(B, nh, L, hd)
    buf = G.pack_heads(d["q"], pitch, 0, fill=G.SENTINEL)
    G.pack_heads(d["k"], pitch, hid, buf)
    assert torch.equal(G.unpack_heads(buf, B, nh, L, hd, 0), d["q"]) and torch.equal(G.unpack_heads_strided(buf, B, nh, L, hd, hid), d["k"])
    m = G.heads_mask(B, nh, L, hd, pitch, 0) | G.heads_mask(B, nh, L, hd, pitch, hid)
    assert m.sum().item() == 2 * B * L * hid and (buf[~m] == G.SENTINEL).all()
    assert not m[B * L:].any() and not m[:, 3 * hid:].any() and not m[:, 2 * hid:].any()
    last = G.heads_mask(B, nh, L, hd, pitch, hid) & ~G.heads_mask(B, nh, L, hd, pitch, hid, entries=B * nh - 1)
    assert last.sum().item() == L * hd and last[(B - 1) * L:B * L, hid + (nh - 1) * hd: hid + hid].all()
    # row-stacked buffers (maps, FiLM stacks)
    rb = G.pack_rows(d["P"], L + G.PAD, fill=G.SENTINEL)
    assert rb.shape == (B * nh * L + G.GUARD_ROWS, L + G.PAD) and torch.equal(G.unpack_rows(rb, d["P"].shape), d["P"])
    rm = G.rows_mask(B * nh, L, L, L + G.PAD)
    assert (rb[~rm] == G.SENTINEL).all() and rm.sum().item() == d["P"].numel()
    src = G.pack_rows(d["P"], L + G.PAD)                                    # source buffers: finite junk in the padding
    assert torch.isfinite(src).all() and (src[~rm] >= 50.0).all()


def test_entries_are_scaled_by_powers_of_two_and_products_follow():
    B, nh, L, hd = 3, 2, 8, 4
    assert [G.entry_scale(z) for z in range(6)] == [0.25, 0.5, 1.0, 2.0, 4.0, 0.25]
    d = G.attn_operands(B, nh, L, hd)
    prods = G.attn_products(d)
    for f, (eq, a, b, _) in G.ATTN_FORMS.items():
        p64, p32 = prods[f]
        assert p64.dtype == torch.float64 and p32.dtype == torch.float32
        for z in range(B * nh):
            bi, h = divmod(z, nh)
            A, Bm = d[a][bi, h].double(), d[b][bi, h].double()
            want = A @ Bm.T if f in (1, 4) else (A @ Bm if f in (2, 5) else A.T @ Bm)
            assert torch.allclose(p64[bi, h], want, rtol=1e-12, atol=1e-12), f
    # the unscaled draw times the scale is the scaled draw: entry z of q has the magnitude entry_scale(z) against entry 2 (scale 1)
    rms = d["q"].double().pow(2).mean((2, 3)).sqrt().reshape(-1)
    for z in range(B * nh):
        assert math.isclose(rms[z].item() / G.entry_scale(z), rms[2].item(), rel_tol=0.5)


def test_film_products_and_compose():
    nb, B, E, c2 = 3, 5, 8, 6
    d = G.film_operands(nb, B, E, c2)
    p = G.film_products(d)
    for i in range(nb):
        assert torch.allclose(p[7][0][i], d["ta"].double() @ d["W"][i].double().T, rtol=1e-12, atol=1e-12)
        assert torch.allclose(p[8][0][i], d["df"][i].double() @ d["W"][i].double(), rtol=1e-12, atol=1e-12)
    out = G.compose(p[7][0], -0.5, bias=d["bias"].unsqueeze(1), R=d["R"], c0=d["c0_fwd"])
    want = -0.5 * p[7][0] + d["bias"].double().unsqueeze(1) + d["R"].double() + d["c0_fwd"].double()
    assert out.dtype == torch.float64 and torch.equal(out, want)
