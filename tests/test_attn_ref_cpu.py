"""tests/attn_ref.py proved on the CPU: every input family has the property it is named for, the tiled emulation is the softmax it claims
to be, and the two fp32 yardsticks agree with each other -- so that a failure of tests/test_attn_stress_gpu.py is a finding about a
kernel and not about its inputs.  A failure here means the family is wrong: fix it in attn_ref.py."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as A                                              # noqa: E402

CASES = [pytest.param(f, g, id=f"{f}-{A.gid(g)}") for f in A.FAMILIES for g in A.GEOMS]


def _probs64(c):
    B, nh, L, hd = c.geom
    s = A.logits(c.qkv, B, nh, L, hd, torch.float64)
    return s, torch.softmax(s, -1)


@pytest.mark.parametrize("family,geom", CASES)
def test_family_has_its_stated_property(family, geom):
    B, nh, L, hd = geom
    c = A.case(family, geom)
    T = A.tile_rows(hd)
    nt = L // T
    assert L % T == 0 and nt == (4 if geom in A.GEOMS4 else 1)
    s, p = _probs64(c)
    for t in (c.qkv, c.do, c.o32, c.g32, c.on32, c.lse32, c.on_lse32, c.delta32):
        assert torch.isfinite(t).all(), "the fp32 references of a family must be finite"
    if family in A.STEP_FAMILIES:
        tmax = s.reshape(B, nh, L, nt, T).amax(-1)                 # per-tile maximum of every logit row
        d = tmax[..., 1:] - tmax[..., :-1]
        assert ((d > 0) if family == "ascending" else (d < 0)).all(), "the tile maxima must move strictly in one direction"
        if nt > 1:
            top = nt - 1 if family == "ascending" else 0
            outside = 1.0 - p.reshape(B, nh, L, nt, T)[..., top, :].sum(-1)
            assert outside.min().item() >= 0.04, outside.min().item()
            assert outside.max().item() <= 0.07, outside.max().item()      # ... and the top tile still dominates
    if family == "peaked":
        assert p.amax(-1).mean().item() >= 0.9, p.amax(-1).mean().item()
    if family == "shifted":
        assert s.min().item() >= 480.0, s.min().item()
    if family == "uniform":
        x5 = c.qkv.view(B, L, 3, nh, hd)
        assert (x5[:, :, 0] == 0).all() and (s == 0).all()
        assert (p == 1.0 / L).all()                                # L is a power of two: exactly flat
        q, k, v = A.heads(c.qkv, B, nh, L, hd, torch.float64)
        assert torch.allclose(c.o64, v.mean(-2, keepdim=True).expand(B, nh, L, hd).permute(0, 2, 1, 3).reshape(B, L, nh * hd), rtol=0, atol=1e-14)
        assert torch.allclose(c.lse64, torch.full_like(c.lse64, math.log2(L)), rtol=0, atol=1e-13)


@pytest.mark.parametrize("family,geom", CASES)
def test_emulation_in_fp64_is_the_softmax(family, geom):
    """online() evaluated in fp64 against the direct fp64 softmax: 1e-12 of the quantity's magnitude"""
    B, nh, L, hd = geom
    c = A.case(family, geom)
    o, lse = A.online(c.qkv, B, nh, L, hd, dtype=torch.float64)
    for name, got, want in (("O", o, c.o64), ("lse", lse, c.lse64)):
        err = (got - want).abs().max().item()
        assert err <= 1e-12 * max(1.0, want.abs().max().item()), (name, err)
    # the tile size is the emulation's only degree of freedom: one tile = no rescale at all, and it must not matter
    o1, lse1 = A.online(c.qkv, B, nh, L, hd, dtype=torch.float64, tile=L)
    assert (o1 - c.o64).abs().max().item() <= 1e-12 * max(1.0, c.o64.abs().max().item())
    assert (lse1 - c.lse64).abs().max().item() <= 1e-12 * max(1.0, c.lse64.abs().max().item())


@pytest.mark.parametrize("family,geom", CASES)
def test_fp32_yardsticks_agree(family, geom):
    """torch's direct fp32 result and the fp32 emulation of the tiled algorithm: each within 4 x the other's error against fp64
    + 3e-6 of scale, per (image, head) block as the GPU tests judge"""
    B, nh, L, hd = geom
    c = A.case(family, geom)
    for b in range(B):
        for h in range(nh):
            want = A.head_block(c.o64, b, h, nh, hd)
            scale = want.abs().max().item()
            e_dir = (A.head_block(c.o32, b, h, nh, hd).double() - want).abs().max().item()
            e_onl = (A.head_block(c.on32, b, h, nh, hd).double() - want).abs().max().item()
            assert math.isfinite(e_dir) and math.isfinite(e_onl)
            assert e_dir <= 4 * e_onl + 3e-6 * scale and e_onl <= 4 * e_dir + 3e-6 * scale, (b, h, e_dir, e_onl, scale)
    e_dir = (c.lse32.double() - c.lse64).abs().max().item()
    e_onl = (c.on_lse32.double() - c.lse64).abs().max().item()
    scale = c.lse64.abs().max().item()
    assert e_dir <= 4 * e_onl + 3e-6 * scale and e_onl <= 4 * e_dir + 3e-6 * scale, (e_dir, e_onl, scale)


def test_delta_ref_is_the_row_sum_per_head():
    B, nh, L, hd = 2, 3, 5, 4
    do, o = A.rnd(B, L, nh * hd, seed=1).double(), A.rnd(B, L, nh * hd, seed=2).double()
    d = A.delta_ref(do, o, B, nh, L, hd)
    assert d.shape == (B, nh, L)
    for b in range(B):
        for h in range(nh):
            for l in range(L):
                want = sum(do[b, l, h * hd + i].item() * o[b, l, h * hd + i].item() for i in range(hd))
                assert abs(d[b, h, l].item() - want) < 1e-14
