"""Inputs and references of the attention stress tests (tests/test_attn_ref_cpu.py proves them, tests/test_attn_stress_gpu.py uses them).
Plain torch on the CPU; nothing here touches the library.

Geometries (B, nh, L, hd): three with four key tiles of T = 4096 / hd rows (csrc/attn.hip streams keys through LDS in such tiles, two
stages, so each stage is filled twice), nh = 3 once so that head offsets and the [B nh][L] lse / delta layout are not trivial; and one with
a single tile, where the running maximum is set once and no rescale happens.

Input families, built on the packed projection qkv[B, L, 3 nh hd] viewed as [B, L, 3, nh, hd] (logits = q . k / sqrt(hd)):
  benign      rnd * 1.5                                   logits of about +-11: the input of the existing tests, the control
  peaked      rnd * 6                                     logits of about +-190: nearly one-hot rows, most exp2 underflow
  shifted     rnd * 1.5, q[0] = sqrt(hd), k[0] += 500     every logit is 500 + noise: the maximum sits 500 (721 in the log2 domain) above 0
  ascending   q, k thirds rnd * 0.45, v third rnd * 1.5, q[0] = sqrt(hd), k_j[0] = 3 (j // T)
                                                          the row maximum rises by 3 from tile to tile: a rescale at every tile
  descending  the same with k_j[0] = 3 (ntiles - 1 - j // T)   the maximum is met in tile 0 and never rises: later tiles are the tail
  uniform     benign with the q third zeroed              logits exactly 0: P = 1 / L, O = mean of V, lse = log2 L
In the step families the tiles below the top one hold e^-3 + e^-6 + e^-9 ~ 5 % of a row's mass: a kernel that lost them, or rescaled them
wrongly, is off by per cents where fp32 noise is a few 1e-6.

References: test_kernels_gpu._attn_ref in fp64 (truth) and in fp32 (the natural-noise yardstick) with their autograd; online(), the tiled
algorithm of the fused forward restated in plain torch (the second yardstick of the forward: a running maximum and sum, rescaled tile
by tile); lse2(), the log-sum-exp in the log2 domain; delta_ref(), rowsum(dO * O) per head.  case() builds all of them once per
(family, geometry); callers must not modify what it returns."""
import functools
import math
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernels_gpu import _attn_ref, rnd                      # noqa: E402

LOG2E = math.log2(math.e)
TILE_FLOATS = 4096                                                # csrc/attn.hip: TILE
STEP = 3.0
SHIFT = 500.0

GEOMS4 = [(2, 3, 256, 64), (1, 2, 128, 128), (2, 1, 64, 256)]     # four key tiles each
ONE_TILE = (1, 1, 64, 64)
GEOMS = GEOMS4 + [ONE_TILE]
FAMILIES = ("benign", "peaked", "shifted", "ascending", "descending", "uniform")
STEP_FAMILIES = ("ascending", "descending")


def gid(geom):
    return "x".join(map(str, geom))


def tile_rows(hd):
    return TILE_FLOATS // hd


def make_qkv(family, B, nh, L, hd):
    """the packed fp32 projection [B, L, 3 nh hd] of a family"""
    hid = nh * hd
    # step families: with only T = 16 keys per tile (hd = 256) a row's mass outside the top tile spreads by +-15 % around 5 %; the seed
    # is one at which no row of any geometry falls below the 4 % that test_attn_ref_cpu.py asserts
    x = rnd(B, L, 3 * hid, seed=L + hd + 11 * FAMILIES.index(family) + (2000 if family in STEP_FAMILIES else 0))
    x5 = x.view(B, L, 3, nh, hd)
    if family in ("benign", "uniform"):
        x *= 1.5
        if family == "uniform":
            x5[:, :, 0] = 0.0
    elif family == "peaked":
        x *= 6.0
    elif family == "shifted":
        x *= 1.5
        x5[:, :, 0, :, 0] = math.sqrt(hd)
        x5[:, :, 1, :, 0] += SHIFT
    elif family in STEP_FAMILIES:
        x5[:, :, :2] *= 0.45
        x5[:, :, 2] *= 1.5
        x5[:, :, 0, :, 0] = math.sqrt(hd)
        tile = torch.arange(L) // tile_rows(hd)
        if family == "descending":
            tile = tile.max() - tile
        x5[:, :, 1, :, 0] = (STEP * tile.float())[None, :, None]
    else:
        raise ValueError(family)
    return x


def heads(qkv, B, nh, L, hd, dtype):
    """q, k, v as [B, nh, L, hd] in ``dtype``"""
    x = qkv.to(dtype).reshape(B, L, 3, nh, hd)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def logits(qkv, B, nh, L, hd, dtype):
    q, k, _ = heads(qkv, B, nh, L, hd, dtype)
    return q @ k.transpose(-1, -2) / math.sqrt(hd)


def lse2(qkv, B, nh, L, hd, dtype):
    """log2-domain log-sum-exp of the scaled logits, [B, nh, L]: what vd_attn_fwd stores"""
    return torch.logsumexp(logits(qkv, B, nh, L, hd, dtype), -1) * LOG2E


def online(qkv, B, nh, L, hd, dtype=torch.float32, tile=None):
    """The fused forward's algorithm in plain torch: keys in tiles of ``tile`` rows, q pre-scaled by scale * log2(e), exp2, a running
    maximum m and sum l rescaled by exp2(m_old - m_new), one division at the end.  -> (O [B, L, nh hd], lse [B, nh, L])"""
    T = tile or tile_rows(hd)
    q, k, v = heads(qkv, B, nh, L, hd, dtype)
    sl2 = torch.tensor(1.0 / math.sqrt(hd), dtype=dtype) * torch.tensor(LOG2E, dtype=dtype)
    qs = q * sl2
    m = torch.full((B, nh, L, 1), -math.inf, dtype=dtype)
    l = torch.zeros(B, nh, L, 1, dtype=dtype)
    acc = torch.zeros(B, nh, L, hd, dtype=dtype)
    for t in range(0, L, T):
        s = qs @ k[:, :, t:t + T].transpose(-1, -2)
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        a = torch.exp2(m - mn)
        p = torch.exp2(s - mn)
        l = l * a + p.sum(-1, keepdim=True)
        acc = acc * a + p @ v[:, :, t:t + T]
        m = mn
    o = (acc / l).permute(0, 2, 1, 3).reshape(B, L, nh * hd)
    return o, (m + torch.log2(l)).squeeze(-1)


def delta_ref(do, o, B, nh, L, hd):
    """rowsum(dO * O) per (image, head): [B, nh, L] in the operands' dtype"""
    return (do * o).reshape(B, L, nh, hd).sum(-1).permute(0, 2, 1)


def head_block(x, b, h, nh, hd):
    """[L, hd] of (image b, head h) in an [B, L, >= nh hd] activation"""
    return x[b, :, h * hd:(h + 1) * hd]


def third_block(x, b, h, i, nh, hd):
    """[L, hd] of (image b, head h), third i (0 q, 1 k, 2 v) in a packed [B, L, >= 3 nh hd] tensor"""
    c = (i * nh + h) * hd
    return x[b, :, c:c + hd]


@functools.lru_cache(maxsize=None)
def case(family, geom):
    """operands and every reference of (family, geometry): built once, shared, read-only"""
    B, nh, L, hd = geom
    qkv = make_qkv(family, B, nh, L, hd)
    do = rnd(B, L, nh * hd, seed=3)
    g64 = qkv.double().requires_grad_(True)
    o64 = _attn_ref(g64, B, nh, L, hd, torch.float64)
    o64.backward(do.double())
    g32 = qkv.clone().requires_grad_(True)
    o32 = _attn_ref(g32, B, nh, L, hd, torch.float32)
    o32.backward(do)
    o64, o32 = o64.detach(), o32.detach()
    on32, on_lse32 = online(qkv, B, nh, L, hd)
    return types.SimpleNamespace(
        family=family, geom=geom, qkv=qkv, do=do, o64=o64, o32=o32, on32=on32, g64=g64.grad, g32=g32.grad,
        lse64=lse2(qkv, B, nh, L, hd, torch.float64), lse32=lse2(qkv, B, nh, L, hd, torch.float32), on_lse32=on_lse32,
        delta64=delta_ref(do.double(), o64, B, nh, L, hd), delta32=delta_ref(do, o32, B, nh, L, hd))
