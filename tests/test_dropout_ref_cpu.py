"""tests/dropout_ref.py, the host replay of the GroupNorm kernels' dropout mask, against what does not depend on this project: the
published Philox4x32-10 known answers (Random123, kat_vectors) and a scalar restatement of the element-index convention."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_ref as D                                           # noqa: E402

KAT = [  # counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_philox_known_answers(dtype):
    for ctr, key, want in KAT:
        got = D.philox4x32_10(np.array(ctr, dtype=dtype), np.array(key, dtype=dtype))
        assert got.dtype == np.uint32 and got.tolist() == list(want), ([hex(v) for v in got.tolist()], ctr, key)
    # vectorised over counters, one key broadcast / one key per counter
    ctrs = np.array([k[0] for k in KAT], dtype=dtype)
    keys = np.array([k[1] for k in KAT], dtype=dtype)
    assert D.philox4x32_10(ctrs, keys).tolist() == [list(k[2]) for k in KAT]
    assert D.philox4x32_10(ctrs[:2], keys[0])[0].tolist() == list(KAT[0][2])


def _scalar_block(ctr, key):
    """the ten rounds on Python integers, written out from the paper (independent of the numpy code's masking and broadcasting)"""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_scalar_restatement_reproduces_the_known_answers():
    for ctr, key, want in KAT:
        assert _scalar_block(ctr, key) == list(want)


@pytest.mark.parametrize("seed", [1234, (1 << 40) + 77, (1 << 63) + 5])
def test_keep_scale_element_index_and_values(seed):
    nimg, HW, C, p = 3, 5, 12, 0.2
    m = D.keep_scale(seed, p, nimg, HW, C)
    assert m.shape == (nimg, HW, C) and m.dtype == np.float32
    inv = np.float32(1) / (np.float32(1) - np.float32(p))
    assert set(np.unique(m).tolist()) <= {0.0, float(inv)}
    for b, pix, c in [(0, 0, 0), (0, 0, 3), (0, 0, 4), (0, 1, 0), (1, 0, 0), (2, 4, 11), (1, 3, 6)]:
        vi = (b * HW + pix) * (C // 4) + c // 4
        r = _scalar_block((vi & 0xFFFFFFFF, vi >> 32, 0x243F6A88, 0x85A308D3), (seed & 0xFFFFFFFF, seed >> 32))[c % 4]
        keep = np.float32(r >> 8) * np.float32(2.0 ** -24) >= np.float32(p)
        assert m[b, pix, c] == (inv if keep else np.float32(0)), (b, pix, c)


def test_keep_scale_uses_both_key_words_and_is_bernoulli():
    a = D.keep_scale(1234, 0.2, 2, 64, 64)
    b = D.keep_scale(1234 + (1 << 32), 0.2, 2, 64, 64)              # same low word, other high word
    c = D.keep_scale(1235, 0.2, 2, 64, 64)
    assert ((a != 0) != (b != 0)).mean() > 0.2 and ((a != 0) != (c != 0)).mean() > 0.2
    assert np.array_equal(a, D.keep_scale(1234, 0.2, 2, 64, 64))
    for m in (a, b, c):
        assert abs((m != 0).mean() - 0.8) < 0.015                  # 8192 draws: sigma = 0.0044
    assert (D.keep_scale(7, 0.0, 1, 4, 8) == 1.0).all()


def test_keep_scale_counter_crosses_32_bits():
    """the second counter word: the block of vector index 2^32 + 1 is not the block of index 1"""
    lo = D.philox4x32_10(np.array([1, 0, D.CTR2, D.CTR3], dtype=np.uint64), np.array([5, 0], dtype=np.uint64))
    hi = D.philox4x32_10(np.array([1, 1, D.CTR2, D.CTR3], dtype=np.uint64), np.array([5, 0], dtype=np.uint64))
    assert lo.tolist() == _scalar_block((1, 0, D.CTR2, D.CTR3), (5, 0)) and hi.tolist() == _scalar_block((1, 1, D.CTR2, D.CTR3), (5, 0))
    assert lo.tolist() != hi.tolist()
