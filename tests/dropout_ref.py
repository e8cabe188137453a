"""Host replay of the dropout keep mask of the GroupNorm kernels (csrc/common.h: vd_philox4, vd_dropout_scale4), in numpy.

The kernels never store the mask: forward and every backward form regenerate it from (seed, element index).  This module states
what they must produce, independently of any kernel: the published Philox4x32-10 block function and the element-index convention
of csrc/norm.hip (NHWC, four consecutive channels per counter, pixels of the norm's INPUT resolution)."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # round multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85                                 # key schedule (Weyl) increments
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
CTR2, CTR3 = 0x243F6A88, 0x85A308D3                               # the two fixed counter words of vd_philox4


def philox4x32_10(counter4, key2):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11): counter4 [..., 4] and key2 [..., 2] of
    32-bit words (any unsigned integer dtype, broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter4).astype(np.uint64) & _LO
    k = np.asarray(key2).astype(np.uint64) & _LO
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                                # 32 x 32 -> 64 bit products: no overflow in uint64
        n0 = (p1 >> _S32) ^ c1 ^ k0
        n2 = (p0 >> _S32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _LO, n2, p0 & _LO
        k0 = (k0 + np.uint64(_W0)) & _LO
        k1 = (k1 + np.uint64(_W1)) & _LO
    out = np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)
    return out.astype(np.uint32)


def keep_scale(seed, p, nimg, HW, C):
    """[nimg, HW, C] float32: 1/(1-p) where element (image, pixel, channel) is kept, 0 where it is dropped.
    Element (b, pix, c) takes word c % 4 of the block of counter (b*HW + pix)*(C//4) + c//4 under the key (lo32(seed), hi32(seed))."""
    assert C % 4 == 0 and 0 <= int(seed) < 1 << 64
    seed = int(seed)
    vi = np.arange(nimg * HW * (C // 4), dtype=np.uint64)
    ctr = np.empty((vi.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = vi & _LO, vi >> _S32, CTR2, CTR3
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    r = philox4x32_10(ctr, key)                                    # [n, 4]: word j belongs to channel 4 * (c // 4) + j
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    p32 = np.float32(p)
    inv = np.float32(1) / (np.float32(1) - p32)
    return np.where(u >= p32, inv, np.float32(0)).astype(np.float32).reshape(nimg, HW, C)
