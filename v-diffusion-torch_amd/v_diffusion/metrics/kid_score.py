"""Kernel Inception Distance (Binkowski et al. 2018, "Demystifying MMD GANs") on the fused fp64 kernel of csrc/kid.hip.

The reference has no counterpart; this module is reached as ``v_diffusion.metrics.kid_score`` and is not part of the star-import
surface of ``v_diffusion.metrics``.

  - the metric is the unbiased MMD^2 under the polynomial kernel k(a, b) = (gamma <a, b> + coef0)^degree (defaults: degree 3,
    gamma = 1 / d, coef0 = 1):  Sxx / (mx (mx - 1)) + Syy / (my (my - 1)) - 2 Sxy / (mx my)  with Sxx, Syy the kernel sums over the
    pairs of distinct positions of a set and Sxy the sum over all cross pairs;
  - the three sums of every subset come out of ONE launch that forms 64 x 64 tiles of the Gram matrices in registers and sums
    them there: no m x m matrix exists in memory, so ``polynomial_mmd`` takes whole sets of any size (50 000 x 50 000 included)
    and ``kernel_inception_distance`` is the usual mean over random subsets;
  - the subsets are drawn on the host (``subset_indices``) and their rows are gathered inside the kernel's loads; the index
    arrays are range-checked on the host before they are uploaded, because the kernel cannot check them;
  - features of any float dtype on any device are converted to contiguous fp32 on the GPU; the arithmetic is fp64 with exact
    products, and the same call gives the same bits;
  - non-finite features are not rejected: they make exactly the subsets that draw them non-finite;
  - there is no CPU path: ``device=None`` means the current GPU and a CPU device raises.
"""
from collections import namedtuple

import numpy as np
import torch

from .. import _hip
from .fid_score import GRANULE, _device

KID = namedtuple("KID", ["mean", "std", "values"])


def subset_indices(nx, ny, subsets, subset_size, seed=0):
    """(ix, iy): int32 arrays [subsets, subset_size] of row numbers into sets of nx and ny rows, no repeats inside a row.

    The draw order is this module's definition of "the subsets of seed s": one ``np.random.RandomState(seed)``; for subset
    0, 1, ... in turn first ``choice(nx, subset_size, replace=False)`` for X, then ``choice(ny, subset_size, replace=False)`` for Y."""
    nx, ny, subsets, m = int(nx), int(ny), int(subsets), int(subset_size)
    if subsets < 1:
        raise ValueError(f"subsets = {subsets}: need at least one")
    if m < 2 or m > nx or m > ny:
        raise ValueError(f"subset_size = {m}: need 2 <= subset_size <= the smaller set ({nx} and {ny} rows)")
    rng = np.random.RandomState(seed)
    ix, iy = np.empty((subsets, m), dtype=np.int32), np.empty((subsets, m), dtype=np.int32)
    for s in range(subsets):
        ix[s] = rng.choice(nx, m, replace=False)
        iy[s] = rng.choice(ny, m, replace=False)
    return ix, iy


def _features(feat_x, feat_y, degree):
    """the argument checks that need no device: two [n, d] float sets of one feature length d, a multiple of the kernel's granule"""
    for f in (feat_x, feat_y):
        if not isinstance(f, torch.Tensor) or f.dim() != 2 or not f.is_floating_point():
            raise ValueError(f"features must be a floating-point [n, d] tensor, got {getattr(f, 'dtype', type(f).__name__)} "
                             f"{tuple(getattr(f, 'shape', ()))}")
    d = feat_x.shape[1]
    if feat_y.shape[1] != d:
        raise ValueError(f"the two sets have different feature lengths: {d} vs {feat_y.shape[1]}")
    if d < GRANULE or d % GRANULE:
        raise ValueError(f"feature length {d}: the kernel takes positive multiples of {GRANULE}")
    if feat_x.shape[0] < 2 or feat_y.shape[0] < 2:
        raise ValueError(f"each set needs at least 2 rows, got {feat_x.shape[0]} and {feat_y.shape[0]}")
    if not (isinstance(degree, (int, np.integer)) and 1 <= degree <= 8):
        raise ValueError(f"degree = {degree!r}: need an integer in 1..8")
    return d


def _to_device(f, device):
    return f.detach().to(device=device, dtype=torch.float32).contiguous()


def _mmd2(sums, mx, my):
    """[subsets, 3] fp64 host sums -> per-subset unbiased MMD^2"""
    return sums[:, 0] / (mx * (mx - 1.0)) + sums[:, 1] / (my * (my - 1.0)) - 2.0 * sums[:, 2] / (float(mx) * my)


def polynomial_mmd(feat_x, feat_y, degree=3, gamma=None, coef0=1.0, device=None):
    """the unbiased MMD^2 between the whole sets feat_x [nx, d] and feat_y [ny, d] (nx and ny may differ) as a Python float"""
    _features(feat_x, feat_y, degree)
    device = _device(device)
    with torch.cuda.device(device):
        sums = _hip.kid_sums(_to_device(feat_x, device), _to_device(feat_y, device), None, None, int(degree), gamma, coef0)
    return float(_mmd2(sums.cpu().numpy(), feat_x.shape[0], feat_y.shape[0])[0])


def kernel_inception_distance(feat_x, feat_y, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0, indices=None,
                              device=None):
    """KID(mean, std, values): the unbiased polynomial-kernel MMD^2 of `subsets` random subsets of `subset_size` rows of each set;
    values is the fp64 numpy vector of the per-subset estimates, mean its mean, std its np.std (ddof = 0).
    indices = (ix, iy), int32 numpy arrays [subsets, m], replaces the draw of subset_indices(nx, ny, subsets, subset_size, seed);
    the two may have different m."""
    _features(feat_x, feat_y, degree)
    nx, ny = feat_x.shape[0], feat_y.shape[0]
    if indices is None:
        ix, iy = subset_indices(nx, ny, subsets, subset_size, seed)
    else:
        try:
            ix, iy = indices
        except (TypeError, ValueError):
            raise ValueError("indices must be a pair (ix, iy) of int32 numpy arrays") from None
        ix, iy = _hip.kid_indices(ix, nx, "ix"), _hip.kid_indices(iy, ny, "iy")
        if ix.shape[0] != iy.shape[0]:
            raise ValueError(f"ix and iy hold different numbers of subsets: {ix.shape[0]} vs {iy.shape[0]}")
        if ix.shape[1] < 2 or iy.shape[1] < 2:
            raise ValueError(f"a subset needs at least 2 rows of each set, got {ix.shape[1]} and {iy.shape[1]}")
    device = _device(device)
    with torch.cuda.device(device):
        sums = _hip.kid_sums(_to_device(feat_x, device), _to_device(feat_y, device), ix, iy, int(degree), gamma, coef0)
    values = _mmd2(sums.cpu().numpy(), ix.shape[1], iy.shape[1])
    return KID(float(np.mean(values)), float(np.std(values)), values)
