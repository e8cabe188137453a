"""Inception Score (Salimans et al. 2016) on the fused fp64 kernel of csrc/kid.hip.

The reference's README reports IS beside FID but its code does not compute it; this module is reached as
``v_diffusion.metrics.inception_score`` and is not part of the star-import surface of ``v_diffusion.metrics``.

``inception_score(logits, splits)`` takes the classifier's logits [n, classes] (any float dtype, any device; converted to
contiguous fp32 on the GPU), cuts the rows into `splits` consecutive parts (part k = rows [k n / splits, (k + 1) n / splits))
and returns exp(mean_i KL(p_i || pbar)) of every part, softmax and logarithms in fp64 with the row maximum subtracted and
0 log 0 = 0.  A NaN logit makes its own part's score NaN and no other.  Fixed summation order: the same call gives the same
bits.  There is no CPU path: ``device=None`` means the current GPU and a CPU device raises."""
from collections import namedtuple

import numpy as np
import torch

from .. import _hip
from .fid_score import _device

InceptionScore = namedtuple("InceptionScore", ["mean", "std", "values"])


def inception_score(logits, splits=10, device=None):
    """InceptionScore(mean, std, values): values is the fp64 numpy vector of the per-split scores, std its np.std (ddof = 0)"""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or not logits.is_floating_point():
        raise ValueError(f"logits must be a floating-point [n, classes] tensor, got {getattr(logits, 'dtype', type(logits).__name__)} "
                         f"{tuple(getattr(logits, 'shape', ()))}")
    n, classes = logits.shape
    if classes < 2:
        raise ValueError(f"classes = {classes}: need at least 2")
    if not (isinstance(splits, (int, np.integer)) and 1 <= splits <= n):
        raise ValueError(f"splits = {splits!r}: need an integer with 1 <= splits <= n = {n} (every split holds at least one row)")
    device = _device(device)
    with torch.cuda.device(device):
        scores = _hip.is_scores(logits.detach().to(device=device, dtype=torch.float32).contiguous(), int(splits))
    values = scores.cpu().numpy()
    return InceptionScore(float(np.mean(values)), float(np.std(values)), values)
