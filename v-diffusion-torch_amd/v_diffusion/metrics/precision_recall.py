"""Improved precision and recall (Kynkaenniemi et al., NeurIPS 2019) on the fused k-NN kernels of csrc/metrics.hip.

Same module path and call surface as the reference's v_diffusion/metrics/precision_recall.py, so pickled ``Manifold`` files
move between the two implementations in both directions.  Where the semantics differ from the reference's:
  - distances are fp32 (fp16 operands, fp32 accumulation); the reference's torch.cdist runs in fp16.  ``kth`` is still stored
    as fp16 (round to nearest) and calc_pr compares the fp32 distance against that fp16 radius widened to fp32;
  - ``row_batch_size`` / ``col_batch_size`` are accepted for call compatibility and have no effect: no distance block is ever
    materialised, so there is nothing to batch;
  - the VGG16 weights are never downloaded (VGGFeatureExtractor raises when the TorchScript file is missing);
  - there is no CPU path: ``device=None`` means the current GPU and a CPU device raises.
"""
import math
import os
from collections import namedtuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

from .. import _hip

Manifold = namedtuple("Manifold", ["features", "kth"])
if hasattr(torch.serialization, "add_safe_globals"):
    # torch >= 2.6 loads with weights_only=True by default: a plain torch.load of a saved manifold (eval.py:116) needs this
    torch.serialization.add_safe_globals([Manifold])

MAX_KTH = 16                 # nhood_size + 1 <= 16: the kernels' per-row candidate lists


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("v_diffusion.metrics: no MI355X visible; the k-NN passes have no CPU path")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"v_diffusion.metrics: device {device} -- the k-NN passes run on an MI355X only; there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Prepared:
    """device copy of a feature set as the kernels take it (fp16, padded feature length) and its squared row norms"""

    def __init__(self, features, device):
        if features.dim() != 2 or features.shape[0] < 1:
            raise ValueError(f"features must be a non-empty [n, d] tensor, got shape {tuple(features.shape)}")
        x = features.to(device=device, dtype=torch.float16)
        if not bool(torch.isfinite(x).all()):
            raise ValueError("features contain non-finite fp16 values")
        self.x = _hip.features_f16(x)
        with torch.cuda.device(device):
            self.sq = _hip.rows_sqnorm_f16(self.x)
        self.n = features.shape[0]


class VGGFeatureExtractor:
    WEIGHTS_URL = "https://nvlabs-fi-cdn.nvidia.com/stylegan2-ada-pytorch/pretrained/metrics/vgg16.pt"

    def __init__(self, device=torch.device("cpu")):
        self.model = self._load_model()
        self.device = device

    def _load_model(self):
        path = os.path.join(torch.hub.get_dir(), os.path.basename(self.WEIGHTS_URL))
        if not os.path.exists(path):
            raise FileNotFoundError(f"VGG16 feature network not found at {path}; this package never downloads it: fetch "
                                    f"{self.WEIGHTS_URL} into that file (torch.hub.get_dir()) first")
        model = torch.jit.load(path).eval()
        for p in model.parameters():
            p.requires_grad_(False)
        return model

    def extract_features(self, x):
        return self.model(x, return_features=True)

    def to(self, device):
        self.model.to(device)
        return self

    def __call__(self, x):
        return self.extract_features(x)


def to_uint8(x):
    """[-1, 1] images -> uint8 (the reference's rounding: x * 127.5 + 128, clamped, truncated)"""
    return torch.clamp(x * 127.5 + 128, 0, 255).to(torch.uint8)


def _subsample(size, max_sample_size, random_state):
    np.random.seed(random_state)
    return torch.as_tensor(np.random.choice(size, size=max_sample_size, replace=False))


def _batches(data, model, extr_batch_size, max_sample_size, random_state, num_workers):
    """image batches (uint8) in the reference's order and with its subsampling rule"""
    num_batches = math.ceil(max_sample_size / extr_batch_size)
    if model is not None:
        for i in range(num_batches):
            yield to_uint8(model.sample_x(min(extr_batch_size, max_sample_size - i * extr_batch_size)))
        return
    if hasattr(data, "__getitem__") and hasattr(data, "__len__") and not isinstance(data, (np.ndarray, torch.Tensor, str)):
        if len(data) > max_sample_size:
            data = Subset(data, indices=_subsample(len(data), max_sample_size, random_state))
        loader = DataLoader(data, batch_size=extr_batch_size, shuffle=False, num_workers=num_workers, drop_last=False,
                            pin_memory=True)
        for x in loader:
            yield x[0] if isinstance(x, (list, tuple)) else x
        return
    if isinstance(data, str) and os.path.exists(data):
        ext = data.rsplit(".", 1)[-1]
        data = np.load(data) if ext == "npy" else torch.load(data) if ext == "pt" else data
    data = torch.as_tensor(data)
    if data.dtype != torch.uint8:
        raise ValueError(f"image data must be uint8, got {data.dtype}")
    if data.shape[0] > max_sample_size:
        data = data[_subsample(data.shape[0], max_sample_size, random_state)]
    for i in range(num_batches):
        yield data[i * extr_batch_size: min((i + 1) * extr_batch_size, max_sample_size)]


class ManifoldBuilder:
    """Feature manifold of a sample set: fp16 features and the distance of each to its nhood_size-th nearest neighbour in the set
    (kth, fp16; the point itself counts as its own first neighbour, as in the reference's kthvalue(nhood_size + 1)).
    row_batch_size / col_batch_size: accepted for call compatibility, no effect (no distance block is materialised)."""

    def __init__(self, data=None, model=None, features=None, extr_batch_size=128, max_sample_size=50000, nhood_size=3,
                 row_batch_size=10000, col_batch_size=10000, random_state=1234, num_workers=0, device=None):
        if nhood_size + 1 > MAX_KTH or nhood_size < 0:
            raise ValueError(f"nhood_size = {nhood_size}: the k-NN kernels serve 0 <= nhood_size <= {MAX_KTH - 1}")
        self.device = _device(device)
        if features is None:
            self.extractor = VGGFeatureExtractor().to(self.device)
            parts = []
            with torch.inference_mode():
                for x in _batches(data, model, extr_batch_size, max_sample_size, random_state, num_workers):
                    parts.append(self.extractor(x.to(self.device)).cpu())
            features = torch.cat(parts, dim=0)
        elif not isinstance(features, torch.Tensor) or features.grad_fn is not None:
            raise ValueError("features must be a tensor without autograd history")
        self.nhood_size = nhood_size
        self.row_batch_size = row_batch_size
        self.col_batch_size = col_batch_size
        self.features = features.detach().to(torch.float16).cpu()
        self._prepared = _Prepared(self.features, self.device)       # device copy, reused by compute_kth on the same set
        self.kth = self.compute_kth(self.features)

    def _prepare(self, f):
        return self._prepared if f is self.features else _Prepared(f, self.device)

    def compute_kth(self, row_features, col_features=None):
        """fp16 [rows]: distance of each row feature to its (nhood_size + 1)-th nearest column feature, with multiplicity"""
        rows = self._prepare(row_features)
        cols = rows if col_features is None else self._prepare(col_features)
        if cols.n <= self.nhood_size:
            raise ValueError(f"{cols.n} points cannot have a {self.nhood_size + 1}-th nearest neighbour (nhood_size = {self.nhood_size})")
        if cols.x.shape[1] != rows.x.shape[1]:
            raise ValueError("row and column features differ in length")
        with torch.cuda.device(self.device):
            kth = _hip.knn_kth_f16(rows.x, rows.sq, cols.x, cols.sq, self.nhood_size + 1)
        return kth.to(torch.float16).cpu()

    def save(self, fpath):
        save_dir = os.path.dirname(fpath)
        if save_dir:
            os.makedirs(save_dir, exist_ok=True)
        torch.save(self.manifold, fpath)

    @property
    def manifold(self):
        return Manifold(features=self.features, kth=self.kth)


def calc_pr(manifold_1: Manifold, manifold_2: Manifold, row_batch_size: int, col_batch_size: int, device):
    """(precision, recall) as 0-d float32 CPU tensors.  manifold_1: generated samples, manifold_2: real samples.
    precision = share of manifold_1's points within the k-th radius of some point of manifold_2; recall: the other way round.
    A distance (fp32) is compared against the fp16 radius widened to fp32.  The batch sizes have no effect; device=None: the
    current GPU."""
    device = _device(device)
    m1, m2 = _Prepared(manifold_1.features, device), _Prepared(manifold_2.features, device)
    if m1.x.shape[1] != m2.x.shape[1]:
        raise ValueError("the two manifolds' features differ in length")

    def coverage(q, s, kth):
        if kth.numel() != s.n:
            raise ValueError(f"manifold has {s.n} features but {kth.numel()} radii")
        radius = kth.to(device=device, dtype=torch.float32).contiguous()
        with torch.cuda.device(device):
            hits = _hip.manifold_hits_f16(q.x, q.sq, s.x, s.sq, radius)
        return torch.tensor(int(hits.sum().item()) / q.n, dtype=torch.float32)

    return coverage(m1, m2, manifold_2.kth), coverage(m2, m1, manifold_1.kth)
