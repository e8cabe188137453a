"""Frechet Inception Distance on the fp64 kernels of csrc/fid.hip.

Same module path and call surface as the reference's v_diffusion/metrics/fid_score.py (InceptionStatistics, get_precomputed,
calc_fd, calculate_frechet_distance).  Where the semantics differ from the reference's:
  - the statistics accumulate on the device: each batch of activations goes through one vd_fid_accum launch that adds its
    shifted sums and outer products to fp64 device buffers; nothing is copied to the host and nothing synchronises until
    get_statistics().  The shift (the fp32-rounded column means of the first batch after a reset) keeps the second moments
    from cancelling when |mean| >> std; mean and covariance are formed from the sums once, in get_statistics();
  - a feature map that is not 1 x 1 is averaged over H x W (in fp64, rounded once to fp32).  The reference calls
    adaptive_avg_pool2d on a numpy array at that point and cannot run; this is its evident intent;
  - non-finite activations propagate into the sums (a NaN or Inf in column c spoils row and column c of the covariance and
    entry c of the mean); get_statistics() raises ValueError when the statistics are not finite;
  - the distance is |mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum_i sqrt(lambda_i(R S2 R)) with R = S1^(1/2): R S2 R is symmetric and has
    the eigenvalues of S1 S2, whose non-symmetric scipy.linalg.sqrtm the reference takes.  The three d x d x d products run on
    the device (vd_atb_f64); the two symmetric eigen-solves are torch.linalg.eigh / eigvalsh on CPU fp64 tensors (host LAPACK,
    0.8 s at d = 2048 on 16 threads): the one host step;
  - get_precomputed never reaches the network, and the Inception weights are never downloaded: model=None builds the reference's
    InceptionV3 when VDIFF_REFERENCE_ROOT names a checkout and raises ImportError otherwise;
  - there is no CPU path: ``device=None`` means the current GPU and a CPU device raises.
"""
import importlib
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _hip

GRANULE = 16                     # activation_dim granule of the kernels (one MFMA tile edge)

# dataset name -> (statistics file looked for in download_dir, the address it is published under)
_TTUR = "http://bioinf.jku.at/research/ttur/ttur_stats/"
_VAEGAN = "https://github.com/tqch/VAEGAN/releases/download/precomputed_statistics_celeba/"
PRECOMPUTED = {name: (fname, base + fname) for name, fname, base in [
    ("cropped_celeba", "fid_stats_celeba_148x148.npz", _VAEGAN),
    ("lsun_bedroom", "fid_stats_lsun_train.npz", _TTUR),
    ("cifar10", "fid_stats_cifar10_train.npz", _TTUR),
    ("svhn", "fid_stats_svhn_train.npz", _TTUR),
    ("imagenet_train", "fid_stats_imagenet_train.npz", _TTUR),
    ("imagenet_valid", "fid_stats_imagenet_valid.npz", _TTUR),
]}
_ALIASES = {"celeba": "cropped_celeba"}


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("v_diffusion.metrics: no MI355X visible; the FID kernels have no CPU path")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"v_diffusion.metrics: device {device} -- the FID kernels run on an MI355X only; there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _identity(x):
    return x


def finalize(shift, sum_, outer, count):
    """(mean [d], cov [d, d]) as fp64 device tensors from the running sums of vd_fid_accum over `count` rows.  outer holds the lower
    triangle of tiles; it is mirrored first, and every later step treats (a, b) and (b, a) alike, so cov == cov.T bitwise."""
    lower = torch.tril(outer)
    full = lower + torch.tril(outer, -1).T
    delta = sum_ / count
    cov = (full - count * torch.outer(delta, delta)) / (count - 1)
    return shift + delta, cov


class InceptionStatistics(nn.Module):
    """Running mean and covariance (fp64, on the device) of the activations `model(x)[0]` over the batches passed to forward()."""

    def __init__(self, model=None, input_transform=_identity, activation_dim=2048, device=None):
        super().__init__()
        if activation_dim < GRANULE or activation_dim % GRANULE:
            raise ValueError(f"activation_dim = {activation_dim}: the statistics kernel takes positive multiples of {GRANULE}")
        self.input_transform = input_transform
        self.activation_dim = activation_dim
        self.model = self.load_model() if model is None else model
        self.device = _device(device)
        self.model.eval()
        self.model.to(self.device)
        d = activation_dim
        self._shift = torch.zeros(d, dtype=torch.float64, device=self.device)
        self._sum = torch.zeros(d, dtype=torch.float64, device=self.device)
        self._outer = torch.zeros(d, d, dtype=torch.float64, device=self.device)
        self.count = 0

    def load_model(self):
        """the reference's InceptionV3 for this activation_dim, from the checkout named by VDIFF_REFERENCE_ROOT"""
        from .. import _reference
        try:
            _reference()
        except ImportError as e:
            raise ImportError("InceptionStatistics(model=None) builds the reference's InceptionV3, which this package does not "
                              "re-implement and whose weights it never downloads: set VDIFF_REFERENCE_ROOT to a "
                              "tqch/v-diffusion-torch checkout, or pass the feature network as model=") from e
        inception = importlib.import_module("v_diffusion_ref.metrics.inception")
        return inception.InceptionV3([inception.InceptionV3.BLOCK_INDEX_BY_DIM[self.activation_dim]])

    def forward(self, x):
        x = self.input_transform(x)
        with torch.inference_mode():
            act = self.model(x)[0]
            if act.dim() == 4:
                if act.shape[2] != 1 or act.shape[3] != 1:
                    act = act.mean(dim=(2, 3), dtype=torch.float64)
                else:
                    act = act[:, :, 0, 0]
            self.update(act)

    def update(self, features):
        """add a batch of activations [n, activation_dim] (any float dtype, any device) to the running sums"""
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1:
            raise ValueError(f"activations must be a non-empty [n, d] tensor, got {tuple(getattr(features, 'shape', ()))}")
        if features.shape[1] != self.activation_dim:
            raise ValueError(f"the model returned {features.shape[1]} activations per sample, activation_dim = {self.activation_dim}")
        x = features.detach().to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            if self.count == 0:
                _hip.fid_shift(x, self._shift)
            _hip.fid_accum(x, self._shift, self._sum, self._outer)
        self.count += x.shape[0]

    def get_statistics(self):
        """(mean [d], covariance [d, d]) as fp64 numpy arrays; the covariance carries the count / (count - 1) scaling"""
        assert self.count > 1, "Count must be greater than 1!"
        mean, cov = finalize(self._shift, self._sum, self._outer, self.count)
        mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
        if not (np.isfinite(mean).all() and np.isfinite(cov).all()):
            raise ValueError("the accumulated statistics are not finite: some activation was NaN or Inf")
        return mean, cov

    def reset(self):
        self._shift.zero_()
        self._sum.zero_()
        self._outer.zero_()
        self.count = 0


def get_precomputed(dataset, download_dir="precomputed"):
    """(mu, sigma) of a published reference set from `download_dir`; the file is never fetched"""
    dataset = _ALIASES.get(dataset, dataset)
    if dataset not in PRECOMPUTED:
        raise KeyError(f"no precomputed statistics known for {dataset!r}; known: {sorted(PRECOMPUTED)}")
    filename, url = PRECOMPUTED[dataset]
    path = os.path.join(download_dir if download_dir is not None else ".", filename)
    if not os.path.exists(path):
        raise FileNotFoundError(f"precomputed FID statistics not found at {path}; this package never downloads them: fetch {url} "
                                f"into that file first")
    with np.load(path) as data:
        return data["mu"][:], data["sigma"][:]


def _sym_eigh_sqrt_trace(s1, s2, device):
    """sum_i sqrt(max(lambda_i, 0)) of R S2 R, R = S1^(1/2), for symmetric fp64 CPU tensors s1, s2"""
    w, v = torch.linalg.eigh(s1)                                   # host LAPACK
    # R = Q^T Q with Q = diag(w+^(1/4)) V^T; then S2 R = atb(S2, R) and R S2 R = atb(S2 R, R): S2 and R are symmetric
    q = (v * w.clamp_min(0.0).pow(0.25)).T.contiguous().to(device)
    with torch.cuda.device(device):
        r = _hip.atb_f64(q, q)
        m = _hip.atb_f64(_hip.atb_f64(s2.to(device), r), r)
    m = m.cpu()
    lam = torch.linalg.eigvalsh((m + m.T) * 0.5)                   # host LAPACK
    return float(lam.clamp_min(0.0).sqrt().sum())


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, device=None):
    """Frechet distance between N(mu1, sigma1) and N(mu2, sigma2) as a Python float (module docstring: formulation, host step).
    eps is added to both diagonals, once, only if the eigen route yields a non-finite value."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    if mu1.ndim != 1 or mu1.shape != mu2.shape:
        raise ValueError(f"training and test mean vectors have different lengths: {mu1.shape} vs {mu2.shape}")
    if sigma1.shape != sigma2.shape:
        raise ValueError(f"training and test covariances have different dimensions: {sigma1.shape} vs {sigma2.shape}")
    d = mu1.shape[0]
    if sigma1.shape != (d, d):
        raise ValueError(f"covariances of shape {sigma1.shape} do not belong to means of length {d}")
    if d < GRANULE or d % GRANULE:
        raise ValueError(f"d = {d}: the product kernel takes positive multiples of {GRANULE}")
    device = _device(device)
    s1, s2 = torch.from_numpy(sigma1), torch.from_numpy(sigma2)
    s1, s2 = (s1 + s1.T) * 0.5, (s2 + s2.T) * 0.5
    diff = mu1 - mu2
    fixed = float(diff.dot(diff)) + float(np.trace(sigma1)) + float(np.trace(sigma2))
    tr = _sym_eigh_sqrt_trace(s1, s2, device)
    if not np.isfinite(tr):
        print(f"fid calculation produces a non-finite value; adding {eps} to diagonal of cov estimates")
        offset = torch.eye(d, dtype=torch.float64) * eps
        tr = _sym_eigh_sqrt_trace(s1 + offset, s2 + offset, device)
    return fixed - 2.0 * tr


def calc_fd(mean1, var1, mean2, var2, eps=1e-6):
    return calculate_frechet_distance(mean1, var1, mean2, var2, eps)
