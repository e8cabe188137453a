"""Evaluation metrics behind the call surface of the reference's v_diffusion.metrics (reference metrics/__init__.py).

The precision / recall metric (ManifoldBuilder, Manifold, calc_pr) is implemented here on the fused k-NN kernels of
csrc/metrics.hip.  The FID names (InceptionStatistics, get_precomputed, calc_fd) resolve, by default, lazily from the reference
checkout named by ``VDIFF_REFERENCE_ROOT`` (``v_diffusion_ref.metrics``) like the control-plane names of the parent package, so
the reference's ``eval.py --metrics pr fid`` runs unchanged with this package first on ``sys.path``.  With ``VDIFF_NATIVE_FID=1``
in the environment they resolve to this package's own fid_score module (fp64 statistics and products on the kernels of
csrc/fid.hip) instead and are always listed.  The Kernel Inception Distance and the Inception Score, which the reference does not
have, live in the submodules ``kid_score`` and ``inception_score`` (kernels of csrc/kid.hip) and are not star-imported.
``import v_diffusion`` does not import this subpackage."""
import importlib
import os

from .precision_recall import Manifold, ManifoldBuilder, calc_pr

_NATIVE = ["ManifoldBuilder", "Manifold", "calc_pr"]
_DELEGATED = ["InceptionStatistics", "get_precomputed", "calc_fd"]
_NATIVE_FID = os.environ.get("VDIFF_NATIVE_FID") == "1"


def __getattr__(name):
    if name in _DELEGATED:
        if _NATIVE_FID:
            return getattr(importlib.import_module(__name__ + ".fid_score"), name)
        from .. import _reference
        _reference()                                   # loads the checkout as v_diffusion_ref (or raises the ImportError)
        return getattr(importlib.import_module("v_diffusion_ref.metrics"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# `from v_diffusion.metrics import *` (reference eval.py:10) resolves every name of __all__: list the delegated ones only when they can be
__all__ = _NATIVE + (_DELEGATED if _NATIVE_FID or os.environ.get("VDIFF_REFERENCE_ROOT") else [])
