"""MI355X-native v-diffusion hot path behind the call surface of tqch/v-diffusion-torch
(reference v_diffusion/__init__.py:1-21).

The three hot-path names are implemented here, and progressive distillation on top of them (``DistillationDiffusion``,
``distill_coefs``: v_diffusion/distill.py, not part of the reference) and the DPM-Solver++(2M) multistep sampler
(``GaussianDiffusion.p_sample_solver``, ``solver_coefs``: v_diffusion/solver.py, not part of the reference either) and the RePaint inpainting / SDEdit sampler
(``GaussianDiffusion.p_sample_inpaint``, ``resampling_schedule``, ``known_coefs``, ``jump_coefs``: v_diffusion/inpaint.py, likewise) and image inversion
(``GaussianDiffusion.p_invert_noise`` / ``p_sample_replay`` / ``p_encode``, ``encode_coefs``, ``slerp``: v_diffusion/invert.py, likewise) and loss-aware
timestep resampling (``LossSecondMomentResampler``: v_diffusion/resample.py, likewise) and the UniPC predictor-corrector sampler
(``GaussianDiffusion.p_sample_unipc``, ``unipc_coefs``: v_diffusion/unipc.py, likewise) and consistency distillation / training with
multistep consistency sampling (``ConsistencyDiffusion``, ``GaussianDiffusion.p_sample_consistency``, ``consistency_coefs``,
``consistency_sample_coefs``, ``consistency_schedule``: v_diffusion/consistency.py, likewise) and Diffusion Posterior Sampling
(``GaussianDiffusion.p_sample_dps``, ``dps_measure``, ``blur``, ``gaussian_kernel``: v_diffusion/dps.py, likewise; ``UNet.forward_vjp`` is its input
gradient) and
DDNM null-space restoration (``GaussianDiffusion.p_sample_ddnm``, ``ddnm_rule``, ``ddnm_pinv``: v_diffusion/ddnm.py, likewise) and post-hoc EMA
(``posthoc_ema``, ``solve_weights``, ``profile_dot``, ``power_ema_rate``, ``sigma_rel_to_gamma``, ``gamma_to_sigma_rel``: v_diffusion/phema.py, likewise;
``HotPathTrainer(ema_sigma_rels=...)`` and ``optim.PowerEMA`` track its profiles).  The other nine names the reference package re-exports (data loading,
config helpers, its Trainer / Evaluator: control plane, out of scope) are NOT re-implemented: when the environment
variable ``VDIFF_REFERENCE_ROOT`` points at a checkout of the reference they are resolved lazily from it (loaded under
the alias ``v_diffusion_ref`` so its relative imports stay inside the reference), which lets the reference's
``train.py`` / ``generate.py`` run unchanged with this package first on ``sys.path``: they receive this package's
``UNet`` / ``GaussianDiffusion`` / ``get_logsnr_schedule`` and the reference's own plumbing around them."""
import importlib.util
import os
import sys

from .consistency import ConsistencyDiffusion, consistency_coefs, consistency_sample_coefs, consistency_schedule
from .ddnm import ddnm_pinv, ddnm_rule
from .diffusion import GaussianDiffusion, get_logsnr_schedule
from .distill import DistillationDiffusion, distill_coefs
from .dps import blur, dps_measure, gaussian_kernel, p_sample_dps
from .inpaint import jump_coefs, known_coefs, resampling_schedule
from .invert import encode_coefs, slerp
from .models.unet import UNet
from .phema import gamma_to_sigma_rel, posthoc_ema, power_ema_rate, profile_dot, sigma_rel_to_gamma, solve_weights
from .resample import LossSecondMomentResampler
from .solver import dynamic_threshold, solver_coefs, threshold_rank
from .unipc import p_sample_unipc, unipc_coefs

_HOT = ["GaussianDiffusion", "get_logsnr_schedule", "UNet", "DistillationDiffusion", "distill_coefs", "solver_coefs", "threshold_rank",
        "dynamic_threshold", "resampling_schedule", "known_coefs", "jump_coefs", "encode_coefs", "slerp", "LossSecondMomentResampler",
        "unipc_coefs", "p_sample_unipc", "ConsistencyDiffusion", "consistency_coefs", "consistency_sample_coefs", "consistency_schedule",
        "dps_measure", "p_sample_dps", "ddnm_rule", "ddnm_pinv", "sigma_rel_to_gamma", "gamma_to_sigma_rel", "power_ema_rate", "profile_dot",
        "solve_weights", "posthoc_ema", "blur", "gaussian_kernel"]
_DELEGATED = ["get_dataloader", "DATA_INFO", "dict2str", "seed_all", "update_config", "fill_with_defaults", "Trainer",
              "Evaluator", "DummyScheduler"]
_ref_pkg = None


def _reference():
    global _ref_pkg
    if _ref_pkg is None:
        root = os.environ.get("VDIFF_REFERENCE_ROOT")
        init = os.path.join(root, "v_diffusion", "__init__.py") if root else None
        if not init or not os.path.exists(init):
            raise ImportError("this name belongs to the reference's control plane, which this package does not re-implement; "
                              "set VDIFF_REFERENCE_ROOT to a tqch/v-diffusion-torch checkout to have it delegated")
        spec = importlib.util.spec_from_file_location("v_diffusion_ref", init,
                                                      submodule_search_locations=[os.path.dirname(init)])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["v_diffusion_ref"] = mod
        try:
            spec.loader.exec_module(mod)
        except BaseException:
            sys.modules.pop("v_diffusion_ref", None)
            raise
        _ref_pkg = mod
    return _ref_pkg


def __getattr__(name):
    if name in _DELEGATED:
        return getattr(_reference(), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# `from v_diffusion import *` (reference train.py) resolves every name of __all__: list the delegated ones only when they can be
__all__ = _HOT + (_DELEGATED if os.environ.get("VDIFF_REFERENCE_ROOT") else [])
