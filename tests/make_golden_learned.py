"""Writes tests/golden/learned_var.npz: learned variances as the reference's v_diffusion/diffusion.py:320-324 intends them, composed
from the reference's own functions on the CPU -- sigmoid of the variance channels as the tensor ``intp_frac`` of
``logsnr_to_posterior(..., "fixed_medium")``, ``pred_x0_from_v`` on the prediction channels, ``normal_kl`` and
``discretized_gaussian_loglik`` as ``_loss_term_bpd`` (:446-464) applies them.  (The reference's own method cannot run: it feeds the
undivided output to the prediction and forwards "learned" as the variance type.)  Run once where a checkout of the reference exists:

    VDIFF_REFERENCE_ROOT=/path/to/v-diffusion-torch python tests/make_golden_learned.py

Inputs in the style of oracle.cases.kl_case(): 6 x 3 x 16 x 16, 8-bit x0 with both saturation rows, T = 8 with t snapped to the grid and
row 0 the decoder row (s = 0); out has 6 channels, kl_case's v-output and nu = 3 * N(0, 1).  Contents: x0, xt, out, logsnr_s, logsnr_t
(fp32), logvar (per element), kl and nll (per sample, bits per dimension)."""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "learned_var.npz")
T = 8


def case():
    """(x0, xt, out, logsnr_s, logsnr_t): the tensors the fixture holds, from the project's own deterministic generators"""
    sys.path.insert(0, ROOT)
    from oracle import detrand, diffusion_ref as dref
    from oracle.cases import kl_case
    _, x0, t, _, noise, out_v = kl_case()
    t[3] = 0.3                                                    # kl_case's 0.0081 would snap to 1/T as well: one decoder row
    t = torch.ceil(t * T) / T
    s = (t - 1.0 / T).clamp(min=0.0)
    assert float(s[0]) == 0.0 and bool((s[1:] > 0).all())
    sched = dref.make_schedule("cosine")
    ls, lt = sched(s).float().reshape(-1, 1, 1, 1), sched(t).float().reshape(-1, 1, 1, 1)
    xt = dref.q_sample(x0, lt, noise)
    out = torch.cat([out_v, 3.0 * detrand.normal("nu", tuple(x0.shape), 5)], dim=1)
    return x0, xt, out, ls, lt


def main():
    root = os.environ.get("VDIFF_REFERENCE_ROOT")
    if not root or not os.path.exists(os.path.join(root, "v_diffusion", "diffusion.py")):
        sys.exit("set VDIFF_REFERENCE_ROOT to a checkout of the reference")
    pkg = types.ModuleType("ref_v_diffusion")                     # the reference's package under another name: ours stays importable
    pkg.__path__ = [os.path.join(root, "v_diffusion")]
    sys.modules["ref_v_diffusion"] = pkg
    ref = importlib.import_module("ref_v_diffusion.diffusion")
    fn = importlib.import_module("ref_v_diffusion.functions")

    x0, xt, out, ls, lt = case()
    v, nu = out.chunk(2, dim=1)                                   # :321
    frac = torch.sigmoid(nu)                                      # :322
    pred = ref.pred_x0_from_v(xt, v, lt)
    # the function upcasts the log-SNRs to fp64 and torch.lerp wants its weight in the same dtype: the fp32 sigmoid, widened
    c1, c2, lv = ref.logsnr_to_posterior(ls, lt, "fixed_medium", intp_frac=frac.double())
    t1, t2, tlv = ref.logsnr_to_posterior(ls, lt, "fixed_small")
    kl = fn.flat_mean(fn.normal_kl(t1 * xt + t2 * x0, tlv, c1 * xt + c2 * pred, lv)) / math.log(2.0)
    nll = fn.flat_mean(-fn.discretized_gaussian_loglik(x0, pred, log_scale=0.5 * lv)) / math.log(2.0)
    assert lv.shape == x0.shape and lv.dtype == torch.float32 and bool(torch.isfinite(kl[1:]).all()) and bool(torch.isfinite(nll).all())
    np.savez_compressed(OUT, x0=x0.numpy(), xt=xt.numpy(), out=out.numpy(), logsnr_s=ls.numpy(), logsnr_t=lt.numpy(), logvar=lv.numpy(),
                        kl=kl.numpy(), nll=nll.numpy())
    print("kl", kl.numpy(), "\nnll", nll.numpy())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
