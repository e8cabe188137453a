"""tests/optim_ref.py, the references of the optimizer-tail tests, against torch itself: torch.optim.AdamW + clip_grad_norm_ on separate
fp64 parameters, one of which goes without a gradient for two steps, and the restated utils.py EMA (test_optim_gpu.RefEMA).  Plus, as
numbers only, what forming 1 - beta and 1 - decay in fp32 from fp32-rounded constants costs: the magnitudes the GPU tests of
tests/test_optim_kernels_gpu.py are built to see."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R                                             # noqa: E402
from test_optim_gpu import RefEMA                                 # noqa: E402

U = 2.0 ** -24
SIZES = (37, 64, 21)                                              # the third parameter is the range
KW = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.01, max_norm=1.0)
STEPS, NO_GRAD = 6, (2, 3)                                        # the range receives no gradient in steps 2 and 3 (counted from 1)


def _randn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _torch_run():
    """(states after each step as flat fp64 dicts, the gradients, the squared norms, the decays) of the torch loop"""
    model = torch.nn.Module()
    model.w = torch.nn.ParameterList([torch.nn.Parameter(_randn(n, 10 + i)) for i, n in enumerate(SIZES)])
    params = list(model.w)
    opt = torch.optim.AdamW(params, lr=KW["lr"], betas=KW["betas"], eps=KW["eps"], weight_decay=KW["wd"])
    ema = RefEMA(model, 0.9999)
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])
    start = {"p": flat(params), "m": torch.zeros(sum(SIZES), dtype=torch.float64), "v": torch.zeros(sum(SIZES), dtype=torch.float64),
             "ema": flat(ema.shadow[k] for k, _ in ema.named)}
    out, grads, norms, decays = [], [], [], []
    for s in range(1, STEPS + 1):
        # alternately clipped (norm about 11) and not (norm about 0.2)
        gs = [_randn(n, 100 * s + i, 1.0 if s % 2 else 0.02) for i, n in enumerate(SIZES)]
        if s in NO_GRAD:
            gs[2] = None
        for p, g in zip(params, gs):
            p.grad = None if g is None else g.clone()
        torch.nn.utils.clip_grad_norm_(params, KW["max_norm"])
        opt.step()
        ema.update()
        st = opt.state_dict()["state"]
        out.append({"p": flat(params), "m": flat(st[i]["exp_avg"] for i in range(3)), "v": flat(st[i]["exp_avg_sq"] for i in range(3)),
                    "ema": flat(ema.shadow[k] for k, _ in ema.named)})
        grads.append(torch.cat([torch.zeros(n, dtype=torch.float64) if g is None else g for g, n in zip(gs, SIZES)]))
        norms.append(float(R.sumsq64(grads[-1])))
        decays.append(min(0.9999, (1 + s) / (10 + s)))
    assert [int(float(st[i]["step"])) for i in range(3)] == [STEPS, STEPS, STEPS - len(NO_GRAD)]
    return start, out, grads, norms, decays


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("fn,tol", [(R.step64, 1e-14), (R.step32_torch, 2e-5)])
def test_the_references_follow_torch_adamw_clip_and_ema(fn, tol):
    """six steps; step64 equals the torch loop to 1e-14 of each buffer's largest element with the range in mode 1 (steps 2, 3) and in
    mode 2 (its count lags from step 4 on), step32_torch to fp32 rounding (its proof as an fp32 restatement is that it is the same code
    path with the same operators; here it must only not be a different recurrence)"""
    start, want, grads, norms, decays = _torch_run()
    lo, hi = sum(SIZES[:2]), sum(SIZES)
    state, rk = start, 0
    for s in range(1, STEPS + 1):
        mode = 1 if s in NO_GRAD else 2
        rk += mode == 2
        prev = state
        state = fn(state, grads[s - 1], gnorm_sq=norms[s - 1], decay=decays[s - 1], k=s, rng=(lo, hi), rng_mode=mode, rng_k=rk, **KW)
        for key in R.KEYS:
            assert _rel(state[key].double(), want[s - 1][key]) <= tol, (s, key, _rel(state[key].double(), want[s - 1][key]))
        if mode == 1:
            for key in ("p", "m", "v"):
                assert torch.equal(state[key][lo:hi], prev[key][lo:hi]), (s, key)
    assert rk == STEPS - len(NO_GRAD)


def test_step64_leaves_its_arguments_alone_and_reads_the_norm_rules():
    n = 11
    state = {"p": _randn(n, 1), "m": _randn(n, 2, 0.05), "v": _randn(n, 3, 0.05) ** 2, "ema": _randn(n, 4)}
    keep = {k: v.clone() for k, v in state.items()}
    g = _randn(n, 5)
    kw = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, wd=0.01, decay=0.99, k=3)
    clipped = R.step64(state, g, max_norm=1.0, gnorm_sq=float(R.sumsq64(g)), **kw)
    for k in R.KEYS:
        assert torch.equal(state[k], keep[k])
    plain = R.step64(state, g, max_norm=1.0, gnorm_sq=None, **kw)
    assert torch.equal(R.step64(state, g, max_norm=0.0, gnorm_sq=float(R.sumsq64(g)), **kw)["m"], plain["m"])
    assert not torch.equal(clipped["m"], plain["m"])
    c = 1.0 / (float(R.sumsq64(g)) ** 0.5 + 1e-6)
    assert _rel(clipped["m"], 0.9 * state["m"] + (1 - 0.9) * c * g) <= 1e-15
    assert float(R.sumsq64(torch.tensor([3.0, 4.0], dtype=torch.float32))) == 25.0


# Why the optimizer entries take their betas and decay as doubles: a rate formed in fp32 from the fp32-rounded constant, (1.f - 0.9999f),
# is off by the `rel` below; torch.optim.AdamW and utils.py:149 form it in Python doubles and round once, (float)(1.0 - 0.9999).
@pytest.mark.parametrize("c,rel", [(0.9999, 1.66e-4), (0.999, -1.29e-5), (0.9, 2.4e-7)])
def test_emulated_kernel_constants(c, rel):
    old = float(np.float32(1) - np.float32(c))
    new = float(np.float32(1.0 - c))
    assert abs((old / (1.0 - c) - 1.0) / rel - 1.0) < 0.02, (c, old, old / (1.0 - c) - 1.0)
    assert abs(new / (1.0 - c) - 1.0) <= U, (c, new)


def test_emulated_kernel_constant_values():
    assert abs(float(np.float32(1) - np.float32(0.9999)) - 1.00016594e-4) < 1e-12
    assert abs(float(np.float32(1) - np.float32(0.999)) - 9.99987e-4) < 1e-9
    assert abs(float(np.float32(1) - np.float32(0.9)) - 0.100000024) < 1e-9
