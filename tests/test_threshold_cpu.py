"""Host side of dynamic thresholding in the DPM-Solver++ sampler: the rank rule against numpy's "higher" quantile, the argument checks,
the properties of the float64 restatement the GPU tests are held to (tests/threshold_ref.py), and the public names.  No kernel is
launched here."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import threshold_ref as T                                         # noqa: E402

SIZES = (1, 2, 75, 192, 972, 3072, 12288, 49152)
QUANTILES = (0.5, 0.9, 0.95, 0.995, 0.999, 1.0)


def _gd(T_=4, **kw):
    import v_diffusion as vd
    return vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine"), T_, "v", "fixed_large", "snr_trunc", "mse", w_guide=0.3, p_uncond=0.0, **kw)


@pytest.mark.parametrize("N", SIZES)
def test_rank_is_numpys_higher_quantile(N):
    """on a permutation of 0 .. N-1 the "higher" quantile IS its own rank"""
    import v_diffusion as vd
    perm = np.random.default_rng(N).permutation(N).astype(np.float64)
    for q in QUANTILES:
        want = int(np.quantile(perm, q, method="higher"))
        assert vd.threshold_rank(N, q) == want == T.rank(N, q), (N, q)
        assert isinstance(vd.threshold_rank(N, q), int) and 0 <= want < N
    assert vd.threshold_rank(N, 1.0) == N - 1
    assert vd.threshold_rank(N, 1e-300) == min(N - 1, 1)           # any positive quantile of two or more elements is above the minimum


def test_argument_checks():
    import v_diffusion as vd
    net = lambda x, t, y: x
    for q in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="quantile"):
            vd.threshold_rank(75, q)
        with pytest.raises(ValueError, match="quantile"):
            _gd().p_sample_solver(net, (1, 3, 4, 4), clip_denoised="dynamic", dynamic_quantile=q)
    with pytest.raises(ValueError, match="N must be"):
        vd.threshold_rank(0, 0.5)
    for m in (0.999, 0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match=">= 1"):
            _gd().p_sample_solver(net, (1, 3, 4, 4), clip_denoised="dynamic", dynamic_max=m)
        with pytest.raises(ValueError, match=">= 1"):
            vd.dynamic_threshold(torch.zeros(2, 3), max_value=m)
    with pytest.raises(ValueError, match="clip_denoised"):
        _gd().p_sample_solver(net, (1, 3, 4, 4), clip_denoised="static")
    with pytest.raises(ValueError, match="quantile"):
        vd.dynamic_threshold(torch.zeros(2, 3), quantile=0.0)
    with pytest.raises(ValueError, match="fp32"):
        vd.dynamic_threshold(torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="non-empty"):
        vd.dynamic_threshold(torch.zeros(0, 3))
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path, as everywhere else here
        _gd().p_sample_solver(net, (1, 3, 4, 4), clip_denoised="dynamic", device="cpu")
    with pytest.raises(RuntimeError, match="MI355X|CPU tensor"):
        vd.dynamic_threshold(torch.zeros(2, 3))
    # the static modes are not checked against the dynamic arguments: they do not use them
    with pytest.raises(RuntimeError, match="MI355X"):
        _gd().p_sample_solver(net, (1, 3, 4, 4), clip_denoised=True, dynamic_quantile=7.0, device="cpu")
    assert vd.DistillationDiffusion.p_sample_solver is vd.GaussianDiffusion.p_sample_solver


def _draw(B, N, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, N), generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize("N", (1, 2, 75, 972))
def test_properties_of_the_restatement(N):
    for q in QUANTILES:
        r = T.rank(N, q)
        for scale in (0.2, 1.0, 4.0):
            g = _draw(4, N, 7 * N + int(100 * q), scale)
            gp, s = T.threshold(g, r)
            raw = T.s_raw(g, r)
            assert bool((s >= 1.0).all()) and bool((gp.abs() <= 1.0).all())
            assert torch.equal(s, raw.clamp(min=1.0))
            for b in range(g.shape[0]):
                if raw[b] <= 1.0:                                   # below the data range: the plain clamp
                    assert torch.equal(gp[b], g[b].clamp(-1.0, 1.0))
                assert int((g[b].abs() > s[b]).sum()) <= N - 1 - r   # strictly clamped: only ranks above r
                if raw[b] > 1.0:
                    assert bool((gp[b].abs() == 1.0).any())          # the element that holds s_raw maps to +-1
            if q == 1.0:                                            # a pure rescale
                m = g.abs().amax(dim=1, keepdim=True).clamp(min=1.0)
                assert torch.equal(gp, g / m)
            cap, sc = T.threshold(g, r, s_max=1.5)
            assert bool((sc <= 1.5).all()) and bool((sc >= 1.0).all()) and bool((cap.abs() <= 1.0).all())
            one, s1 = T.threshold(g, r, s_max=1.0)                  # s_max = 1: the static clip
            assert torch.equal(one, g.clamp(-1.0, 1.0)) and bool((s1 == 1.0).all())


def test_restated_step_and_chain_agree_with_the_solver_restatement():
    """with s_max = 1 and no guidance the thresholded step is solver_ref's clipped step, and a chain of them its clipped chain"""
    import solver_ref as R
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    table, t_net = vd.solver_coefs(fn, 6, order=2, model_out_type="v", w_guide=0.0)
    x = _draw(2, 48, 3, 1.0).reshape(2, 3, 4, 4)
    net = lambda z, t, y: 0.4 * z + 0.3 * torch.tanh(z)
    r = T.rank(48, 0.995)
    assert torch.equal(T.chain_dyn(net, x, table, t_net, r, s_max=1.0), R.chain(net, x, table, t_net, clip=True))
    assert not torch.equal(T.chain_dyn(net, x, table, t_net, r), R.chain(net, x, table, t_net, clip=False))
    out, hist = _draw(2, 48, 4, 0.8).reshape(2, 3, 4, 4), _draw(2, 48, 5, 0.7).reshape(2, 3, 4, 4)
    xn, gp, s = T.step_dyn(table[3], x, out, hist, False, False, r, 1.0)
    g = R.guided_x0(lambda z, t, y: out, x, None, torch.ones(2), table[3].double(), clip=True)
    assert torch.equal(gp, g) and torch.equal(xn, R.step(x, g, hist, table[3].double())) and bool((s == 1.0).all())


def test_the_two_entries_have_public_names_and_wrappers():
    """(declarations and ctypes signatures of the entry points: tests/test_host_cpu.py pins the whole C ABI)"""
    import v_diffusion as vd
    from v_diffusion import _hip
    for name in ("threshold_rank", "dynamic_threshold"):
        assert name in vd.__all__ and callable(getattr(vd, name))
    assert callable(_hip.abs_kth_rows) and callable(_hip.solver_step_dyn)
    assert math.isinf(vd.solver._threshold_max(None))
