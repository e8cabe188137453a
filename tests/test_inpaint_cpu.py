"""Host side of the RePaint inpainting sampler (v_diffusion/inpaint.py): the resampling schedule, the jump and known-region coefficients
against their defining identities in fp64, the public names, and the refusals that need no GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref as R                                           # noqa: E402

import v_diffusion as vd                                          # noqa: E402

SWEEP = [(8, 1, 1), (8, 2, 3), (10, 3, 2), (5, 5, 4), (250, 10, 10), (4, 1, 2), (1, 1, 3), (7, 2, 2), (9, 4, 5)]
RTOL = 1e-6                      # the fp32 rounding of the returned values (2^-24 = 6e-8 each, a handful of them per identity)


def test_schedule_example_verbatim():
    assert vd.resampling_schedule(4, 1, 2) == [4, 3, 4, 3, 2, 3, 2, 1, 2, 1, 0]
    assert vd.resampling_schedule(4, jump_length=1, resamplings=2) == vd.resampling_schedule(4, 1, 2)


@pytest.mark.parametrize("T,j,r", SWEEP)
def test_schedule_properties(T, j, r):
    s = vd.resampling_schedule(T, j, r)
    assert s[0] == T and s[-1] == 0 and max(s) <= T and min(s) >= 0
    moves = [b - a for a, b in zip(s, s[1:])]
    assert set(moves) <= {-1, j}
    assert all(a != 0 for a, b in zip(s, s[1:]) if b > a)         # never up from 0
    assert s.index(0) == len(s) - 1                               # 0 is visited once, at the end
    P = len(range(j, T - j + 1, j))
    assert moves.count(-1) == T + (r - 1) * j * P
    assert sum(1 for d in moves if d > 0) == (r - 1) * P
    if r == 1:
        assert s == list(range(T, -1, -1))
    assert vd.resampling_schedule(T, j, 1) == list(range(T, -1, -1))
    # every jump leaves from a resampling point, each point exactly r - 1 times
    starts = [a for a, b in zip(s, s[1:]) if b > a]
    assert sorted(starts) == sorted(list(range(j, T - j + 1, j)) * (r - 1))


@pytest.mark.parametrize("args", [(0, 1, 1), (4, 0, 1), (4, 1, 0), (-3, 1, 1), (4.0, 1, 1), (4, 1.5, 1), (4, 1, "2"), (True, 1, 1)])
def test_schedule_refuses_bad_arguments(args):
    with pytest.raises(ValueError):
        vd.resampling_schedule(*args)


@pytest.mark.parametrize("T", (8, 1024))
@pytest.mark.parametrize("lim", (20.0, 6.0))
def test_jump_coefs_identities(lim, T):
    """a alpha_s = alpha_t and a^2 sigma_s^2 + b^2 = sigma_t^2 in fp64 from the fp32-rounded log-SNRs the coefficients are made from;
    a jump of j composes from j unit jumps"""
    fn = vd.get_logsnr_schedule("cosine", -lim, lim)
    l = fn(torch.arange(T + 1, dtype=torch.float64) / T).float().double()
    al, sg = R.alpha_sigma(l)
    close = lambda got, want: abs(got - want) <= RTOL * abs(want)
    pairs = [(i, j) for j in (1, 2, 3, T // 2, T) for i in (0, 1, T // 3, T - j) if 0 <= i and i + j <= T]
    for i, j in sorted(set(pairs)):
        a, b = vd.jump_coefs(fn, T, i, j)
        assert a == float(torch.tensor(a, dtype=torch.float32)) and b == float(torch.tensor(b, dtype=torch.float32))   # fp32 values
        assert close(a * float(al[i]), float(al[i + j])), (i, j)
        assert close(a * a * float(sg[i]) ** 2 + b * b, float(sg[i + j]) ** 2), (i, j)
        ra, rb = R.jump_weights(l[i], l[i + j])
        assert close(a, ra), (i, j)
        if j <= 3:                                              # the composition of j unit jumps: a = prod a_q, b^2 = sum of b_q^2 (prod of later a)^2
            ca, cb2 = 1.0, 0.0
            for q in range(i, i + j):
                ua, ub = vd.jump_coefs(fn, T, q, 1)
                ca, cb2 = ca * ua, cb2 * ua * ua + ub * ub
            assert close(ca, a) and close(cb2, b * b), (i, j)


def test_jump_coefs_leave_their_argument_alone_and_refuse_bad_indices():
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    rs = vd.get_logsnr_schedule("cosine", -20.0, 20.0, rescale=0.5)         # rewrites its argument in place: each call sees a fresh tensor
    assert vd.jump_coefs(rs, 8, 2, 3) == vd.jump_coefs(fn, 8, 2, 3) == vd.jump_coefs(rs, 8, 2, 3)
    assert vd.known_coefs(rs, 8, 5) == vd.known_coefs(fn, 8, 5)
    for bad in ((8, 7, 2), (8, -1, 1), (8, 0, 0), (0, 0, 1), (8, 1.0, 1)):
        with pytest.raises(ValueError):
            vd.jump_coefs(fn, *bad)
    for bad in ((8, 9), (8, -1), (8, 2.0)):
        with pytest.raises(ValueError):
            vd.known_coefs(fn, *bad)


def test_known_coefs():
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    assert vd.known_coefs(fn, 8, 0) == (1.0, 0.0)
    for T, i in ((8, 1), (8, 8), (1024, 300)):
        ak, bk = vd.known_coefs(fn, T, i)
        a, s = R.alpha_sigma(fn(torch.tensor([i / T], dtype=torch.float64)).float())
        assert ak == float(a.float()) and bk == float(s.float())
        assert abs(ak * ak + bk * bk - 1.0) <= RTOL
    # the log-SNR is the one _step_coefs rounds for the state the step lands on: the DDPM posterior of step i keeps alpha_i
    gd = vd.GaussianDiffusion(fn, 8, "v", "fixed_large", "snr_trunc", "mse")
    k8, _ = gd._step_coefs(3, use_ddim=True)
    al_t = vd.known_coefs(fn, 8, 4)
    ak, bk = vd.known_coefs(fn, 8, 3)
    # DDIM: c1 = sigma_s/sigma_t, and c1 alpha_t + c2 = alpha_s
    assert abs(k8[3] - bk / al_t[1]) <= RTOL * k8[3] and abs(k8[3] * al_t[0] + k8[4] - ak) <= RTOL * ak


def test_public_names_and_bindings():
    from v_diffusion import _hip
    for name in ("resampling_schedule", "known_coefs", "jump_coefs"):
        assert name in vd.__all__ and callable(getattr(vd, name))
    assert callable(_hip.inpaint_step) and callable(_hip.forward_jump)
    assert hasattr(vd.GaussianDiffusion, "p_sample_inpaint")
    assert vd.DistillationDiffusion.p_sample_inpaint is vd.GaussianDiffusion.p_sample_inpaint


class _Net:
    training = False

    def __call__(self, x, t, y):
        raise AssertionError("the network must not be called")


def _gd(var="fixed_large"):
    return vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), 8, "v", var, "snr_trunc", "mse", w_guide=0.0)


def test_cpu_tensors_raise_the_package_error():
    known, mask = torch.zeros((2, 3, 4, 4)), torch.zeros((1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        _gd().p_sample_inpaint(_Net(), known, mask, seed=1)
    with pytest.raises(RuntimeError, match="MI355X"):
        _gd().p_sample_inpaint(_Net(), known, mask, seed=1, device="cpu")
    with pytest.raises(NotImplementedError):
        _gd("learned").p_sample_inpaint(_Net(), known, mask, seed=1)


def test_shape_and_range_errors_come_before_any_launch():
    gd, known = _gd(), torch.zeros((2, 3, 4, 4))
    ok = torch.zeros((1, 1, 4, 4))
    for mask in (torch.zeros((3, 1, 4, 4)), torch.zeros((2, 2, 4, 4)), torch.zeros((2, 1, 4, 5)), torch.zeros((4, 4)),
                 torch.full((1, 1, 4, 4), 1.5), torch.full((1, 1, 4, 4), -0.1), torch.full((1, 1, 4, 4), float("nan")),
                 torch.zeros((1, 1, 4, 4), dtype=torch.int32)):
        with pytest.raises(ValueError, match="mask"):
            gd.p_sample_inpaint(_Net(), known, mask, seed=1)
    with pytest.raises(ValueError, match="known"):
        gd.p_sample_inpaint(_Net(), torch.zeros((3, 4, 4)), ok, seed=1)
    for start in (0, 9, -1, 2.0):
        with pytest.raises(ValueError, match="start"):
            gd.p_sample_inpaint(_Net(), known, ok, seed=1, start=start)
    for kw in (dict(jump_length=0), dict(resamplings=0), dict(jump_length=1.5)):
        with pytest.raises(ValueError):
            gd.p_sample_inpaint(_Net(), known, ok, seed=1, **kw)
