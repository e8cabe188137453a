"""Image inversion without a GPU (v_diffusion/invert.py): the float64 restatement of tests/invert_ref.py held to the properties the
feature rests on -- inversion then replay reconstructs, for any network; the ascending solver rows undo the descending ones; encoding
then decoding converges on a problem with a known solution; slerp's ends, norm and lerp branch -- and the host side of the package:
``encode_coefs`` against the definitions, ``solver_coefs`` unchanged, the public names and every refusal that comes before a launch.
Every bound here was reasoned for the restatement in fp64 on the CPU.  No kernel is launched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import invert_ref as R                                            # noqa: E402
import solver_ref as S                                            # noqa: E402

import v_diffusion as vd                                          # noqa: E402

F64 = torch.float64
U32 = 2.0 ** -24                                                  # relative rounding of one fp32 slot
MOTS = ("v", "eps", "x0", "both")
W_GUIDE = 1.5


def cosine(lim=20.0):
    return vd.get_logsnr_schedule("cosine", -lim, lim)


def _gd(T=8, mot="v", var="fixed_large", w=0.0, fn=None, **kw):
    return vd.GaussianDiffusion(fn or cosine(), T, mot, var, "snr_trunc", "mse", w_guide=w, p_uncond=0.0, **kw)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def _ulp32(x):
    x = torch.as_tensor(x).float().abs()
    return float(torch.nextafter(x, torch.full_like(x, float("inf"))) - x)


# ------------------------------------------------------------------------------------------------ noise-space inversion
def _invert_and_replay(T, var, mot, cfg, start, y_replay=None, zero_residual=False):
    gd = _gd(T, mot, var, W_GUIDE if cfg else 0.0)
    Tc = T if start is None else start
    shape = (2, 3, 5, 5)
    x0 = rnd(shape, 3, 0.6).clamp(-1, 1)
    y = torch.tensor([1.0, 4.0], dtype=F64) if cfg else None
    eps = [rnd(shape, 100 + i) for i in range(Tc)]
    row = lambda i: R.ddpm_row(vd, gd, i)
    net = R.Stub(both=mot == "both")
    start_x, maps = R.invert(net, x0, row, Tc, eps, y, mot == "both", cfg)
    if zero_residual:
        maps = [torch.zeros_like(maps[0])] + maps[1:]
    back = R.replay(net, start_x, row, maps, y if y_replay is None else y_replay, mot == "both", cfg)
    return x0, start_x, maps, back


@pytest.mark.parametrize("start", (None, 2), ids=("full", "start2"))
@pytest.mark.parametrize("cfg", (False, True), ids=("plain", "guided"))
@pytest.mark.parametrize("mot", MOTS)
@pytest.mark.parametrize("var", ("fixed_small", "fixed_large"))
@pytest.mark.parametrize("T", (4, 50))
def test_inversion_then_replay_reconstructs(T, var, mot, cfg, start):
    """every step of the replay re-forms the mean the inversion subtracted, from the same state: the chain returns x_0 up to the fp64
    rounding of (x - mu)/s * s + mu per step, whatever the network"""
    x0, start_x, maps, back = _invert_and_replay(T, var, mot, cfg, start)
    Tc = T if start is None else start
    assert len(maps) == Tc and all(m.shape == x0.shape for m in maps) and start_x.shape == x0.shape
    err = float((back - x0).abs().max())
    assert err <= 1e-12 * float(x0.abs().max()), err


def test_another_label_is_an_edit_and_the_residual_is_the_last_map():
    x0, _, maps, back = _invert_and_replay(4, "fixed_large", "v", True, None)
    _, _, _, edit = _invert_and_replay(4, "fixed_large", "v", True, None, y_replay=torch.tensor([2.0, 7.0], dtype=F64))
    assert float((edit - x0).abs().max()) > 1e-3                 # the label moves the image
    _, _, _, dropped = _invert_and_replay(4, "fixed_large", "v", True, None, zero_residual=True)
    assert torch.equal(dropped + 1.0 * maps[0], back)             # the last step adds 1.0 * maps[0] to the prediction and nothing else
    assert float((x0 - dropped - maps[0]).abs().max()) <= 1e-12 and float(maps[0].abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ encode_coefs
@pytest.mark.parametrize("spacing", ("time", "logsnr"))
@pytest.mark.parametrize("T", (1, 2, 8, 50))
def test_encode_rows_against_the_definitions(T, spacing):
    """slots 3, 4 (order 1) against alpha, sigma written out in fp64 from the fp32-rounded log-SNRs, to 1 fp32 ulp: fp64 values rounded
    once; slot 5 of order 2 likewise; the prediction weights and the network time are those of the state the step starts from"""
    fn = cosine()
    table, t_net = vd.encode_coefs(fn, T, order=1, spacing=spacing, model_out_type="both", w_guide=0.3)
    second, t2 = vd.encode_coefs(fn, T, order=2, spacing=spacing, model_out_type="both", w_guide=0.3)
    down, t_down = vd.solver_coefs(fn, T, order=1, spacing=spacing, model_out_type="both", w_guide=0.3)
    assert table.shape == (T, 8) and table.dtype == torch.float32 and t_net.shape == (T,) and t_net.dtype == F64
    assert torch.equal(t_net, t2) and torch.equal(table[:, :5], second[:, :5]) and torch.equal(table[:, 6:], second[:, 6:])
    assert bool((table[:, 5] == 0).all()) and float(second[0, 5]) == 0.0
    tau = [0.0] + t_down.tolist()
    assert t_net.tolist() == tau[:-1]                              # the time of the state the step starts from
    l = [float(fn(torch.tensor([v], dtype=F64)).float()) for v in tau]
    for i in range(T):
        c1, c2, rho = R.encode_weights(l[i], l[i + 1], l[i - 1] if i else None)
        assert c2 < 0 < c1 and (i == 0 or rho > 0)
        assert abs(float(table[i, 3]) - c1) <= _ulp32(c1) and abs(float(table[i, 4]) - c2) <= _ulp32(c2), (i, table[i], c1, c2)
        assert abs(float(second[i, 5]) - c2 * rho) <= _ulp32(c2 * rho), (i, float(second[i, 5]), c2 * rho)
        want = [float(torch.tensor(v, dtype=F64).float()) for v in S.x0_weights(l[i], "both")]
        assert all(abs(g - w_) <= _ulp32(w_) for g, w_ in zip(table[i, :3].tolist(), want)), (i, table[i], want)
        assert float(table[i, 6]) == float(torch.tensor(0.3).float()) and float(table[i, 7]) == 0.0


@pytest.mark.parametrize("lim", (20.0, 6.0))
@pytest.mark.parametrize("T", (2, 8, 50))
def test_ascending_rows_undo_the_descending_rows(T, lim):
    """order 1, rows i >= 1 (row 0 of ``solver_coefs`` is the prediction (0, 1, 0), not a step): c1_up c1_down = 1 and
    c2_down + c1_down c2_up = 0.  Before rounding both hold to fp64; each slot carries a relative rounding of at most 2^-24, so the
    product is off 1 by at most 2 * 2^-24 (1 + 2^-24), and the sum by at most 2^-24 (|c2_down| + 2 |c1_down c2_up|), first order --
    bounds with 1 % headroom for the second-order terms and the fp64 evaluation."""
    fn = cosine(lim)
    up, _ = vd.encode_coefs(fn, T, order=1)
    down, _ = vd.solver_coefs(fn, T, order=1)
    up, down = up.double(), down.double()
    for i in range(1, T):
        assert abs(float(up[i, 3] * down[i, 3]) - 1.0) <= 2.02 * U32, i
        bound = 1.01 * U32 * (abs(float(down[i, 4])) + 2.0 * abs(float(down[i, 3] * up[i, 4])))
        assert abs(float(down[i, 4] + down[i, 3] * up[i, 4])) <= bound, (i, float(down[i, 4] + down[i, 3] * up[i, 4]), bound)


# rows of solver_coefs(cosine +-20, 8 steps, order 2, "v", w_guide 0.3) and of (..., spacing "logsnr", "both") on the commit before
# v_diffusion/invert.py existed
PINNED_TIME = {0: [0.9807786345481873, -0.19512371718883514, 0.0, 0.0, 1.0, 0.0, 0.30000001192092896, 0.0],
               3: [0.7071067690849304, -0.7071067690849304, 0.0, 0.7857083082199097, 0.27588364481925964, 0.13794182240962982,
                   0.30000001192092896, 0.0],
               7: [4.539993096841499e-05, -1.0, 0.0, 0.9807786345481873, 0.19507919251918793, 0.0, 0.30000001192092896, 0.0]}
PINNED_LOGSNR_5 = [0.0067377942614257336, 0.9999545812606812, -0.006737641058862209, 0.9966706037521362, 0.07509448379278183,
                   0.037547241896390915, 0.30000001192092896, 0.0]


def test_solver_coefs_is_unchanged():
    """``encode_coefs`` shares ``solver_coefs``'s grid and checks: the descending table has the values it had, and building an ascending
    one in between changes nothing (also with a schedule that rewrites its argument)"""
    fn = cosine()
    before = vd.solver_coefs(fn, 8, order=2, spacing="time", model_out_type="v", w_guide=0.3)
    for i, row in PINNED_TIME.items():
        assert before[0][i].double().tolist() == row, i
    ls = vd.solver_coefs(fn, 8, order=2, spacing="logsnr", model_out_type="both", w_guide=0.3)
    assert ls[0][5].double().tolist() == PINNED_LOGSNR_5
    rs = vd.get_logsnr_schedule("cosine", -20.0, 20.0, rescale=0.5)
    before_rs = vd.solver_coefs(rs, 8, order=2)
    for f_ in (fn, rs):
        vd.encode_coefs(f_, 8, order=2, spacing="logsnr")
        vd.encode_coefs(f_, 8, order=1)
    after, after_rs = vd.solver_coefs(fn, 8, order=2, spacing="time", model_out_type="v", w_guide=0.3), vd.solver_coefs(rs, 8, order=2)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(before_rs[0], after_rs[0]) and torch.equal(before_rs[1], after_rs[1])
    up_rs, t_rs = vd.encode_coefs(rs, 8)
    assert t_rs.tolist() == [0.5 * i / 8 for i in range(8)]       # the time as the schedule left it
    assert torch.equal(up_rs, vd.encode_coefs(fn, 8)[0])


# ------------------------------------------------------------------------------------------------ encode -> decode, known solution
def gaussian_round_trip(T, order, run=None):
    """the exactly solvable problem of the solver tests (cosine schedule on [-6, 6], uniform log-SNR steps, data N(0, 2^2), the optimal
    linear denoiser as an x0-network, no clip): encode x(tau_0) to the latent, decode it back down to tau_1, and compare with the
    encoder's own state at tau_1, relative.  tau_1 is the last index at which both chains hold a STATE: the decoder's final row
    returns the x0 prediction instead, which on this schedule (logsnr(0) = 6) differs from the state at tau_0 by 6e-4 whatever T."""
    fn = cosine(6.0)
    _, net = S.gaussian_problem(fn)
    x0 = torch.tensor([1.0, -0.7, 0.25], dtype=F64).reshape(1, 3, 1, 1)
    up, t_up = vd.encode_coefs(fn, T, order=order, spacing="logsnr", model_out_type="x0")
    down, t_down = vd.solver_coefs(fn, T, order=order, spacing="logsnr", model_out_type="x0")
    latent = R.solver_chain(net, x0, up.double(), t_up, range(T))
    x1_back = R.solver_chain(net, latent, down.double(), t_down, reversed(range(1, T)))
    x1 = R.solver_chain(net, x0, up.double(), t_up, range(1))
    return float(((x1_back - x1).abs() / x1.abs()).max())


def test_round_trip_converges_on_the_gaussian_problem():
    """Measured with the restatement in fp64 (T = 16, 32, 64): order 1 1.693e-1, 8.858e-2, 4.532e-2 (ratios per doubling 1.911, 1.954);
    order 2 1.111e-3, 1.993e-4, 4.565e-5 (ratios 5.575, 4.366).  Asserted: monotone, and each ratio at least 75 % of its measured value."""
    measured = {1: (1.911, 1.954), 2: (5.575, 4.366)}
    for order in (1, 2):
        e = [gaussian_round_trip(T, order) for T in (16, 32, 64)]
        r = (e[0] / e[1], e[1] / e[2])
        print(f"[encode -> decode round trip, order {order}] {e[0]:.3e} {e[1]:.3e} {e[2]:.3e} (ratios {r[0]:.3f} {r[1]:.3f})")
        assert e[0] > e[1] > e[2], e
        assert r[0] >= 0.75 * measured[order][0] and r[1] >= 0.75 * measured[order][1], r


# ------------------------------------------------------------------------------------------------ slerp restatement
def test_slerp_ends_norm_and_lerp_branch():
    a, b = rnd((3, 4, 5), 1), rnd((3, 4, 5), 2)
    eps64 = 2.0 ** -52
    o0, wa0, wb0 = R.slerp(a, b, 0.0)
    o1, wa1, wb1 = R.slerp(a, b, 1.0)
    assert bool(((o0 - a).abs() <= eps64 * a.abs()).all()) and bool(((o1 - b).abs() <= eps64 * b.abs()).all())    # within 1 ulp
    # equal norms: |out|^2 = (wa^2 + wb^2 + 2 wa wb cos w) |a|^2 = |a|^2
    bn = b * (a.reshape(3, -1).norm(dim=1) / b.reshape(3, -1).norm(dim=1)).reshape(3, 1, 1)
    for f in (0.25, 0.5, torch.tensor([0.1, 0.6, 0.9], dtype=F64)):
        out, _, _ = R.slerp(a, bn, f)
        n_out, n_a = out.reshape(3, -1).norm(dim=1), a.reshape(3, -1).norm(dim=1)
        assert float(((n_out - n_a).abs() / n_a).max()) <= 1e-12
    # a generic pair takes the spherical weights, which are not the linear ones
    _, wa, wb = R.slerp(a, b, 0.3)
    assert float((wa - 0.7).abs().min()) > 1e-3 and float((wa + wb).min()) > 1.0
    # parallel, antiparallel and zero inputs take the lerp weights
    zero = torch.zeros_like(a)
    for other in (2.0 * a, -0.5 * a, zero):
        for x, y in ((a, other), (other, a)):
            out, wa, wb = R.slerp(x, y, 0.3)
            assert wa.tolist() == [0.7] * 3 and wb.tolist() == [0.3] * 3
            assert torch.equal(out, 0.7 * x + 0.3 * y)
    per = torch.tensor([0.0, 0.5, 1.0], dtype=F64)
    out, wa, wb = R.slerp(a, 2.0 * a, per)
    assert wa.tolist() == [1.0, 0.5, 0.0] and wb.tolist() == [0.0, 0.5, 1.0]


# ------------------------------------------------------------------------------------------------ names and refusals
def test_public_names_and_bindings():
    from v_diffusion import _hip
    for name in ("encode_coefs", "slerp"):
        assert name in vd.__all__ and callable(getattr(vd, name))
    assert callable(_hip.noise_extract) and callable(_hip.slerp_rows)
    for name in ("p_invert_noise", "p_sample_replay", "p_encode"):
        assert getattr(vd.DistillationDiffusion, name) is getattr(vd.GaussianDiffusion, name)
    import inspect
    assert "use_ddim" not in inspect.signature(vd.GaussianDiffusion.p_invert_noise).parameters
    assert "1.5 GB" in vd.GaussianDiffusion.p_invert_noise.__doc__ and "2^-24" in vd.GaussianDiffusion.p_encode.__doc__


class _Net:
    training = False

    def __call__(self, x, t, y):
        raise AssertionError("the network must not be called")


X = torch.zeros((2, 3, 4, 4))


def _plateau(t):
    """log-SNR 10, 10, 0, 0, -10 on the 4-step grid: the steps landing on 2 (and on 0) join equal log-SNRs, so their noise scale is 0"""
    return 10.0 - 20.0 * torch.floor(t * 2.0) / 2.0


def test_refusals_come_before_any_launch():
    net, maps = _Net(), torch.zeros((8,) + tuple(X.shape))
    for gd, exc, pat in ((_gd(var="learned"), NotImplementedError, "learned"), (_gd(x0eps_coef=True), NotImplementedError, "x0eps_coef")):
        with pytest.raises(exc, match=pat):
            gd.p_invert_noise(net, X, seed=1)
        with pytest.raises(exc, match=pat):
            gd.p_sample_replay(net, X, maps)
        with pytest.raises(exc, match=pat):
            gd.p_encode(net, X)
    gd = _gd()
    for start in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="start"):
            gd.p_invert_noise(net, X, seed=1, start=start)
    flat = _gd(T=4, fn=_plateau)
    with pytest.raises(ValueError, match="noise_scale"):
        flat.p_invert_noise(net, X, seed=1)
    with pytest.raises(ValueError, match="noise_scale"):
        flat.p_sample_replay(net, X, torch.zeros((4,) + tuple(X.shape)))
    for bad in (torch.zeros((8, 2, 3, 4, 5)), torch.zeros((8, 3, 3, 4, 4)), torch.zeros((2, 3, 4, 4)), torch.zeros((9,) + tuple(X.shape)),
                torch.zeros((0,) + tuple(X.shape)), None):
        with pytest.raises(ValueError, match="maps"):
            gd.p_sample_replay(net, X, bad)
    for call in (lambda x: gd.p_invert_noise(net, x, seed=1), lambda x: gd.p_sample_replay(net, x, maps), lambda x: gd.p_encode(net, x)):
        with pytest.raises(ValueError, match="B, C, H, W"):
            call(torch.zeros((3, 4, 4)))
    for kw in (dict(order=0), dict(order=3), dict(steps=0), dict(stop=0), dict(stop=9), dict(stop=2.0), dict(spacing="karras")):
        with pytest.raises(ValueError):
            gd.p_encode(net, X, **kw)
    for order in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            vd.encode_coefs(cosine(), 4, order=order)
    with pytest.raises(ValueError, match="steps"):
        vd.encode_coefs(cosine(), 0)


def test_cpu_tensors_raise_the_package_error():
    gd, net = _gd(), _Net()
    maps = torch.zeros((8,) + tuple(X.shape))
    for call in (lambda **kw: gd.p_invert_noise(net, X, seed=1, **kw), lambda **kw: gd.p_sample_replay(net, X, maps, **kw),
                 lambda **kw: gd.p_encode(net, X, **kw)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
        with pytest.raises(RuntimeError, match="MI355X"):
            call(device="cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        vd.slerp(X, X + 1.0, 0.5)
    for a, b, f in ((X, torch.zeros((2, 3, 4, 5)), 0.5), (X, X.double(), 0.5), (X, X, torch.zeros(3)), (X, X, "half"), (X, X, None),
                    (torch.zeros(()), torch.zeros(()), 0.5), (torch.zeros((0, 3)), torch.zeros((0, 3)), 0.5)):
        with pytest.raises(ValueError):
            vd.slerp(a, b, f)
