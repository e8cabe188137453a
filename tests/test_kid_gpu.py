"""The polynomial-kernel sums of csrc/kid.hip (vd_kid_sums) and v_diffusion.metrics.kid_score on the MI355X against the
definition evaluated in numpy (np.longdouble for the small shapes, row-blocked fp64 for the one large one).

Tolerance model of every sum (derived, not measured).  u = 2^-53, P the set of summed pairs, k(a, b) = (gamma <a, b> + coef0)^degree,
q_ij = gamma sum_k |x_ik y_jk| + |coef0|.  The kernel widens fp32 features to fp64, so every product is exact and only sums
round.  A d-term dot product, the affine map and the power carry at most degree (d + 4) u q_ij^degree per entry; the sum of |P|
entries carries at most |P| u sum_P q^degree.  Twice that is allowed, one share for the kernel and one for an fp64 reference:

    |S_gpu - S_ref| <= 2 (degree (d + 4) + |P|) u sum_P q_ij^degree

An MMD^2 = Sxx / (mx (mx - 1)) + Syy / (my (my - 1)) - 2 Sxy / (mx my) inherits, by the triangle inequality, the three bounds
divided by their pair counts (the cross one doubled), plus the host combination's own roundings: three divisions and two
additions on each side, at most 10 u (|Sxx| / (mx (mx - 1)) + |Syy| / (my (my - 1)) + 2 |Sxy| / (mx my)).
A bound that fails is a finding about the kernel; the constants are not to be enlarged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
L = np.longdouble
N_ROWS = 200


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make_features(n, d, seed, signed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(n, d)) * (0.25 + rng.random(d))
    return (z if signed else np.abs(z) + 0.5 * rng.random(d)).astype(np.float32)


def make_indices(n, subsets, m, seed):
    """[subsets, m] int32 rows without repeats; with three subsets, subset 1 holds one index at two positions"""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(n)[:m] for _ in range(subsets)]).astype(np.int32)
    if subsets > 1:
        idx[1, 1] = idx[1, 0]
    return idx


def ref_sums(x, y, ix, iy, degree, gamma, coef0):
    """(sums [subsets, 3], bounds [subsets, 3]) from the definition in np.longdouble; the bounds are the docstring's"""
    d = x.shape[1]
    gamma = 1.0 / d if gamma is None else gamma
    sums, bounds = np.zeros((ix.shape[0], 3)), np.zeros((ix.shape[0], 3))
    for s in range(ix.shape[0]):
        xs, ys = x[ix[s]].astype(L), y[iy[s]].astype(L)
        for kind, (a, b) in enumerate(((xs, xs), (ys, ys), (xs, ys))):
            k = (L(gamma) * (a @ b.T) + L(coef0)) ** degree
            q = (L(abs(gamma)) * (np.abs(a) @ np.abs(b).T) + L(abs(coef0))) ** degree
            pairs = a.shape[0] * b.shape[0]
            if kind < 2:                                             # equal POSITIONS are left out, equal indices are not
                np.fill_diagonal(k, 0)
                np.fill_diagonal(q, 0)
                pairs -= a.shape[0]
            sums[s, kind] = float(k.sum())
            bounds[s, kind] = 2.0 * (degree * (d + 4) + pairs) * U * float(q.sum())
    return sums, bounds


def ref_mmd2(sums, bounds, mx, my):
    """(per-subset MMD^2, its bound) from reference sums and their bounds"""
    w = np.array([1.0 / (mx * (mx - 1.0)), 1.0 / (my * (my - 1.0)), 2.0 / (float(mx) * my)])
    values = sums[:, 0] * w[0] + sums[:, 1] * w[1] - sums[:, 2] * w[2]
    return values, (bounds * w).sum(axis=1) + 10.0 * U * (np.abs(sums) * w).sum(axis=1)


def device_sums(x, y, ix, iy, degree=3, gamma=None, coef0=1.0, ld=None):
    from v_diffusion import _hip
    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        if ld is not None:
            wide = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)     # the padding is never read
            wide[:, :t.shape[1]] = t
            t = wide[:, :t.shape[1]]
            assert t.stride(0) == ld
        return t
    return _hip.kid_sums(up(x), up(y), ix, iy, degree, gamma, coef0)


def check(what, got, sums, bounds):
    got = got.cpu().numpy()
    ratio = np.abs(got - sums) / bounds
    print(f"{what}: worst |S_gpu - S_ref| / bound = {ratio.max():.3e} (relative error {np.max(np.abs(got - sums) / np.abs(sums)):.3e})")
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), f"{what}: off by {ratio.max():.3e} x the bound\n{got}\n{sums}"


# (mx, my): one tile with two rows, either side of the 64-row tile edge, two and three tiles (lower triangle + a rectangular XY)
# d: one K step, two (both LDS buffers), five (an odd count)
@pytest.mark.parametrize("subsets", [1, 3])
@pytest.mark.parametrize("d", [16, 32, 80])
@pytest.mark.parametrize("mx,my", [(2, 2), (63, 65), (64, 64), (65, 130), (130, 63)])
def test_sums_against_the_definition(mx, my, d, subsets):
    ix, iy = make_indices(N_ROWS, subsets, mx, 11 * mx + d), make_indices(N_ROWS, subsets, my, 13 * my + d + 1)
    for signed in (False, True):
        x, y = make_features(N_ROWS, d, 1000 + d, signed), make_features(N_ROWS, d, 2000 + d, signed)
        for degree in (1, 2, 3):
            sums, bounds = ref_sums(x, y, ix, iy, degree, None, 1.0)
            got = device_sums(x, y, ix, iy, degree)
            check(f"m = ({mx}, {my}) d = {d} subsets = {subsets} degree = {degree} {'signed' if signed else 'positive'}", got, sums, bounds)


def test_sums_at_the_inception_feature_length():
    d, m = 2048, 130
    x, y = make_features(N_ROWS, d, 5, False), make_features(N_ROWS, d, 6, True)
    ix, iy = make_indices(N_ROWS, 1, m, 7), make_indices(N_ROWS, 1, m, 8)
    sums, bounds = ref_sums(x, y, ix, iy, 3, None, 1.0)
    check("m = 130 d = 2048", device_sums(x, y, ix, iy, 3), sums, bounds)


def test_other_kernel_parameters_and_row_pitch():
    """gamma, coef0 (negative too) and degree up to 8 reach the kernel; with a row pitch above d the NaN padding is never read"""
    d = 48
    x, y = make_features(N_ROWS, d, 21, True), make_features(N_ROWS, d, 22, True)
    ix, iy = make_indices(N_ROWS, 3, 70, 23), make_indices(N_ROWS, 3, 66, 24)
    for degree, gamma, coef0 in ((3, 0.05, -0.5), (8, 0.01, 1.0), (1, 2.0, 0.0)):
        sums, bounds = ref_sums(x, y, ix, iy, degree, gamma, coef0)
        check(f"degree = {degree} gamma = {gamma} coef0 = {coef0}", device_sums(x, y, ix, iy, degree, gamma, coef0), sums, bounds)
    sums, bounds = ref_sums(x, y, ix, iy, 3, None, 1.0)
    got = device_sums(x, y, ix, iy, 3, ld=d + 12)
    check("ld = d + 12 with NaN padding", got, sums, bounds)
    assert np.array_equal(bits(got), bits(device_sums(x, y, ix, iy, 3)))


def test_identity_path_equals_the_gathered_path_bitwise():
    d = 32
    x, y = make_features(65, d, 31, False), make_features(130, d, 32, True)
    ax, ay = np.arange(65, dtype=np.int32)[None], np.arange(130, dtype=np.int32)[None]
    ident = device_sums(x, y, None, None)
    assert ident.shape == (1, 3)
    for ix, iy in ((ax, ay), (None, ay), (ax, None)):
        assert np.array_equal(bits(ident), bits(device_sums(x, y, ix, iy)))
    sums, bounds = ref_sums(x, y, ax, ay, 3, None, 1.0)
    check("identity", ident, sums, bounds)


def test_same_call_same_bits_and_swapped_sets_swap_the_sums():
    d = 80
    x, y = make_features(N_ROWS, d, 41, False), make_features(N_ROWS, d, 42, False)
    ix, iy = make_indices(N_ROWS, 3, 130, 43), make_indices(N_ROWS, 3, 65, 44)
    a, b = device_sums(x, y, ix, iy), device_sums(x, y, ix, iy)
    assert np.array_equal(bits(a), bits(b))
    s = device_sums(y, x, iy, ix)
    assert np.array_equal(bits(s[:, 0]), bits(a[:, 1])) and np.array_equal(bits(s[:, 1]), bits(a[:, 0]))


def test_kid_and_mmd_end_to_end():
    """the host combination against the same reference; features of another dtype on the host are accepted"""
    from v_diffusion.metrics import kid_score as K
    d = 32
    x, y = make_features(150, d, 51, False), make_features(120, d, 52, False)
    fx, fy = torch.from_numpy(x).double(), torch.from_numpy(y).half().float()     # fp64 on the host; fp32 values that fp16 holds
    y = fy.numpy()
    kid = K.kernel_inception_distance(fx, fy.half(), subsets=6, subset_size=70, seed=3, device=DEV)
    ix, iy = K.subset_indices(150, 120, 6, 70, seed=3)
    values, tol = ref_mmd2(*ref_sums(x, y, ix, iy, 3, None, 1.0), 70, 70)
    print("KID values: worst error / bound =", np.max(np.abs(kid.values - values) / tol))
    assert kid.values.dtype == np.float64 and kid.values.shape == (6,) and (np.abs(kid.values - values) <= tol).all()
    assert kid.mean == float(np.mean(kid.values)) and kid.std == float(np.std(kid.values))
    # explicit indices override the draw (other sizes per side, other kernel parameters)
    jx, jy = make_indices(150, 2, 66, 53), make_indices(120, 2, 40, 54)
    kid2 = K.kernel_inception_distance(fx, fy, degree=2, gamma=0.1, coef0=0.5, indices=(jx, jy), device=DEV)
    values2, tol2 = ref_mmd2(*ref_sums(x, y, jx, jy, 2, 0.1, 0.5), 66, 40)
    assert (np.abs(kid2.values - values2) <= tol2).all()
    # whole sets of different sizes
    ax, ay = np.arange(150, dtype=np.int32)[None], np.arange(120, dtype=np.int32)[None]
    whole, wtol = ref_mmd2(*ref_sums(x, y, ax, ay, 3, None, 1.0), 150, 120)
    got = K.polynomial_mmd(fx, fy, device=DEV)
    assert isinstance(got, float) and abs(got - whole[0]) <= wtol[0]


def test_sign_conventions():
    """two sets from one distribution: the mean estimate lies within three of its subset standard deviations of zero; a set shifted
    by 0.5 in every coordinate: clearly positive.  (The numpy reference alone passes both with these seeds: checked on the CPU.)"""
    from v_diffusion.metrics import kid_score as K
    d, n = 32, 400
    rng = np.random.default_rng(61)
    x, y = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    same = K.kernel_inception_distance(torch.from_numpy(x), torch.from_numpy(y), subsets=20, subset_size=64, seed=1, device=DEV)
    assert abs(same.mean) <= 3.0 * same.std, same
    far = K.kernel_inception_distance(torch.from_numpy(x), torch.from_numpy(y + np.float32(0.5)), subsets=20, subset_size=64, seed=1, device=DEV)
    assert far.mean > 3.0 * far.std and far.mean > 10.0 * abs(same.mean) and (far.values > 0).all(), (same, far)
    assert K.polynomial_mmd(torch.from_numpy(x), torch.from_numpy(y + np.float32(0.5)), device=DEV) > 0.0


def test_a_nan_row_spoils_exactly_the_subsets_that_draw_it():
    from v_diffusion.metrics import kid_score as K
    d, n, bad_row = 32, 150, 17
    x, y = make_features(n, d, 71, False), make_features(n, d, 72, False)
    rng = np.random.default_rng(73)
    others = np.array([r for r in range(n) if r != bad_row])
    ix = np.stack([rng.permutation(others)[:70] for _ in range(5)]).astype(np.int32)
    iy = make_indices(n, 5, 70, 74)                                    # (Y may draw row 17: only X's is NaN)
    ix[1, 69] = bad_row
    ix[3, 0] = bad_row
    clean = K.kernel_inception_distance(torch.from_numpy(x), torch.from_numpy(y), indices=(ix, iy), device=DEV).values
    xn = x.copy()
    xn[bad_row, 5] = np.nan
    spoiled = K.kernel_inception_distance(torch.from_numpy(xn), torch.from_numpy(y), indices=(ix, iy), device=DEV).values
    assert np.isfinite(clean).all()
    assert np.isnan(spoiled).tolist() == [False, True, False, True, False]
    keep = [0, 2, 4]
    assert np.array_equal(bits(spoiled[keep]), bits(clean[keep]))


def test_whole_sets_without_an_n_by_n_buffer():
    """n = 8192, d = 64: the peak allocation rises by less than an eighth of an n x n fp64 matrix over the inputs, and the value
    agrees with a row-blocked fp64 numpy evaluation (positive features: q_ij = the kernel argument itself)"""
    from v_diffusion.metrics import kid_score as K
    n, d = 8192, 64
    x, y = make_features(n, d, 81, False), make_features(n, d, 82, False)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    sums = np.zeros((1, 3))
    for r in range(0, n, 1024):
        for kind, (a, b) in enumerate(((x64, x64), (y64, y64), (x64, y64))):
            k = ((1.0 / d) * (a[r:r + 1024] @ b.T) + 1.0) ** 3
            if kind < 2:
                k[np.arange(k.shape[0]), r + np.arange(k.shape[0])] = 0.0
            sums[0, kind] += k.sum()
    pairs = np.array([n * (n - 1.0), n * (n - 1.0), float(n) * n])
    bounds = 2.0 * (3 * (d + 4) + pairs) * U * sums                   # sum_P q^3 = the sums themselves here
    want, tol = ref_mmd2(sums, bounds, n, n)
    fx, fy = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    K.polynomial_mmd(fx[:128], fy[:128], device=DEV)                   # library load and the cached workspace are not the subject
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = K.polynomial_mmd(fx, fy, device=DEV)
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak allocation rose by {rise} bytes (n x n fp64 = {8 * n * n}); MMD^2 = {got!r}, reference {want[0]!r}, bound {tol[0]:.3e}")
    assert rise < 8 * n * n // 8
    assert abs(got - want[0]) <= tol[0]


def test_domain_errors():
    from v_diffusion import _hip
    lib = _hip.lib()
    f = lambda n, d: torch.ones(n, d, device=DEV)
    idx = np.zeros((1, 4), dtype=np.int32)
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*multiple of 16"):
        _hip.kid_sums(f(8, 24), f(8, 24))
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*multiples of 4"):
        _hip.kid_sums(torch.ones(8, 18, device=DEV)[:, :16], f(8, 16))
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*2 <= mx"):
        _hip.kid_sums(f(1, 16), f(8, 16))
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*2 <= mx"):
        _hip.kid_sums(f(8, 16), f(8, 16), idx, idx[:, :1])
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*2 <= mx"):
        _hip.kid_sums(f(8, 16), f(8, 16), np.zeros((1, 9), dtype=np.int32), idx)     # more positions than rows
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*degree"):
        _hip.kid_sums(f(8, 16), f(8, 16), degree=9)
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*identity"):
        _hip.kid_sums(f(8, 16), f(8, 16), np.zeros((2, 4), dtype=np.int32), None)
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*16-byte aligned"):
        _hip.kid_sums(torch.ones(8 * 16 + 4, device=DEV)[1:1 + 8 * 16].view(8, 16), f(8, 16))
    with pytest.raises(ValueError, match="must lie in"):
        _hip.kid_sums(f(8, 16), f(8, 16), np.full((1, 4), 8, dtype=np.int32), idx)
    with pytest.raises(_hip.HipError):
        _hip.kid_sums(torch.ones(8, 16), f(8, 16))                                    # CPU tensor
    # a short workspace: the raw entry point with one byte less than it asks for
    x, out = f(130, 16), torch.zeros(1, 3, dtype=torch.float64, device=DEV)
    need = lib.vd_kid_ws_bytes(1, 130, 130)
    assert need == 8 * (6 + 6 + 9) and lib.vd_kid_ws_bytes(1, 1, 130) == 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    args = (x.data_ptr(), 130, 16, x.data_ptr(), 130, 16, 16, None, None, 1, 130, 130, 1.0 / 16, 1.0, 3, out.data_ptr(), ws.data_ptr())
    with pytest.raises(_hip.HipError, match="vd_kid_sums.*workspace"):
        _hip._check(lib.vd_kid_sums(*args, need - 1, _hip.stream()), "vd_kid_sums")
    _hip._check(lib.vd_kid_sums(*args, need, _hip.stream()), "vd_kid_sums")
    want = 130 * 129 * 2.0 ** 3                                                     # all-ones rows: k = (16 / 16 + 1)^3
    assert out.cpu().tolist() == [[want, want, 130 * 130 * 8.0]]
