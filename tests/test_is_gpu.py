"""The Inception Score kernels of csrc/kid.hip (vd_is_scores) and v_diffusion.metrics.inception_score on the MI355X against the
definition evaluated in numpy (np.longdouble).

Tolerance model (derived, not measured).  u = 2^-53, C classes, R rows in the split, p = softmax of a row (fp64, maximum
subtracted), pbar the split's mean row, log s = (1 / R) sum_i sum_c p_ic (log p_ic - log pbar_c).
  - l - max is exact.  exp and log are allowed two ulps = 4 u each.  Z = sum_c exp(l_c - max) has C terms: relative error at most
    (C + 4) u; p = exp / Z adds 4 u + u.  So p carries (C + 9) u, relatively.
  - log p = (l - max) - log Z: both parts have one sign, so nothing cancels: 4 u |log Z| + u |log p| <= 5 u |log p|.  (The
    perturbation of Z itself moves log p_ic and log pbar_c together and drops out of their difference to first order.)
  - S_c = sum_i p_ic has R terms: R u, relatively, on top of p's error; log pbar_c = log(S_c / R) adds u + 4 u |log pbar_c|.
  - the products, the sum over c (C terms), the sum over chunks and rows (R terms) and the division by R: (C + R + 3) u of the
    absolute terms.
Collecting, every term p (|log p| + |log pbar|) carries at most (C + R + 24) u of itself, counting C and R once each as the two
sums are nested, not stacked.  With M = (1 / R) sum_i sum_c p_ic (|log p_ic| + |log pbar_c|) and the same share again for the
reference:

    |log s_gpu - log s_ref| <= b = 2 (C + R + 24) u M,   i.e.   |s_gpu - s_ref| <= s_ref (e^b - 1 + 4 u)

(the last 4 u: the two ulps of the closing exp).  A split whose rows are all one-hot on one class has M = 0 and must give exactly 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
L = np.longdouble


def bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float64).view(np.int64)


def ref_scores(logits, splits):
    """(scores [splits], bounds [splits]) from the definition in np.longdouble"""
    n, classes = logits.shape
    scores, bounds = np.zeros(splits), np.zeros(splits)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(splits):
            rows = logits[k * n // splits:(k + 1) * n // splits].astype(L)
            r = rows.shape[0]
            a = rows - rows.max(axis=1, keepdims=True)
            e = np.exp(a)
            z = e.sum(axis=1, keepdims=True)
            p = e / z
            logp = a - np.log(z)
            logpbar = np.log(p.mean(axis=0, keepdims=True))
            mass = p > 0
            log_s = np.where(mass, p * (logp - logpbar), 0).sum() / r
            if np.isnan(p).any():
                log_s = L(np.nan)
            m = np.where(mass, p * (np.abs(logp) + np.abs(logpbar)), 0).sum() / r
            scores[k] = float(np.exp(log_s))
            bounds[k] = float(scores[k] * (np.expm1(2.0 * (classes + r + 24) * U * m) + 4.0 * U))
    return scores, bounds


def device_scores(logits, splits, ld=None):
    from v_diffusion import _hip
    t = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV)
    if ld is not None:
        wide = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)          # the padding is never read
        wide[:, :t.shape[1]] = t
        t = wide[:, :t.shape[1]]
        assert t.stride(0) == ld
    return _hip.is_scores(t, splits).cpu().numpy()


def check(what, got, want, bounds):
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bounds)
    print(f"{what}: scores {want.min():.6g} .. {want.max():.6g}, worst |s_gpu - s_ref| / bound = {ratio.max():.3e}")
    assert np.isfinite(got).all() and (err <= bounds).all(), f"{what}: off by {ratio.max():.3e} x the bound\n{got}\n{want}"


def make_logits(n, classes, seed):
    rng = np.random.default_rng(seed)
    return (3.0 * rng.normal(size=(n, classes)) + rng.normal(size=classes)).astype(np.float32)


# classes: below, at and above one wave of columns, and 1008 (four columns per thread, the last pass partial)
# (n, splits): one split; uneven splits; splits of several 64-row chunks (100 rows) and of 25 / 26 rows; (7, 5): splits of ONE row
@pytest.mark.parametrize("n,splits", [(7, 1), (10, 3), (257, 10), (1000, 10), (7, 5)])
@pytest.mark.parametrize("classes", [2, 10, 63, 64, 65, 1008])
def test_scores_against_the_definition(classes, n, splits):
    logits = make_logits(n, classes, 100 * classes + n)
    want, bounds = ref_scores(logits, splits)
    got = device_scores(logits, splits)
    check(f"classes = {classes} n = {n} splits = {splits}", got, want, bounds)
    if (n, splits) == (7, 5):
        assert np.abs(want[[0, 1, 3]] - 1.0).max() < 1e-15                       # a split of one row scores 1


def test_row_pitch_above_classes_and_the_module_entry():
    from v_diffusion.metrics.inception_score import inception_score
    logits = make_logits(300, 10, 5)
    want, bounds = ref_scores(logits, 4)
    got = device_scores(logits, 4, ld=13)
    check("ld = 13 with NaN padding", got, want, bounds)
    assert np.array_equal(bits(got), bits(device_scores(logits, 4)))
    res = inception_score(torch.from_numpy(logits).double(), splits=4, device=DEV)       # another dtype, on the host
    assert np.array_equal(bits(res.values), bits(got)) and res.values.dtype == np.float64
    assert res.mean == float(np.mean(got)) and res.std == float(np.std(got))
    half = torch.from_numpy(logits).half()
    want16, bounds16 = ref_scores(half.float().numpy(), 10)
    check("fp16 logits, default splits", inception_score(half.to(DEV)).values, want16, bounds16)


def test_large_logits_keep_the_one_hot_limit():
    classes, per = 10, 6
    n = classes * per
    logits = np.full((n, classes), -1e4, dtype=np.float32)
    logits[np.arange(n), np.arange(n) % classes] = 1e4                           # confident, evenly spread
    for splits in (1, 3):                                                        # 3: 20 rows each, two of every class
        want, bounds = ref_scores(logits, splits)
        check(f"one-hot rows, even classes, {splits} split(s)", device_scores(logits, splits), want, bounds)
        assert np.abs(want - classes).max() < 1e-12
    same = np.full((n, classes), -1e4, dtype=np.float32)
    same[:, 3] = 1e4                                                             # every row on class 3: M = 0, exactly 1
    assert device_scores(same, 2).tolist() == [1.0, 1.0]


def test_uniform_logits_score_one():
    for value in (0.0, -7.5, 1e4):
        logits = np.full((40, 65), value, dtype=np.float32)
        want, bounds = ref_scores(logits, 3)
        got = device_scores(logits, 3)
        check(f"all logits {value}", got, want, bounds)
        assert np.abs(want - 1.0).max() < 1e-15


def test_minus_infinity_logits_count_as_no_mass():
    logits = make_logits(90, 12, 9)
    logits[::3, 2] = -np.inf                                                     # some rows
    logits[7, [0, 1, 5]] = -np.inf
    logits[30:60, 4] = -np.inf                                                   # class 4 has no mass anywhere in split 1
    logits[60:, 6] = -200.0                                                      # a probability around 1e-90: tiny, not zero
    logits[60:, 7] = -2000.0                                                     # exp underflows to 0: an underflowed probability
    want, bounds = ref_scores(logits, 3)
    got = device_scores(logits, 3)
    check("-inf logits", got, want, bounds)


def test_a_nan_logit_spoils_only_its_split():
    logits = make_logits(200, 65, 13)
    clean = device_scores(logits, 4)
    logits[120, 64] = np.nan                                                     # split 2 = rows 100 .. 149
    got = device_scores(logits, 4)
    assert np.isnan(got).tolist() == [False, False, True, False]
    assert np.array_equal(bits(got[[0, 1, 3]]), bits(clean[[0, 1, 3]]))
    assert np.isnan(ref_scores(logits, 4)[0]).tolist() == [False, False, True, False]


def test_same_call_same_bits():
    logits = make_logits(1000, 1008, 17)
    assert np.array_equal(bits(device_scores(logits, 10)), bits(device_scores(logits, 10)))


def test_domain_errors():
    from v_diffusion import _hip
    lib = _hip.lib()
    with pytest.raises(_hip.HipError, match="vd_is_scores.*classes"):
        _hip.is_scores(torch.ones(4, 1, device=DEV), 1)
    with pytest.raises(_hip.HipError, match="vd_is_scores.*splits <= n"):
        _hip.is_scores(torch.ones(4, 10, device=DEV), 5)
    with pytest.raises(_hip.HipError, match="vd_is_scores.*splits"):
        _hip.is_scores(torch.ones(4, 10, device=DEV), 0)
    with pytest.raises(_hip.HipError):
        _hip.is_scores(torch.ones(4, 10), 1)                                     # CPU tensor
    x, scores = torch.zeros(130, 10, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    need = lib.vd_is_ws_bytes(130, 10, 2)
    assert need == 2 * 2 * 11 * 8 and lib.vd_is_ws_bytes(130, 1, 2) == 0 and lib.vd_is_ws_bytes(1, 10, 2) == 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    args = (x.data_ptr(), 130, 10, 10, 2, scores.data_ptr(), ws.data_ptr())
    with pytest.raises(_hip.HipError, match="vd_is_scores.*workspace"):
        _hip._check(lib.vd_is_scores(*args, need - 1, _hip.stream()), "vd_is_scores")
    _hip._check(lib.vd_is_scores(*args, need, _hip.stream()), "vd_is_scores")
    assert np.abs(scores.cpu().numpy() - 1.0).max() < 1e-14
