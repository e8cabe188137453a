"""Host math of post-hoc EMA (v_diffusion/phema.py) against tests/phema_ref.py: widths, rates, inner products, weights, the reconstruction
recipe and the snapshot format.  No kernel is launched here."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phema_ref as R                                              # noqa: E402

SIGMAS = (0.05, 0.10)                                             # the default tracked pair


def P():
    import v_diffusion
    from v_diffusion import phema
    for name in ("sigma_rel_to_gamma", "gamma_to_sigma_rel", "power_ema_rate", "profile_dot", "solve_weights", "posthoc_ema"):
        assert getattr(v_diffusion, name) is getattr(phema, name) and name in v_diffusion.__all__
    return phema


def test_width_round_trip_and_quoted_values():
    p = P()
    for s in (0.01, 0.05, 0.075, 0.10, 0.15, 0.25):
        g = p.sigma_rel_to_gamma(s)
        assert g > 0 and abs(p.gamma_to_sigma_rel(g) - s) <= 1e-12 * s
        assert abs(p.sigma_rel_to_gamma(p.gamma_to_sigma_rel(g)) - g) <= 1e-12 * max(g, 1.0)
        assert abs(g - R.gamma_of(s)) <= 1e-9 * g                  # the bisection of the restatement
    for s, g in ((0.05, 16.9722), (0.075, 10.2891), (0.10, 6.9372), (0.15, 3.5579)):
        assert abs(p.sigma_rel_to_gamma(s) - g) < 5e-5, (s, p.sigma_rel_to_gamma(s))
    for bad in (0.0, -0.1, 0.2886, 12 ** -0.5, 0.3, 1.0):
        with pytest.raises(ValueError):
            p.sigma_rel_to_gamma(bad)


def test_rate_against_50_digit_decimal():
    import decimal
    p = P()
    for s in SIGMAS:
        g = p.sigma_rel_to_gamma(s)
        last = 2.0
        for t in (1, 2, 3, 10, 1000, 10 ** 6, 10 ** 9):
            r = p.power_ema_rate(t, g)
            assert isinstance(r, float)
            want = R.rate_decimal(t, g)
            rel = abs((decimal.Decimal(r) - want) / want)
            print(f"sigma_rel {s} t {t}: rate {r!r}, relative error {float(rel) * 2 ** 52:.2f} x 2^-52")
            assert rel <= decimal.Decimal(4 * 2.0 ** -52), (s, t, r)
            assert r < last
            last = r
        assert p.power_ema_rate(1, g) == 1.0
        rs = [p.power_ema_rate(t, g) for t in range(1, 400)]
        assert all(a > b for a, b in zip(rs, rs[1:]))
    with pytest.raises(ValueError):
        p.power_ema_rate(0, 5.0)


def test_profile_dot_against_quadrature():
    p = P()
    ga, gb = (p.sigma_rel_to_gamma(s) for s in SIGMAS)
    for ta, tb in ((100.0, 350.0), (200.0, 200.0), (512.0, 48.0)):
        for g1, g2 in ((ga, gb), (gb, ga), (ga, ga), (gb, gb)):
            got = float(p.profile_dot(ta, g1, tb, g2))
            quad = R.dot_simpson(ta, g1, tb, g2)
            assert abs(got - quad) <= 1e-8 * quad, (ta, tb, g1, g2, got, quad)
            assert abs(got - R.dot_closed(ta, g1, tb, g2)) <= 1e-12 * got
            assert got == float(p.profile_dot(tb, g2, ta, g1))     # symmetric in its argument pairs
    t = np.array([16.0, 32.0, 48.0])
    A = p.profile_dot(t[:, None], ga, t[None, :], gb)              # vectorised: broadcasting as numpy does
    assert A.shape == (3, 3)
    for i in range(3):
        for j in range(3):
            assert A[i, j] == float(p.profile_dot(t[i], ga, t[j], gb))


def _snapshot_grid(p, times):
    gs = [p.sigma_rel_to_gamma(s) for s in SIGMAS]
    return [t for t in times for _ in gs], [g for _ in times for g in gs]


def test_weights_one_hot_and_unit_invariance():
    p = P()
    st, sg = _snapshot_grid(p, range(16, 129, 16))
    for i in (0, 5, len(st) - 1):
        x = p.solve_weights(st, sg, st[i], sg[i])
        want = np.zeros(len(st))
        want[i] = 1.0
        assert x.dtype == np.float64 and np.array_equal(x, want)
    g = p.sigma_rel_to_gamma(0.075)
    x1 = p.solve_weights(st, sg, 128, g)
    x2 = p.solve_weights([128 * t for t in st], sg, 128 * 128, g)
    assert np.abs(x1 - x2).max() <= 1e-12
    assert np.abs(x1 - R.weights(st, sg, 128, g)).max() <= 1e-6    # the restatement's minimum-norm solve
    with warnings.catch_warnings(record=True) as seen:             # two snapshots a relative 1e-15 apart: singular to working precision, said so
        warnings.simplefilter("always")
        x = p.solve_weights([64.0, 64.0 * (1 + 1e-15), 128.0], [sg[0]] * 3, 100.0, sg[0])
    assert any("condition number" in str(w.message) for w in seen) and np.isfinite(x).all()


@pytest.fixture(scope="module")
def recipe():
    """512 steps of a 64-vector, theta_t = cumsum(0.05 N(0, 1)) + 0.3 N(0, 1); 0.05 and 0.10 tracked, both snapshotted every 16 steps"""
    p = P()
    rng = np.random.default_rng(20240101)
    theta = np.cumsum(0.05 * rng.standard_normal((512, 64)), axis=0) + 0.3 * rng.standard_normal((512, 64))
    gs = [p.sigma_rel_to_gamma(s) for s in SIGMAS]
    tracked = [R.track(theta, g) for g in gs]
    st, sg, snaps = [], [], []
    for t in range(16, 513, 16):
        for g, e in zip(gs, tracked):
            st.append(t), sg.append(g), snaps.append(e[t - 1])
    assert len(snaps) == 64
    return theta, tracked, st, sg, np.stack(snaps)


@pytest.mark.parametrize("sigma_rel", [0.06, 0.075, 0.15])
def test_reconstruction_recipe(recipe, sigma_rel):
    """max error of the reconstruction at t = 512 below 1/10 of the distance from the nearer tracked shadow to the directly tracked profile
    (the restatement alone gives 3e-4 to 9e-4 on this recipe)"""
    p = P()
    theta, tracked, st, sg, snaps = recipe
    g = p.sigma_rel_to_gamma(sigma_rel)
    direct = R.track(theta, g)[-1]
    near = min(np.abs(e[-1] - direct).max() for e in tracked)
    for name, x in (("phema.solve_weights", p.solve_weights(st, sg, 512, g)), ("restatement", R.weights(st, sg, 512, g))):
        err = np.abs(x @ snaps - direct).max()
        print(f"sigma_rel {sigma_rel} {name}: error {err:.3e}, nearer tracked shadow {near:.3e}, ratio {err / near:.2e}, "
              f"sum x {x.sum():.6f}, sum |x| {np.abs(x).sum():.3f}")
        assert err < near / 10


def _snap(p, t, numel=12, layout=(("a", 0, (2, 3)), ("b", 8, (4,))), seed=0):
    gen = torch.Generator().manual_seed(seed)
    return p.make_snapshot(t, SIGMAS, layout, numel, [torch.randn(numel, generator=gen) for _ in SIGMAS])


def test_snapshot_round_trip_and_refusals(tmp_path):
    p = P()
    s = _snap(p, 7)
    assert s["format"] == "vdiff-phema-1" and s["t"] == 7 and s["sigma_rels"] == list(SIGMAS) and s["numel"] == 12
    assert s["gammas"] == [p.sigma_rel_to_gamma(x) for x in SIGMAS] and s["layout"] == [["a", 0, [2, 3]], ["b", 8, [4]]]
    assert all(f.dtype == torch.float32 and f.device.type == "cpu" and f.shape == (12,) for f in s["flat"])
    path = str(tmp_path / "snap.pt")
    torch.save(s, path)
    back = torch.load(path, weights_only=True)                     # a plain dict: no code in the file
    assert {k: v for k, v in back.items() if k != "flat"} == {k: v for k, v in s.items() if k != "flat"}
    assert all(torch.equal(a, b) for a, b in zip(back["flat"], s["flat"]))
    other = _snap(p, 9, layout=(("a", 0, (2, 3)), ("c", 8, (4,))))
    with pytest.raises(ValueError, match="layout"):               # mixed layouts: refused on the host, dicts and paths alike
        p.posthoc_ema([path, other], 0.075)
    with pytest.raises(ValueError):
        p.posthoc_ema([], 0.075)
    with pytest.raises(ValueError):
        p.posthoc_ema([{"format": "something-else"}], 0.075)
    from v_diffusion import _hip
    with pytest.raises(_hip.HipError, match="no CPU fallback"):    # CPU-only use: refused before anything is launched
        p.posthoc_ema([s, _snap(p, 9, seed=1)], 0.075, device="cpu")


C_ABI_PHEMA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c_abi_phema.json")


def _parsed_phema_abi():
    from v_diffusion import _hip
    with open(_hip.PHEMA_HEADER_PATH) as f:
        product, probe = _hip._parse_header(f.read())
    assert probe == {}
    return [[name, ret, params] for name, (ret, params) in product.items()]


def test_the_post_hoc_ema_c_abi_is_as_recorded_and_binds_by_the_type_rule():
    """include/vdiff_phema.h -- names, order, return types, each parameter's type and name -- against tests/golden/c_abi_phema.json, as
    tests/test_host_cpu.py pins include/vdiff_hip.h; its types are among those that header uses, bound by the same rule; the table of
    vdiff_hip.h itself does not carry the new entries.  (python tests/test_phema_cpu.py --record rewrites the fixture.)"""
    import ctypes as C
    import json
    from v_diffusion import _hip
    with open(C_ABI_PHEMA) as f:
        want = json.load(f)
    assert _parsed_phema_abi() == want and [e[0] for e in want] == ["vd_adamw_emas", "vd_ema_combine"]
    assert (len(want[0][2]), len(want[1][2])) == (29, 7)
    by_value = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    pointers = ("const float*", "float*", "const double*", "double*", "int32_t*", "const float* const*", "float* const*", "void*")
    assert list(_hip.PHEMA_SIGNATURES) == [e[0] for e in want] and not set(_hip.PHEMA_SIGNATURES) & set(_hip.EXPORTS)
    for name, ret, decl in want:
        res, args = _hip.PHEMA_SIGNATURES[name]
        assert ret == "int" and res is C.c_int and len(args) == len(decl)
        for q, a in zip(decl, args):
            ctype = q.rpartition(" ")[0]
            assert a is (by_value[ctype] if ctype in by_value else C.c_void_p) and (ctype in by_value or ctype in pointers), (name, q)
    lib = _hip.lib()                                                # the library exports them with exactly these types
    for name, (res, args) in _hip.PHEMA_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # ... and the two headers together declare every vd_* symbol the product library exports: none is bound outside a recorded table
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()[-2:-1] == ["T"] and line.split()[-1].startswith("vd_")}
    assert set(_hip.PHEMA_SIGNATURES) <= exported
    assert exported <= set(_hip.EXPORTS) | set(_hip.PHEMA_SIGNATURES), sorted(exported - set(_hip.EXPORTS) - set(_hip.PHEMA_SIGNATURES))


def test_a_name_declared_in_both_headers_is_refused(tmp_path):
    from v_diffusion import _hip
    twice = tmp_path / "vdiff_phema.h"
    twice.write_text(open(_hip.PHEMA_HEADER_PATH).read() + "\nint vd_sumsq(const float* g, int64_t n, void* stream);\n")
    with pytest.raises(RuntimeError, match="vd_sumsq.*also declared"):
        _hip._phema_signatures(str(twice))
    assert _hip._phema_signatures() == _hip.PHEMA_SIGNATURES


def test_power_ema_without_a_flat_store():
    """optim.PowerEMA over parameters no flat store owns (plain torch: runs on the CPU): the multi-tensor lerp_ against the fp64 recurrence
    within the summed per-step bound, apply / restore per tensor, restore without apply refused, the packed snapshot layout"""
    p = P()
    from v_diffusion import optim
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))
    pe = optim.PowerEMA(model, sigma_rels=(0.05, 0.10))
    assert pe._store is None
    names = [k for k, _ in model.named_parameters()]
    flat = lambda d: np.concatenate([d[k].detach().double().numpy().reshape(-1) for k in names])
    e64, budget, before = [None, None], [0.0, 0.0], [None, None]
    for i in range(5):
        with torch.no_grad():
            for q in model.parameters():
                q.add_(0.1 * torch.randn_like(q))
        pe.update()
        p64 = flat(dict(model.named_parameters()))
        for j, g in enumerate(pe.gammas):
            r = float(np.float32(p.power_ema_rate(i + 1, g)))
            e64[j] = p64.copy() if i == 0 else e64[j] + r * (p64 - e64[j])
            budget[j] = budget[j] + R.shadow_step_bound(r, p64, p64 if i == 0 else before[j], e64[j])
            before[j] = flat(pe.shadows[j])
    for j in range(2):
        assert (np.abs(before[j] - e64[j]) <= budget[j]).all()
    raw = {k: v.detach().clone() for k, v in model.named_parameters()}
    with pytest.raises(RuntimeError, match="apply"):
        pe.restore()
    pe.apply(0.10)
    assert all(torch.equal(v.detach(), pe.shadows[1][k]) for k, v in model.named_parameters())
    pe.restore()
    with pe:
        assert all(torch.equal(v.detach(), pe.shadows[0][k]) for k, v in model.named_parameters())
    assert all(torch.equal(v.detach(), raw[k]) for k, v in model.named_parameters())
    snap = pe.snapshot()
    assert snap["t"] == 5 and snap["sigma_rels"] == [0.05, 0.10] and snap["numel"] == 36 + 8 + 24 + 4
    assert snap["layout"] == [["0.weight", 0, [7, 5]], ["0.bias", 36, [7]], ["2.weight", 44, [3, 7]], ["2.bias", 68, [3]]]
    for j in range(2):
        for k, o, shape in snap["layout"]:
            n = int(np.prod(shape))
            assert torch.equal(snap["flat"][j][o:o + n].view(shape), pe.shadows[j][k])
        assert float(snap["flat"][j][35]) == 0.0 and float(snap["flat"][j][43]) == 0.0 and float(snap["flat"][j][71]) == 0.0      # padding
    other = optim.PowerEMA(model, sigma_rels=(0.05, 0.10))
    other.load_state_dict(pe.state_dict())
    assert other.num_updates == 5 and all(torch.equal(other.shadows[1][k], pe.shadows[1][k]) for k in names)


if __name__ == "__main__":
    import json
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "v-diffusion-torch_amd")]
    assert sys.argv[1:] == ["--record"], "python tests/test_phema_cpu.py --record"
    with open(C_ABI_PHEMA, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in _parsed_phema_abi()) + "\n]\n")
