"""Device-free checks of the blur operator of Diffusion Posterior Sampling (``("blur", kernel)``: v_diffusion/restore.py, v_diffusion/dps.py,
include/vdiff_blur.h):

  * ``dps_measure`` and the fp64 restatement tests/blur_ref.py against explicit index loops; the gather formula of the header against
    autograd of the restatement where the radius reaches H - 1; <A x, r> = <x, A^T r>;
  * ``gaussian_kernel``; every refusal that needs no device, those of DDNM among them; the exported names;
  * the C ABI of include/vdiff_blur.h against tests/golden/c_abi_blur.json, its binding by the type rule, and the closure of the vdx_*
    prefix; the refusals of the two entries through the library (nothing is launched);
  * a chain of the restatement that does reduce the measurement residual."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
import blur_ref as BR                                             # noqa: E402

F64 = torch.float64
C_ABI_BLUR = os.path.join(_HERE, "golden", "c_abi_blur.json")
# (plane, taps): every one with a radius that reaches the plane's side minus one on at least one axis, or close to it
SMALL = (((3, 4), (5, 7)), ((5, 7), (3, 5)), ((6, 5), (9, 3)), ((2, 2), (3, 3)))


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def rho(p, n):
    return -p if p < 0 else (2 * (n - 1) - p if p > n - 1 else p)


def loops_A(x, taps):
    """A x of one plane, the formula of the header term by term"""
    (H, W), (kh, kw) = x.shape, taps.shape
    out = torch.zeros((H, W), dtype=F64)
    for y in range(H):
        for xx in range(W):
            out[y, xx] = sum(float(taps[i, j]) * float(x[rho(y + i - kh // 2, H), rho(xx + j - kw // 2, W)]) for i in range(kh) for j in range(kw))
    return out


# ------------------------------------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("plane,ksize", SMALL)
def test_the_operator_against_index_loops_and_its_adjoint(plane, ksize):
    from v_diffusion import dps_measure
    taps = rnd(ksize, 1)                                            # asymmetric: a flipped kernel would show
    x = rnd((2, 3) + plane, 2)
    want = torch.stack([torch.stack([loops_A(x[b, c], taps) for c in range(3)]) for b in range(2)])
    for name, got in (("dps_measure", dps_measure(x, ("blur", taps))), ("blur_ref", BR.apply_A(x, taps))):
        err = float((got - want).abs().max())
        assert got.dtype == F64 and tuple(got.shape) == tuple(x.shape) and err <= 1e-14 * float(want.abs().max()), (name, err)
    assert dps_measure(x.float(), ("blur", taps)).dtype == torch.float32           # the image's dtype, whatever the kernel's
    # the gather formula of include/vdiff_blur.h against autograd of the sum of slices
    r = rnd((2, 3) + plane, 3)
    At = BR.apply_At(r, taps)
    for b, c in ((0, 0), (1, 2)):
        err = float((BR.gather_At(r[b, c], taps) - At[b, c]).abs().max())
        assert err <= 1e-14 * float(At.abs().max()), (plane, ksize, err)
    lhs, rhs = float((BR.apply_A(x, taps) * r).sum()), float((x * At).sum())
    assert abs(lhs - rhs) <= 1e-13 * float((x.abs() * At.abs()).sum()), (lhs, rhs)


def test_gaussian_kernel():
    import v_diffusion as vd
    for size, std in ((9, 1.5), (33, 5.0), (3, 0.1), (5, 100.0)):
        k = vd.gaussian_kernel(size, std)
        assert k.dtype == torch.float32 and tuple(k.shape) == (size, size) and bool((k >= 0).all())
        assert abs(float(k.double().sum()) - 1.0) <= 2.0 ** -23, (size, std)        # each tap rounded once: at most 2^-24 of the sum, 1
        assert torch.equal(k, k.t()) and torch.equal(k, k.flip(0)) and torch.equal(k, k.flip(1))
        assert float(k[size // 2, size // 2]) == float(k.max())
    d = torch.arange(9, dtype=F64) - 4
    g = torch.exp(-d * d / (2 * 1.5 ** 2))
    assert torch.equal(vd.gaussian_kernel(9, 1.5), (torch.outer(g, g) / torch.outer(g, g).sum()).float())
    assert vd.gaussian_kernel(1, 2.0).tolist() == [[1.0]]
    for size in (0, 2, 35, 3.0, True, -3):
        with pytest.raises(ValueError, match="size"):
            vd.gaussian_kernel(size, 1.0)
    for std in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="std"):
            vd.gaussian_kernel(5, std)


# ------------------------------------------------------------------------------------------------ 2. refusals without a device
def test_refusals_that_need_no_device():
    import v_diffusion as vd
    from test_dps_cpu import Stub, _gd
    from v_diffusion.restore import parse_operator
    shape = (2, 3, 8, 8)
    ok = torch.ones(3, 5)
    assert parse_operator(("blur", ok), shape) == ("blur", 0, None, shape)
    assert parse_operator(["blur", torch.ones(15, 15, dtype=F64)], shape)[0] == "blur"               # the radius 7 = H - 1 fits
    assert parse_operator(("blur", torch.ones(33, 1)), (1, 1, 17, 1))[3] == (1, 1, 17, 1)
    # ... and the existing kinds return what they returned
    m = torch.ones(1, 1, 8, 8)
    assert parse_operator(("gray",), shape) == ("gray", 0, None, (2, 1, 8, 8)) and parse_operator(("down", 4), shape) == ("down", 4, None, (2, 3, 2, 2))
    assert parse_operator(("mask", m), shape)[:2] == ("mask", 1) and parse_operator(("mask", m), shape)[2] is m
    bad = (("blur", 3), ("blur",), ("blur", ok, ok), ("blur", torch.ones(3)), ("blur", torch.ones(1, 3, 3)), ("blur", [[1.0]]),
           ("blur", torch.ones(3, 3, dtype=torch.int32)), ("blur", torch.ones(3, 3, dtype=torch.bool)), ("blur", torch.ones(2, 3)),
           ("blur", torch.ones(3, 4)), ("blur", torch.ones(35, 3)), ("blur", torch.ones(3, 35)),
           ("blur", torch.tensor([[1.0, float("nan"), 0.0]])), ("blur", torch.tensor([[float("inf")]])), ("blur", torch.ones(17, 3)),
           ("blur", torch.ones(3, 17)))
    gd, meas = _gd(4), torch.zeros(shape)
    for op in bad:
        for call in (lambda: parse_operator(op, shape), lambda: vd.dps_measure(meas, op), lambda: gd.p_sample_dps(Stub(), meas, op, shape),
                     lambda: gd.p_sample_ddnm(Stub(), meas, op, shape), lambda: vd.ddnm_pinv(meas, op, shape)):
            with pytest.raises(ValueError, match="operator"):
                call()
    with pytest.raises(ValueError, match="measurement"):
        gd.p_sample_dps(Stub(), torch.zeros(2, 1, 8, 8), ("blur", ok), shape)
    with pytest.raises(ValueError, match="at most 4096"):                      # the plane bound, before any tensor is looked at
        gd.p_sample_dps(Stub(), torch.zeros(1, 1, 64, 65), ("blur", ok), (1, 1, 64, 65))
    with pytest.raises(RuntimeError, match="MI355X"):                          # CPU tensors, after everything else passed
        gd.p_sample_dps(Stub(), meas, ("blur", ok), shape)
    with pytest.raises(RuntimeError, match="MI355X"):
        vd.blur(meas.float(), ok)
    with pytest.raises(ValueError, match="shape"):
        vd.blur(torch.zeros(3, 8, 8), ok)
    # DDNM: the operator parses, then the refusal, before anything else is looked at (and before any launch: these are CPU tensors)
    for call in (lambda: gd.p_sample_ddnm(Stub(), meas, ("blur", ok), shape), lambda: vd.ddnm_pinv(meas, ("blur", ok), shape),
                 lambda: gd.p_sample_ddnm(Stub(), meas, ("blur", ok), shape, sigma_y=-1.0)):
        with pytest.raises(NotImplementedError, match="not a per-thread preimage"):
            call()
    with pytest.raises(ValueError, match="measurement"):                       # ... after the operator and the measurement's shape
        gd.p_sample_ddnm(Stub(), torch.zeros(2, 1, 8, 8), ("blur", ok), shape)


def test_the_names_are_exported_and_the_bounds_agree():
    import v_diffusion as vd
    from v_diffusion import _hip, dps, restore
    for name in ("blur", "gaussian_kernel", "dps_measure"):
        assert name in vd.__all__ and name in vd._HOT and callable(getattr(vd, name))
    assert vd.blur is dps.blur and vd.gaussian_kernel is restore.gaussian_kernel
    assert _hip.DPS_OPS == {"mask": 0, "down": 1, "gray": 2}                  # the blur is a launch of its own, not a fourth op
    with open(_hip.BLUR_HEADER_PATH) as f:
        defines = dict(re.findall(r"#define\s+(VDX_BLUR_\w+)\s+(\d+)", f.read()))
    assert defines == {"VDX_BLUR_KMAX": "33", "VDX_BLUR_PLANE_MAX": "4096"}
    assert (_hip.BLUR_KMAX, _hip.BLUR_PLANE_MAX, restore.BLUR_KMAX) == (33, 4096, 33)


# ------------------------------------------------------------------------------------------------ 3. the C ABI
def _parsed_blur_abi():
    from v_diffusion import _hip
    with open(_hip.BLUR_HEADER_PATH) as f:
        product, probe = _hip._parse_header(f.read(), _hip.BLUR_PREFIX)
    assert probe == {}
    return [[name, ret, params] for name, (ret, params) in product.items()]


def test_the_blur_c_abi_is_as_recorded_binds_by_the_type_rule_and_closes_over_its_prefix():
    """include/vdiff_blur.h -- names, order, return types, each parameter's type and name -- against tests/golden/c_abi_blur.json, as
    tests/test_phema_cpu.py pins include/vdiff_phema.h; bound by the type rule of the other headers; every vdx_* symbol the product
    library exports is in that table, and no name stands in two headers.  (python tests/test_blur_cpu.py --record rewrites the fixture.)"""
    from v_diffusion import _hip
    with open(C_ABI_BLUR) as f:
        want = json.load(f)
    assert _parsed_blur_abi() == want and [e[0] for e in want] == ["vdx_dps_residual_blur", "vdx_blur_planes"]
    assert (len(want[0][2]), len(want[1][2])) == (19, 10)
    # the parameter order of vd_dps_residual with (taps, kh, kw) for (mask, op, par)
    with open(os.path.join(_HERE, "golden", "c_abi.json")) as f:
        res = {e[0]: e for e in json.load(f)["product"]}["vd_dps_residual"][2]
    swap = {"const float* mask": "const float* taps", "int32_t op": "int32_t kh", "int32_t par": "int32_t kw"}
    assert want[0][2] == [swap.get(q, q) for q in res]
    by_value, pointers = {"int32_t": ctypes.c_int32}, ("const float*", "float*", "void*")
    assert list(_hip.BLUR_SIGNATURES) == [e[0] for e in want]
    for name, ret, decl in want:
        rtype, args = _hip.BLUR_SIGNATURES[name]
        assert ret == "int" and rtype is ctypes.c_int and len(args) == len(decl)
        for q, a in zip(decl, args):
            ctype = q.rpartition(" ")[0]
            assert a is (by_value[ctype] if ctype in by_value else ctypes.c_void_p) and (ctype in by_value or ctype in pointers), (name, q)
    lib = _hip.lib()                                                # the library exports them with exactly these types
    for name, (rtype, args) in _hip.BLUR_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is rtype and list(fn.argtypes) == args
    # closure: the vdx_* symbols of the product library are exactly this table ...
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()[-2:-1] == ["T"] and line.split()[-1].startswith("vdx_")}
    assert exported == set(_hip.BLUR_SIGNATURES), sorted(exported ^ set(_hip.BLUR_SIGNATURES))
    # ... and no name is declared in two headers: the three tables are disjoint, this header declares nothing under vd_, the other two
    # nothing under vdx_
    tables = (set(_hip.EXPORTS) | set(_hip.PROBE_EXPORTS), set(_hip.PHEMA_SIGNATURES), set(_hip.BLUR_SIGNATURES))
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    for path, prefix in ((_hip.BLUR_HEADER_PATH, "vd_"), (_hip.HEADER_PATH, "vdx_"), (_hip.PHEMA_HEADER_PATH, "vdx_")):
        with open(path) as f:
            assert _hip._parse_header(f.read(), prefix) == ({}, {}), (path, prefix)


def test_a_name_in_the_wrong_header_is_refused(tmp_path):
    from v_diffusion import _hip
    text = open(_hip.BLUR_HEADER_PATH).read()
    extra = tmp_path / "vdiff_blur.h"
    extra.write_text(text + "\nint vd_sumsq(const float* g, int64_t n, void* stream);\n")
    with pytest.raises(RuntimeError, match="vd_sumsq.*belong in"):
        _hip._blur_signatures(str(extra))
    extra.write_text(text + "\nint vdx_blur_planes(const float* x);\n")
    with pytest.raises(RuntimeError, match="declared twice"):
        _hip._blur_signatures(str(extra))
    extra.write_text(text + "\nstatic inline int vdx_helper(int a) { return a; }\n")
    with pytest.raises(RuntimeError, match="not of the form"):
        _hip._blur_signatures(str(extra))
    assert _hip._blur_signatures() == _hip.BLUR_SIGNATURES


def test_the_entries_refuse_before_any_launch():
    """a bad model_out_type, a null required buffer, n, C, H, W or planes < 1, an even or out-of-range kh or kw, a radius beyond H - 1 or
    W - 1, a plane over the bound, a bad adjoint: 1, with the reason, and nothing launched (the addresses are never dereferenced)"""
    from v_diffusion import _hip
    lib = _hip.lib()
    err = lambda: lib.vd_last_error().decode(errors="replace")
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf) // 16 * 16 + 16
    k = (ctypes.c_float * 8)(0.8, -0.6, 0.0, 0.3, 0.7, 0.1, 0.0, 0.0)
    good = dict(xt=a, out=a, meas=a, taps=a, k=k, type=0, cfg=0, clip=1, kh=3, kw=3, dout=a, dxt=a, sumsq=a, x0hat=None, n=1, C=3, H=4, W=4,
                stream=None)
    r = lambda **kw: lib.vdx_dps_residual_blur(*{**good, **kw}.values())
    gp = dict(x=a, taps=a, kh=3, kw=3, adjoint=0, y=a, planes=1, H=4, W=4, stream=None)
    p = lambda **kw: lib.vdx_blur_planes(*{**gp, **kw}.values())
    assert r(type=4) == 1 and "model_out_type" in err() and r(type=-1) == 1
    for name in ("xt", "out", "meas", "taps", "k", "dout", "dxt", "sumsq"):
        assert r(**{name: None}) == 1 and "null" in err(), name
    for name in ("x", "taps", "y"):
        assert p(**{name: None}) == 1 and "null" in err(), name
    for name in ("n", "C", "H", "W"):
        assert r(**{name: 0}) == 1 and "empty" in err() and r(**{name: -1}) == 1, name
    for name in ("planes", "H", "W"):
        assert p(**{name: 0}) == 1 and "empty" in err(), name
    for f in (r, p):
        for kh, kw in ((2, 3), (3, 4), (0, 3), (3, 0), (-1, 3), (35, 3), (3, 35), (34, 34)):
            assert f(kh=kh, kw=kw, H=40, W=40) == 1 and "odd" in err(), (kh, kw)
        for kh, kw, H, W in ((9, 3, 4, 4), (3, 9, 4, 4), (5, 1, 2, 2), (1, 3, 1, 1), (33, 33, 16, 64), (33, 33, 64, 16)):
            assert f(kh=kh, kw=kw, H=H, W=W) == 1 and "do not fit" in err(), (kh, kw, H, W)
        for H, W in ((64, 65), (65, 64), (1, 4097), (4097, 1), (65536, 65536), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert f(H=H, W=W, kh=1, kw=1) == 1 and "over the bound" in err(), (H, W)
    assert p(adjoint=2) == 1 and "adjoint" in err() and p(adjoint=-1) == 1


# ------------------------------------------------------------------------------------------------ 4. a chain of the restatement
def test_a_chain_with_a_step_size_ends_nearer_the_measurement(capsys):
    """on the stand-in network, from the same draws, in fp64: the blur chain with zeta > 0 ends with a smaller ||meas - A x|| than the
    zeta = 0 chain (the ordinary sampler, which does not know the measurement).  Both distances go to the test's output."""
    import v_diffusion as vd
    from test_dps_cpu import Stub, _gd
    T, shape, zeta = 8, (2, 3, 8, 8), 0.5
    gd = _gd(T)
    row = lambda i: gd._step_coefs(i, False, True)
    taps = vd.gaussian_kernel(5, 1.0).double()
    meas = BR.apply_A(rnd(shape, 2, 0.5).clamp(-1, 1), taps)
    x_T, noises = rnd(shape, 3), [rnd(shape, 10 + i) for i in range(T)]
    ends = {z: float((meas - BR.apply_A(BR.chain(Stub(), x_T, meas, taps, row, noises, [z] * T, clip=True), taps)).norm()) for z in (0.0, zeta)}
    with capsys.disabled():
        print(f"\n[blur chain, fp64 restatement, T={T}] ||meas - A x||: zeta=0 {ends[0.0]:.6f}   zeta={zeta} {ends[zeta]:.6f}")
    assert ends[zeta] < 0.9 * ends[0.0], ends


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(os.path.dirname(_HERE), "v-diffusion-torch_amd")]
    assert sys.argv[1:] == ["--record"], "python tests/test_blur_cpu.py --record"
    with open(C_ABI_BLUR, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in _parsed_blur_abi()) + "\n]\n")
