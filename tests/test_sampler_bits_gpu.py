"""The bits of the six reverse-step kernels whose arithmetic csrc/diffusion.hip spells out with contraction off and without a
transcendental function: vd_sample_step, vd_solver_step, vd_solver_step_dyn, vd_inpaint_step, vd_forward_jump, vd_noise_extract.  Their
output bits are a property of the source text, not of the compiler, so they are pinned: tests/golden/sampler_bits.json holds one SHA-256
per case over the bytes of every output tensor, recorded from the library as it was BEFORE these kernels were moved onto their shared
helpers.  A change that is meant to leave the samplers alone must leave every digest alone.  (The distillation, loss and bound-term kernels
are not pinned: their grouping is the compiler's.)

The fixture also carries the coefficient rows (fp32 values, exact as JSON numbers), so the digests depend on no host arithmetic: rows 7, 3
and 0 of the 8-step cosine +-20 tables -- first, interior and last step -- for every output type, the "eps" rows without clipping from a
posterior over (eps, x0), whose c3 is not zero.  Inputs are seeded CPU draws in fp64, rounded to fp32.  Grid: C*HW = 75 (scalar form) and
972 (dwordx4 form) x four output types x plain / guided x clip on / off x the three rows with host coefficients, the interior row also
with device coefficients; inpaint with a one-channel and a C-channel mask.

``python tests/test_sampler_bits_gpu.py OUT.json`` writes a fixture from the library in use (VDIFF_HIP_LIB selects one): only for a
change that moves a sampler's bits on purpose."""
import hashlib
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_bits.json")
SHAPES = {"75": (3, 3, 5, 5), "972": (2, 3, 18, 18)}
MOTS = ("v", "eps", "x0", "both")
STEPS, ROWS, DEV_ROW = 8, (7, 3, 0), 3
W_GUIDE = 1.5
KERNELS = ("sample_step", "solver_step", "solver_step_dyn", "inpaint_step", "forward_jump", "noise_extract")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float()


def inputs(shape, mot, cfg):
    """device fp32 inputs shared by the kernels (they only read them)"""
    B, C = shape[:2]
    t = dict(xt=(0.8 * rnd(shape, 1).clamp(-1, 1).double() + 0.6 * rnd(shape, 2).double()).float(),
             out=rnd((B * (1 + cfg), C * (2 if mot == "both" else 1)) + tuple(shape[2:]), 3, 0.8),
             hist=rnd(shape, 4, 0.7), noise=rnd(shape, 5), knoise=rnd(shape, 6), known=rnd(shape, 7, 0.6).clamp(-1, 1))
    for c in (1, C):                                           # a mix of exact 0, exact 1 and values strictly between
        m = rnd((B, c) + tuple(shape[2:]), 8 + c)
        t[f"mask{c}"] = torch.where(m < -0.4, torch.zeros_like(m), torch.where(m > 0.4, torch.ones_like(m), (m + 0.4) / 0.8))
    return {k: v.to(DEV) for k, v in t.items()}


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def coef_forms(k, row):
    """(tag, host list or None, device tensor or None)"""
    yield "host", list(k), None
    if row == DEV_ROW:
        yield "dev", None, torch.tensor(k, dtype=torch.float32, device=DEV)


def cases(H, kernel, rows):
    """(case name, digest of the outputs) over the kernel's grid; ``rows`` = the fixture's coefficient rows"""
    for sname, shape in SHAPES.items():
        B, C = shape[:2]
        HW, N = shape[2] * shape[3], shape[1] * shape[2] * shape[3]
        new = lambda: torch.empty(shape, device=DEV)
        if kernel == "forward_jump":
            t = inputs(shape, "v", 0)
            for dup in (0, 1):
                for tag, k, kd in coef_forms(rows["jump"], DEV_ROW):
                    xn, xdup = new(), torch.empty((2 * B,) + shape[1:], device=DEV) if dup else None
                    H.forward_jump(t["xt"], t["noise"], k, xn, xdup, B, N, k_dev=kd)
                    yield f"{sname}-dup{dup}-{tag}", digest(xn, xdup)
            continue
        for mot in MOTS:
            for cfg in (0, 1):
                t = inputs(shape, mot, cfg)
                m = H.OUT_TYPES[mot]
                dup = lambda: torch.empty((2 * B,) + shape[1:], device=DEV) if cfg else None
                for clip in (0, 1):
                    if kernel == "solver_step_dyn" and clip:
                        continue                               # no clip argument: the cap takes its place below
                    for row in ROWS:
                        table = "solver" if kernel.startswith("solver") else "step"
                        key = f"{mot}/{row}" if table == "solver" else f"{mot}/{clip}/{row}"
                        for tag, k, kd in coef_forms(rows[table][key], row):
                            name = f"{sname}-{mot}-cfg{cfg}-clip{clip}-row{row}-{tag}"
                            xn, xdup = new(), dup()
                            if kernel == "sample_step":
                                H.sample_step(t["xt"], t["out"], t["noise"], k and k[:8], m, cfg, row == 0, clip, xn, xdup, B, C, HW,
                                              k_dev=kd)
                                yield name, digest(xn, xdup)
                            elif kernel == "solver_step":
                                hist = t["hist"].clone()
                                H.solver_step(t["xt"], t["out"], hist, k, m, cfg, clip, xn, xdup, B, C, HW, k_dev=kd)
                                yield name, digest(xn, hist, xdup)
                            elif kernel == "solver_step_dyn":
                                for cap in (math.inf, 1.25):
                                    hist, s = t["hist"].clone(), torch.empty((B,), device=DEV)
                                    H.solver_step_dyn(t["xt"], t["out"], hist, k, m, cfg, (9 * N) // 10, cap, s, xn, xdup, B, C, HW, k_dev=kd)
                                    yield f"{name}-cap{cap}", digest(xn, hist, s, xdup)
                            elif kernel == "inpaint_step":
                                for mc in (1, C):
                                    H.inpaint_step(t["xt"], t["out"], t["noise"], t["known"], t[f"mask{mc}"], t["knoise"], k, m, cfg, row == 0,
                                                   clip, mc, xn, xdup, B, C, HW, k_dev=kd)
                                    yield f"{name}-mask{mc}", digest(xn, xdup)
                            else:
                                z = new()
                                if row == 0:
                                    k = k[:5] + [1.0] + k[6:]                  # the residual's scale (p_invert_noise); host form only
                                H.noise_extract(t["xt"], t["out"], t["known"], t["knoise"] if row else None, k, m, cfg, row == 0, clip, xn, z,
                                                xdup if row else None, B, C, HW, k_dev=kd)
                                yield name, digest(xn, z, xdup if row else None)


def coefficient_rows():
    """the coefficient rows of the fixture, from the package's own host arithmetic"""
    import v_diffusion as vd
    fn = vd.get_logsnr_schedule("cosine", -20.0, 20.0)
    f32 = lambda k: torch.tensor(list(k), dtype=torch.float64).float().tolist()
    rows = {"step": {}, "solver": {}, "jump": f32(vd.jump_coefs(fn, STEPS, 3, 2))}
    for mot in MOTS:
        table, _ = vd.solver_coefs(fn, STEPS, order=2, spacing="time", model_out_type=mot, w_guide=W_GUIDE)
        for row in ROWS:
            rows["solver"][f"{mot}/{row}"] = table[row].tolist()
            for clip in (0, 1):
                gd = vd.GaussianDiffusion(fn, STEPS, mot, "fixed_large", "snr_trunc", "mse", w_guide=W_GUIDE, p_uncond=0.0,
                                          x0eps_coef=(mot == "eps" and not clip))
                k8, _ = gd._step_coefs(row, False, bool(clip))
                rows["step"][f"{mot}/{clip}/{row}"] = f32(list(k8) + list(vd.known_coefs(fn, STEPS, row)))
    return rows


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("kernel", KERNELS)
def test_bits_are_the_recorded_ones(H, fixture, kernel):
    want = fixture["digests"][kernel]
    got = dict(cases(H, kernel, fixture["rows"]))
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    moved = sorted(name for name in got if got[name] != want[name])
    assert not moved, f"{len(moved)} of {len(got)} cases of vd_{kernel} changed bits, first: {moved[:8]}"


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "v-diffusion-torch_amd")]
    from v_diffusion import _hip
    _hip.lib()
    rows = coefficient_rows()
    with torch.cuda.device(0):
        digests = {kernel: dict(cases(_hip, kernel, rows)) for kernel in KERNELS}
    with open(sys.argv[1], "w") as f:
        json.dump({"rows": rows, "digests": digests}, f, indent=0, sort_keys=True)
    print({k: len(v) for k, v in digests.items()})
