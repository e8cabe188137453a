"""Post-hoc EMA (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3.5 and appendix C; not part
of the reference): the averaging length of the sampled network chosen AFTER training.  During training a few power-function EMA profiles

    beta_t = (1 - 1/t)^(gamma + 1),   e <- beta_t e + (1 - beta_t) theta_t          (t = 1, 2, ...: the profile's own updates; e_1 = theta_1)

ride in the fused optimizer tail (vd_adamw_emas) and snapshots of them are kept; afterwards ANY profile at ANY snapshot time is the
least-squares combination of the stored snapshots, formed by one fp64-accumulating kernel (vd_ema_combine).

The host math is fp64 numpy / python.  A profile's width is sigma_rel = (gamma + 1)^(1/2) (gamma + 2)^(-1) (gamma + 3)^(-1/2), the standard
deviation of its weight density p_{t,gamma}(tau) = (gamma + 1) tau^gamma / t^(gamma + 1) on [0, t] relative to t; valid widths lie in
(0, 1/sqrt(12)).  Times are update counts; the solve does not depend on their unit.

Snapshot (a plain dict, so a file is ``torch.save`` of it):
    {"format": "vdiff-phema-1", "t": int, "sigma_rels": [float], "gammas": [float], "layout": [[name, offset, shape], ...], "numel": int,
     "flat": [1-D fp32 CPU tensor per tracked profile, in the flat store's own layout]}
"""
import math
import warnings

import numpy as np

FORMAT = "vdiff-phema-1"
SIGMA_REL_MAX = 0.2886     # 1/sqrt(12) = 0.28868 (gamma = 0; sigma_rel falls as gamma grows) cut to four digits: widths from here on are refused


def gamma_to_sigma_rel(g):
    g = float(g)
    if not g > -1.0:
        raise ValueError(f"gamma must exceed -1, got {g}")
    return math.sqrt(g + 1.0) / ((g + 2.0) * math.sqrt(g + 3.0))


def sigma_rel_to_gamma(s):
    """the largest real root of gamma^3 + 7 gamma^2 + (16 - s^-2) gamma + (12 - s^-2); s outside (0, 0.2886) is refused (beyond 1/sqrt(12) = 0.28868 there is no
    positive root)"""
    s = float(s)
    if not (0.0 < s < SIGMA_REL_MAX):
        raise ValueError(f"sigma_rel must lie in (0, {SIGMA_REL_MAX:.4f}), got {s}")
    q = s ** -2
    roots = np.roots([1.0, 7.0, 16.0 - q, 12.0 - q])
    g = float(max(r.real for r in roots if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real))))
    for _ in range(3):                      # polish the eigenvalue estimate: Newton on the cubic
        f = ((g + 7.0) * g + (16.0 - q)) * g + (12.0 - q)
        g -= f / ((3.0 * g + 14.0) * g + (16.0 - q))
    return g


def power_ema_rate(t, gamma):
    """1 - beta_t = 1 - (1 - 1/t)^(gamma + 1) as a double, formed without the cancellation of ``1 - beta``; exactly 1.0 at t = 1"""
    t = int(t)
    if t < 1:
        raise ValueError(f"a profile's updates count from 1, got t = {t}")
    if t == 1:
        return 1.0
    return -math.expm1((float(gamma) + 1.0) * math.log1p(-1.0 / t))


def profile_dot(ta, ga, tb, gb):
    """<p_{ta,ga}, p_{tb,gb}> = int_0^min(ta,tb) p_a p_b dtau
    = (ga + 1)(gb + 1) / ((ga + gb + 1) max(ta, tb)) (ta / tb)^e,  e = gb if ta < tb else -ga.  Vectorised (numpy broadcasting)."""
    ta, ga, tb, gb = (np.asarray(x, dtype=np.float64) for x in (ta, ga, tb, gb))
    hi = np.maximum(ta, tb)                         # (ta / tb)^e as (min / max)^(gamma of the later profile): the same bits either way round
    return (ga + 1.0) * (gb + 1.0) / ((ga + gb + 1.0) * hi) * (np.minimum(ta, tb) / hi) ** np.where(ta < tb, gb, ga)


def solve_weights(snap_t, snap_gamma, t_r, gamma_r):
    """x (float64[K]) with sum_i x_i snapshot_i the least-squares reconstruction of the profile (t_r, gamma_r) from snapshots at
    (snap_t[i], snap_gamma[i]): A x = b, A_ij = <p_i, p_j>, b_i = <p_i, p_r>.  A target that IS a snapshot selects it: the exact one-hot
    vector, not the output of a solve."""
    t = np.asarray(snap_t, dtype=np.float64).reshape(-1)
    g = np.asarray(snap_gamma, dtype=np.float64).reshape(-1)
    if t.size == 0 or t.shape != g.shape:
        raise ValueError("solve_weights: one time and one gamma per snapshot, at least one snapshot")
    if not (np.all(t > 0) and np.all(g > 0) and t_r > 0 and gamma_r > 0):
        raise ValueError("solve_weights: times and gammas must be positive")
    hit = np.flatnonzero((t == float(t_r)) & (g == float(gamma_r)))
    if hit.size:
        x = np.zeros(t.size)
        x[hit[0]] = 1.0
        return x
    A = profile_dot(t[:, None], g[:, None], t[None, :], g[None, :])
    A = 0.5 * (A + A.T)
    b = profile_dot(t, g, float(t_r), float(gamma_r))
    cond = np.linalg.cond(A)
    if not cond <= 1e12:
        warnings.warn(f"solve_weights: the snapshots' Gram matrix has condition number {cond:.2e} > 1e12 (near-duplicate snapshots); "
                      "using the minimum-norm least-squares solution")
        return np.linalg.lstsq(A, b, rcond=None)[0]
    return np.linalg.solve(A, b)


def make_snapshot(t, sigma_rels, layout, numel, flats):
    """the snapshot dict of the module docstring; ``flats``: one flat fp32 tensor per profile (moved to the CPU as it is, no gather)"""
    import torch
    sig = [float(s) for s in sigma_rels]
    flat = [f.detach().to("cpu", torch.float32).contiguous() for f in flats]
    if len(flat) != len(sig) or any(f.dim() != 1 or f.numel() != int(numel) for f in flat):
        raise ValueError("snapshot: one 1-D buffer of `numel` elements per tracked profile")
    return {"format": FORMAT, "t": int(t), "sigma_rels": sig, "gammas": [sigma_rel_to_gamma(s) for s in sig],
            "layout": [[str(k), int(o), [int(d) for d in shape]] for k, o, shape in layout], "numel": int(numel), "flat": flat}


def _open(snap):
    """a snapshot dict as it is; a path through torch.load, memory-mapped: its buffers are read when they are copied to the device"""
    if isinstance(snap, dict):
        s = snap
    else:
        import torch
        s = torch.load(snap, map_location="cpu", mmap=True, weights_only=True)
    if not isinstance(s, dict) or s.get("format") != FORMAT:
        raise ValueError(f"not a {FORMAT} snapshot: {snap if not isinstance(snap, dict) else sorted(snap)[:4]}")
    return s


def posthoc_ema(snapshots, sigma_rel, t=None, device=None, chunk=16):
    """{name: fp32 tensor on ``device``}: the profile of width ``sigma_rel`` at time ``t`` (default: the latest snapshot's) rebuilt from
    ``snapshots`` (snapshot dicts or paths to ``torch.save``d ones; every profile of every snapshot is a source).  The sources go to the
    device ``chunk`` at a time and vd_ema_combine chains the chunks through its fp64 accumulator, so the result is the one fma chain over
    all sources in order, rounded to fp32 once, whatever ``chunk`` is.  Sources of weight 0 are never loaded (a target that is a stored
    profile is returned bit for bit).  The result loads with ``model.load_state_dict(..., strict=False)`` or as the ``shadow`` of a
    reference-format EMA state.  There is no CPU path."""
    import torch
    from . import _hip
    if not snapshots:
        raise ValueError("posthoc_ema: no snapshots")
    chunk = int(chunk)
    if not 1 <= chunk <= 32:
        raise ValueError("posthoc_ema: chunk must lie in 1..32 (the sources of one vd_ema_combine launch)")
    gamma_r = sigma_rel_to_gamma(sigma_rel)
    metas, layout, numel = [], None, None
    for i, snap in enumerate(snapshots):
        s = _open(snap)
        if layout is None:
            layout, numel = s["layout"], int(s["numel"])
        elif [list(map(_norm, e)) for e in s["layout"]] != [list(map(_norm, e)) for e in layout] or int(s["numel"]) != numel:
            raise ValueError(f"posthoc_ema: snapshot {i} has another layout than snapshot 0")
        for j, g in enumerate(s["gammas"]):
            metas.append((i, j, float(s["t"]), float(g)))
        del s
    t_r = max(m[2] for m in metas) if t is None else float(t)
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _hip.HipError("posthoc_ema combines the snapshots on an MI355X only (no CPU fallback)")
    w = solve_weights([m[2] for m in metas], [m[3] for m in metas], t_r, gamma_r)
    live = [(m, float(x)) for m, x in zip(metas, w) if x != 0.0]
    out = torch.empty(numel, dtype=torch.float32, device=dev)
    if not live:
        out.zero_()
    acc = torch.zeros(numel, dtype=torch.float64, device=dev) if len(live) > chunk else None
    with torch.cuda.device(dev):
        for lo in range(0, len(live), chunk):
            part = live[lo:lo + chunk]
            opened, srcs = {}, []
            for (i, j, _, _), _x in part:
                if i not in opened:
                    opened[i] = _open(snapshots[i])
                srcs.append(opened[i]["flat"][j].to(dev, torch.float32).contiguous())
            last = lo + chunk >= len(live)
            _hip.ema_combine(out if last else None, acc, srcs, [x for _, x in part])
            del opened, srcs
    return {k: out[o:o + int(np.prod(shape, dtype=np.int64))].view(tuple(shape)) for k, o, shape in layout}


def _norm(v):
    return list(v) if isinstance(v, (list, tuple)) else v
