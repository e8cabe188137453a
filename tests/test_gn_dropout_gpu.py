"""The dropout path of the GroupNorm kernels (GroupNorm -> FiLM -> SiLU -> dropout, every residual block's second norm) against the
host replay of the keep mask in tests/dropout_ref.py.  The mask is never stored: forward (vd_gn_apply, vd_gn_apply_from_partials)
and every backward form (plain single-pass at 256 / 1024 threads, SPLIT siblings, the widened 96-channel slab, the two-pass pair)
regenerate it from (seed, element index), each with its own index arithmetic.  Here the mask comes from the generator's published
definition, NOT from the kernel's own forward, so a forward and a backward that agree on a wrong index fail too.  Backward references
are fp64 / fp32 autograd of test_kernels_gpu.ref_gn_block with the replayed mask, under the yardstick of test_gn_forward_backward
(slack 6 x torch's own fp32 error + 5e-6 of the scale).  Needs an MI355X."""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_ref as D                                           # noqa: E402
from test_kernels_gpu import H, close, from_nhwc, nhwc, ref_gn_block, rnd      # noqa: E402,F401  (H: the module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED_LO = 1234                                   # below 2^32: the high key word is zero
SEED_HI = 0x3A5F19C47E21B6D3                     # a 62-bit seed, as the engine draws them: both key words in use
TWO_PASS = "two-pass"

CASES = [  # nimg, C, H, W, p, film, act, resample, expected backward form (siblings, threads, pixels per thread, non-temporal) or TWO_PASS or None
    (3, 64, 8, 8, 0.2, True, True, 0, (0, 256, 2, False)),            # CIFAR 8x8: plain, 32-channel slab
    (2, 256, 16, 16, 0.2, True, True, 0, (0, 256, 8, True)),          # CIFAR 16x16: plain, 8 pixels per thread
    (2, 64, 32, 32, 0.2, True, True, 0, (0, 1024, 8, True)),          # CIFAR 32x32: plain, 1024 threads
    (3, 64, 64, 64, 0.1, True, True, 0, (4, 1024, 8, True)),          # 32-channel slabs at 64x64: SPLIT, 4 siblings, 6 units padded to 8
    (3, 384, 32, 32, 0.1, True, True, 0, (4, 1024, 8, True)),         # CelebA level 2: SPLIT, 4 siblings, widened 96-channel slab
    (2, 192, 64, 64, 0.1, True, True, 0, TWO_PASS),                   # CelebA level 1: 24-channel slabs, chan_reduce<1> + gn_bwd_apply
    (2, 576, 16, 16, 0.1, True, True, 0, (0, 1024, 4, False)),        # CelebA level 3: plain, 1024 threads, 36-channel slab
    (2, 768, 8, 8, 0.1, True, True, 0, (0, 256, 8, True)),            # CelebA level 4: plain, 96-channel non-temporal slab
    (2, 64, 8, 8, 0.2, False, True, 1, None),                         # API contract: the mask is applied BEFORE the pooling
    (2, 64, 8, 8, 0.2, False, True, 2, None),                         # ... and before the up-sampling
    (2, 128, 4, 4, 0.2, False, False, 0, (0, 256, 1, False)),         # no activation: the mask alone
]
IDS = [f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-rs{c[7]}" for c in CASES]


def decode_form(k):
    """vd_gn_bwd_last_kernel() -> TWO_PASS or (siblings, threads, pixels per thread, non-temporal), as _hip._gn_bwd_name reads it"""
    if k == -1:
        return TWO_PASS
    assert k > 0, k
    return (k // 10 ** 8, k % 10 ** 4, (k % 10 ** 6) // 10 ** 4, k % 10 ** 8 >= 10 ** 6)


def replay(seed, p, nimg, Hh, Ww, Cc):
    """the keep mask the kernels must use, NCHW float32 (values 0 or 1/(1-p))"""
    m = torch.from_numpy(D.keep_scale(seed, p, nimg, Hh * Ww, Cc))
    return m.reshape(nimg, Hh, Ww, Cc).permute(0, 3, 1, 2).contiguous()


def out_hw(Hh, Ww, rs):
    return (Hh // 2, Ww // 2) if rs == 1 else ((Hh * 2, Ww * 2) if rs == 2 else (Hh, Ww))


@functools.lru_cache(maxsize=None)
def operands(case):
    """inputs and the fp64 / fp32 autograd references of one case (computed once, shared by the tests, never written to)"""
    nimg, Cc, Hh, Ww, p, use_film, act, rs, _ = case
    x = rnd(nimg, Cc, Hh, Ww, seed=1) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * rnd(Cc, seed=2), 0.1 * rnd(Cc, seed=3)
    film = 0.3 * rnd(nimg, 2 * Cc, seed=4) if use_film else None
    Ho, Wo = out_hw(Hh, Ww, rs)
    dy = rnd(nimg, Cc, Ho, Wo, seed=5)
    add = rnd(nimg, Cc, Hh, Ww, seed=6)
    dx0 = rnd(nimg, Cc, Hh, Ww, seed=7)                        # what dx holds before the call (accumulate_dx)
    mask = replay(SEED_HI, p, nimg, Hh, Ww, Cc)

    def run(dt):
        xs, g, b_ = x.to(dt).requires_grad_(True), gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
        fl = None if film is None else film.to(dt).requires_grad_(True)
        out = ref_gn_block(xs, g, b_, fl, act, rs, mask.to(dt))
        out.backward(dy.to(dt))
        return out.detach(), xs.grad + add.to(dt) + dx0.to(dt), g.grad, b_.grad, (None if fl is None else fl.grad)
    return dict(x=x, gamma=gamma, beta=beta, film=film, dy=dy, add=add, dx0=dx0, mask=mask, r64=run(torch.float64), r32=run(torch.float32))


def measured(got, ref64, ref32, name, slack=6, floor=5e-6):
    """close() of test_kernels_gpu with the yardstick of test_gn_forward_backward; prints err / tol before it asserts"""
    r64, r32 = ref64.detach().double(), ref32.detach().double()
    err = (got.detach().cpu().double() - r64).abs().max().item()
    tol = slack * (r32 - r64).abs().max().item() + floor * max(r64.abs().max().item(), 1e-30)
    print(f"{name}: err {err:.3e} tol {tol:.3e} err/tol {err / tol:.3f}")
    close(got, ref64, ref32, slack=slack, floor=floor, name=name)
    return err / tol


def forward(H, case, seed, p, pad, want_coef=False):
    """vd_gn_stats + vd_gn_apply of a case on leading dimensions C + pad -> NCHW cpu output (and the coefficient table, the device x)"""
    nimg, Cc, Hh, Ww, _, use_film, act, rs, _ = case
    op = operands(case)
    ld = Cc + pad
    xd = nhwc(op["x"], ld)
    stats = torch.empty(nimg, 32, 2, device=DEV)
    H.gn_stats(xd, ld, nimg, Hh * Ww, Cc, stats)
    coef = torch.empty(nimg, 4, Cc, device=DEV)
    Ho, Wo = out_hw(Hh, Ww, rs)
    y = torch.full((nimg, Ho, Wo, ld), -7.0, device=DEV)
    fd = None if op["film"] is None else op["film"].to(DEV)
    H.gn_apply(xd, ld, stats, op["gamma"].to(DEV), op["beta"].to(DEV), fd, act, p, seed, rs, y, ld, nimg, Hh, Ww, Cc, coef)
    torch.cuda.synchronize()
    if pad:
        assert (y[..., Cc:] == -7.0).all(), "gn_apply wrote into the padding of y"
    return (from_nhwc(y, Cc), coef, xd) if want_coef else from_nhwc(y, Cc)


def check_mask_exact(y_drop, y0, mask, name):
    """zero pattern == replayed mask wherever the undropped output is non-zero; kept values == y0 * scale (rtol = atol = 1e-6)"""
    live = y0 != 0
    assert live.float().mean().item() > 0.99, name
    wrong = ((y_drop != 0) != (mask != 0)) & live
    assert not wrong.any(), f"{name}: {int(wrong.sum())} of {wrong.numel()} elements kept / dropped against the replayed mask"
    assert (y_drop[~live] == 0).all(), name
    torch.testing.assert_close(y_drop, y0 * mask, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gn_apply_dropout_mask_is_the_replayed_mask(H, case):
    """vd_gn_apply with p_drop > 0: for a seed below 2^32 and a 62-bit one, on tight and on padded leading dimensions.  The mask is indexed
    by pixels of the norm's INPUT: the up-sampled output repeats each masked input pixel 2x2 (exact zero pattern), the pooled output
    averages four masked pixels -- no zero pattern to read there, so the pooled case is compared with the fp64 reference of the replayed
    mask under the forward yardstick of test_gn_forward_backward (4 x torch's fp32 error + 2e-6 of the scale), as every case is."""
    nimg, Cc, Hh, Ww, p, use_film, act, rs, _ = case
    op = operands(case)
    y0 = forward(H, case, 0, 0.0, 0)
    for seed in (SEED_LO, SEED_HI):
        mask = op["mask"] if seed == SEED_HI else replay(seed, p, nimg, Hh, Ww, Cc)
        y1 = forward(H, case, seed, p, 0)
        y1p = forward(H, case, seed, p, 8)
        assert torch.equal(y1p != 0, y1 != 0), "the mask moved with the leading dimensions"
        torch.testing.assert_close(y1p, y1, rtol=1e-6, atol=1e-6)
        if rs == 1:
            frac = None
        else:
            m_out = F.interpolate(mask, scale_factor=2, mode="nearest") if rs == 2 else mask
            check_mask_exact(y1, y0, m_out, f"gn_apply seed {seed:#x}")
            frac = (y1 != 0).float().mean().item()
            assert abs(frac - (1 - p)) < 4 * math.sqrt(p * (1 - p) / mask.numel()) + 1e-3, frac
        xs, g, b_ = op["x"], op["gamma"], op["beta"]
        refs = [ref_gn_block(xs.to(dt), g.to(dt), b_.to(dt), None if op["film"] is None else op["film"].to(dt), act, rs, mask.to(dt))
                for dt in (torch.float64, torch.float32)]
        close(y1, refs[0], refs[1], name=f"gn fwd with dropout, seed {seed:#x}")
    assert ((replay(SEED_LO, p, nimg, Hh, Ww, Cc) != 0) != (op["mask"] != 0)).float().mean().item() > p    # (two seeds, two masks)


@pytest.mark.parametrize("pcase", [(3, 8, 8, 64, 96, 0), (2, 32, 32, 64, 64, 64)], ids=["one-source", "two-source-concat"])
def test_gn_apply_from_partials_dropout_mask_is_the_replayed_mask(H, pcase):
    """vd_gn_apply_from_partials (the form the engine mostly runs) with p_drop > 0; producers as in test_gn_stats_from_producer_epilogues:
    a 3x3 convolution with a residual, and -- second source of the virtual concat -- a 1x1 convolution into the same buffer"""
    nimg, Hh, Ww, Cin, C1, C2 = pcase
    HW, Ct, p = Hh * Ww, C1 + C2, 0.2
    x = rnd(nimg, Cin, Hh, Ww, seed=1)
    w1, b1 = rnd(C1, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5), rnd(C1, seed=3)
    res = rnd(nimg, C1, Hh, Ww, seed=4)
    wf = torch.empty(C1, 9, Cin, device=DEV)
    H.pack_conv3x3(w1.to(DEV), C1, Cin, wf=wf, Cin_p=Cin)
    buf = torch.zeros(nimg, Hh, Ww, Ct, device=DEV)
    part1 = torch.full((H.stats_part_numel(nimg, HW, C1),), 7.0, device=DEV)
    H.conv3x3(nhwc(x), Cin, wf, b1.to(DEV), buf[..., :C1], Ct, nimg, Hh, Ww, Cin, C1, res=nhwc(res), ldres=C1, stats_part=part1)
    parts = [(part1, C1, HW // (H.last_row_tile() // 2))]
    if C2:
        w2, b2 = rnd(C2, Cin, seed=5, scale=Cin ** -0.5), rnd(C2, seed=6)
        part2 = torch.full((H.stats_part_numel(nimg, HW, C2),), 7.0, device=DEV)
        H.gemm(nhwc(x), w2.to(DEV), buf[0, 0, 0, C1:], nimg * HW, C2, Cin, lda=Cin, ldb=Cin, ldc=Ct, bias=b2.to(DEV), stats=part2,
               stats_hw=HW)
        parts.append((part2, C2, HW // (H.last_row_tile() // 2)))
    gamma, beta, film = rnd(Ct, seed=7).to(DEV), rnd(Ct, seed=8).to(DEV), (rnd(nimg, 2 * Ct, seed=9) * 0.1).to(DEV)
    y0 = torch.empty_like(buf)
    coef0 = torch.empty(nimg, 4, Ct, device=DEV)
    H.gn_apply_from_partials(buf, Ct, parts, gamma, beta, film, 1, 0.0, 0, H.RS_NONE, y0, Ct, nimg, Hh, Ww, Ct, coef0)
    for seed in (SEED_LO, SEED_HI):
        y1 = torch.empty_like(buf)
        coef1 = torch.full((nimg, 4, Ct), 5.0, device=DEV)
        H.gn_apply_from_partials(buf, Ct, parts, gamma, beta, film, 1, p, seed, H.RS_NONE, y1, Ct, nimg, Hh, Ww, Ct, coef1)
        torch.cuda.synchronize()
        assert torch.equal(coef1, coef0)                          # the table does not depend on the dropout
        check_mask_exact(from_nhwc(y1, Ct), from_nhwc(y0, Ct), replay(seed, p, nimg, Hh, Ww, Ct), f"from partials, seed {seed:#x}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gn_apply_bwd_with_dropout_in_every_form(H, case):
    """vd_gn_apply_bwd with the replayed mask in the references: dx (on top of a skip-path gradient `add` and a running dx), dgamma / dbeta
    (accumulated onto 1), dfilm -- and the form that ran, as the dispatcher (gn_apply_bwd_impl, fused_slab) derives it for the shape."""
    nimg, Cc, Hh, Ww, p, use_film, act, rs, want = case
    op = operands(case)
    o64, dx64, dg64, db64, df64 = op["r64"]
    o32, dx32, dg32, db32, df32 = op["r32"]
    y, coef, xd = forward(H, case, SEED_HI, p, 8, want_coef=True)
    close(y, o64, o32, name="gn fwd")
    ldx = Cc + 8
    gd, bd = op["gamma"].to(DEV), op["beta"].to(DEV)
    fd = None if op["film"] is None else op["film"].to(DEV)
    dx = nhwc(op["dx0"])
    dfilm = None if fd is None else torch.full((nimg, 2 * Cc), float("nan"), device=DEV)
    dgam, dbet = torch.ones(Cc, device=DEV), torch.ones(Cc, device=DEV)
    H.gn_apply_bwd(nhwc(op["dy"]), Cc, xd, ldx, coef, gd, bd, fd, act, p, SEED_HI, rs, nhwc(op["add"]), Cc, dx, Cc, True, dfilm, dgam, dbet,
                   True, nimg, Hh, Ww, Cc)
    torch.cuda.synchronize()
    form = decode_form(H.lib().vd_gn_bwd_last_kernel())
    print(f"case {case[:8]}: backward form {form}")
    if want is not None:
        assert form == want, f"backward form {form}, the dispatcher's rules give {want}"
    ratios = [measured(from_nhwc(dx, Cc), dx64, dx32, "gn dx"), measured(dgam, dg64 + 1.0, dg32 + 1.0, "dgamma"),
              measured(dbet, db64 + 1.0, db32 + 1.0, "dbeta")]
    if fd is not None:
        ratios.append(measured(dfilm, df64, df32, "dfilm"))
    print(f"form {form}: largest err/tol {max(ratios):.3f}")


NORMS = [  # nimg, C, H, W, p, accumulate: one "backward pass" of four norms (the 19-image one: the sum kernels stride the images by 16)
    (3, 64, 8, 8, 0.2, 1), (2, 576, 16, 16, 0.1, 0), (19, 64, 4, 4, 0.2, 1), (2, 256, 16, 16, 0.2, 0)]


def test_kept_per_image_terms_and_batched_param_sums(H):
    """vd_gn_apply_bwd_keep + ONE vd_gn_param_sums_batched over the arena, as engine._pgb / _pgb_finish lay it out, with dropout and FiLM:
    dgamma / dbeta against fp64 autograd (replayed mask), accumulating rows onto prefilled gradients and overwriting rows over NaN;
    every result also bit for bit that of the direct call (sum_over_images_kernel and its batched form add in the same order)."""
    GUARD = 64
    total = sum(n * 2 * c for n, c, *_ in NORMS)
    arena = torch.full((total + GUARD,), float("nan"), device=DEV)
    rows, kept, off, blk = [], [], 0, 0
    for i, (nimg, Cc, Hh, Ww, p, acc) in enumerate(NORMS):
        seed = SEED_HI + 2 * i + 1
        x = rnd(nimg, Cc, Hh, Ww, seed=10 + i) * 1.5 + 0.3
        gamma, beta = 1 + 0.1 * rnd(Cc, seed=20 + i), 0.1 * rnd(Cc, seed=30 + i)
        film, dy = 0.3 * rnd(nimg, 2 * Cc, seed=40 + i), rnd(nimg, Cc, Hh, Ww, seed=50 + i)
        pre_g, pre_b = (rnd(Cc, seed=60 + i), rnd(Cc, seed=70 + i)) if acc else (torch.full((Cc,), float("nan")),) * 2
        mask = replay(seed, p, nimg, Hh, Ww, Cc)

        def run(dt):
            xs, g, b_, fl = (v.to(dt).requires_grad_(True) for v in (x, gamma, beta, film))
            ref_gn_block(xs, g, b_, fl, True, 0, mask.to(dt)).backward(dy.to(dt))
            base = (pre_g.to(dt), pre_b.to(dt)) if acc else (0.0, 0.0)
            return xs.grad, g.grad + base[0], b_.grad + base[1], fl.grad
        r64, r32 = run(torch.float64), run(torch.float32)
        xd, gd, bd, fd, dyd = nhwc(x), gamma.to(DEV), beta.to(DEV), film.to(DEV), nhwc(dy)
        stats, coef = torch.empty(nimg, 32, 2, device=DEV), torch.empty(nimg, 4, Cc, device=DEV)
        H.gn_stats(xd, Cc, nimg, Hh * Ww, Cc, stats)
        y = torch.empty(nimg, Hh, Ww, Cc, device=DEV)
        H.gn_apply(xd, Cc, stats, gd, bd, fd, 1, p, seed, 0, y, Cc, nimg, Hh, Ww, Cc, coef)
        # the direct call: sums over the images in its own launch
        dx_d, df_d = torch.empty(nimg, Hh, Ww, Cc, device=DEV), torch.empty(nimg, 2 * Cc, device=DEV)
        dg_d, db_d = pre_g.to(DEV), pre_b.to(DEV)
        H.gn_apply_bwd(dyd, Cc, xd, Cc, coef, gd, bd, fd, 1, p, seed, 0, None, 0, dx_d, Cc, False, df_d, dg_d, db_d, bool(acc), nimg, Hh, Ww, Cc)
        # the keep call: per-image terms into this norm's slice of the arena, dgamma / dbeta not passed
        dx_k, df_k = torch.empty(nimg, Hh, Ww, Cc, device=DEV), torch.empty(nimg, 2 * Cc, device=DEV)
        dg_k, db_k = pre_g.to(DEV), pre_b.to(DEV)
        sl = arena[off: off + nimg * 2 * Cc]
        H.gn_apply_bwd(dyd, Cc, xd, Cc, coef, gd, bd, fd, 1, p, seed, 0, None, 0, dx_k, Cc, False, df_k, None, None, False, nimg, Hh, Ww, Cc,
                       pgb_keep=sl)
        torch.cuda.synchronize()
        for t, pre in ((dg_k, pre_g), (db_k, pre_b)):             # untouched until the batched launch
            assert torch.equal(t.cpu(), pre) if acc else torch.isnan(t).all()
        assert torch.isfinite(sl).all() and torch.isnan(arena[off + nimg * 2 * Cc:]).all(), "per-image terms outside the norm's slice"
        rows.append([sl.data_ptr(), dg_k.data_ptr(), db_k.data_ptr(), nimg, Cc, acc, 0, blk])
        kept.append(dict(i=i, dx_k=dx_k, df_k=df_k, dg_k=dg_k, db_k=db_k, dx_d=dx_d, df_d=df_d, dg_d=dg_d, db_d=db_d, r64=r64, r32=r32, Cc=Cc))
        off += nimg * 2 * Cc
        blk += (Cc + 15) // 16
    assert [r[7] for r in rows] == [0, 4, 40, 44] and blk == 60
    H.gn_param_sums_batched(torch.tensor(rows, dtype=torch.int64).to(DEV), len(rows), blk)
    torch.cuda.synchronize()
    assert torch.isnan(arena[total:]).all()
    for k in kept:
        (dx64, dg64, db64, df64), (dx32, dg32, db32, df32) = k["r64"], k["r32"]
        measured(from_nhwc(k["dx_k"], k["Cc"]), dx64, dx32, f"norm {k['i']} dx")
        measured(k["df_k"], df64, df32, f"norm {k['i']} dfilm")
        measured(k["dg_k"], dg64, dg32, f"norm {k['i']} dgamma (batched sums)")
        measured(k["db_k"], db64, db32, f"norm {k['i']} dbeta (batched sums)")
        assert torch.equal(k["dx_k"], k["dx_d"]) and torch.equal(k["df_k"], k["df_d"]), f"norm {k['i']}: keep call differs from the direct call"
        assert torch.equal(k["dg_k"], k["dg_d"]) and torch.equal(k["db_k"], k["db_d"]), f"norm {k['i']}: batched sums differ from the direct sums"
