"""Explicit forward/backward engine of the UNet on the HIP kernels (no autograd graph inside, no tracing compiler).

Replaces what ATen/cuDNN/cuBLAS + autograd do for reference ``UNet.forward`` (v_diffusion/models/unet.py:286-322),
``ResidualBlock.forward`` (:137-148) and ``AttentionBlock.forward`` (:55-81).

Data layout in HBM
  * activations: NHWC fp32 ``[B, H, W, C]`` torch buffers; a tensor handed between ops is a *view* whose
    ``stride(2)`` (= per-pixel stride ``ld``) may exceed C.  The concat of reference unet.py:315 is never
    materialised: each up-block owns one ``[B,H,W,Ch+Cs]`` buffer, the producer of ``h`` writes channels
    ``[0,Ch)`` and the producer of the skip tensor (a down-block, run much earlier) writes ``[Ch,Ch+Cs)``
    directly from their conv epilogues; gradients flow back the same way (the down-block's input gradient is
    accumulated into the skip slice of the up-block's input gradient).
  * weights stay in the reference's OIHW / (out,in) storage; the 3x3 kernels of the residual blocks are transformed per call
    into the Winograd domain by ONE launch for the whole network -- U = G w G^T as [16][Cout][Cin] (forward), [16][Cin][Cout]
    (F(2x2,3x3) input gradient) or the 36-plane lane-ordered image of csrc/wino43.hip (F(4x4,3x3) input gradient): 0.2 ms per
    train step, always coherent with whatever mutated the parameters (optimizer, load_state_dict, EMA swap through ``.data``).
    The direct [Cout][tap][Cin] / [Cin][tap'][Cout] packs exist only for geometries the Winograd kernels decline.
  * the tape (what backward needs) is a python list of per-block dicts of buffers; with 288 GB of HBM nothing is
    recomputed except the dropout mask (counter-based Philox, regenerated from (seed, element index)).
"""
import collections
import contextlib
import math

import torch

from . import _hip as H

GROUPS = 32
EPS = 1e-6
THIN = 8          # in/out convolutions with at most this many channels on the thin side take the GEMM + tap kernels


def _ld(t):
    return t.stride(2)


def _chk(t):
    B, Hh, Ww, C = t.shape
    ld = t.stride(2)
    assert t.stride(3) == 1 and t.stride(1) == Ww * ld and t.stride(0) == Hh * Ww * ld, "not an NHWC view"
    return B, Hh, Ww, C, ld


def _splitk(M, N, K, n=1):
    """split-K factor for the small-output weight-gradient GEMMs (K = batch*pixels); ``n`` = entries of a grouped launch"""
    tiles = ((M + 63) // 64) * ((N + 63) // 64) * n
    return max(1, min(64, 1024 // max(tiles, 1), K // 256))


# ---- the static plan: every fact the drivers below need about a block is stated HERE, once (_plan), and read from the record
_Spec = collections.namedtuple("_Spec", "prefix kind cin cout rs level consumes mods")          # a block as the module tree has it
# a skip-stack entry: block ``producer`` ("in_conv": the first) pushes ``cs`` channels, channels [ch, ch + cs) of block ``consumer``'s concat buffer
_Push = collections.namedtuple("_Push", "producer cs consumer ch")
# where an output goes: channels [c0, c0 + width) of the concat buffer of block ``cat``; cat None: a buffer of its own
_Dest = collections.namedtuple("_Dest", "cat c0 width")
# parameter-name suffixes of a residual / attention block in the order backward finishes their gradients, and those finished at the
# end of backward (GroupNorm scales / shifts: _pgb_finish)
_RES_GRADS = ("conv2.weight", "conv2.bias", "conv1.weight", "conv1.bias", "skip.weight", "skip.bias", "fc.weight", "fc.bias")
_RES_NORMS = ("norm2.weight", "norm2.bias", "norm1.weight", "norm1.bias")
_ATT_GRADS = ("proj_out.weight", "proj_out.bias", "proj_in.weight", "proj_in.bias")
_ATT_NORMS = ("norm.weight", "norm.bias")


class _Blk(collections.namedtuple("_Blk", _Spec._fields[:-1] + ("shift", "res", "att", "res_prefix", "att_prefix", "res_names", "att_names",
           "film", "seed", "src_hs", "push_hs", "ch_h", "in_hs", "dest", "grads", "norm_grads", "report", "ends_group"))):
    """One entry of the plan: a residual block, an attention block (kind "midattn") or a residual block followed by an attention block.
      prefix, kind ("down" / "mid" / "midattn" / "up"), cin, cout, level: as the module tree has them; rs: RS_* resampling in front of
          conv1, shift: levels its output lies below its input (+1 down-sampling, -1 up-sampling)
      res, att / res_prefix, att_prefix / res_names, att_names: the two modules (None: absent), their parameter-name prefixes (also
          their tape keys) and {suffix: parameter name}
      film: (2*cout, index) of the residual part in the batched FiLM projection of its width group; seed: dropout seed index
      consumes: its input is a concat buffer of cin = ch_h + Cs channels, [0, ch_h) from the previous block and the rest from
          skip-stack entry src_hs;  push_hs: the entry a down block pushes;  in_hs: the entry a block reads as its input WITHOUT popping
          it (down blocks and middle.0; None for the others) -- its input gradient accumulates into that entry's gradient
      dest: _Dest of its output
      grads: its parameter names in the order backward finishes them, norm_grads: those finished at the end of backward; report: the
          name backward yields when its gradients are final; ends_group: the last block backward runs of a (level, down / middle / up)
          group -- the deferred weight gradients are flushed and ``report`` is yielded there"""
    __slots__ = ()


def _plan(model):
    """(plan: [_Blk] in forward order, pushes: [_Push], film_groups: {2*cout: [residual modules]}) of a UNet module"""
    hid, mult, nrb = model.hid_channels, list(model.ch_multipliers), model.num_res_blocks
    levels = len(mult)
    chs = [hid * k for k in mult]
    specs = []
    for i in range(levels):                                                   # reference unet.py:250-263
        mods = model.downsamples[f"level_{i}"]
        prev = chs[i - 1] if i else hid
        for j in range(nrb):
            specs.append(_Spec(f"downsamples.level_{i}.{j}", "down", prev if j == 0 else chs[i], chs[i], H.RS_NONE, i, False, mods[j]))
        if i != levels - 1:
            specs.append(_Spec(f"downsamples.level_{i}.{nrb}", "down", chs[i], chs[i], H.RS_DOWN, i, False, mods[nrb]))
    for j, kind in enumerate(("mid", "midattn", "mid")):
        specs.append(_Spec(f"middle.{j}", kind, chs[-1], chs[-1], H.RS_NONE, levels - 1, False, model.middle[j]))
    for i in range(levels - 1, -1, -1):                                       # reference unet.py:265-284
        mods = model.upsamples[f"level_{i}"]
        nxt = hid if i == 0 else chs[i - 1]
        prv = chs[-1] if i == levels - 1 else chs[i + 1]
        for j, cin in enumerate([prv + chs[i]] + [2 * chs[i]] * (nrb - 1) + [nxt + chs[i]]):
            specs.append(_Spec(f"upsamples.level_{i}.{j}", "up", cin, chs[i], H.RS_NONE, i, True, mods[j]))
        if i != 0:
            specs.append(_Spec(f"upsamples.level_{i}.{nrb + 1}", "up", chs[i], chs[i], H.RS_UP, i, False, mods[nrb + 1]))
    # the skip stack, statically: which concat buffer does every pushed tensor land in, and who reads the stack top without popping it?
    pushes, stack = [["in_conv", hid, None, None]], [0]
    push_hs, src_hs, in_hs = {}, {}, {}
    for bi, s in enumerate(specs):
        if s.kind == "down" or s.prefix == "middle.0":
            in_hs[bi] = stack[-1]
        if s.kind == "down":
            pushes.append([bi, s.cout, None, None])
            stack.append(len(pushes) - 1)
            push_hs[bi] = stack[-1]
        elif s.consumes:
            k = src_hs[bi] = stack.pop()
            pushes[k][2:] = bi, s.cin - pushes[k][1]
    assert not stack, "skip stack not emptied"
    pushes = [_Push(*p) for p in pushes]
    group = lambda s: (s.level, "mid" if s.kind.startswith("mid") else s.kind)
    plan, film_groups = [], {}
    for bi, s in enumerate(specs):
        nxt = specs[bi + 1] if bi + 1 < len(specs) else None
        if s.kind == "midattn":
            res, att = None, s.mods
        else:
            res, att = (s.mods[0], s.mods[1]) if s.kind != "mid" and model.apply_attn[s.level] else (s.mods, None)
        res_prefix = None if res is None else s.prefix + (".0" if att is not None else "")
        att_prefix = None if att is None else s.prefix + (".1" if res is not None else "")
        res_names = {k: f"{res_prefix}.{k}" for k in _RES_GRADS + _RES_NORMS if s.cin != s.cout or not k.startswith("skip.")} if res else {}
        att_names = {k: f"{att_prefix}.{k}" for k in _ATT_GRADS + _ATT_NORMS} if att else {}
        grads = tuple(att_names[k] for k in _ATT_GRADS if att) + tuple(res_names[k] for k in _RES_GRADS if k in res_names)   # (backward
        norm_grads = tuple(att_names[k] for k in _ATT_NORMS if att) + tuple(res_names[k] for k in _RES_NORMS if res)         # runs att first)
        film = None
        if res is not None:                 # FiLM projections of equal width run as ONE batched GEMM per pass (_film_fwd)
            grp = film_groups.setdefault(2 * s.cout, [])
            film = (2 * s.cout, len(grp))
            grp.append(res)
        if s.kind == "down":
            p = pushes[push_hs[bi]]
            dest = _Dest(p.consumer, p.ch, p.cs)
        else:
            dest = _Dest(bi + 1 if nxt is not None and nxt.consumes else None, 0, s.cout)
        shift = {H.RS_DOWN: 1, H.RS_UP: -1}.get(s.rs, 0)
        assert nxt is None or nxt.level == s.level + shift, "a block's output is not at the next block's level"
        plan.append(_Blk(*s[:-1], shift, res, att, res_prefix, att_prefix, res_names, att_names, film, seed=2 * bi + 1,
                         src_hs=src_hs.get(bi), push_hs=push_hs.get(bi), ch_h=s.cin - pushes[src_hs[bi]].cs if s.consumes else None,
                         in_hs=in_hs.get(bi), dest=dest, grads=grads, norm_grads=norm_grads, report=grads[-1],
                         ends_group=bi == 0 or group(specs[bi - 1]) != group(s)))
    return plan, pushes, film_groups


class _Pack(collections.namedtuple("_Pack", "uf ud u43 u43f wf wd", defaults=(None,) * 6)):
    """Images of one 3x3 kernel; None = not packed for this weight set and geometry.  uf / ud: F(2x2,3x3) U = G w G^T as [16][Cout][Cin]
    (forward) / [16][Cin][Cout] (input gradient, rotated); u43f / u43: the 36-plane lane-ordered F(4x4,3x3) images of csrc/wino43.hip
    (forward / input gradient); wf / wd: the direct [Cout][tap][Cin] / [Cin][tap'][Cout] packs."""
    __slots__ = ()


_NO_PACK = _Pack()            # a kernel ConvPacks does not hold (in / out convolution, nothing packed yet)


class _NoGrads(dict):
    """the gradient set of the input-only backward pass (``backward(tape, dout, None, need_dx=True)``): every parameter's gradient
    tensor is None, and whoever would fill it launches nothing"""
    def __missing__(self, key):
        return None


_NO_GRADS = _NoGrads()


class ConvPacks:
    """Everything that belongs to the packed images of ONE weight set's residual-block 3x3 kernels at one (need_d, geometry): the
    persistent buffers (``bufs``), the per-layer views into them (``layers``: id(weight) -> _Pack), the device tables of the batched pack
    launches (``tables``: name -> (table, rows, blocks)) and the F(2x2,3x3) images made on demand (``fallback``).  Buffers and tables
    never move while the object lives, so a captured HIP graph stays valid for as long as it references the object.
    With H.WINO every layer gets Winograd-domain images -- F(4x4,3x3) for the directions ``geoms`` ([(weight, rows, H, W, Cin, Cout)],
    dense pitches) lets those kernels serve, F(2x2,3x3) otherwise; a layer served by F(4x4,3x3) gets no F(2x2,3x3) image for that direction
    (a call that declines asks image()) and the direct packs are made per tensor, on demand, by UNetEngine._pack_f / _pack_d for the
    geometries that fall back (none in the shipped configs).  Without H.WINO every layer gets the direct packs."""
    LAUNCHES = (("wino", "wino_pack_batched"), ("wino43", "wino43_pack_batched"), ("direct", "pack_conv3x3_batched"))

    def __init__(self, ws, need_d, geoms):
        dev, self.wino = ws[0].device, H.WINO
        use43 = {id(w): need_d and H.wino43_supported(nb, lh, lw, ci, co, co, ci) for (w, nb, lh, lw, ci, co) in geoms if self.wino}
        use43f = {id(w): H.wino43_fwd_supported(nb, lh, lw, ci, co, ci, co, co) for (w, nb, lh, lw, ci, co) in geoms if self.wino}

        def forms(w):                                     # [(field, buffer, shape)] of one layer, in the order the buffers are carved
            co, ci = w.shape[0], w.shape[1]
            if not self.wino:
                return [("wf", "wf", (co, 9, ci))] + ([("wd", "wd", (ci, 9, co))] if need_d else [])
            out = [("u43f", "u43", (36 * co * ci,)) if use43f.get(id(w)) else ("uf", "uf", (16, co, ci))]
            if need_d:
                out.append(("u43", "u43", (36 * co * ci,)) if use43.get(id(w)) else ("ud", "ud", (16, ci, co)))
            return out
        lay = [(w, forms(w)) for w in ws]
        self.bufs, self.layers, self.fallback = {}, {}, {}
        for name in ("uf", "ud", "u43", "wf", "wd"):
            n = sum(math.prod(shape) for _, fs in lay for _, buf, shape in fs if buf == name)
            if n:
                self.bufs[name] = torch.empty(n, dtype=torch.float32, device=dev)
        off = dict.fromkeys(self.bufs, 0)
        rows = {name: [] for name, _ in self.LAUNCHES}
        blocks = dict.fromkeys(rows, 0)

        def carve(buf, shape):                            # the next `shape` elements of a persistent buffer
            n = math.prod(shape)
            off[buf] += n
            return self.bufs[buf][off[buf] - n: off[buf]].view(shape)

        def row(tab, w, *cols, nblk):                     # [weight, destinations / flags ..., first block of the launch's grid]
            rows[tab].append([w.data_ptr()] + [c.data_ptr() if torch.is_tensor(c) else int(c or 0) for c in cols] + [blocks[tab]])
            blocks[tab] += nblk
        for w, fs in lay:
            p = self.layers[id(w)] = _Pack(**{field: carve(buf, shape) for field, buf, shape in fs})
            co, ci = w.shape[0], w.shape[1]
            if p.wf is not None:
                row("direct", w, p.wf, p.wd, co, ci, ci, co, nblk=(w.numel() + 255) // 256)
            if p.uf is not None or p.ud is not None:
                tiled = int(co % 16 == 0 and ci % 16 == 0)
                row("wino", w, p.uf, p.ud, co, ci, tiled, 0, nblk=(co // 16) * (ci // 16) if tiled else (co * ci + 255) // 256)
            if p.u43f is not None:
                row("wino43", w, p.u43f, 1, co, ci, 0, 0, nblk=(co // 32) * (ci // 8))
            if p.u43 is not None:
                row("wino43", w, p.u43, 0, co, ci, 0, 0, nblk=(ci // 32) * (co // 8))
        self.tables = {k: (torch.tensor(r, dtype=torch.int64).to(dev), len(r), blocks[k]) for k, r in rows.items() if r}

    def repack(self):
        """the images follow the weights as they are NOW: one batched launch per table"""
        for name, launch in self.LAUNCHES:
            if name in self.tables:
                getattr(H, launch)(*self.tables[name])

    def image(self, w, dgrad):
        """F(2x2,3x3) image -- rotated for the input gradient -- of a layer that was packed for an F(4x4,3x3) form: one allocation per
        (weight, direction) that lives with this object (stable address: also valid inside a captured HIP graph), re-packed on every
        call like every other image"""
        co, ci = w.shape[0], w.shape[1]
        U = self.fallback.get((id(w), dgrad))
        if U is None:
            U = self.fallback[(id(w), dgrad)] = torch.empty((16, ci, co) if dgrad else (16, co, ci), dtype=torch.float32, device=w.device)
        H.wino_pack(w, co, ci, **{"ud" if dgrad else "uf": U})
        return U


class _Cat:
    """The concat buffer ``[B,H,W,Ch+Cs]`` of one consuming up-block with the GroupNorm partials its two producers left behind
    (``parts``: channel offset -> what _parts returns)"""
    __slots__ = ("buf", "parts")

    def __init__(self, buf):
        self.buf, self.parts = buf, {}

    def joined(self, ch_h):
        """partials of the whole buffer -- both channel ranges, in channel order -- or None when a producer left none"""
        pa, pb = self.parts.get(0), self.parts.get(ch_h)
        return pa + pb if (pa is not None and pb is not None) else None


class UNetEngine:
    """Static execution plan + forward/backward drivers for one ``UNet`` module."""

    def __init__(self, model):
        self.m = model
        self.levels = len(model.ch_multipliers)
        # film_groups: FiLM projections (reference unet.py:129,143: one Linear per residual block, all fed by the SAME activated
        # embedding) of equal width, run as ONE batched GEMM per pass instead of a launch-latency-bound M = batch GEMM per block;
        # film_slot: residual-block prefix -> (2*Cout, index inside its group)
        self.plan, self.pushes, self.film_groups = _plan(model)
        self.film_slot = {b.res_prefix: b.film for b in self.plan if b.res is not None}
        self._pack_lru = {}               # {weight-set key: ConvPacks}, at most PACK_STATES_MAX (_pack_all)
        self._packs = None                # the ConvPacks of the forward (or backward) in flight
        self._fixed = None                # {} inside fixed_weights(): what one sampler chain packs once; None otherwise -- training repacks
                                          # every step because the optimizer rewrites the weights
        self._norm_channels = sum(p.numel() for k, p in model.named_parameters()
                                  if k.endswith(".weight") and p.ndim == 1)          # all GroupNorm weights (the only 1-D weights)
        self._pgb_arena = self._pgb_table = None
        self._side = self._side_stream = None     # side stream of the 3x3 weight gradients (VD_WGRAD_STREAM)
        self._wq = None                   # {shape key: [(dY, X, dW, dbias)]} of deferred weight-gradient GEMMs (inside backward only)
        self._active_run = None           # the chain-of-nodes backward pass in flight (models/unet.py::_BackwardRun), one at a time
        self._segments = None

    # ------------------------------------------------------------------------------------------ small helpers
    @staticmethod
    def _new(ref, *shape):
        return torch.empty(shape, dtype=torch.float32, device=ref.device)

    def _res_of(self, level, H0, W0):
        return H0 >> level, W0 >> level

    # ---- GroupNorm statistics ride on the producer: the conv / 1x1 epilogue that writes a tensor also leaves per-
    # (image, row-chunk, channel) sums behind, and the consuming norm only runs the tiny finalize (no read pass)
    def _part(self, ref, nimg, HW, C):
        if HW % 32:
            return None                                   # tiny images: the norm computes its own statistics
        return torch.empty(H.stats_part_numel(nimg, HW, C), dtype=torch.float32, device=ref.device)

    @staticmethod
    def _parts(part, C, HW, rows=None):
        """[(partials, channels, chunks per image)] of the launch that just wrote `part`.  ``rows`` = pixel rows per chunk as the launch
        that wrote it reported (what _conv returns); None: a vd_gemm launch made immediately before this call -- its chunk is half the
        row tile it picked (vd_gemm_last_tile)"""
        if part is None:
            return None
        return [(part, C, HW // (rows or (H.last_row_tile() // 2)))]

    def _norm(self, x, x_parts, gn, film, act, p_drop, seed, rs, y, B, Hh, Ww, C):
        """y = resample(dropout(act(FiLM(GroupNorm(x))))); returns the [B][4][C] coefficient table the backward pass needs.
        With producer partials the statistics never exist as a tensor: one tiny kernel goes from partials to the table."""
        coef = self._new(x, B, 4, C)
        stats = None
        # the folded form lets EVERY workgroup of the apply pass re-reduce the partials of the groups it touches: a few chunks (one per image
        # from the F(4x4,3x3) forward kernel, four on 64-wide images) cost nothing, HW / 64 of them (tile-engine / F(2x2,3x3) producers on
        # 32x32 and larger images) would be read back by every 64-pixel workgroup -- those keep the separate finalize launch
        if x_parts is not None and H.GN_FOLD and max(k for _, _, k in x_parts) <= H.GN_FOLD_MAX_CHUNKS:
            H.gn_apply_from_partials(x, _ld(x), x_parts, gn.weight, gn.bias, film, act, p_drop, seed, rs, y, _ld(y), B, Hh, Ww, C, coef,
                                     GROUPS, EPS)
            return coef
        if x_parts is not None:
            H.gn_coef_from_partials(x_parts, B, Hh * Ww, gn.weight, gn.bias, film, coef, GROUPS, EPS)
        else:
            stats = self._new(x, B, GROUPS, 2)
            H.gn_stats(x, _ld(x), B, Hh * Ww, C, stats, GROUPS, EPS)
        H.gn_apply(x, _ld(x), stats, gn.weight, gn.bias, film, act, p_drop, seed, rs, y, _ld(y), B, Hh, Ww, C, coef, GROUPS)
        return coef

    # ---- 1x1-convolution / linear weight gradients dW = dY^T X (skip, proj_in, proj_out, fc): nothing downstream in backward
    # depends on them, so they are queued per shape and run as ONE grouped launch per shape at the end of a UNet level
    # (vd_gemm_grouped_wgrad) instead of one short split-K GEMM + one slab reduction per block.  The queue keeps the operands alive.
    def _wgrad(self, dy, x, dw, db, M, N, K, lda, ldb, ldc):
        if self._wq is None or not H.GROUPED_WGRAD:
            H.gemm(dy, x, dw, M, N, K, a_kind=H.COL, b_kind=H.COL, lda=lda, ldb=ldb, ldc=ldc, splitk=_splitk(M, N, K), colsum=db)
            return
        key = (M, N, K, lda, ldb, ldc, db is not None)
        q = self._wq.setdefault(key, [])
        q.append((dy, x, dw, db))
        if len(q) == H.GROUP_MAX:
            self._wgrad_flush_key(key)

    # ---- weight gradients on a side stream: nothing downstream in backward reads them, so they run beside the input-gradient /
    # GroupNorm chain of the following blocks (an HBM-bound transform or GroupNorm pass next to an MFMA-bound GEMM or convolution instead
    # of after it).  The side stream waits for the main stream before every launch (its operands are final), the operands are marked as
    # used on it (the caching allocator must not hand their memory out while it still reads them), and the main stream waits for it
    # wherever a gradient is declared complete: at every `progress` call when a reducer listens, else once at the end of backward.
    # Results are bitwise those of the one-stream order (every gradient tensor has one writer); per-kernel profiling (H.PROFILE) runs
    # on one stream so that a kernel's events bracket that kernel alone.
    def _cwgrad(self, x, ldx, dy, lddy, *args, v=None, **kw):
        if v is not None:                      # the forward went through planes and kept V in place of x (_conv): the transform of x is skipped
            kw["v"] = v
        side = self._side
        if side is None:
            return H.conv3x3_wgrad(x, ldx, dy, lddy, *args, **kw)
        side.wait_stream(torch.cuda.current_stream())
        (x if v is None else v).record_stream(side)
        dy.record_stream(side)
        with torch.cuda.stream(side):
            H.conv3x3_wgrad(x, ldx, dy, lddy, *args, **kw)

    def _conv_bwd_planes(self, w, v, dy, lddy, dx, lddx, B, Hh, Ww, Cin, Cout, gw, gb):
        """Both gradients of a Cin -> Cout convolution whose forward kept V, from ONE image of dy: the main stream writes dM = A dY A^T, the
        side stream runs the weight gradient on (V, dM), the main stream goes on with the input gradient through planes (dM -> dx).  False
        (nothing launched): no V, or the rule / this call's pitches decline -- the caller takes the fused kernels as before.  ``gw`` None
        (the input-only pass): the weight-gradient half is not launched; dM and the input gradient are those of the full pass."""
        if v is None or not H.dgrad_planes_supported(B, Hh, Ww, Cin, Cout, lddy, lddx):
            return False
        dm = torch.empty(H.lib().vd_conv3x3_wino43_dm_floats(B, Hh, Ww, Cout), dtype=torch.float32, device=dy.device)
        H.conv3x3_wino43_dy_image(dy, lddy, B, Hh, Ww, Cout, dm)
        side = self._side
        if gw is None:
            pass
        elif side is None:
            H.conv3x3_wgrad_wino43_vm(v, dm, B, Hh, Ww, Cin, Cout, gw, Cin, Cout, dbias=gb)
        else:
            side.wait_stream(torch.cuda.current_stream())
            v.record_stream(side)
            dm.record_stream(side)
            with torch.cuda.stream(side):
                H.conv3x3_wgrad_wino43_vm(v, dm, B, Hh, Ww, Cin, Cout, gw, Cin, Cout, dbias=gb)
        H.conv3x3_wino43_dgrad_planes(dm, w, dx, lddx, B, Hh, Ww, Cin, Cout)
        return True

    def _side_join(self):
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)

    def _wgrad_flush_key(self, key):
        q = self._wq.pop(key, None)
        if not q:
            return
        M, N, K, lda, ldb, ldc, _ = key
        # the grouped launch exists on the LDS-DMA tile engine only: every entry needs what that kernel needs (16-byte aligned operands,
        # pitches that are multiples of 4 floats and inside its 32-bit offset range); anything else takes the per-entry launches
        ok = M % 4 == 0 and N % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and max(lda, ldb, ldc) * 128 + 128 < 0x70000000 // 4 and \
            all(dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 for dy, x, _, _ in q)
        if len(q) == 1 or not ok:
            for dy, x, dw, db in q:
                H.gemm(dy, x, dw, M, N, K, a_kind=H.COL, b_kind=H.COL, lda=lda, ldb=ldb, ldc=ldc, splitk=_splitk(M, N, K), colsum=db)
            return
        # slab count that fills whole residency rounds of the chip (vd_gemm_grouped_wgrad_auto_split), or the per-entry rule over all tiles
        S = H.lib().vd_gemm_grouped_wgrad_auto_split(len(q), M, N, K, 1, 64) if H.GROUPED_AUTO_SPLIT else _splitk(M, N, K, len(q))
        H.gemm_grouped_wgrad(q, M, N, K, lda, ldb, ldc, S)

    def _wgrad_flush(self):
        if not self._wq:
            return
        side = self._side
        if side is None:
            for key in list(self._wq):
                self._wgrad_flush_key(key)
            return
        side.wait_stream(torch.cuda.current_stream())
        for q in self._wq.values():
            for dy, x, _, _ in q:
                dy.record_stream(side)
                x.record_stream(side)
        with torch.cuda.stream(side):
            for key in list(self._wq):
                self._wgrad_flush_key(key)

    # ---- GroupNorm parameter gradients: every norm's backward leaves its per-image dgamma / dbeta terms in a slice of one arena and
    # ONE launch at the end of backward sums them over the images for all norms (73 five-microsecond launches per CIFAR step before)
    def _pgb_begin(self, ref, B):
        need = B * 2 * self._norm_channels
        if self._pgb_arena is None or self._pgb_arena.numel() < need or self._pgb_arena.device != ref.device:
            self._pgb_arena = torch.empty(need, dtype=torch.float32, device=ref.device)
            self._pgb_table = None
        self._pgb_rows, self._pgb_off, self._pgb_blk = [], 0, 0

    def _pgb(self, B, C, dgamma, dbeta):
        """the slice of the arena a norm's backward leaves its per-image terms in; ``dgamma`` None (the input-only pass): the slice is
        scratch that nothing sums"""
        sl = self._pgb_arena[self._pgb_off: self._pgb_off + B * 2 * C]
        if dgamma is not None:
            self._pgb_rows.append([sl.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), B, C, 0, 0, self._pgb_blk])
        self._pgb_off += B * 2 * C
        self._pgb_blk += (C + 15) // 16
        return sl

    def _pgb_finish(self):
        key = tuple(tuple(r) for r in self._pgb_rows)
        if self._pgb_table is None or self._pgb_table[0] != key:            # (flat gradient buffers: built once)
            self._pgb_table = (key, torch.tensor(self._pgb_rows, dtype=torch.int64).to(self._pgb_arena.device))
        H.gn_param_sums_batched(self._pgb_table[1], len(self._pgb_rows), self._pgb_blk)

    PACK_STATES_MAX = 4       # weight sets (raw / EMA) x (training / inference) whose packed images are kept at a time

    def _conv_geoms(self, B, H0, W0):
        """[(weight, rows, H, W, Cin, Cout)] of every residual-block convolution for a (B, C, H0, W0) input: the resolution its two
        convolutions run at (a down-sampling block pools in front of conv1, an up-sampling block up-samples in front of it)"""
        out = []
        for b in self.plan:
            if b.res is None:
                continue
            lh, lw = H._resampled(*self._res_of(b.level, H0, W0), b.rs)
            out.append((b.res.conv1.weight, B, lh, lw, b.cin, b.cout))
            out.append((b.res.conv2.weight, B, lh, lw, b.cout, b.cout))
        return out

    def _pack_all(self, need_d, geom=None):
        """Re-pack the 3x3 kernels of every residual block (ConvPacks.repack: ONE launch per image family for the whole network) and
        make the result ``self._packs``, the packs of the forward in flight.  The ConvPacks objects are kept PER WEIGHT SET -- the key
        is the parameters' storage pointers, so raw weights and an EMA view swap (trainer.ema_weights) each keep their own stable
        buffers and tables instead of freeing and re-allocating them on every alternation -- in a small LRU; whoever still needs an
        evicted one (a tape, a captured HIP graph: diffusion._sample_loop_graph) holds a reference to it.
        ``geom`` = (B, H0, W0) of the input: the layers the F(4x4,3x3) kernels serve at that geometry take those images."""
        ws = [c.weight for b in self.plan if b.res is not None for c in (b.res.conv1, b.res.conv2)]
        key = (bool(need_d), H.WINO, H.WINO43_FWD, geom) + tuple(w.data_ptr() for w in ws)
        pk = self._pack_lru.pop(key, None)               # (re-inserted below as the most recent entry)
        if pk is None:
            pk = ConvPacks(ws, need_d, self._conv_geoms(*geom) if geom is not None else [])
            while len(self._pack_lru) >= self.PACK_STATES_MAX:
                self._pack_lru.pop(next(iter(self._pack_lru)))          # least recently used
        self._pack_lru[key] = self._packs = pk
        pk.repack()
        return pk

    @property
    def packs(self):
        """the ConvPacks of the last forward (or of the backward in flight): what a captured graph of that forward must keep alive"""
        return self._packs

    @contextlib.contextmanager
    def fixed_weights(self):
        """A sampler holds the weights fixed for one reverse chain: inside the context the first forward's ConvPacks, the FiLM stacks and
        the thin-kernel / input-convolution images are made once and every later forward uses THEM, whatever was packed in between."""
        self._fixed = {}
        try:
            yield
        finally:
            self._fixed = None

    def _layer(self, w):
        """the images the packs in flight hold for kernel ``w``"""
        return self._packs.layers.get(id(w), _NO_PACK) if self._packs is not None else _NO_PACK

    def _conv(self, x, ldx, w, bias, y, ldy, B, Hh, Ww, Cin, Cout, dgrad=False, res=None, ldres=0, stats_part=None, keep_v=None):
        """3x3 convolution with kernel ``w`` (forward) or its input gradient (``dgrad``: x = dy, Cin/Cout are the GEMM's):
        Winograd F(4x4,3x3) / F(2x2,3x3) wherever the geometry is served, the direct implicit GEMM otherwise.  Returns the pixel rows per
        chunk of the GroupNorm partial sums it left in ``stats_part`` (the consuming norm needs the chunk count: _parts).
        ``keep_v`` (a list, training forwards with a tape): a forward that goes through planes appends the V image it made -- the tape
        keeps it in place of ``x``, which only the weight gradient would read."""
        pk, p = self._packs, self._layer(w)
        if not dgrad and p is not _NO_PACK and pk.wino and H.conv_planes_supported(B, Hh, Ww, Cin, Cout, ldx, ldy, ldres if res is not None else 0,
                                                                                 training=keep_v is not None):
            v = None
            if keep_v is not None:
                v = torch.empty(36 * B * (Hh // 4) * (Ww // 4) * Cin, dtype=torch.float32, device=x.device)
                keep_v.append(v)
            H.conv3x3_wino43_fwd_planes(x, ldx, w, bias, y, ldy, B, Hh, Ww, Cin, Cout, res=res, ldres=ldres, stats_part=stats_part, v=v)
            return H.wino43_fwd_chunk_rows(Hh, Ww)
        if not dgrad and p.u43f is not None and H.wino43_fwd_supported(B, Hh, Ww, Cin, Cout, ldx, ldy, ldres if res is not None else 0):
            # forward pass through F(4x4,3x3) (csrc/wino43.hip, dyadic interpolation points); its GroupNorm partials come one chunk per
            # (image, work item)
            H.conv3x3_wino43_fwd(x, ldx, p.u43f, bias, y, ldy, B, Hh, Ww, Cin, Cout, res=res, ldres=ldres, stats_part=stats_part)
            return H.wino43_fwd_chunk_rows(Hh, Ww)
        if dgrad and p.u43 is not None and H.wino43_supported(B, Hh, Ww, Cout, Cin, ldx, ldy):
            # F(4x4,3x3) input gradient (csrc/wino43.hip): x = dy [.., Cin = conv Cout], y = dx [.., Cout = conv Cin].  The pack-time choice
            # (ConvPacks) saw dense pitches; the check above is the one with the pitches of THIS call (dy may be a channel slice of a concat
            # buffer) and of this geometry -- a layer it declines falls through to the F(2x2,3x3) / direct forms below.
            assert res is None and bias is None and stats_part is None
            H.conv3x3_dgrad_wino43(x, ldx, p.u43, y, ldy, B, Hh, Ww, Cout, Cin)
            return None
        if p is not _NO_PACK and pk.wino and H.wino_supported(B, Hh, Ww, Cin, Cout, ldx, ldy, ldres if res is not None else 0):
            U = p.ud if dgrad else p.uf
            if U is None:                              # packed for an F(4x4,3x3) form that THIS call's pitches declined
                U = pk.image(w, dgrad)
            H.conv3x3_wino(x, ldx, U, bias, y, ldy, B, Hh, Ww, Cin, Cout, res=res, ldres=ldres, stats_part=stats_part)
            return H.last_row_tile() // 2              # the F(2x2,3x3) kernels: one chunk per 64 output rows, reported like a 128-row tile
        H.conv3x3(x, ldx, self._pack_d(w) if dgrad else self._pack_f(w), bias, y, ldy, B, Hh, Ww, Cin, Cout, res=res, ldres=ldres,
                  stats_part=stats_part)
        return H.last_row_tile() // 2                  # the tile engine: half its row tile

    def _pack_f(self, w, cin_p=None):
        p = self._layer(w)
        if p.wf is not None:
            return p.wf
        cache = self._fixed
        if cache is not None and id(w) in cache:
            return cache[id(w)]
        co, ci = w.shape[0], w.shape[1]
        cin_p = cin_p or ci
        wf = self._new(w, co, 9, cin_p)
        H.pack_conv3x3(w, co, ci, wf=wf, Cin_p=cin_p)
        if cache is not None:
            cache[id(w)] = wf
        return wf

    def _pack_d(self, w, cout_p=None):
        p = self._layer(w)
        if p.wd is not None:
            return p.wd
        cache, key = self._fixed, ("wd", id(w))              # (a chain that takes input gradients packs the input convolution's once)
        if cache is not None and key in cache:
            return cache[key]
        co, ci = w.shape[0], w.shape[1]
        cout_p = cout_p or co
        wd = self._new(w, ci, 9, cout_p)
        H.pack_conv3x3(w, co, ci, wd=wd, Cout_p=cout_p)
        if cache is not None:
            cache[key] = wd
        return wd

    def _pack_thin(self, w, rows):
        """[rows][Cin] image of a thin-output 3x3 kernel: row co*9+tap = w[co][:, tap], rows beyond 9*Cout are zero"""
        cache = self._fixed
        key = ("thin", id(w))
        if cache is not None and key in cache:
            return cache[key]
        co, ci = w.shape[0], w.shape[1]
        wz = torch.zeros((rows, ci), dtype=torch.float32, device=w.device)
        H.pack_conv3x3(w, co, ci, wf=wz, Cin_p=ci)
        if cache is not None:
            cache[key] = wz
        return wz

    @staticmethod
    def _linear(x, w, b, out, accumulate=False):
        """out[M,N] (+)= x[M,K] @ w[N,K]^T + b"""
        M, K = x.shape
        N = w.shape[0]
        H.gemm(x, w, out, M, N, K, a_kind=H.ROW, b_kind=H.ROW, lda=x.stride(0), ldb=w.stride(0), ldc=out.stride(0), bias=b,
               accumulate=accumulate)

    def _linear_bwd(self, x, w, dy, dw, db, dx, dx_accumulate=False):
        """dw[N,K] = dy^T x ; db[N] = colsum(dy) ; dx[M,K] (+)= dy @ w"""
        M, K = x.shape
        N = w.shape[0]
        self._wgrad(dy, x, dw, db, N, K, M, dy.stride(0), x.stride(0), K)      # db = column sums of dy, from the same staged tiles
        if dx is not None:
            H.gemm(dy, w, dx, M, K, N, a_kind=H.ROW, b_kind=H.COL, lda=dy.stride(0), ldb=w.stride(0), ldc=dx.stride(0),
                   accumulate=dx_accumulate)

    # ------------------------------------------------------------------------------------------ embeddings
    def _embed_fwd(self, t, y, tape):
        m = self.m
        B = t.shape[0]
        dev_ref = m.in_conv.weight
        if t.dtype != torch.float64:
            t = t.to(torch.float64)
        te0 = self._new(dev_ref, B, m.hid_channels)
        H.timestep_embedding(t.contiguous(), te0, B, m.hid_channels)
        l0, l2 = m.time_embed[0], m.time_embed[2]
        h0 = self._new(dev_ref, B, m.embedding_dim)
        self._linear(te0, l0.weight, l0.bias, h0)
        a0 = torch.empty_like(h0)
        H.silu(h0, a0)
        te = torch.empty_like(h0)
        self._linear(a0, l2.weight, l2.bias, te)
        yn = None
        if m.num_classes and y is not None:
            y = y.to(torch.float32).contiguous().clone()      # callers mutate y after the forward (diffusion.py:527-529)
            if m.multitags:
                assert y.ndim == 2 and y.shape[1] == m.num_classes
                yn = torch.empty_like(y)
                H.multitag_norm(y, yn, B, m.num_classes)
                self._linear(yn, m.class_embed.weight, m.class_embed.bias, te, accumulate=True)
            else:
                lin = m.class_embed[1]
                H.class_embed(y.reshape(-1), lin.weight, lin.bias, te, B, m.embedding_dim, m.num_classes)
                yn = y.reshape(-1)
        ta = torch.empty_like(te)
        H.silu(te, ta)
        if tape is not None:
            tape["embed"] = dict(te0=te0, h0=h0, a0=a0, te=te, yn=yn)
        return ta

    def _embed_bwd(self, ctx, dta, G):
        m = self.m
        B = dta.shape[0]
        te0, h0, a0, te, yn = ctx["te0"], ctx["h0"], ctx["a0"], ctx["te"], ctx["yn"]
        dte = torch.empty_like(dta)
        H.silu_bwd(te, dta, dte)
        if yn is not None:
            if m.multitags:
                self._linear_bwd(yn, m.class_embed.weight, dte, G["class_embed.weight"], G["class_embed.bias"], None)
            else:
                H.class_embed_bwd(yn, dte, G["class_embed.1.weight"], G["class_embed.1.bias"], B, m.embedding_dim, m.num_classes)
        elif m.num_classes:
            # class-conditional network called without labels: the reference leaves these gradients None and its optimizer
            # skips them; every entry of G must be written (flat buffers are reused across steps), so they are exact zeros
            # here and HotPathTrainer.step tells the fused optimizer kernel to leave that range alone (vd_adamw_ema r_mode 1:
            # no moment decay, no weight decay, no update, step not advanced -- what torch.optim.AdamW does for grad None)
            for k in G:
                if k.startswith("class_embed."):
                    G[k].zero_()
        l0, l2 = m.time_embed[0], m.time_embed[2]
        da0 = torch.empty_like(dte)
        self._linear_bwd(a0, l2.weight, dte, G["time_embed.2.weight"], G["time_embed.2.bias"], da0)
        dh0 = torch.empty_like(da0)
        H.silu_bwd(h0, da0, dh0)
        self._linear_bwd(te0, l0.weight, dh0, G["time_embed.0.weight"], G["time_embed.0.bias"], None)

    # ------------------------------------------------------------------------------------------ FiLM projections
    def _film_fwd(self, ta, tape):
        """film[g][i] = fc_i(ta) for every residual block i of width group g: [nb][B][2*Cout], one launch per group"""
        B, E = ta.shape
        films, stacks = {}, {}
        cache = self._fixed
        for c2, mods in self.film_groups.items():
            key = ("film", c2)
            if cache is not None and key in cache:
                W, bv = cache[key]
            else:
                W = torch.stack([mm.fc.weight.detach() for mm in mods])          # [nb][2C][E]
                bv = torch.stack([mm.fc.bias.detach() for mm in mods])           # [nb][2C]
                if cache is not None:
                    cache[key] = (W, bv)
            nb = len(mods)
            out = self._new(ta, nb, B, c2)
            H.gemm(ta, W, out, B, c2, E, a_kind=H.ROW, b_kind=H.ROW, lda=E, ldb=E, ldc=c2, bias=bv, sBias=c2, batch=nb,
                   sA=(0, 0), sB=(c2 * E, 0), sC=(B * c2, 0))
            films[c2], stacks[c2] = out, W
        if tape is not None:
            tape["film_w"] = stacks
        return films

    def _film_bwd(self, dfilms, stacks, dta):
        """dta += sum_i dfilm_i @ W_i : one batched GEMM per width group into per-block partials + one column sum"""
        B, E = dta.shape
        for c2, df in dfilms.items():
            nb, W = df.shape[0], stacks[c2]
            P = self._new(dta, nb, B * E)
            H.gemm(df, W, P, B, E, c2, a_kind=H.ROW, b_kind=H.COL, lda=c2, ldb=E, ldc=E, batch=nb, sA=(B * c2, 0), sB=(c2 * E, 0),
                   sC=(B * E, 0))
            H.colsum(P, B * E, nb, B * E, dta.view(-1), accumulate=True)

    # ------------------------------------------------------------------------------------------ residual block
    def _res_fwd(self, blk, x, films, dest, p_drop, seed, tape, x_parts=None):
        mod, prefix = blk.res, blk.res_prefix
        B, Hh, Ww, Cin, ldx = _chk(x)
        Cout, rs = blk.cout, blk.rs
        Ho, Wo = H._resampled(Hh, Ww, rs)
        a1 = self._new(x, B, Ho, Wo, Cin)
        coef1 = self._norm(x, x_parts, mod.norm1, None, 1, 0.0, 0, rs, a1, B, Hh, Ww, Cin)
        h1 = self._new(x, B, Ho, Wo, Cout)
        ph = self._part(x, B, Ho * Wo, Cout)
        v1, v2 = ([], []) if tape is not None else (None, None)
        rows = self._conv(a1, Cin, mod.conv1.weight, mod.conv1.bias, h1, Cout, B, Ho, Wo, Cin, Cout, stats_part=ph, keep_v=v1)
        h1_parts = self._parts(ph, Cout, Ho * Wo, rows)
        c2, fi = blk.film
        film = films[c2][fi]                              # [B][2*Cout], contiguous slice of the group's batched GEMM output
        a2 = self._new(x, B, Ho, Wo, Cout)
        coef2 = self._norm(h1, h1_parts, mod.norm2, film, 1, p_drop, seed, H.RS_NONE, a2, B, Ho, Wo, Cout)
        if rs != H.RS_NONE:
            xs = self._new(x, B, Ho, Wo, Cin)
            H.gn_apply(x, ldx, None, None, None, None, 0, 0.0, 0, rs, xs, Cin, B, Hh, Ww, Cin, None, GROUPS)
        else:
            xs = x
        has_skip = Cin != Cout
        if has_skip:
            sk = self._new(x, B, Ho, Wo, Cout)
            w = mod.skip.weight
            H.gemm(xs, w, sk, B * Ho * Wo, Cout, Cin, a_kind=H.ROW, b_kind=H.ROW, lda=_ld(xs), ldb=Cin, ldc=Cout, bias=mod.skip.bias)
        else:
            sk = xs
        pd = self._part(x, B, Ho * Wo, Cout)
        rows = self._conv(a2, Cout, mod.conv2.weight, mod.conv2.bias, dest, _ld(dest), B, Ho, Wo, Cout, Cout, res=sk,
                          ldres=_ld(sk), stats_part=pd, keep_v=v2)
        out_parts = self._parts(pd, Cout, Ho * Wo, rows)
        if tape is not None:
            # (a convolution that went through planes left its V image: the tape keeps that in place of the activation)
            tape[prefix] = dict(x=x, coef1=coef1, a1=None if v1 else a1, h1=h1, coef2=coef2, a2=None if v2 else a2, film=film,
                                xs=xs if has_skip else None, seed=seed, p=p_drop, v1=v1[0] if v1 else None, v2=v2[0] if v2 else None)
        return out_parts

    def _res_bwd(self, blk, ctx, dy, dx, dx_accumulate, ta, dfilms, G):
        """``G`` None: the input-only pass -- the dx chain's launches with their arguments, none of the weight-gradient ones"""
        mod = blk.res
        only_dx = G is None
        g = _NO_GRADS if only_dx else {s: G[name] for s, name in blk.res_names.items()}      # this block's gradient tensors by parameter-name suffix
        x, a1, h1, a2, film = ctx["x"], ctx["a1"], ctx["h1"], ctx["a2"], ctx["film"]
        B, Hh, Ww, Cin, ldx = _chk(x)
        _, Ho, Wo, Cout, lddy = _chk(dy)
        rs = blk.rs
        # conv2
        da2 = self._new(x, B, Ho, Wo, Cout)
        if not self._conv_bwd_planes(mod.conv2.weight, ctx["v2"], dy, lddy, da2, Cout, B, Ho, Wo, Cout, Cout, g["conv2.weight"], g["conv2.bias"]):
            if not only_dx:
                self._cwgrad(a2, Cout, dy, lddy, B, Ho, Wo, Cout, Cout, g["conv2.weight"], Cout, Cout, dbias=g["conv2.bias"], v=ctx["v2"])
            self._conv(dy, lddy, mod.conv2.weight, None, da2, Cout, B, Ho, Wo, Cout, Cout, dgrad=True)
        # norm2 + FiLM + SiLU + dropout
        dh1 = self._new(x, B, Ho, Wo, Cout)
        c2, fi = blk.film
        dfilm = dfilms[c2][0 if only_dx else fi]          # (input-only: one scratch slot per width, never summed)
        H.gn_apply_bwd(da2, Cout, h1, Cout, ctx["coef2"], mod.norm2.weight, mod.norm2.bias, film, 1, ctx["p"], ctx["seed"],
                       H.RS_NONE, None, 0, dh1, Cout, False, dfilm, None, None, False, B, Ho, Wo, Cout, GROUPS,
                       pgb_keep=self._pgb(B, Cout, g["norm2.weight"], g["norm2.bias"]))
        del da2
        # conv1
        da1 = self._new(x, B, Ho, Wo, Cin)
        if not self._conv_bwd_planes(mod.conv1.weight, ctx["v1"], dh1, Cout, da1, Cin, B, Ho, Wo, Cin, Cout, g["conv1.weight"], g["conv1.bias"]):
            if not only_dx:
                self._cwgrad(a1, Cin, dh1, Cout, B, Ho, Wo, Cin, Cout, g["conv1.weight"], Cin, Cout, dbias=g["conv1.bias"], v=ctx["v1"])
            self._conv(dh1, Cout, mod.conv1.weight, None, da1, Cin, B, Ho, Wo, Cout, Cin, dgrad=True)
        del dh1
        # skip path
        if Cin != Cout:
            xs = ctx["xs"]
            P = B * Ho * Wo
            w = mod.skip.weight
            if not only_dx:
                self._wgrad(dy, xs, g["skip.weight"], g["skip.bias"], Cout, Cin, P, lddy, _ld(xs), Cin)
            dsk = self._new(x, B, Ho, Wo, Cin)
            H.gemm(dy, w, dsk, P, Cin, Cout, a_kind=H.ROW, b_kind=H.COL, lda=lddy, ldb=Cin, ldc=Cin)
        else:
            dsk = dy
        if rs != H.RS_NONE:
            addt = self._new(x, B, Hh, Ww, Cin)
            H.gn_apply_bwd(dsk, _ld(dsk), None, 0, None, None, None, None, 0, 0.0, 0, rs, None, 0, addt, Cin, False, None, None,
                           None, False, B, Hh, Ww, Cin, GROUPS)
        else:
            addt = dsk
        # norm1 + SiLU (+ resample) and the sum with the skip-path gradient
        H.gn_apply_bwd(da1, Cin, x, ldx, ctx["coef1"], mod.norm1.weight, mod.norm1.bias, None, 1, 0.0, 0, rs, addt, _ld(addt),
                       dx, _ld(dx), dx_accumulate, None, None, None, False, B, Hh, Ww, Cin, GROUPS,
                       pgb_keep=self._pgb(B, Cin, g["norm1.weight"], g["norm1.bias"]))
        # FiLM projection film = fc(ta): weight/bias gradient here (keeps the gradient-completion order); the embedding
        # gradient of all blocks is one batched GEMM at the end of backward (_film_bwd)
        if not only_dx:
            self._linear_bwd(ta, mod.fc.weight, dfilm, g["fc.weight"], g["fc.bias"], None)

    # ------------------------------------------------------------------------------------------ attention block
    def _attn_fwd(self, blk, x, dest, tape, x_parts=None):
        mod, prefix = blk.att, blk.att_prefix
        B, Hh, Ww, C, ldx = _chk(x)
        L, nh, hd = Hh * Ww, mod.num_heads, mod.head_dim
        hid = nh * hd
        xn = self._new(x, B, Hh, Ww, C)
        coef = self._norm(x, x_parts, mod.norm, None, 0, 0.0, 0, H.RS_NONE, xn, B, Hh, Ww, C)
        qkv = self._new(x, B, L, 3 * hid)
        H.gemm(xn, mod.proj_in.weight, qkv, B * L, 3 * hid, C, a_kind=H.ROW, b_kind=H.ROW, lda=C, ldb=C, ldc=3 * hid,
               bias=mod.proj_in.bias)
        ld = 3 * hid
        alpha = 1.0 / math.sqrt(hd)
        q, k, v = qkv[0, 0, 0:], qkv[0, 0, hid:], qkv[0, 0, 2 * hid:]
        O = self._new(x, B, L, hid)
        S = lse = None
        if B * nh <= 65535 and H.attn_use_fused(L, hd, B * nh, tape is not None):
            # fused kernels (csrc/attn.hip): the [B, nh, L, L] maps never reach HBM; the backward recomputes them from the
            # per-row log-sum-exp.  Which shapes take them in training is decided by measurement (_hip.attn_use_fused).
            if tape is not None:
                lse = self._new(x, B * nh * L)
            H.attn_fwd(q, k, v, ld, O, hid, lse, B, nh, L, hd, alpha)
        else:
            S = self._new(x, B, nh, L, L)
            H.gemm(q, k, S, L, L, hd, a_kind=H.ROW, b_kind=H.ROW, lda=ld, ldb=ld, ldc=L, batch=B * nh, nh=nh, sA=(L * ld, hd),
                   sB=(L * ld, hd), sC=(nh * L * L, L * L), alpha=alpha)
            H.softmax_rows(S, B * nh * L, L)
            H.gemm(S, v, O, L, hd, L, a_kind=H.ROW, b_kind=H.COL, lda=L, ldb=ld, ldc=hid, batch=B * nh, nh=nh, sA=(nh * L * L, L * L),
                   sB=(L * ld, hd), sC=(L * hid, hd))
        pd = self._part(x, B, L, C)
        if pd is not None and L % 64:
            pd = None                                     # the plain GEMM picks its own row tile: only ask when any tile fits
        H.gemm(O, mod.proj_out.weight, dest, B * L, C, hid, a_kind=H.ROW, b_kind=H.ROW, lda=hid, ldb=hid, ldc=_ld(dest),
               bias=mod.proj_out.bias, R=x, ldr=ldx, stats=pd, stats_hw=L)
        out_parts = self._parts(pd, C, L)
        if tape is not None:
            tape[prefix] = dict(x=x, coef=coef, xn=xn, qkv=qkv, P=S, O=O, lse=lse)
        return out_parts

    def _attn_bwd(self, blk, ctx, dy, dx, dx_accumulate, G):
        mod = blk.att
        only_dx = G is None                                   # the input-only pass: see _res_bwd
        g = _NO_GRADS if only_dx else {s: G[name] for s, name in blk.att_names.items()}
        x, xn, qkv, P, O = ctx["x"], ctx["xn"], ctx["qkv"], ctx["P"], ctx["O"]
        B, Hh, Ww, C, ldx = _chk(x)
        lddy = _ld(dy)
        L, nh, hd = Hh * Ww, mod.num_heads, mod.head_dim
        hid, ld = nh * hd, 3 * nh * hd
        M = B * L
        # proj_out
        if not only_dx:
            self._wgrad(dy, O, g["proj_out.weight"], g["proj_out.bias"], C, hid, M, lddy, hid, hid)
        dO = self._new(x, B, L, hid)
        H.gemm(dy, mod.proj_out.weight, dO, M, hid, C, a_kind=H.ROW, b_kind=H.COL, lda=lddy, ldb=hid, ldc=hid)
        dqkv = self._new(x, B, L, ld)
        q, k, v = qkv[0, 0, 0:], qkv[0, 0, hid:], qkv[0, 0, 2 * hid:]
        dq, dk, dv = dqkv[0, 0, 0:], dqkv[0, 0, hid:], dqkv[0, 0, 2 * hid:]
        sP, sQ, sO = (nh * L * L, L * L), (L * ld, hd), (L * hid, hd)
        alpha = 1.0 / math.sqrt(hd)
        if P is None:
            # the forward ran fused: probabilities are recomputed from the saved log-sum-exp
            H.attn_bwd(q, k, v, ld, O, hid, dO, hid, ctx["lse"], self._new(x, B * nh * L), dq, dk, dv, ld, B, nh, L, hd, alpha)
        else:
            # dV[j][d] = sum_l P[l][j] dO[l][d]
            H.gemm(P, dO, dv, L, hd, L, a_kind=H.COL, b_kind=H.COL, lda=L, ldb=hid, ldc=ld, batch=B * nh, nh=nh, sA=sP, sB=sO, sC=sQ)
            # dP[l][j] = sum_d dO[l][d] V[j][d]
            dP = self._new(x, B, nh, L, L)
            H.gemm(dO, v, dP, L, L, hd, a_kind=H.ROW, b_kind=H.ROW, lda=hid, ldb=ld, ldc=L, batch=B * nh, nh=nh, sA=sO, sB=sQ, sC=sP)
            H.softmax_rows_bwd(P, dP, B * nh * L, L, alpha)                 # dP <- dS (already scaled by 1/sqrt(hd))
            # dQ[l][d] = sum_j dS[l][j] K[j][d] ; dK[j][d] = sum_l dS[l][j] Q[l][d]
            H.gemm(dP, k, dq, L, hd, L, a_kind=H.ROW, b_kind=H.COL, lda=L, ldb=ld, ldc=ld, batch=B * nh, nh=nh, sA=sP, sB=sQ, sC=sQ)
            H.gemm(dP, q, dk, L, hd, L, a_kind=H.COL, b_kind=H.COL, lda=L, ldb=ld, ldc=ld, batch=B * nh, nh=nh, sA=sP, sB=sQ, sC=sQ)
            del dP
        del dO
        # proj_in
        if not only_dx:
            self._wgrad(dqkv, xn, g["proj_in.weight"], g["proj_in.bias"], ld, C, M, ld, C, C)
        dxn = self._new(x, B, Hh, Ww, C)
        H.gemm(dqkv, mod.proj_in.weight, dxn, M, C, ld, a_kind=H.ROW, b_kind=H.COL, lda=ld, ldb=C, ldc=C)
        # norm (no activation) + the residual branch
        H.gn_apply_bwd(dxn, C, x, ldx, ctx["coef"], mod.norm.weight, mod.norm.bias, None, 0, 0.0, 0, H.RS_NONE, dy, lddy, dx,
                       _ld(dx), dx_accumulate, None, None, None, False, B, Hh, Ww, C, GROUPS,
                       pgb_keep=self._pgb(B, C, g["norm.weight"], g["norm.bias"]))

    # ------------------------------------------------------------------------------------------ input / output convolution
    def _in_conv_fwd(self, x_nchw, d, tape):
        """3x3 convolution of the (B,Cin,H,W) NCHW input into the NHWC view ``d``; returns the GroupNorm partials it left of ``d``"""
        m = self.m
        B, Ci, H0, W0 = x_nchw.shape
        hid, cip = m.hid_channels, (Ci + 3) // 4 * 4
        x4 = self._new(x_nchw, B, H0, W0, cip)
        H.nchw_to_nhwc(x_nchw, x4, B, Ci, H0, W0, cip)
        pp = self._part(x_nchw, B, H0 * W0, hid)
        if pp is not None and (H0 * W0) % 64:
            pp = None
        xc = None
        if cip <= THIN:
            # thin input (3 -> hid): im2col of the 4-channel image once, then a plain K = 36 GEMM (see vd_im2col3x3)
            xc = self._new(x_nchw, B * H0 * W0, 9 * cip)
            H.im2col3x3(x4, cip, xc, B, H0, W0, cip)
            H.gemm(xc, self._pack_f(m.in_conv.weight, cip), d, B * H0 * W0, hid, 9 * cip, a_kind=H.ROW, b_kind=H.ROW,
                   lda=9 * cip, ldb=9 * cip, ldc=_ld(d), bias=m.in_conv.bias, stats=pp, stats_hw=H0 * W0)
        else:
            H.conv3x3(x4, cip, self._pack_f(m.in_conv.weight, cip), m.in_conv.bias, d, _ld(d), B, H0, W0, cip, hid, stats_part=pp)
        if tape is not None:
            tape["in"] = dict(x4=x4 if xc is None else None, xc=xc, cip=cip)
        return self._parts(pp, hid, H0 * W0)

    def _in_conv_bwd(self, ctx, dy0, G):
        """weight and bias gradient of the input convolution"""
        B, H0, W0, hid, lddy = _chk(dy0)
        xc, cip, ci = ctx["xc"], ctx["cip"], self.m.in_channels
        if xc is not None:
            gw = self._new(dy0, hid, 9 * cip)
            H.gemm(dy0, xc, gw, hid, 9 * cip, B * H0 * W0, a_kind=H.COL, b_kind=H.COL, lda=lddy, ldb=9 * cip, ldc=9 * cip,
                   splitk=_splitk(hid, 9 * cip, B * H0 * W0), colsum=G["in_conv.bias"])
            H.thin_wgrad_finish(gw, hid, cip, ci, G["in_conv.weight"])
        else:
            H.conv3x3_wgrad(ctx["x4"], cip, dy0, lddy, B, H0, W0, cip, hid, G["in_conv.weight"], ci, hid, dbias=G["in_conv.bias"])

    def _in_conv_dgrad(self, ctx, dy0):
        """d/dx (NCHW) of the network input"""
        m = self.m
        B, H0, W0, hid, lddy = _chk(dy0)
        cip = ctx["cip"]
        d4 = self._new(dy0, B, H0, W0, cip)
        if cip != m.in_channels:
            d4.zero_()
        H.conv3x3(dy0, lddy, self._pack_d(m.in_conv.weight, hid), None, d4, cip, B, H0, W0, hid, m.in_channels)
        dx = self._new(dy0, B, m.in_channels, H0, W0)
        H.nhwc_to_nchw(d4, cip, dx, B, m.in_channels, H0, W0)
        return dx

    def _out_conv_fwd(self, h, h_parts, tape):
        """GN -> SiLU -> 3x3 into a zeroed ``[B,H,W,Cp]`` (Cp = out_channels rounded up to 4)"""
        m = self.m
        B, H0, W0, C0, _ = _chk(h)
        gn, conv = m.out_conv[0], m.out_conv[2]
        a = self._new(h, B, H0, W0, C0)
        coef = self._norm(h, h_parts, gn, None, 1, 0.0, 0, H.RS_NONE, a, B, H0, W0, C0)
        co, cop = m.out_channels, (m.out_channels + 3) // 4 * 4
        out = torch.zeros((B, H0, W0, cop), dtype=torch.float32, device=h.device)
        wz = None
        if co <= THIN:
            # thin output (hid -> 3): z[q][co*9+tap] = a[q] . w[co][tap] as a plain GEMM, then the 9-tap gather (vd_tap_gather)
            nz = (9 * co + 3) // 4 * 4
            wz = self._pack_thin(conv.weight, nz)
            z = self._new(h, B * H0 * W0, nz)
            H.gemm(a, wz, z, B * H0 * W0, 9 * co, C0, a_kind=H.ROW, b_kind=H.ROW, lda=C0, ldb=C0, ldc=nz)
            H.tap_gather(z, nz, conv.bias, out, cop, B, H0, W0, co)
        else:
            H.conv3x3(a, C0, self._pack_f(conv.weight), conv.bias, out, cop, B, H0, W0, C0, co)
        if tape is not None:
            tape["out"] = dict(h=h, coef=coef, a=a, wz=wz)
        return out

    def _out_conv_bwd(self, o, dout, G):
        """gradients of the output convolution and its norm; returns the gradient of the last block's output.  ``G`` None (the
        input-only pass): the weight-gradient launches are left out"""
        m = self.m
        only_dx = G is None
        G = _NO_GRADS if only_dx else G
        B, H0, W0, cop, _ = _chk(dout)
        gn, conv = m.out_conv[0], m.out_conv[2]
        C0, co, P0 = o["a"].shape[3], m.out_channels, B * H0 * W0
        da = self._new(dout, B, H0, W0, C0)
        if o["wz"] is not None:
            wz = o["wz"]
            nz = wz.shape[0]
            dz = self._new(dout, P0, nz)
            H.tap_spread(dout, cop, dz, nz, B, H0, W0, co)                   # dz[q][co*9+tap] = dout[q - off(tap)][co]
            if not only_dx:
                gz, cs = self._new(dout, nz, C0), self._new(dout, nz)
                H.gemm(dz, o["a"], gz, nz, C0, P0, a_kind=H.COL, b_kind=H.COL, lda=nz, ldb=C0, ldc=C0, splitk=_splitk(nz, C0, P0),
                       colsum=cs)
                H.thin_wgrad_finish(gz, co, C0, C0, G["out_conv.2.weight"], colsum=cs, cs_stride=9, cs_off=4, dbias=G["out_conv.2.bias"])
            H.gemm(dz, wz, da, P0, C0, nz, a_kind=H.ROW, b_kind=H.COL, lda=nz, ldb=C0, ldc=C0)
            del dz
        else:
            if not only_dx:
                H.conv3x3_wgrad(o["a"], C0, dout, cop, B, H0, W0, C0, cop, G["out_conv.2.weight"], C0, co, dbias=G["out_conv.2.bias"])
            H.conv3x3(dout, cop, self._pack_d(conv.weight, cop), None, da, C0, B, H0, W0, cop, C0)
        dh = self._new(dout, B, H0, W0, C0)
        H.gn_apply_bwd(da, C0, o["h"], _ld(o["h"]), o["coef"], gn.weight, gn.bias, None, 1, 0.0, 0, H.RS_NONE, None, 0, dh, C0,
                       False, None, None, None, False, B, H0, W0, C0, GROUPS,
                       pgb_keep=self._pgb(B, C0, G["out_conv.0.weight"], G["out_conv.0.bias"]))
        return dh

    # ------------------------------------------------------------------------------------------ whole network
    def forward(self, x_nchw, t, y, training, save):
        """x (B,Cin,H,W) NCHW -> output NHWC ``[B,H,W,Cp]`` (Cp = out_channels rounded up to 4) and the tape."""
        m = self.m
        B, Ci, H0, W0 = x_nchw.shape
        assert Ci == m.in_channels and H0 % (1 << (self.levels - 1)) == 0 and W0 % (1 << (self.levels - 1)) == 0
        tape = {} if save else None
        x_nchw = x_nchw.to(torch.float32).contiguous()
        fixed = self._fixed
        if fixed is not None and "packs" in fixed and (fixed["packs_d"] or not save):
            self._packs = fixed["packs"]                 # a sampler holds the weights fixed: packed once per chain
        else:
            # (a chain that takes input gradients -- p_sample_dps -- saves: the first saving forward of the context packs the
            # input-gradient images too, once, and every later forward uses that set)
            self._pack_all(need_d=save, geom=(B, H0, W0))
            if fixed is not None:
                fixed["packs"], fixed["packs_d"] = self._packs, bool(save)
        ta = self._embed_fwd(t, y, tape)
        films = self._film_fwd(ta, tape)
        p_drop = float(m.drop_rate) if training else 0.0
        base_seed = int(torch.empty((), dtype=torch.int64).random_().item()) if p_drop > 0 else 0
        # concat buffers, one per consuming up-block; the GroupNorm partials of each channel range travel with it
        cats = {bi: _Cat(self._new(x_nchw, B, *self._res_of(b.level, H0, W0), b.cin)) for bi, b in enumerate(self.plan) if b.consumes}

        def place(d, hh, ww):                            # the output view of a _Dest and the concat buffer it is a slice of (or None)
            if d.cat is None:
                return self._new(x_nchw, B, hh, ww, d.width), None
            return cats[d.cat].buf[..., d.c0:d.c0 + d.width], cats[d.cat]

        p0 = self.pushes[0]
        hs_top, cat = place(_Dest(p0.consumer, p0.ch, p0.cs), H0, W0)
        top_parts = cat.parts[p0.ch] = self._in_conv_fwd(x_nchw, hs_top, tape)
        h = h_parts = None
        for bi, b in enumerate(self.plan):
            if b.in_hs is not None:
                inp, inp_parts = hs_top, top_parts
            elif b.consumes:
                inp, inp_parts = cats[bi].buf, cats[bi].joined(b.ch_h)
            else:
                inp, inp_parts = h, h_parts
            oh, ow = H._resampled(inp.shape[1], inp.shape[2], b.rs)
            out, cat = place(b.dest, oh, ow)
            if b.res is None:
                out_parts = self._attn_fwd(b, inp, out, tape, inp_parts)
            elif b.att is not None:
                mid = self._new(x_nchw, B, oh, ow, b.cout)
                mid_parts = self._res_fwd(b, inp, films, mid, p_drop, base_seed + b.seed, tape, inp_parts)
                out_parts = self._attn_fwd(b, mid, out, tape, mid_parts)
            else:
                out_parts = self._res_fwd(b, inp, films, out, p_drop, base_seed + b.seed, tape, inp_parts)
            if cat is not None:
                cat.parts[b.dest.c0] = out_parts
            if b.kind == "down":
                hs_top, top_parts = out, out_parts
            else:
                h, h_parts = out, out_parts
        out = self._out_conv_fwd(h, h_parts, tape)
        if tape is not None:
            tape["ta"] = ta
            tape["packs"] = self._packs
        return out, tape

    def new_grads(self):
        return {k: torch.empty_like(p) for k, p in self.m.named_parameters()}

    def backward(self, tape, dout, G, need_dx=False, progress=None):
        """Fills ``G`` (name -> tensor, every entry overwritten) and returns d/dx (NCHW) when asked.  ``progress(name)`` is called whenever
        the gradient of ``name`` and of everything before it in completion_order() is final (gradient-bucket overlap).  The deferred
        weight-gradient queue and the side stream never outlive the call, whatever it raises (``_steps``' ``finally``, both passes).
        ``G`` None with ``need_dx``: the INPUT-ONLY pass, for a network whose weights are held fixed (guidance, posterior sampling, any loss
        on the prediction).  It runs what d/dx depends on -- the input-gradient convolutions, the GroupNorm and attention backward, the
        skip-path GEMMs, the resample backward: the launches of the full pass with their arguments, so d/dx is that pass's bit for bit
        -- and none of the weight-gradient, GroupNorm-parameter, FiLM or embedding work; it opens no side stream and allocates no
        parameter-shaped tensor.  There is no gradient to report: a ``progress`` listener is refused."""
        if G is None:
            self._refuse_no_grads(need_dx, progress is not None)
            steps = self._steps(tape, dout, None, True, False)
        else:
            steps = self.backward_steps(tape, dout, G, need_dx, join=progress is not None)
        try:
            while True:
                name = next(steps)
                if progress is not None:
                    progress(name)
        except StopIteration as fin:
            return fin.value

    @staticmethod
    def _refuse_no_grads(need_dx, listening):
        if not need_dx:
            raise ValueError("backward without a gradient set (G=None) computes d/dx only: need_dx=True is required")
        if listening:
            raise ValueError("backward without a gradient set (G=None) finishes no parameter gradient: there is nothing to report to a "
                             "progress listener / backward_steps")

    def progress_points(self):
        """The names ``backward_steps`` yields, in order (static: a function of the plan): the output convolution, the last block of every
        (UNet level, down / middle / up) group -- of every block under VD_READY_PER_BLOCK when a listener joins -- the input convolution,
        and None for the end of backward (GroupNorm parameters and the embeddings finish there)."""
        return ["out_conv.2.bias"] + [b.report for b in reversed(self.plan) if b.ends_group] + ["in_conv.bias", None]

    def grad_segments(self):
        """[(boundary name, [parameter names])] in BACKWARD order: segment j's gradients are final when ``backward_steps`` yields its
        boundary; the last segment (input convolution, every GroupNorm scale / shift, the embeddings) is final when the pass ends
        (boundary None).  The cut points of the chain of autograd nodes of models/unet.py."""
        if self._segments is None:
            bounds = self.progress_points()[:-2]             # (the input convolution finishes with the rest)
            segs, names = [], []
            for n in self.completion_order():
                names.append(n)
                if n in bounds:
                    segs.append((n, names))
                    names = []
            self._segments = segs + [(None, names)]
            assert [bnd for bnd, _ in segs] == bounds and all(n for _, n in self._segments)
        return self._segments

    def completion_order(self):
        """Parameter names in the order ``backward_steps`` finishes their gradients: block by block from the output back (the
        matmul-shaped gradients, i.e. all the bytes), then the GroupNorm scales / shifts of the whole network (their per-image terms
        are summed by one launch at the end of backward: _pgb_finish), then the embeddings."""
        back = self.plan[::-1]
        names = ["out_conv.2.weight", "out_conv.2.bias"] + [n for b in back for n in b.grads] + ["in_conv.weight", "in_conv.bias"] + \
                ["out_conv.0.weight", "out_conv.0.bias"] + [n for b in back for n in b.norm_grads]
        have = dict(self.m.named_parameters())
        seen = set(names)
        names += [k for k in have if k not in seen]          # embeddings: finished last
        assert sorted(names) == sorted(have), "completion order does not cover the parameter set"
        return names

    def backward_steps(self, tape, dout, G, need_dx=False, join=True):
        """Generator form of the backward pass: runs up to the next point at which a prefix of completion_order() is final, yields the
        last finished name (progress_points() lists them), and returns d/dx through StopIteration.  ``join``: a listener consumes the
        gradients at every yield (a gradient reducer, or autograd handing a segment's gradients to DDP's hooks: models/unet.py), so the
        weight-gradient side stream is joined there; without one it is joined once, at the end.  ``G`` None (the input-only pass of
        ``backward``) is refused: it has nothing to report."""
        if G is None:
            self._refuse_no_grads(need_dx, True)               # (at the call, not at the first next())
        return self._steps(tape, dout, G, need_dx, join)

    def _steps(self, tape, dout, G, need_dx, join):
        try:
            dx = yield from self._backward(tape, dout, G, need_dx, join)
            return dx
        finally:
            self._wq = None
            self._side = None

    def _backward(self, tape, dout, G, need_dx=False, join=False):
        """dout: NHWC ``[B,H,W,Cp]`` gradient of the padded output (padding channels zero).  ``G`` None: the input-only pass."""
        only_dx = G is None
        self._join_at_progress = bool(join)                    # a listener consumes gradients at every yield: finished means finished on every stream
        B = dout.shape[0]
        self._packs = tape["packs"]                            # the images THIS forward packed (another forward may have run since)
        ta = tape["ta"]
        dta = None if only_dx else torch.zeros_like(ta)
        # (input-only: vd_gn_apply_bwd wants a dfilm wherever it is given a film -- one scratch slot per width, as the per-image GroupNorm
        # parameter terms go to the arena and are never summed)
        dfilms = {c2: self._new(ta, 1 if only_dx else len(mods), B, c2) for c2, mods in self.film_groups.items()}
        self._pgb_begin(dout, B)
        self._wq = None if only_dx else {}
        self._side = None
        if not only_dx and H.WGRAD_STREAM and H.PROFILE is None:
            if self._side_stream is None or self._side_stream.device != dout.device:
                self._side_stream = torch.cuda.Stream(device=dout.device)
            self._side = self._side_stream
        dh_cur = self._out_conv_bwd(tape["out"], dout, G)      # gradient of the running `h`
        yield "out_conv.2.bias"                # (the GroupNorm parameter gradients are finished by ONE launch at the end: _pgb_finish)
        dskip = {}                     # hs id -> gradient view (written by the consuming up-block)
        for b in reversed(self.plan):
            dy = dskip.pop(b.push_hs) if b.kind == "down" else dh_cur       # a down block: total gradient of the tensor it pushed
            # the input gradient of a block that read the top of the skip stack joins what the consuming up-block already wrote there
            acc = b.in_hs is not None
            dxbuf = dskip[b.in_hs] if acc else self._new(dout, *tape[b.res_prefix or b.att_prefix]["x"].shape)
            if b.res is None:
                self._attn_bwd(b, tape[b.att_prefix], dy, dxbuf, acc, G)
            elif b.att is not None:
                dmid = self._new(dout, *tape[b.att_prefix]["x"].shape)
                self._attn_bwd(b, tape[b.att_prefix], dy, dmid, False, G)
                self._res_bwd(b, tape[b.res_prefix], dmid, dxbuf, acc, ta, dfilms, G)
                del dmid
            else:
                self._res_bwd(b, tape[b.res_prefix], dy, dxbuf, acc, ta, dfilms, G)
            # the deferred weight-gradient GEMMs of a level run when backward leaves it; only then is everything up to this block's last
            # tensor final (gradient-bucket overlap: trainer.GradReducer.ready).  With a gradient reducer listening and H.READY_PER_BLOCK the
            # queue is flushed (and the gradients declared final) after EVERY block instead: buckets leave as early as they can (28 report
            # points instead of 7 for CIFAR) at the price of ungrouped 1x1 / linear weight gradients and a side-stream join per block
            # (measured cost: DESIGN section 4)
            if b.ends_group or (self._join_at_progress and H.READY_PER_BLOCK):
                self._wgrad_flush()
                if self._join_at_progress:
                    self._side_join()
                yield b.report
            if b.consumes:
                dh_cur = dxbuf[..., :b.ch_h]
                dskip[b.src_hs] = dxbuf[..., b.ch_h:]
            elif not acc:
                dh_cur = dxbuf
        dy0 = dskip.pop(0)
        assert not dskip
        if only_dx:
            return self._in_conv_dgrad(tape["in"], dy0)
        self._in_conv_bwd(tape["in"], dy0, G)
        yield "in_conv.bias"
        dx = self._in_conv_dgrad(tape["in"], dy0) if need_dx else None
        self._pgb_finish()
        self._film_bwd(dfilms, tape["film_w"], dta)
        self._embed_bwd(tape["embed"], dta, G)
        self._wgrad_flush()
        self._side_join()
        self._side = None
        self._wq = None
        yield None
        return dx
