"""``UNet`` with the reference's constructor, parameter names/order and ``forward(x, t, y=None)`` contract
(reference v_diffusion/models/unet.py:151-322) -- executed by the HIP engine (``..engine``), MI355X only.

The module tree exists to own parameters under the reference's state_dict keys (``downsamples.level_1.0.0.conv1.weight``,
``middle.1.proj_in.weight``, ``out_conv.2.bias`` ...), so reference checkpoints load and DDP / EMA / optimizers see the
same ``parameters()`` order.  No sub-module computes anything by itself.
"""
import torch
import torch.nn as nn

from .. import _hip
from ..flat import owner
from ..modules import Linear, Conv2d, Sequential, OneHot, GroupNorm32


class AttentionBlock(nn.Module):
    """GN -> 1x1 QKV -> softmax(QK^T/sqrt(d)) V -> 1x1 (zero-init) -> + x   (reference unet.py:33-81)"""

    def __init__(self, in_dim, head_dim=None, num_heads=None):
        super().__init__()
        if head_dim is None:
            assert num_heads is not None and in_dim % num_heads == 0
            head_dim = in_dim // num_heads
        if num_heads is None:
            assert head_dim is not None and in_dim % head_dim == 0
            num_heads = in_dim // head_dim
        self.head_dim, self.num_heads = head_dim, num_heads
        self.hid_dim = head_dim * num_heads
        self.norm = GroupNorm32(in_dim)
        self.proj_in = Conv2d(in_dim, 3 * self.hid_dim, 1)
        self.proj_out = Conv2d(self.hid_dim, in_dim, 1, init_scale=0.)


class ResidualBlock(nn.Module):
    """GN -> SiLU -> [resample] -> 3x3 -> FiLM(GN) -> SiLU -> dropout -> 3x3 (zero-init) + skip   (reference unet.py:106-148)"""

    def __init__(self, in_channels, out_channels, embed_dim, drop_rate=0., resampling="none"):
        super().__init__()
        assert resampling in ("none", "upsample", "downsample")
        self.in_channels, self.out_channels, self.resampling, self.drop_rate = in_channels, out_channels, resampling, drop_rate
        self.norm1 = GroupNorm32(in_channels)
        self.conv1 = Conv2d(in_channels, out_channels, 3, 1, 1)
        self.fc = Linear(embed_dim, 2 * out_channels)
        self.norm2 = GroupNorm32(out_channels)
        self.conv2 = Conv2d(out_channels, out_channels, 3, 1, 1, init_scale=0.)
        self.skip = nn.Identity() if in_channels == out_channels else Conv2d(in_channels, out_channels, 1)


class _UNetFn(torch.autograd.Function):
    """One autograd node for the whole network -- the form the flat-buffer trainer uses (``trainer.FlatState``: the kernels write into
    the caller's flat gradient buffer and ``GradReducer`` listens to the engine's progress itself), and the A/B form of the chain below
    (``VD_AUTOGRAD_CHAIN=0``).  Forward runs the engine and keeps its tape, backward runs the engine's hand-written backward and hands
    one gradient per parameter to autograd."""

    @staticmethod
    def forward(ctx, model, x, t, y, *params):
        eng = model.engine()
        with torch.cuda.device(x.device):            # kernels go to the current stream of the tensor's device
            out, tape = eng.forward(x, t, y, model.training, save=True)
            ctx.model, ctx.tape, ctx.need_dx = model, tape, x.requires_grad
            return model._to_nchw(out)

    @staticmethod
    @torch.autograd.function.once_differentiable      # hand-written kernels: a second-order backward through them raises instead of returning constants
    def backward(ctx, dout):
        model, tape = ctx.model, ctx.tape
        if tape is None:
            raise RuntimeError(_TWICE)
        ctx.tape = None
        eng = model.engine()
        flat = model._flat_grad_views is not None
        G = model._grad_targets()
        with torch.cuda.device(dout.device):
            d4 = model._dout_nhwc(dout)
            dx = eng.backward(tape, d4, G, need_dx=ctx.need_dx, progress=getattr(model, "_grads_ready_hook", None))
        if flat:
            # the kernels already wrote into the caller's flat gradient buffer (trainer.FlatState): autograd gets nothing
            # to accumulate, which avoids a 243 MB clone per step
            return (None, dx, None, None) + (None,) * len(G)
        # class-conditional network called without labels: the class embedding took no part in the forward, so -- as in the
        # reference, where autograd never reaches those parameters -- their gradient is None (torch optimizers then skip them)
        no_labels = bool(model.num_classes) and tape["embed"]["yn"] is None
        return (None, dx, None, None) + tuple(None if (no_labels and k.startswith("class_embed.")) else G[k]
                                              for k, _ in model.named_parameters())


_TWICE = "UNet backward called twice (the tape is freed after the first backward)"


class _UNetInputFn(torch.autograd.Function):
    """One autograd node for a network that is held fixed: no parameter requires a gradient and the input does (guidance, posterior
    sampling, any loss on the prediction of a frozen checkpoint).  Forward runs the engine and keeps its tape; backward is the engine's
    INPUT-ONLY pass (``UNetEngine.backward(tape, dout, None, need_dx=True)``): none of the weight-gradient work, no gradient slot or flat
    store touched, and d/dx bit for bit that of the full pass."""

    @staticmethod
    def forward(ctx, model, x, t, y):
        with torch.cuda.device(x.device):
            out, tape = model.engine().forward(x, t, y, model.training, save=True)
            ctx.model, ctx.tape = model, tape
            return model._to_nchw(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        model, tape = ctx.model, ctx.tape
        if tape is None:
            raise RuntimeError(_TWICE)
        ctx.tape = None
        return None, model._input_grad(tape, dout), None, None


class _BackwardRun:
    """What one forward shares with its chain of ``_SegFn`` nodes: the tape, then the running backward pass (the engine's generator),
    the gradient tensors not yet handed to autograd, and d/dx."""

    def __init__(self, model, tape, need_dx, segs, device):
        self.model, self.tape, self.need_dx, self.segs, self.device = model, tape, need_dx, segs, device
        self.out = self.gen = self.G = self.dx = None
        self.no_labels = False
        self.reached = -1                  # index (backward order) of the last segment whose gradients are final
        self.finished = False
        self.task_id = None                # the autograd graph task (one ``backward()`` / ``autograd.grad`` call) this pass runs inside

    def start(self, dout):
        if self.tape is None:
            raise RuntimeError(_TWICE)
        tape, self.tape = self.tape, None
        self.task_id = torch._C._current_graph_task_id()
        self.gen, self.G, self.no_labels = self.model._chain_begin(self, tape, dout, self.need_dx)

    def advance(self, j):
        """run the backward pass until the gradients of segment ``j`` are final (the last segment: until it ends)"""
        last = len(self.segs) - 1
        try:
            while self.reached < j:
                try:
                    name = next(self.gen)
                except StopIteration as fin:
                    self.dx, self.reached = fin.value, last
                    self._end()
                    break
                hook = getattr(self.model, "_grads_ready_hook", None)
                if hook is not None:
                    hook(name)              # (the engine's progress report, as in the single-node form)
                bound = self.segs[self.reached + 1][0]
                if bound is not None and name == bound:
                    self.reached += 1
        except BaseException:
            self._end()
            raise

    def take(self, j):
        """segment j's gradients, in the order of its parameter list; the run lets go of them (autograd's AccumulateGrad keeps a
        gradient tensor nobody else holds instead of cloning it)"""
        G, skip = self.G, self.no_labels
        return [None if (skip and k.startswith("class_embed.")) else G.pop(k) for k in self.segs[j][1]]

    def drain(self):
        """finish the pass now (another backward of the same engine is about to start: the engine's queue / side-stream / arena state
        belongs to one pass at a time); the remaining nodes find their gradients in G"""
        if not self.finished and self.gen is not None:
            self.advance(len(self.segs) - 1)

    def stop_early(self):
        """nothing upstream of the current node takes part in this backward (frozen parameters, input without gradient): end the pass
        at the yield it stands at (the side stream is joined at every yield of a listening pass)"""
        if self.gen is not None:
            self.gen.close()
        self._end()

    def _end(self):
        self.finished, self.gen = True, None
        self.model._chain_end(self)

    def __del__(self):
        # an abandoned pass (its autograd graph was freed before the last node ran): close the engine's generator at the yield it stands
        # at instead of leaving its tape, gradient tensors and side-stream state to whoever starts the next backward
        gen = self.gen
        if gen is not None and not self.finished:
            try:
                gen.close()
            except Exception:
                pass
            try:
                self._end()
            except Exception:
                pass


class _SegFn(torch.autograd.Function):
    """One node of the CHAIN of autograd nodes a training forward returns (SURVEY section 5 option (1); reference train.py:141-148 wraps
    the model in DDP and train_utils.py:154 relies on DDP's hooks firing as gradients become ready).  The network is cut at the engine's
    progress points (engine.grad_segments: the output convolution, every UNet level of the up / middle / down path, the rest); node j
    owns the parameters of segment j and is linked to node j+1 through a one-element token, so autograd runs the nodes strictly in
    backward order.  Each node resumes the engine's backward pass (a generator) until its segment's gradients are final and returns
    them: their AccumulateGrad nodes -- and with them DDP's per-parameter hooks and bucket all-reduces -- run BEFORE the next node
    launches the next level's kernels, which is how the reference's own ``DDP(model)`` overlaps communication with backward here.
    The kernels, their order and their results are those of the single-node form, bit for bit."""

    @staticmethod
    def forward(ctx, run, j, carrier, *params):
        ctx.run, ctx.j = run, j
        if j == 0:                          # the node backward starts from returns the network's output
            out, run.out = run.out, None
            return out
        return carrier.new_empty((1,), dtype=torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        run, j = ctx.run, ctx.j
        with torch.cuda.device(run.device) if run.device.type == "cuda" else _nullctx():
            if j == 0:
                run.start(g)
            run.advance(j)
            grads = run.take(j)
            if j == len(run.segs) - 1:
                cg = run.dx
            else:
                cg = run.model._chain_token(run.device)
                if not ctx.needs_input_grad[2]:
                    run.stop_early()
        return (None, None, cg) + tuple(grads)


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class UNet(nn.Module):
    def __init__(self, in_channels, hid_channels, out_channels, ch_multipliers, num_res_blocks, apply_attn,
                 embedding_dim=None, drop_rate=0., head_dim=None, num_heads=None, num_classes=0, multitags=False,
                 resample_with_res=True, use_xformers=False):
        super().__init__()
        self.in_channels, self.hid_channels, self.out_channels = in_channels, hid_channels, out_channels
        self.embedding_dim = embedding_dim or 4 * hid_channels
        self.levels = levels = len(ch_multipliers)
        self.ch_multipliers = ch_multipliers
        if isinstance(apply_attn, bool):
            apply_attn = [apply_attn] * levels
        self.apply_attn = apply_attn
        self.num_res_blocks, self.drop_rate = num_res_blocks, drop_rate
        if head_dim is None and num_heads is None:
            num_heads = 1
        self.head_dim, self.num_heads = head_dim, num_heads
        self.num_classes, self.multitags = num_classes, multitags
        self.resample_with_res = resample_with_res
        if not resample_with_res:
            raise NotImplementedError("resample_with_res=False (strided-conv resampling, reference unet.py:258-260,279-282) "
                                      "is not on the hot path: no shipped config uses it")
        if use_xformers:
            print("xFormers not available! Resetting to False.")       # reference unet.py:192-194 (same fallback message)
        if hid_channels % 32 or any((hid_channels * k) % 32 for k in ch_multipliers):
            raise ValueError("channel counts must be multiples of 32 (GroupNorm(32, C))")

        emb = self.embedding_dim
        self.time_embed = nn.Sequential(Linear(hid_channels, emb), nn.SiLU(), Linear(emb, emb))
        if num_classes > 0:
            if multitags:
                self.class_embed = nn.Linear(num_classes, emb)
            else:
                self.class_embed = nn.Sequential(OneHot(num_classes, exclude_zero=True), Linear(num_classes, emb))
        self.in_conv = Conv2d(in_channels, hid_channels, 3, 1, 1)
        chs = [hid_channels * k for k in ch_multipliers]

        def block(level, cin, cout, resampling="none"):
            rb = ResidualBlock(cin, cout, emb, drop_rate, resampling)
            if apply_attn[level]:
                return Sequential(rb, AttentionBlock(cout, head_dim=head_dim, num_heads=num_heads))
            return rb

        downs = {}
        for i in range(levels):
            prev = chs[i - 1] if i else hid_channels
            mods = [block(i, prev, chs[i])] + [block(i, chs[i], chs[i]) for _ in range(num_res_blocks - 1)]
            if i != levels - 1:
                mods.append(block(i, chs[i], chs[i], "downsample"))
            downs[f"level_{i}"] = nn.ModuleList(mods)
        self.downsamples = nn.ModuleDict(downs)
        mid = chs[-1]
        self.middle = Sequential(ResidualBlock(mid, mid, emb, drop_rate),
                                 AttentionBlock(mid, head_dim=head_dim, num_heads=num_heads),
                                 ResidualBlock(mid, mid, emb, drop_rate))
        ups = {}
        for i in range(levels):
            nxt = hid_channels if i == 0 else chs[i - 1]
            prv = chs[-1] if i == levels - 1 else chs[i + 1]
            mods = [block(i, prv + chs[i], chs[i])] + [block(i, 2 * chs[i], chs[i]) for _ in range(num_res_blocks - 1)]
            mods.append(block(i, nxt + chs[i], chs[i]))
            if i != 0:
                mods.append(block(i, chs[i], chs[i], "upsample"))
            ups[f"level_{i}"] = nn.ModuleList(mods)
        self.upsamples = nn.ModuleDict(ups)
        self.out_conv = Sequential(GroupNorm32(chs[0]), nn.SiLU(), Conv2d(chs[0], out_channels, 3, 1, 1, init_scale=0.))
        self._engine = None
        self._flat_grad_views = None
        self._grad_pool = {}                # per-parameter gradient slots of the autograd path, see _grad_targets
        self._grads_ready_hook = None
        self._tokens = {}

    def detached_copy(self):
        """A deep copy that shares nothing with this module: every parameter in a compact storage of its own (``Parameter.__deepcopy__``
        clones the data, so a view of a flat store becomes a tensor of the parameter's size, not a copy of the store), and none of this
        module's run state -- engine, gradient slots, tokens are built again on first use.  That run state is taken off ``self`` for the
        duration of the copy and put back: not to be called while a forward or backward of this module is in flight."""
        import copy
        keep = {k: self.__dict__[k] for k in ("_engine", "_flat_grad_views", "_grad_pool", "_grads_ready_hook", "_tokens")}
        self._engine, self._flat_grad_views, self._grad_pool, self._grads_ready_hook, self._tokens = None, None, {}, None, {}
        try:
            return copy.deepcopy(self)
        finally:
            self.__dict__.update(keep)

    # ------------------------------------------------------------------ engine plumbing
    def engine(self):
        if self._engine is None:
            from ..engine import UNetEngine
            _hip.lib()                                   # fail loudly if the HIP library is missing
            self._engine = UNetEngine(self)
        return self._engine

    def _grad_targets(self):
        """the tensors the backward kernels write the parameter gradients into.  The flat-buffer trainer installs its own views
        (trainer.FlatState).  Otherwise (autograd path: ``loss.backward()``, ``DDP(model)``) every parameter has a persistent gradient SLOT and
        autograd is handed a fresh alias of it: ``AccumulateGrad`` keeps a gradient tensor nobody else holds instead of cloning it, so
        ``param.grad`` ends up in the slot and ``zero_grad(set_to_none=True)`` only drops a reference -- no 243 MB / 1.07 GB of allocations
        per step (with the side stream's ``record_stream`` holds the caching allocator could not recycle them in time: 78.8 -> 65.8 ms per step
        of the reference-style loop, tests/probe/ddp_style_step.py).
          * default: one tensor per parameter with its OWN storage; it is handed out only while nothing but this module references that
            storage (a ``.grad`` that was not reset -- gradient accumulation -- or a gradient tensor the caller kept get an ordinary fresh
            tensor, exactly as before);
          * a parameter in a flat store (``flat.FlatParams`` of v_diffusion.optim.FusedAdamW): a view of the store's gradient buffer under the
            same rule, ``FlatParams.grad_slot`` (the optimizer's documented contract: gradients live in its buffer until the next backward,
            as with DDP's ``gradient_as_bucket_view=True``)."""
        if self._flat_grad_views is not None:
            return self._flat_grad_views
        pool, use_count = self._grad_pool, torch._C._storage_Use_Count
        out = {}
        for k, p in self.named_parameters():
            own = owner(p)
            if own is not None:
                out[k] = own[0].grad_slot(own[1])
                continue
            t = pool.get(k)
            if t is None or t.device != p.device or t.shape != p.shape:
                t = pool[k] = torch.empty(p.shape, dtype=p.dtype, device=p.device)
            # 2 = this module's tensor + the temporary Python storage object of this very query: nobody else holds the memory
            out[k] = t.detach() if use_count(t.untyped_storage()._cdata) == 2 else torch.empty_like(p)
        return out

    def _dout_nhwc(self, dout):
        """NCHW output gradient -> the engine's NHWC layout, channels padded to a multiple of 4 (padding never read as data)"""
        B, co, Hh, Ww = dout.shape
        cop = (co + 3) // 4 * 4
        d4 = torch.empty((B, Hh, Ww, cop), dtype=torch.float32, device=dout.device)
        _hip.nchw_to_nhwc(dout.to(torch.float32).contiguous(), d4, B, co, Hh, Ww, cop)
        return d4

    # ---- chain of autograd nodes (see _SegFn)
    def _chain_begin(self, run, tape, dout, need_dx):
        eng = self.engine()
        self._settle_active_run(run, run.task_id)
        G = self._grad_targets()
        no_labels = bool(self.num_classes) and tape["embed"]["yn"] is None
        gen = eng.backward_steps(tape, self._dout_nhwc(dout), G, need_dx=need_dx, join=True)
        import weakref
        eng._active_run = weakref.ref(run)
        return gen, G, no_labels

    def _settle_active_run(self, run, task_id):
        """before a backward pass of this engine starts: the engine's queue / side-stream / arena state belongs to one pass at a time"""
        eng = self.engine()
        # the pass in flight is held through a weak reference (round-5 advice): a run whose graph is gone -- backward stopped between nodes
        # because a hook raised, or autograd.grad over a subset pruned the upstream nodes -- must not be kept alive (its tape is GBs of
        # activations) nor be run to completion here; a run that still has live nodes (two forwards, one backward) is drained first
        other = eng._active_run() if eng._active_run is not None else None
        if other is not None and other is not run and not other.finished:
            if other.task_id == task_id:
                other.drain()               # two forwards inside ONE backward call: finish the first pass, its remaining nodes find their gradients
            else:
                other.stop_early()          # left over from an EARLIER backward call (it raised, or it never reached the pass's last nodes): its
                                            # nodes can no longer run -- PyTorch keeps a failed call's graph alive until the next call starts

    def _input_grad(self, tape, dout):
        """d/dx (NCHW fp32) of ``dout`` through the engine's input-only backward pass of ``tape``"""
        self._settle_active_run(None, torch._C._current_graph_task_id())
        with torch.no_grad(), torch.cuda.device(dout.device):
            return self.engine().backward(tape, self._dout_nhwc(dout), None, need_dx=True)

    def forward_vjp(self, x, t, y=None):
        """``(out, vjp)``: ``out`` is what ``forward(x, t, y)`` returns and ``vjp(dout)`` -- ``dout`` of ``out``'s shape -- returns d/dx of
        ``x``'s shape, fp32 on the device: the vector-Jacobian product of the network with its weights held fixed, through the engine's
        input-only backward pass (``UNetEngine.backward`` with ``G=None``).  No autograd: it works under ``no_grad`` and ``inference_mode``
        and touches no ``.grad``, no gradient slot and no flat store.  ``vjp`` runs once -- the tape is freed on the first call, a second
        raises.  ``self.training`` is honoured (dropout as the module is set)."""
        if not x.is_cuda:
            raise RuntimeError("v_diffusion.UNet runs on an MI355X through libvdiff_hip.so only; there is no CPU path "
                               "(the CPU restatement lives under oracle/ and is test infrastructure)")
        out_shape = (x.shape[0], self.out_channels) + tuple(x.shape[2:])
        if x.shape[0] == 0:                                   # empty batch: nothing to launch
            tape = ()
            out = x.new_zeros(out_shape, dtype=torch.float32)
        else:
            with torch.no_grad(), torch.cuda.device(x.device):
                out, tape = self.engine().forward(x.detach(), t, y, self.training, save=True)
                out = self._to_nchw(out)
        state = [tape]

        def vjp(dout):
            if state[0] is None:
                raise RuntimeError(_TWICE)
            tape, state[0] = state[0], None
            if not torch.is_tensor(dout) or tuple(dout.shape) != out_shape:
                raise ValueError(f"dout must have the output's shape {out_shape}, got {tuple(getattr(dout, 'shape', ()))}")
            if not tape:
                return x.new_zeros(tuple(x.shape), dtype=torch.float32)
            if not dout.is_cuda:
                raise RuntimeError("v_diffusion.UNet.forward_vjp: dout must be on the device of the forward")
            return self._input_grad(tape, dout.detach())
        return out, vjp

    def _chain_end(self, run):
        eng = self._engine
        if eng is not None and eng._active_run is not None and eng._active_run() in (run, None):
            eng._active_run = None

    def _chain_token(self, device):
        tok = self._tokens.get(device)
        if tok is None:
            tok = self._tokens[device] = torch.zeros((1,), dtype=torch.float32, device=device)
        return tok

    def _forward_chain(self, x, t, y):
        eng = self.engine()
        with torch.no_grad(), torch.cuda.device(x.device):
            out, tape = eng.forward(x, t, y, self.training, save=True)
            out = self._to_nchw(out)
        segs = eng.grad_segments()
        named = dict(self.named_parameters())
        run = _BackwardRun(self, tape, x.requires_grad, segs, x.device)
        run.out = out
        carrier = x
        for j in range(len(segs) - 1, -1, -1):         # forward order: the segment backward finishes LAST is the first node
            carrier = _SegFn.apply(run, j, carrier, *[named[k] for k in segs[j][1]])
        return carrier

    def _to_nchw(self, out_nhwc):
        B, Hh, Ww, cop = out_nhwc.shape
        y = torch.empty((B, self.out_channels, Hh, Ww), dtype=torch.float32, device=out_nhwc.device)
        _hip.nhwc_to_nchw(out_nhwc, cop, y, B, self.out_channels, Hh, Ww)
        return y

    def forward(self, x, t, y=None):
        """x (B,C,H,W) fp32, t (B,) fp64 in [0,1] (or step/T), y (B,) float labels 0..num_classes / (B,num_classes) tags."""
        if not x.is_cuda:
            raise RuntimeError("v_diffusion.UNet runs on an MI355X through libvdiff_hip.so only; there is no CPU path "
                               "(the CPU restatement lives under oracle/ and is test infrastructure)")
        if x.shape[0] == 0:                                   # empty batch: nothing to launch (F.conv2d returns an empty tensor too)
            return x.new_zeros((0, self.out_channels) + tuple(x.shape[2:]), dtype=torch.float32)
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            if x.requires_grad and not any(p.requires_grad for p in params):
                return _UNetInputFn.apply(self, x, t, y)      # a frozen network: d/dx without the weight-gradient work
            if self._flat_grad_views is None and _hip.AUTOGRAD_CHAIN:
                return self._forward_chain(x, t, y)
            return _UNetFn.apply(self, x, t, y, *params)
        with torch.cuda.device(x.device):
            out, _ = self.engine().forward(x, t, y, self.training, save=False)
            return self._to_nchw(out)
