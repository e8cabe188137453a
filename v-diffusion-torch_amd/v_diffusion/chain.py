"""What the chains of this package share -- ``p_sample``, ``p_sample_solver``, ``p_sample_unipc``, ``p_sample_inpaint``,
``p_invert_noise``, ``p_sample_replay``, ``p_encode`` and the captured-graph paths: the guided label rows, the state buffers and the network call
(``Chain``), the capture of one step into a HIP graph (``captured_step``), and the argument checks more than one of them makes.  A sampler
keeps what is its own: its coefficient table, its random draws and its one launch per step."""
import contextlib
import numbers

import torch

from . import _hip

F64 = torch.float64


def refuse_variants(gd, what):
    if gd.model_var_type == "learned":
        raise NotImplementedError("model_var_type='learned'")
    if gd.x0eps_coef:
        raise NotImplementedError(f"x0eps_coef=True with {what}")


def image_batch(name, x):
    if not torch.is_tensor(x) or x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"{name} must be a non-empty (B, C, H, W) tensor, got shape {tuple(getattr(x, 'shape', ()))}")


def chain_length(gd, start):
    """the grid index a chain begins at: ``start``, an integer in [1, sample_timesteps], or sample_timesteps for None"""
    T = gd.sample_timesteps
    if start is None:
        return T
    if isinstance(start, bool) or not isinstance(start, numbers.Integral) or not 1 <= start <= T:
        raise ValueError(f"start must be an integer in [1, {T}], got {start!r}")
    return int(start)


def guided_labels(gd, label, device):
    """(cfg, the label rows the network sees on the device: with guidance cond, uncond interleaved, the uncond rows 0 -- reference :372)"""
    if label is not None:
        label = label.to(device)
    cfg = gd._use_cfg(label)
    if cfg:
        label = label.repeat_interleave(2, dim=0).clone()
        label[1::2] = 0
    return cfg, label


class Chain:
    """The state of one chain over a (B, C, H, W) batch and its network.  ``x`` is the current state, fp32 on ``device``; with guidance
    ``x_in`` holds it twice, rows 2b and 2b+1, the network's input (every step launch writes that copy beside the state: its xdup), and
    without guidance the network's input is ``x`` itself.  Ping-pong (default): a step reads ``x`` and writes ``dst`` = (x_next,
    x_in_next), then ``advance()`` swaps.  ``in_place=True``: ``dst`` = (x, x_in), for the launches that may alias their input, and
    ``advance()`` does nothing.  ``dup=False`` leaves x_in unwritten: the caller's first launch or copy fills it."""

    def __init__(self, gd, denoise_fn, x_t, label, device, in_place=False, dup=True):
        self.gd, self.denoise_fn, self.device, self.in_place = gd, denoise_fn, device, in_place
        self.cfg, self.y_in = guided_labels(gd, label, device)
        self.x = x_t
        self.B, self.C = x_t.shape[:2]
        self.HW = x_t.shape[2] * x_t.shape[3]
        self.rows = self.B * (1 + self.cfg)
        self.mot = _hip.OUT_TYPES[gd.model_out_type]
        self.x_in = self.x_next = self.x_in_next = None
        if self.cfg:
            self.x_in = x_t.repeat_interleave(2, dim=0) if dup else torch.empty((self.rows,) + tuple(x_t.shape[1:]), dtype=torch.float32,
                                                                                device=device)
        if not in_place:
            self.x_next = torch.empty_like(x_t)
            self.x_in_next = torch.empty_like(self.x_in) if self.cfg else None

    @property
    def net_in(self):
        return self.x_in if self.cfg else self.x

    @property
    def dst(self):
        """(xn, xdup) of the step's launch"""
        return (self.x, self.x_in) if self.in_place else (self.x_next, self.x_in_next)

    def advance(self):
        if not self.in_place:
            self.x, self.x_next = self.x_next, self.x
            self.x_in, self.x_in_next = self.x_in_next, self.x_in

    def net(self, t):
        """the network's fp32 output at the current state; ``t`` = the time as a python float, or a (rows,) fp64 device tensor"""
        if not torch.is_tensor(t):
            t = torch.full((self.rows,), t, dtype=F64, device=self.device)
        return self.denoise_fn(self.net_in, t, self.y_in).to(torch.float32).contiguous()

    def load(self, x_t, label):
        """refill an in-place chain's own buffers: a captured graph replays through them"""
        self.x.copy_(x_t)
        if self.cfg:
            self.x_in.copy_(x_t.repeat_interleave(2, dim=0))
        if self.y_in is not None:
            self.y_in.copy_(guided_labels(self.gd, label, self.device)[1])

    def fixed_weights(self):
        """the context of the step loop: the weights do not change inside one chain"""
        net = getattr(self.denoise_fn, "module", self.denoise_fn)
        eng = net.engine() if hasattr(net, "engine") else None
        return eng.fixed_weights() if eng is not None else contextlib.nullcontext()


def captured_step(cache, limit, gd, denoise_fn, shape, label, device, launch, key=(), bufs=(), kwidth=8):
    """``(graph, state, pinned packs)`` of one step -- the network's forward and ``launch(chain, state, out)`` on the device-resident
    coefficients ``state["k"]`` -- captured once into a HIP graph and kept in ``cache``, a small LRU (a graph pins its activations).
    ``state`` = dict(chain = an in-place ``Chain`` over buffers of its own, t = the (rows,) network time, k = the ``kwidth`` coefficients,
    and one image-shaped buffer per name in ``bufs``); the caller fills them and replays.  ``key``: what else the launch depends on."""
    net = getattr(denoise_fn, "module", denoise_fn)
    key = (id(denoise_fn), tuple(shape), gd._use_cfg(label), gd.model_out_type, None if label is None else tuple(label.shape),
           hash(tuple(p.data_ptr() for p in net.parameters())) if isinstance(net, torch.nn.Module) else None) + tuple(key)
    entry = cache.get(key)
    if entry is not None:
        cache[key] = cache.pop(key)                    # most recently used last
        return entry
    zeros = lambda shp, dtype=torch.float32: torch.zeros(shp, dtype=dtype, device=device)
    ch = Chain(gd, denoise_fn, zeros(shape), label, device, in_place=True, dup=False)
    if ch.cfg:
        ch.x_in.zero_()                                # the warm-up and the capture run on these buffers before load() fills them
    if ch.y_in is not None:
        ch.y_in = torch.zeros_like(ch.y_in)
    st = dict(chain=ch, t=zeros((ch.rows,), F64), k=zeros((kwidth,)), **{name: zeros(shape) for name in bufs})
    body = lambda: launch(ch, st, ch.net(st["t"]))
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):                      # warm-up outside capture (lazy initialisation, workspace growth)
        body()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    # the graph's pack / convolution nodes hold raw pointers into the forward's ConvPacks (device tables, U images): the entry keeps that
    # object referenced, so an engine-side eviction can never free memory a cached graph replays through
    eng = net.engine() if hasattr(net, "engine") else None
    while len(cache) >= limit:
        cache.pop(next(iter(cache)))
    entry = cache[key] = (graph, st, None if eng is None else eng.packs)
    return entry
