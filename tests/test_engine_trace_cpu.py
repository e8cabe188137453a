"""The complete launch trace of the UNet engine (v_diffusion/engine.py: forward, backward, backward_steps), without a device.

A ``UNet`` built on the CPU gives CPU buffers; every launch wrapper of ``v_diffusion._hip`` is replaced by a recorder while the host
predicates (``*_supported``, ``*_preferred``, ``attn_use_fused``, ``stats_part_numel``, ``wino43_fwd_chunk_rows`` and the library's
``vd_gemm_grouped_wgrad_auto_split``) stay real, ``last_row_tile`` answers 128 and the weight-gradient side stream is off (no stream on
the CPU).  What the engine WOULD launch -- which wrapper, in which order, with which arguments, and where it reports progress -- is then
observable here.  Arguments are normalised so that a trace does not depend on addresses:

  * a parameter becomes its name, a gradient tensor of ``G`` becomes ``grad:<name>``;
  * any other tensor becomes [buffer number by first appearance in the log, storage offset, shape, strides] (the recorder holds a
    reference to every tensor it sees, so no address is handed out twice);
  * the entry lists of the grouped weight-gradient launch and the pointer columns of the GroupNorm parameter-sum table likewise;
  * the tables of the batched pack launches as (rows, blocks) only: tests/golden/conv_packs.json pins their contents;
  * every yield of the backward pass enters the log as ["yield", name].

Pinned to tests/golden/engine_trace.json, recorded through seams that exist on both sides of the change that made the block plan
single-sourced -- ``forward(x, t, y, training, save)``, ``backward``, ``backward_steps``, ``fixed_weights`` and the four static tables
``progress_points`` / ``completion_order`` / ``grad_segments`` / ``_conv_geoms`` -- from the engine as it stood BEFORE that change.  The
fixture keeps the launch counts by wrapper and the yield list readable and the launches between consecutive yields as digests: a digest
that moved names its scenario and segment, and --record on both sides shows the difference.

Scenarios, for tinyA (batch 3, 16x16), tinyB (2, 16x16), tinyC (2, 8x8), CIFAR_COND (2, 32x32), CELEBA (1, 64x64):
  a  training forward with tape, then the backward pass nobody listens to (``backward_steps(join=False)``: what ``backward`` runs
     without ``progress``, with its yields visible)
  b  the same through ``backward(progress=listener, need_dx=True)``
  c  two ``save=False`` forwards inside one ``fixed_weights()``
  d  the four static tables
  e  (tinyA, CIFAR) b with READY_PER_BLOCK;   tinyA only, each as b:  f  y=None on the class-conditional model,  g  GROUPED_WGRAD off,
  h  GN_FOLD off,  i  WINO off

    python tests/test_engine_trace_cpu.py --record      rewrites the fixture from the package on sys.path -- only for a change that is
                                                        MEANT to move a launch
"""
import collections
import hashlib
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_trace.json")
if not any(os.path.isdir(os.path.join(p, "v_diffusion")) for p in sys.path if p):       # (--record: the package under test may come first)
    sys.path.insert(0, os.path.join(ROOT, "v-diffusion-torch_amd"))
if ROOT not in sys.path:
    sys.path.append(ROOT)

PACKERS = ("wino_pack_batched", "wino43_pack_batched", "pack_conv3x3_batched")
KEEP = ("lib", "ptr", "stream", "tile_fields", "stats_part_numel", "workspace", "attn_use_fused", "attn_supported")
KNOBS = ("VD_WINO", "VD_WINO43", "VD_WINO43_FWD", "VD_WINO43_OCC", "VD_WINO43_MIN_W", "VD_WINO_WIDE", "VD_GROUPED_WGRAD",
         "VD_GROUPED_AUTO_SPLIT", "VD_GN_FOLD", "VD_GN_FOLD_MAX_CHUNKS", "VD_READY_PER_BLOCK", "VD_FUSED_ATTN")    # (each would move a launch)
SWITCHES = {"e": dict(READY_PER_BLOCK=True), "g": dict(GROUPED_WGRAD=False), "h": dict(GN_FOLD=False), "i": dict(WINO=False)}


def _configs():
    from oracle.cases import CIFAR_COND, CELEBA, TINY
    out = {k: (v["cfg"], v["B"], v["R"], v["label"]) for k, v in TINY.items()}
    out.update(cifar=(CIFAR_COND, 2, 32, "single"), celeba=(CELEBA, 1, 64, "multi"))
    return out


def _scenarios(mname):
    return "abcd" + ("e" if mname in ("tinyA", "cifar") else "") + ("fghi" if mname == "tinyA" else "")


class Recorder:
    """replaces the launch wrappers of the ``_hip`` module ``H`` by recorders; ``log``: [[wrapper, args..., {kwargs}] | ["yield", name] |
    ["mark", what]]; undo() puts the wrappers back"""

    def __init__(self, H, model, **switches):
        self.H, self.saved = H, {}
        self.params = {id(p): k for k, p in model.named_parameters()}
        for name, fn in list(vars(H).items()):
            if isinstance(fn, types.FunctionType) and not name.startswith("_") and name not in KEEP \
                    and not name.endswith(("_supported", "_preferred", "_chunk_rows")):
                self._set(name, lambda *a, _n=name, **k: self._launch(_n, a, k))
        self._set("last_row_tile", lambda: 128)
        self._set("WGRAD_STREAM", False)
        for k, v in switches.items():
            self._set(k, v)
        self.begin({})

    def _set(self, name, value):
        self.saved.setdefault(name, getattr(self.H, name))
        setattr(self.H, name, value)

    def undo(self):
        for k, v in self.saved.items():
            setattr(self.H, k, v)

    def begin(self, G):
        """a new log; ``G``: the gradient tensors of the backward pass that follows (name -> tensor)"""
        self.log, self.keep, self.buffers, self.extent = [], [], {}, {}
        self.grads = {id(g): "grad:" + k for k, g in G.items()}
        self.grad_ptrs = {g.data_ptr(): "grad:" + k for k, g in G.items()}
        self.keep.extend(G.values())

    def mark(self, what):
        self.log.append(["mark", what])

    def listen(self, name):
        self.log.append(["yield", name])

    def _tensor(self, t):
        name = self.params.get(id(t)) or self.grads.get(id(t))
        if name is not None:
            return name
        self.keep.append(t)
        base = t.untyped_storage().data_ptr()
        n = self.buffers.setdefault(base, len(self.buffers))
        self.extent[base] = t.untyped_storage().nbytes()
        return [n, t.storage_offset(), list(t.shape), list(t.stride())]

    def _pointer(self, p):
        if p in self.grad_ptrs:
            return self.grad_ptrs[p]
        for base, n in self.buffers.items():
            if base <= p < base + self.extent[base]:
                return [n, (p - base) // 4]
        raise AssertionError(f"a table names an address no launch has seen: {p:#x}")

    def _norm(self, v):
        if torch.is_tensor(v):
            return self._tensor(v)
        if isinstance(v, (list, tuple)):
            return [self._norm(e) for e in v]
        assert v is None or isinstance(v, (bool, int, float, str)), type(v)
        return v

    def _launch(self, name, a, k):
        if name in PACKERS:
            self.log.append([name, a[1], a[2]])
        elif name == "gn_param_sums_batched":
            rows = [[self._pointer(p) for p in r[:3]] + r[3:] for r in a[0].tolist()]
            self.log.append([name, rows, a[1], a[2]])
        else:
            self.log.append([name] + self._norm(a) + [{key: self._norm(k[key]) for key in sorted(k)}])


def _digest(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()[:12]


def _compact(log):
    """what the fixture keeps of one trace: launches per wrapper, the yields, and per segment -- the launches up to and including the
    next yield or mark -- a digest"""
    counts = collections.Counter(e[0] for e in log if e[0] not in ("yield", "mark"))
    segments, cur = [], []
    for e in log:
        cur.append(e)
        if e[0] in ("yield", "mark"):
            segments.append(_digest(cur))
            cur = []
    assert not cur, "a trace ends with a yield or a mark"
    return dict(counts=dict(sorted(counts.items())), yields=[e[1] for e in log if e[0] == "yield"], segments=segments)


def _train_trace(eng, rec, inputs, steps, listen=True, need_dx=True):
    """training forward with tape, then backward: through backward_steps(join=False) (``steps``) or backward(progress=listener)"""
    x, t, y = inputs
    G = eng.new_grads()
    rec.begin(G)
    torch.manual_seed(7)
    out, tape = eng.forward(x, t, y, True, True)
    rec.mark("forward")
    dout = torch.zeros_like(out)
    if steps:
        gen = eng.backward_steps(tape, dout, G, need_dx=False, join=False)
        try:
            while True:
                rec.listen(next(gen))
        except StopIteration as fin:
            dx = fin.value
    else:
        dx = eng.backward(tape, dout, G, need_dx=need_dx, progress=rec.listen if listen else None)
    rec.mark("dx" if dx is not None else "no dx")
    assert eng._wq is None and eng._side is None
    return _compact(rec.log)


def _sample_trace(eng, rec, inputs):
    x, t, y = inputs
    rec.begin({})
    with eng.fixed_weights():
        for i in range(2):
            torch.manual_seed(7)
            eng.forward(x, t, y, False, False)
            rec.mark(f"forward {i}")
    return _compact(rec.log)


def _static_tables(eng, B, R):
    names = {id(p): k for k, p in eng.m.named_parameters()}
    order, segs = eng.completion_order(), eng.grad_segments()
    geoms = [[names[id(g[0])]] + list(g[1:]) for g in eng._conv_geoms(B, R, R)]
    return dict(progress_points=eng.progress_points(), completion_order=[len(order), _digest(order)],
                grad_segments=[[b, len(n)] for b, n in segs], grad_segments_names=_digest([list(s) for s in segs]),
                conv_geoms=[len(geoms), _digest(geoms)])


def _sweep(H, v_diffusion, mname):
    from oracle.cases import make_inputs
    cfg, B, R, label = _configs()[mname]
    torch.manual_seed(0)
    eng = v_diffusion.UNet(**cfg).engine()
    inputs = make_inputs(cfg, B, R, label)
    table = {}
    for s in _scenarios(mname):
        rec = Recorder(H, eng.m, **SWITCHES.get(s, {}))
        try:
            if s == "a":
                row = _train_trace(eng, rec, inputs, steps=True)
            elif s == "c":
                row = _sample_trace(eng, rec, inputs)
            elif s == "d":
                row = _static_tables(eng, B, R)
            else:
                row = _train_trace(eng, rec, (inputs[0], inputs[1], None) if s == "f" else inputs, steps=False)
        finally:
            rec.undo()
        table[f"{mname}/{s}"] = row
    return table


@pytest.fixture(scope="module")
def H():
    from v_diffusion import _hip
    set_knobs = [k for k in KNOBS if os.environ.get(k) is not None]
    assert not set_knobs, f"the recorded launches are those of the defaults: unset {set_knobs}"
    return _hip


@pytest.fixture(scope="module")
def want():
    assert os.path.exists(GOLDEN), f"{GOLDEN} missing"
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("mname", ["tinyA", "tinyB", "tinyC", "cifar", "celeba"])
def test_the_launch_trace_matches_the_recorded_one(H, want, mname):
    import v_diffusion
    got = _sweep(H, v_diffusion, mname)
    keys = [k for k in want if k.startswith(mname + "/")]
    assert sorted(got) == sorted(keys) and len(keys) == len(_scenarios(mname))
    for k in keys:
        if k.endswith("/d"):
            for part, w in want[k].items():
                assert got[k][part] == w, f"{k}: {part} moved: recorded {w}, now {got[k][part]}"
            continue
        assert got[k]["yields"] == want[k]["yields"], f"{k}: the yields moved"
        assert got[k]["counts"] == want[k]["counts"], f"{k}: launches per wrapper moved"
        g, w = got[k]["segments"], want[k]["segments"]
        moved = [i for i in range(len(w)) if g[i] != w[i]]
        ends = [f"yield {y}" for y in want[k]["yields"]]
        assert len(g) == len(w) and not moved, \
            f"{k}: segment {moved[0]} of {len(w)} moved (segments end at marks and yields; the yields: {ends})"


def test_the_fixture_is_small_and_holds_every_scenario(want):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert sorted(want) == sorted(f"{m}/{s}" for m in _configs() for s in _scenarios(m))
    per_level, per_block = want["cifar/b"]["yields"], want["cifar/e"]["yields"]
    # output convolution + (3 up levels, the middle, 3 down levels | each of the 14 + 3 + 11 blocks) + input convolution + the end
    assert per_level == want["cifar/d"]["progress_points"] and len(per_level) == 1 + 7 + 2 and len(per_block) == 1 + 28 + 2
    assert want["tinyA/g"]["counts"].get("gemm_grouped_wgrad", 0) == 0 < want["tinyA/b"]["counts"]["gemm_grouped_wgrad"]
    assert "gn_apply_from_partials" not in want["tinyA/h"]["counts"] and "conv3x3" in want["tinyA/i"]["counts"]
    assert "class_embed_bwd" in want["tinyA/b"]["counts"] and "class_embed_bwd" not in want["tinyA/f"]["counts"]
    assert want["tinyA/b"]["counts"]["nhwc_to_nchw"] == 1 and "nhwc_to_nchw" not in want["tinyA/a"]["counts"]      # d/dx only when asked


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    import v_diffusion
    from v_diffusion import _hip
    table = {}
    for m in _configs():
        table.update(_sweep(_hip, v_diffusion, m))
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in table.items()) + "\n}\n")
    print(f"{len(table)} traces from {os.path.dirname(v_diffusion.__file__)} -> {GOLDEN}")
