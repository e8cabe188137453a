"""Packed 3x3 weight images of the engine (v_diffusion/engine.py: ConvPacks), without a device.

A ``UNet`` built on the CPU gives CPU buffers, the library's ``*_supported`` / ``*_preferred`` predicates are host arithmetic (without a
device the CU count answers 256) and the launch wrappers are replaced by recorders, so what the engine WOULD launch is observable here:

  * layout: the device tables of the batched pack launches (weights as layer indices, every destination column relative to its
    smallest non-null entry, in floats), their row and block counts, and the element counts of the persistent buffers;
  * selection: per layer, direction and pitch case which convolution wrapper ``_conv`` calls, where its image argument lies (offset in
    its buffer, shape, buffer size), the chunk rows it returns, and whether an image was packed on demand.

Both are pinned to tests/golden/conv_packs.json, recorded through the two private seams ``engine._pack_all(need_d, geom)`` and
``engine._conv(...)`` from the engine as it stood BEFORE the pack state became one object (untyped dicts and positional tuples), so the
recorder runs unmodified on either side.  The fixture keeps the counts and the per-layer choice readable and the bulk (tables, image
locations) as digests (_compact): a digest that moved names its pack call, and --record on both sides shows the difference.

    python tests/test_conv_packs_cpu.py --record      rewrites the fixture from the package on sys.path -- only for a change that is
                                                      MEANT to move a layout or a choice
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_packs.json")
if not any(os.path.isdir(os.path.join(p, "v_diffusion")) for p in sys.path if p):       # (--record: the package under test may come first)
    sys.path.insert(0, os.path.join(ROOT, "v-diffusion-torch_amd"))
if ROOT not in sys.path:
    sys.path.append(ROOT)

PACKERS = ("wino_pack_batched", "wino43_pack_batched", "pack_conv3x3_batched")
CONVS = ("conv3x3_wino43_fwd", "conv3x3_dgrad_wino43", "conv3x3_wino", "conv3x3")
DEST_COLS = {"wino_pack_batched": (1, 2), "wino43_pack_batched": (1,), "pack_conv3x3_batched": (1, 2)}
KNOBS = ("VD_WINO", "VD_WINO43", "VD_WINO43_FWD", "VD_WINO43_OCC", "VD_WINO43_MIN_W", "VD_WINO_WIDE")     # (each would move a choice)


def _models():
    from oracle.cases import CIFAR_COND, CELEBA, TINY
    out = {"cifar": (CIFAR_COND, 32), "celeba": (CELEBA, 64)}
    out.update({k: (v["cfg"], v["R"]) for k, v in TINY.items()})
    return out


class Recorder:
    """replaces the launch wrappers of v_diffusion._hip by recorders (``log``: [(name, args, kwargs)]); undo() puts them back"""

    def __init__(self, H, **switches):
        self.H, self.log, self.allocs, self.saved = H, [], [], {}
        for name in PACKERS + CONVS + ("wino_pack", "pack_conv3x3"):
            self._set(name, lambda *a, _n=name, **k: self.log.append((_n, a, k)))
        self._set("last_row_tile", lambda: 128)
        real_rows = H.wino43_fwd_chunk_rows
        self._set("wino43_fwd_chunk_rows", lambda Hh, Ww: self.log.append(("wino43_fwd_chunk_rows", (Hh, Ww), {})) or real_rows(Hh, Ww))
        for k, v in switches.items():
            self._set(k, v)
        real_empty = torch.empty
        self.saved_empty = real_empty

        def empty(*a, **k):
            t = real_empty(*a, **k)
            self.allocs.append(t.numel())
            return t
        torch.empty = empty

    def _set(self, name, value):
        self.saved.setdefault(name, getattr(self.H, name))
        setattr(self.H, name, value)

    def undo(self):
        torch.empty = self.saved_empty
        for k, v in self.saved.items():
            setattr(self.H, k, v)

    def take(self):
        log, allocs = self.log[:], self.allocs[:]
        del self.log[:], self.allocs[:]
        return log, allocs


def _engine(cfg):
    import v_diffusion
    torch.manual_seed(0)
    return v_diffusion.UNet(**cfg).engine()


def _weights(eng):
    return [c.weight for b in eng.plan if b.res is not None for c in (b.res.conv1, b.res.conv2)]


def _pack_record(eng, rec, need_d, geom):
    """one _pack_all call -> {launches: [[name, n, total_blocks, normalised table]], allocs: element counts of what it allocated}"""
    index = {w.data_ptr(): i for i, w in enumerate(_weights(eng))}
    rec.take()
    made = eng._pack_all(need_d, geom)
    if hasattr(eng, "_packed"):          # the engine the fixture was recorded from: its forward stored the direct packs _pack_all returned
        eng._packed = made
    log, allocs = rec.take()
    launches = []
    for name, (table, n, blocks), _ in log:
        rows = [list(r) for r in table.tolist()]
        assert len(rows) == n and all(r[0] in index for r in rows)
        for c in DEST_COLS[name]:
            base = min((r[c] for r in rows if r[c]), default=0)
            for r in rows:
                assert (r[c] - base) % 4 == 0
                r[c] = (r[c] - base) // 4 if r[c] else -1
        for r in rows:
            r[0] = index[r[0]]
        launches.append([name, n, blocks, rows])
    return dict(launches=launches, allocs=allocs)


def _image(t):
    return [t.storage_offset(), list(t.shape), t.untyped_storage().nbytes() // 4]


def _conv_cases(dgrad, Cin, Cout):
    """(ldx, ldy, residual?) of the three pitch cases: dense; the output a channel slice of a concat buffer; forward with a residual /
    input gradient of a tensor that is itself such a slice (the input gradient never takes a residual)"""
    return [(Cin, Cout, False), (Cin, 2 * Cout, False), (2 * Cin, Cout, False) if dgrad else (Cin, Cout, True)]


def _conv_record(eng, rec, need_d, call_geom):
    """per layer, direction and pitch case: [wrapper, image, chunk rows, images packed on demand]"""
    out = []
    for (w, nb, lh, lw, ci, co) in eng._conv_geoms(*call_geom):
        for dgrad in ((False, True) if need_d else (False,)):
            Cin, Cout = (co, ci) if dgrad else (ci, co)
            for ldx, ldy, has_res in _conv_cases(dgrad, Cin, Cout):
                rec.take()
                rows = eng._conv("x", ldx, w, None if dgrad else "bias", "y", ldy, nb, lh, lw, Cin, Cout, dgrad=dgrad,
                                 res="res" if has_res else None, ldres=Cout if has_res else 0, stats_part=None if dgrad else "part")
                log, _ = rec.take()
                calls = [e for e in log if e[0] in CONVS]
                assert len(calls) == 1, log
                name, a, k = calls[0]
                assert a[0] == "x" and a[1] == ldx and (k.get("res") == "res") == has_res
                packed = [e[0] for e in log if e[0] in ("wino_pack", "pack_conv3x3")]
                out.append([CONVS.index(name), _image(a[2]), rows, len(packed)])
    return out


def _geoms(R):
    return [(128, R, R), (256, R, R), (2, R, R), None]


def _switch_sets():
    return {"default": {}, "no_wino": dict(WINO=False), "no_f43_fwd": dict(WINO43_FWD=False)}


def _sweep(H, models=None):
    table = {}
    for mname, (cfg, R) in _models().items():
        if models is not None and mname not in models:
            continue
        for sname, switches in _switch_sets().items():
            rec = Recorder(H, **switches)
            try:
                eng = _engine(cfg)
                for need_d in (True, False):
                    for geom in _geoms(R):
                        rowkey = f"{mname}/{sname}/need_d={int(need_d)}/{'none' if geom is None else geom[0]}"
                        row = _pack_record(eng, rec, need_d, geom)
                        row["conv"] = _conv_record(eng, rec, need_d, geom or (128, R, R))
                        table[rowkey] = row
            finally:
                rec.undo()
    return table


def _digest(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()[:12]


def _compact(row):
    """what the fixture keeps of one pack call: per launch [wrapper, rows, blocks, digest of the normalised table], the allocation sizes,
    ``pick`` = the convolution wrapper (index into CONVS) per (layer, direction) -- one digit where the three pitch cases agree, "(abc)"
    where they do not -- and the digest of the full selection record (images, chunk rows, on-demand packs)"""
    conv = row["conv"]
    groups = ["".join(str(c[0]) for c in conv[i:i + 3]) for i in range(0, len(conv), 3)]
    return dict(launches=[[name, n, blocks, _digest(rows)] for name, n, blocks, rows in row["launches"]], allocs=row["allocs"],
                pick="".join(g[0] if len(set(g)) == 1 else f"({g})" for g in groups), conv=_digest(conv))


@pytest.fixture(scope="module")
def H():
    from v_diffusion import _hip
    set_knobs = [k for k in KNOBS if os.environ.get(k) is not None]
    assert not set_knobs, f"the recorded choices are the defaults: unset {set_knobs}"
    return _hip


@pytest.fixture(scope="module")
def want():
    assert os.path.exists(GOLDEN), f"{GOLDEN} missing"
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("mname", ["cifar", "celeba", "tinyA", "tinyB", "tinyC"])
def test_layout_and_selection_match_the_recorded_table(H, want, mname):
    got = {k: _compact(v) for k, v in _sweep(H, models=(mname,)).items()}
    keys = [k for k in want if k.startswith(mname + "/")]
    assert len(keys) == 24 and sorted(got) == sorted(keys)
    for k in keys:
        for part in ("launches", "allocs", "pick", "conv"):
            assert got[k][part] == want[k][part], f"{k}: {part} moved: recorded {want[k][part]}, now {got[k][part]}"


def test_the_fixture_has_both_answers_of_every_choice(want):
    import re
    fwd = lambda k: re.findall(r"\(\d+\)|\d", want[k]["pick"])[0::2]              # (need_d rows: forward, input gradient per layer)
    tabs = lambda k: {l[0]: l[1] for l in want[k]["launches"]}
    big, small = "cifar/default/need_d=1/128", "cifar/default/need_d=1/2"
    assert len(fwd(big)) == len(fwd(small)) == 54
    assert fwd(big).count("0") == 34 and fwd(small).count("0") == 0             # forward F(4x4,3x3): 34 of the 54 layers at B = 128, none at B = 2
    assert "wino43_pack_batched" in tabs(big) and "wino43_pack_batched" not in tabs(small) and tabs(small)["wino_pack_batched"] == 54
    assert {ch for row in want.values() for ch in row["pick"] if ch.isdigit()} == set("0123")      # every wrapper is some layer's answer
    assert list(tabs("cifar/no_wino/need_d=1/128")) == ["pack_conv3x3_batched"]
    assert "0" not in want["cifar/no_f43_fwd/need_d=1/128"]["pick"] and "1" in want["cifar/no_f43_fwd/need_d=1/128"]["pick"]


# ------------------------------------------------------------------------------------------------ fallback image and ownership
def _mute(H, monkeypatch):
    """every launch wrapper of _hip becomes a no-op (the predicates and host-side helpers stay): a whole forward / backward then runs on
    CPU buffers and only moves the engine's state"""
    import types
    keep = ("lib", "ptr", "stream", "tile_fields", "stats_part_numel", "workspace", "attn_use_fused", "attn_supported")
    for name, fn in list(vars(H).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith("_") and name not in keep \
                and not name.endswith(("_supported", "_preferred", "_chunk_rows")):
            monkeypatch.setattr(H, name, lambda *a, **k: None)
    monkeypatch.setattr(H, "last_row_tile", lambda: 128)
    monkeypatch.setattr(H, "WGRAD_STREAM", False)
    monkeypatch.setattr(H, "GROUPED_WGRAD", False)
    monkeypatch.setattr(H, "WINO43_OCC", False)


def _tiny(B=4):
    from oracle.cases import TINY, make_inputs
    case = TINY["tinyA"]
    eng = _engine(case["cfg"])
    x, t, y = make_inputs(case["cfg"], B, case["R"], case["label"])
    return eng, x, t, y


def test_declined_f43_layer_takes_one_stable_fallback_image_per_weight_and_direction(H, monkeypatch):
    _mute(H, monkeypatch)
    eng, x, t, y = _tiny()
    out, tape = eng.forward(x, t, y, True, True)
    packs = eng._packs
    assert packs is eng.packs and tape["packs"] is packs
    w = next(w for (w, nb, lh, lw, ci, co) in eng._conv_geoms(4, 16, 16)
             if H.wino43_fwd_supported(nb, lh, lw, ci, co, ci, co, co) and H.wino43_supported(nb, lh, lw, ci, co, co, ci))
    co, ci = w.shape[0], w.shape[1]
    calls, packs_made = [], []
    monkeypatch.setattr(H, "conv3x3_wino", lambda *a, **k: calls.append(a[2]))
    monkeypatch.setattr(H, "conv3x3_wino43_fwd", lambda *a, **k: calls.append("f43"))
    monkeypatch.setattr(H, "conv3x3_dgrad_wino43", lambda *a, **k: calls.append("d43"))
    monkeypatch.setattr(H, "wino_pack", lambda w_, co_, ci_, uf=None, ud=None: packs_made.append((w_, uf, ud)))
    eng._conv("x", ci, w, "b", "y", co, 4, 16, 16, ci, co)
    assert calls == ["f43"] and not packs_made                                  # as packed: the F(4x4,3x3) image
    real = H.wino43_fwd_supported
    monkeypatch.setattr(H, "wino43_fwd_supported", lambda *a: False if a[3:5] == (ci, co) else real(*a))     # declines at call time
    monkeypatch.setattr(H, "wino43_supported", lambda *a: False)
    del calls[:]
    real_empty, allocs = torch.empty, []
    monkeypatch.setattr(torch, "empty", lambda *a, **k: allocs.append(a) or real_empty(*a, **k))
    for _ in range(2):
        eng._conv("x", ci, w, "b", "y", co, 4, 16, 16, ci, co)
        eng._conv("dy", co, w, None, "dx", ci, 4, 16, 16, co, ci, dgrad=True)
    monkeypatch.setattr(torch, "empty", real_empty)
    assert len(allocs) == 2, allocs                                             # one allocation per (weight, direction)
    assert all(torch.is_tensor(c) for c in calls) and calls[0].data_ptr() == calls[2].data_ptr() and calls[1].data_ptr() == calls[3].data_ptr()
    assert tuple(calls[0].shape) == (16, co, ci) and tuple(calls[1].shape) == (16, ci, co) and calls[0].data_ptr() != calls[1].data_ptr()
    assert len(packs_made) == 4 and all(p[0] is w for p in packs_made)          # re-packed on every call
    assert [p[1] is not None for p in packs_made] == [True, False, True, False] and [p[2] is not None for p in packs_made] == [False, True] * 2
    # the images live with the packs object the tape and the engine name: nothing else has to keep them alive
    held = {t_.data_ptr() for t_ in packs.fallback.values()}
    assert held == {calls[0].data_ptr(), calls[1].data_ptr()} and tape["packs"] is eng.packs is packs


def test_a_sampler_chain_keeps_its_packs_and_the_tape_keeps_its_forwards(H, monkeypatch):
    _mute(H, monkeypatch)
    eng, x, t, y = _tiny()
    seen = []
    real_conv = eng._conv
    monkeypatch.setattr(eng, "_conv", lambda *a, **k: seen.append(eng._packs) or real_conv(*a, **k))
    with eng.fixed_weights():
        eng.forward(x, t, y, False, False)
        chain = eng.packs
        assert chain is not None and set(seen) == {chain}
        foreign = eng._pack_all(True, (8, 16, 16))                              # somebody else packs between two steps of the chain
        assert eng._packs is not chain
        del seen[:]
        eng.forward(x, t, y, False, False)
        assert seen and all(p is chain for p in seen) and eng.packs is chain
        assert eng._fixed["packs"] is chain
    assert eng._fixed is None                                                   # nothing stays cached after the chain
    # backward uses the packs of ITS forward, whatever ran since
    out, tape = eng.forward(x, t, y, True, True)
    mine = tape["packs"]
    eng.forward(x[:2], t[:2], y[:2], True, True)
    assert eng._packs is not mine
    del seen[:]
    eng.backward(tape, torch.zeros_like(out), eng.new_grads())
    assert seen and all(p is mine for p in seen)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    import v_diffusion
    from v_diffusion import _hip
    table = {k: _compact(v) for k, v in _sweep(_hip).items()}
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in table.items()) + "\n}\n")
    print(f"{len(table)} pack calls from {os.path.dirname(v_diffusion.__file__)} -> {GOLDEN}")
