"""tests/poison.py does what it says -- on the CPU, with a stand-in for v_diffusion._hip's workspace cache."""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison                                                     # noqa: E402


def test_pitched_pads_with_nan_and_keeps_the_real_columns_exact():
    x = torch.randn(2, 5, 3, 4)
    p = poison.pitched(x, 8, device="cpu")
    assert p.shape == (2, 3, 4, 8)
    assert torch.equal(p[..., :5], x.permute(0, 2, 3, 1))
    assert torch.isnan(p[..., 5:]).all()
    q = poison.pitched(x, 8, pad=poison.SENTINEL, device="cpu")
    assert (q[..., 5:] == -777.0).all() and torch.equal(q[..., :5], p[..., :5])
    assert torch.equal(poison.pitched(x, 5, device="cpu"), x.permute(0, 2, 3, 1))           # no pitch columns: nothing but the data
    m = poison.pitched_rows(torch.arange(6.0).reshape(2, 3), 4, device="cpu")
    assert torch.equal(m[:, :3], torch.arange(6.0).reshape(2, 3)) and torch.isnan(m[:, 3]).all()


def test_same_bits_is_equality_of_bit_patterns():
    nan = torch.tensor([float("nan"), 1.0])
    assert poison.same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not poison.same_bits(torch.tensor([-0.0]), torch.tensor([0.0])) and torch.equal(torch.tensor([-0.0]), torch.tensor([0.0]))
    other_nan = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert not poison.same_bits(torch.tensor([float("nan")]), other_nan)                   # two NaNs of different payload
    assert not poison.same_bits(torch.zeros(3), torch.zeros(4)) and not poison.same_bits(torch.zeros(3), torch.zeros(3, dtype=torch.float64))
    a = torch.randn(4, 6)
    assert poison.same_bits(a[:, :3], a[:, :3].clone())                                    # non-contiguous views
    b = a.clone()
    b[3, 2] = torch.nextafter(b[3, 2], torch.tensor(9.0))
    assert not poison.same_bits(a[:, :3], b[:, :3])


def test_poison_workspaces_fills_only_the_named_tags_whole_on_every_stream():
    cache = {("cpu", 0, "splitk"): torch.zeros(8), ("cpu", 7, "splitk"): torch.ones(5), ("cpu", 0, "gn"): torch.zeros(4),
             ("cpu", 0, "knn"): torch.arange(4.0), ("cpu", 0, "default"): torch.zeros(2)}
    stand_in = types.SimpleNamespace(_ws_cache=cache)
    found = poison.poison_workspaces(stand_in, ("splitk", "wgrad43"))
    assert found == {"splitk"}                                                             # "wgrad43" has no buffer: not reported
    assert torch.isnan(cache[("cpu", 0, "splitk")]).all() and torch.isnan(cache[("cpu", 7, "splitk")]).all()
    assert torch.equal(cache[("cpu", 0, "gn")], torch.zeros(4)) and torch.equal(cache[("cpu", 0, "knn")], torch.arange(4.0))
    assert torch.equal(cache[("cpu", 0, "default")], torch.zeros(2))
    assert poison.poison_workspaces(stand_in, poison.FLOAT_TAGS) == {"splitk", "gn"}
    assert torch.isnan(cache[("cpu", 0, "gn")]).all() and torch.equal(cache[("cpu", 0, "knn")], torch.arange(4.0))
    assert not set(poison.FLOAT_TAGS) & {"knn", "knn_hits", "kid", "is"}


def test_band_sizes_hold_an_image_and_256_rows_in_whole_512_byte_lines():
    for shape, least in (((3, 16, 16, 40), 1 << 16), ((2, 64, 64, 264), 64 * 64 * 264), ((1000, 300), 256 * 300), ((5,), 1 << 16),
                         ((100003,), 1 << 16), ((4, 32, 2), 1 << 16), ((1, 8, 128, 1000), 8 * 128 * 1000)):
        b = poison.band_elems(shape)
        assert b >= least and b % 128 == 0 and b - least < 128, (shape, b)
        assert b >= 256 * shape[-1] * (len(shape) > 1) and b >= 1 << 16
    assert poison.band_elems((7, 3), itemsize=1, floor=1) == 1024 and poison.band_elems((7, 3), itemsize=8, floor=1) == 768
    assert poison.band_elems((10,), floor=poison.WS_BAND_BYTES // 4) * 4 == 1 << 20


def test_banded_view_aliases_the_middle_and_keeps_its_alignment():
    poison.forget_bands()
    for shift in (0, 4):
        b = poison.Banded((3, 5, 7), 7.0, poison.SENTINEL, device="cpu", shift=shift)
        n, band = 3 * 5 * 7, b.band
        assert b.real.shape == (3, 5, 7) and b.real.is_contiguous() and b.whole.numel() == 2 * band + shift + n
        assert b.real.data_ptr() - b.whole.data_ptr() == 4 * (band + shift) and (4 * band) % 512 == 0
        assert (b.real == 7.0).all() and (b.whole[:band + shift] == poison.SENTINEL).all() and (b.whole[band + shift + n:] == poison.SENTINEL).all()
        b.real[2, 4, 6] = 1.5                                     # the view IS the middle of the allocation
        assert b.whole[band + shift + n - 1] == 1.5 and b.intact()
        front, back = b.bands()
        assert front.numel() == band + shift and back.numel() == band
    x = torch.randn(2, 5, 3, 4)
    for pad in (3.0, poison.NAN):
        p = poison.pitched(x, 8, pad=pad, device="cpu")
        rec = poison._ledger[-1]
        assert rec.real is p and p.data_ptr() - rec.whole.data_ptr() == 4 * rec.band and rec.band >= 1 << 16
        assert all(bool(torch.isnan(t).all() if pad != pad else (t == pad).all()) for t in rec.bands())
        assert rec.intact() and not rec.check                   # a source's bands hold the pad value and are not a destination's
    m = poison.pitched_rows(torch.arange(6.0).reshape(2, 3), 4, pad=3.0, device="cpu", shift=4)
    rec = poison._ledger[-1]
    assert m.data_ptr() - rec.whole.data_ptr() == 4 * (rec.band + 4) and torch.equal(m[:, :3], torch.arange(6.0).reshape(2, 3))
    u8 = poison.Banded((2, 4, 4, 3), 0, 9, dtype=torch.uint8, device="cpu")
    assert u8.band % 512 == 0 and u8.intact()
    poison.forget_bands()


def test_intact_notices_one_changed_float_in_either_band():
    poison.forget_bands()
    for fill in (poison.SENTINEL, poison.NAN):
        b = poison.Banded((4, 6), 0.0, fill, device="cpu", shift=4)
        n = b.whole.numel()
        for where in (0, b.lo - 1, b.lo + 24, n - 1):                # first and last float of each band
            assert b.intact() and b.damage() == ""
            keep = b.whole[where].clone()
            b.whole[where] = 0.25
            assert not b.intact() and "1 elements" in b.damage(), (fill, where)
            assert ("front" in b.damage()) == (where < b.lo)
            b.whole[where] = keep
        b.real.fill_(poison.NAN)                                  # the real part is not a band
        assert b.intact()
    assert poison.bands_damage(clear=False) == ""
    poison._ledger[0].whole[3] = 1.0
    assert "(4, 6)" in poison.bands_damage() and poison._ledger == []
    a = poison.banded((5,), 1.0, device="cpu")
    assert a.shape == (5,) and len(poison._ledger) == 1 and poison._ledger[0].check
    a.data.as_strided((1,), (1,), a.storage_offset() + 5)[0] = 2.0    # one float behind the end
    assert "behind its end" in poison.bands_damage()


def test_exact_workspace_hands_out_exactly_the_bytes_asked_for():
    poison.forget_bands()
    ws = poison.ExactWorkspace(stream_of=lambda device: 0)
    a = ws(100, "cpu", "gn")
    assert a.numel() * 4 == 112 and torch.isnan(a).all() and ws.requests == [("gn", 100)]
    rec = ws.cache[("cpu", 0, "gn")]
    assert rec.band * 4 >= 1 << 20 and (rec.band * 4) % 512 == 0 and a.data_ptr() - rec.whole.data_ptr() == 4 * rec.band
    a.fill_(1.0)
    assert ws(100, "cpu", "gn") is a and torch.isnan(a).all()              # same key, same size: the same buffer, NaN again
    c = ws(4096, "cpu", "gn")
    assert c.numel() == 1024 and c is not a and len(ws.all) == 2            # another size: never more than asked for
    d = ws(16, "cpu", "splitk")
    assert d.numel() == 4 and ws.tags() == {"gn", "splitk"} and ws.intact()
    other = poison.ExactWorkspace(stream_of=lambda device: 7)
    assert other(16, "cpu", "splitk") is not d
    rec.whole[rec.lo + 28] = 0.0                                            # the first float behind the 112 bytes of the FIRST buffer
    assert not ws.intact() and "112 bytes" in ws.damage()
    assert poison._ledger == []                                             # scratch is checked through the stand-in, not the ledger


def test_shifted_moves_every_new_banded_tensor_but_no_scratch():
    poison.forget_bands()
    x = torch.randn(2, 5, 3, 4)
    with poison.shifted(4):
        a = poison.pitched(x, 8, device="cpu")
        b = poison.on_device(torch.arange(5, dtype=torch.int32), device="cpu")
        c = poison.banded((3, 7), 1.0, device="cpu")
        with poison.shifted(0):
            d = poison.banded((3, 7), 1.0, device="cpu")
        e = poison.banded((3, 7), 1.0, device="cpu", shift=0)
        ws = poison.ExactWorkspace(stream_of=lambda device: 0)(64, "cpu", "gn")
    f = poison.banded((3, 7), 1.0, device="cpu")
    recs = {id(r.real): r for r in poison._ledger}
    off = lambda t: (t.data_ptr() - recs[id(t)].whole.data_ptr()) % 512
    assert [off(t) for t in (a, c)] == [16, 16] and off(b) == 16 and [off(t) for t in (d, e, f)] == [0, 0, 0]
    assert (recs[id(b)].bands()[0] == torch.iinfo(torch.int32).max).all() and torch.equal(b, torch.arange(5, dtype=torch.int32))
    assert torch.equal(a[..., :5], x.permute(0, 2, 3, 1)) and all(r.intact() for r in poison._ledger)
    assert ws.numel() == 16 and len(poison._ledger) == 6          # the scratch buffer is not in the ledger, nor shifted
    serials = [r.serial for r in poison._ledger]
    assert serials == sorted(serials) and len(set(serials)) == 6 and poison.Banded.made >= serials[-1]
    poison.forget_bands()


def test_exact_workspace_forces_one_request_of_a_tag():
    ws = poison.ExactWorkspace(stream_of=lambda device: 0, force={"gn": 40}, only={"gn": 1})
    sizes = [ws(100, "cpu", "gn").numel() * 4, ws(100, "cpu", "gn").numel() * 4, ws(100, "cpu", "gn").numel() * 4, ws(100, "cpu", "wgrad").numel() * 4]
    assert sizes == [112, 40, 112, 112] and ws.requests == [("gn", 100)] * 3 + [("wgrad", 100)]
    every = poison.ExactWorkspace(stream_of=lambda device: 0, force={"gn": 96})
    assert [every(100, "cpu", "gn").numel() * 4 for _ in range(2)] == [96, 96] and every.intact()
    poison.forget_bands()


def test_float_tags_are_workspace_tags_of_the_binding():
    """every poisoned tag is one _hip.workspace is called with (a renamed tag would silently leave its buffer clean)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "v-diffusion-torch_amd", "v_diffusion", "_hip.py")) as f:
        used = set(re.findall(r'workspace\([^\n]*?, "(\w+)"\)', f.read()))
    assert set(poison.FLOAT_TAGS) <= used, set(poison.FLOAT_TAGS) - used
    assert used - set(poison.FLOAT_TAGS) == {"knn", "knn_hits", "kid", "is"}, used
