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


def test_float_tags_are_workspace_tags_of_the_binding():
    """every poisoned tag is one _hip.workspace is called with (a renamed tag would silently leave its buffer clean)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "v-diffusion-torch_amd", "v_diffusion", "_hip.py")) as f:
        used = set(re.findall(r'workspace\([^\n]*?, "(\w+)"\)', f.read()))
    assert set(poison.FLOAT_TAGS) <= used, set(poison.FLOAT_TAGS) - used
    assert used - set(poison.FLOAT_TAGS) == {"knn", "knn_hits", "kid", "is"}, used
