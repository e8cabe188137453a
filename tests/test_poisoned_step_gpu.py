"""The whole network on recycled memory: one tinyA backward, then NaN in every cached scratch buffer of v_diffusion._hip and in every block
the caching allocator will hand out next (tests/poison.py), then the same backward again -- the parameter gradients must come out bit for
bit the same, finite.  In a training run the engine's activations, tapes and gradient tensors are torch.empty on the previous step's bytes
and the scratch holds the previous layer's data; a test process otherwise sees zeros or small finite leftovers there.  Needs an MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison as P                                                # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from v_diffusion import _hip
    _hip.lib()
    return _hip


# B = 4: the product's default dispatch (fused kernels at this size); B = 32 with forwards and input gradients through planes wherever
# supported (512 tiles at 16x16: V kept on the tape, dM written per layer, weight gradients from (V, dM) on the side stream)
@pytest.mark.parametrize("B,planes", [(4, False), (32, True)], ids=["B4_default", "B32_planes"])
def test_tiny_backward_twice_on_poisoned_memory(H, B, planes):
    import v_diffusion
    from oracle import detrand
    from oracle.cases import TINY, make_inputs, make_weights
    case = TINY["tinyA"]
    cfg, R = case["cfg"], case["R"]
    x, t, y = (v.to(DEV) for v in make_inputs(cfg, B, R, case["label"]))
    gout = detrand.normal("gout", (B, cfg["out_channels"], R, R), 1).to(DEV)
    model = v_diffusion.UNet(**cfg)
    model.load_state_dict(make_weights(cfg))
    model.to(DEV).train()
    saved, calls = (H.CONV_PLANES, H.DGRAD_PLANES), [0]
    real = H.conv3x3_wino43_dgrad_planes

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    def grads():
        model.zero_grad(set_to_none=True)
        torch.manual_seed(5)                                    # dropout seeds are drawn from the default generator
        (model(x, t, y) * gout).sum().backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in model.named_parameters()}
    H.conv3x3_wino43_dgrad_planes = spy
    try:
        if planes:
            H.CONV_PLANES = H.DGRAD_PLANES = "2"
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        first = grads()
        peak = torch.cuda.max_memory_allocated()
        assert (calls[0] > 0) == planes, calls[0]
        model.zero_grad(set_to_none=True)                       # the gradient tensors go back to the allocator too
        found = P.poison_workspaces(H, P.FLOAT_TAGS)
        want = {"wgrad", "gn"} | ({"planes", "wgrad43", "dgrad_planes"} if planes else set())
        assert want <= found, f"scratch the step uses was not poisoned: cached {sorted(found)}"
        why = P.poison_allocator(peak)
        assert not why, f"the allocator was not poisoned: {why}"
        second = grads()
    finally:
        (H.CONV_PLANES, H.DGRAD_PLANES), H.conv3x3_wino43_dgrad_planes = saved, real
    assert first.keys() == second.keys()
    for k, a in first.items():
        assert torch.isfinite(a).all(), f"{k}: first run not finite"
        b = second[k]
        assert torch.isfinite(b).all(), f"{k}: {int((~torch.isfinite(b)).sum())} of {b.numel()} gradient elements not finite on poisoned memory"
        assert P.same_bits(a, b), f"{k}: {int((a != b).sum())} of {a.numel()} gradient elements differ on poisoned memory"
