"""The mask rule of v_diffusion/restore.py is ONE rule: the inpainting entry (``p_sample_inpaint``) and the measurement operator of DPS and
DDNM (``("mask", mask)`` through ``dps_measure``, ``ddnm_pinv``, ``p_sample_dps``, ``p_sample_ddnm``) refuse the same bad masks and accept
the same good ones.  Images of a few pixels, CPU tensors: a refusal comes before anything touches a device, and an accepted mask shows as
the NEXT refusal of a sampler entry -- its tensors are not on an MI355X."""
import pytest
import torch

import v_diffusion as vd

B, C, H, W = SHAPE = (2, 3, 4, 5)
BAD = {
    "rank 3": torch.ones(C, H, W), "rank 5": torch.ones(1, B, C, H, W), "not a tensor": [[[[1.0]]]],
    "batch": torch.ones(B + 1, 1, H, W), "channels": torch.ones(B, 2, H, W), "height": torch.ones(B, 1, H + 1, W),
    "width": torch.ones(B, 1, H, W - 1), "int32": torch.ones(B, 1, H, W, dtype=torch.int32), "uint8": torch.ones(1, 1, H, W, dtype=torch.uint8),
    "above 1": torch.full((B, 1, H, W), 1.5), "below 0": torch.full((1, C, H, W), -0.1), "nan": torch.full((B, C, H, W), float("nan")),
    "one nan": torch.cat([torch.full((1, 1, H, W - 1), 0.5), torch.full((1, 1, H, 1), float("nan"))], dim=3),
}
GOOD = {
    "bool": torch.ones(B, 1, H, W) > 0, "bool shared": torch.zeros(1, 1, H, W) > 0, "float (1,1,H,W)": torch.full((1, 1, H, W), 0.25),
    "float (B,C,H,W)": torch.rand((B, C, H, W), generator=torch.Generator().manual_seed(1)), "float (1,C,H,W)": torch.ones(1, C, H, W),
    "fp64 ends": torch.tensor([0.0, 1.0], dtype=torch.float64).repeat(B, 1, H * W // 2).reshape(B, 1, H, W),
}


class _Net:
    training = False

    def __call__(self, x, t, y):
        raise AssertionError("the network must not be called")


def _entries():
    """name -> call(mask), every way a mask enters the package"""
    gd = vd.GaussianDiffusion(vd.get_logsnr_schedule("cosine", -20.0, 20.0), 4, "v", "fixed_large", "snr_trunc", "mse", w_guide=0.0)
    x = torch.zeros(SHAPE)
    return {"p_sample_inpaint": lambda m: gd.p_sample_inpaint(_Net(), x, m, seed=1),
            "p_sample_dps": lambda m: gd.p_sample_dps(_Net(), x, ("mask", m), SHAPE, seed=1),
            "p_sample_ddnm": lambda m: gd.p_sample_ddnm(_Net(), x, ("mask", m), SHAPE, seed=1),
            "dps_measure": lambda m: vd.dps_measure(x, ("mask", m)),
            "ddnm_pinv": lambda m: vd.ddnm_pinv(x, ("mask", m), SHAPE)}


@pytest.mark.parametrize("case", BAD)
def test_every_entry_refuses_the_bad_mask(case):
    said = {}
    for name, call in _entries().items():
        with pytest.raises(ValueError, match="mask") as e:
            call(BAD[case])
        said[name] = str(e.value)
    # one rule, one wording: the entries differ in what they call the image batch and in nothing else
    assert len({s.replace("known of shape", "images of shape") for s in said.values()}) == 1, said
    assert ("known of shape" in said["p_sample_inpaint"]) == ("images of shape" in said["dps_measure"])


@pytest.mark.parametrize("case", GOOD)
def test_every_entry_accepts_the_good_mask(case):
    m = GOOD[case]
    for name, call in _entries().items():
        if name.startswith("p_sample"):
            with pytest.raises(RuntimeError, match="MI355X"):          # past every argument check: the tensors are CPU tensors
                call(m)
        else:
            assert tuple(call(m).shape) == SHAPE
    assert vd.restore.mask_channels(m, SHAPE) == m.shape[1]
