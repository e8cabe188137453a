"""What the restoration samplers share -- ``p_sample_inpaint`` (RePaint), ``p_sample_dps`` and ``p_sample_ddnm``: the mask rule, the
measurement operator A of the latter two (its parser, A itself, its pseudo-inverse), the parser of a per-grid-index parameter, and the
opening of a chain: device, seeded draws, the given image and the mask on the device, the ``Chain``."""
import numbers

import torch
import torch.nn.functional as F

from .chain import Chain
from .diffusion import _device_ctx

OPERATORS = ("mask", "down", "gray")
DOWN_FACTORS = (2, 4, 8)


def mask_channels(mask, shape, what="images"):
    """the mask rule, for ``what`` of ``shape`` = (B, C, H, W): a tensor of shape (B or 1, 1 or C, H, W), bool, or float with every
    value in [0, 1].  Returns its channel count."""
    B, C, H, W = shape
    if not torch.is_tensor(mask) or mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, C) \
            or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f"mask must have shape (B or 1, 1 or C, H, W) for {what} of shape {tuple(shape)}, got "
                         f"{tuple(getattr(mask, 'shape', ()))}")
    if mask.dtype != torch.bool:
        if not mask.dtype.is_floating_point:
            raise ValueError(f"mask must be float or bool, got {mask.dtype}")
        lo, hi = float(mask.min()), float(mask.max())
        if not (lo >= 0.0 and hi <= 1.0):                              # (a NaN fails both)
            raise ValueError(f"mask values must lie in [0, 1], got [{lo}, {hi}]")
    return int(mask.shape[1])


def parse_operator(operator, shape, y=None, name=None):
    """``(kind, par, mask or None, the shape of A's image)`` of an operator on images of ``shape`` = (B, C, H, W); everything about it
    that can be refused without a device.  par: the mask's channel count / the down-sampling factor / 0.  With ``name``, ``y`` is
    held to the shape of A's image under that name."""
    if not isinstance(operator, (tuple, list)) or not operator or operator[0] not in OPERATORS:
        raise ValueError(f"operator must be ('mask', mask), ('down', f) or ('gray',), got {operator!r}")
    if len(shape) != 4 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 for v in shape):
        raise ValueError(f"shape must be (B, C, H, W) of positive integers, got {tuple(shape)!r}")
    B, C, H, W = (int(v) for v in shape)
    kind = operator[0]
    if len(operator) != (1 if kind == "gray" else 2):
        raise ValueError(f"operator {kind!r} takes {'no argument' if kind == 'gray' else 'one argument'}, got {len(operator) - 1}")
    if kind == "gray":
        par, mask, mshape = 0, None, (B, 1, H, W)
    elif kind == "down":
        f = operator[1]
        if isinstance(f, bool) or not isinstance(f, numbers.Integral) or f not in DOWN_FACTORS:
            raise ValueError(f"the down-sampling factor must be one of {DOWN_FACTORS}, got {f!r}")
        if H % f or W % f:
            raise ValueError(f"the down-sampling factor {f} must divide H = {H} and W = {W}")
        par, mask, mshape = int(f), None, (B, C, H // f, W // f)
    else:
        par, mask, mshape = mask_channels(operator[1], (B, C, H, W)), operator[1], (B, C, H, W)
    if name is not None and (not torch.is_tensor(y) or tuple(y.shape) != mshape):
        raise ValueError(f"{name} must have shape {mshape}, the image of shape {tuple(shape)} under {kind!r}, got "
                         f"{tuple(getattr(y, 'shape', ()))}")
    return kind, par, mask, mshape


def dps_measure(x, operator):
    """A x of an image batch ``x`` (B, C, H, W) with plain torch operations on ``x``'s device: M (.) x for ``("mask", mask)``, the mean
    over f x f blocks for ``("down", f)``, the channel mean (B, 1, H, W) for ``("gray",)``.  Not hot path: it makes the measurement a
    caller hands to ``p_sample_dps`` (adding the measurement noise is the caller's)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"x must be a (B, C, H, W) tensor, got shape {tuple(getattr(x, 'shape', ()))}")
    kind, par, mask, _ = parse_operator(operator, tuple(x.shape))
    if kind == "mask":
        return mask.to(device=x.device, dtype=x.dtype) * x
    if kind == "down":
        return F.avg_pool2d(x, par)
    return x.mean(dim=1, keepdim=True)


def ddnm_pinv(y, operator, shape):
    """A^+ y for a measurement batch ``y`` of images of ``shape`` = (B, C, H, W), with plain torch operations on ``y``'s device: y / M
    where M > 0 and 0 elsewhere for ``("mask", mask)``, every measurement element spread over its f x f block for ``("down", f)`` and
    over the C channels for ``("gray",)`` (both means: A^+ copies).  The companion of ``dps_measure``: A A^+ y = y on the range of A.
    Not hot path."""
    kind, par, mask, mshape = parse_operator(operator, tuple(shape), y, "y")
    if kind == "mask":
        m = mask.to(device=y.device, dtype=y.dtype).expand(mshape)
        return torch.where(m > 0, y / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(y))
    if kind == "down":
        return y.repeat_interleave(par, dim=2).repeat_interleave(par, dim=3)
    return y.expand(tuple(int(v) for v in shape)).clone()


def per_index(name, v, T, ok, rule, allow_none=False):
    """the ``name`` of every destination grid index 0 ... T-1 as python floats: ``v`` is a float for all of them or T floats (list, tuple,
    tensor of at most one dimension); None stays None where allowed.  ``ok(value)`` holds for each, or the refusal says ``rule``."""
    if v is None and allow_none:
        return None
    if isinstance(v, numbers.Real) and not isinstance(v, bool):
        vs = [float(v)] * T
    else:
        if torch.is_tensor(v):
            v = v.detach().reshape(-1).tolist() if v.dim() <= 1 else None
        if not isinstance(v, (list, tuple)) or len(v) != T or any(isinstance(z, bool) or not isinstance(z, numbers.Real) for z in v):
            raise ValueError(f"{name} must be {'None, ' if allow_none else ''}a float or {T} floats (one per destination grid index), got "
                             f"{len(v) if isinstance(v, (list, tuple)) else v!r}")
        vs = [float(z) for z in v]
    bad = [z for z in vs if not ok(z)]
    if bad:
        raise ValueError(f"{name} must {rule}, got {bad[0]!r}")
    return vs


def open_chain(gd, denoise_fn, image, mask, mask_c, shape, label, device, seed, dup=True):
    """``(ctx, draw, image, mask, chain)`` at the start of a restoration chain over images of ``shape``: the device context (the caller
    enters it again for its loop), ``draw()`` = one image-shaped normal tensor from the generator seeded with ``seed``, the measurement
    or known image fp32 contiguous on the device, the mask (or None) expanded to (B, mask_c, H, W) there, and the ``Chain`` on the
    FIRST draw.  ``dup=False`` leaves the chain's x_in to the caller."""
    device = torch.device(gd._default_device(denoise_fn) if device is None else device)
    ctx = _device_ctx(device)
    B, _, H, W = shape = tuple(int(v) for v in shape)
    with ctx, torch.no_grad():
        generator = None if seed is None else torch.Generator(device).manual_seed(seed)
        draw = lambda: torch.randn(shape, device=device, generator=generator)
        image = image.to(device=device, dtype=torch.float32).contiguous()
        m = None if mask is None else mask.to(device=device, dtype=torch.float32).expand(B, mask_c, H, W).contiguous()
        return ctx, draw, image, m, Chain(gd, denoise_fn, draw(), label, device, dup=dup)
