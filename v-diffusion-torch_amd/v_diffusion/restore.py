"""What the restoration samplers share -- ``p_sample_inpaint`` (RePaint), ``p_sample_dps`` and ``p_sample_ddnm``: the mask rule, the
measurement operator A of the latter two (its parser, A itself, its pseudo-inverse), the parser of a per-grid-index parameter, and the
opening of a chain: device, seeded draws, the given image and the mask on the device, the ``Chain``."""
import numbers

import torch
import torch.nn.functional as F

from .chain import Chain
from .diffusion import _device_ctx

OPERATORS = ("mask", "down", "gray", "blur")
DOWN_FACTORS = (2, 4, 8)
BLUR_KMAX = 33                 # the most taps per side of a blur kernel (VDX_BLUR_KMAX of include/vdiff_blur.h)
NO_PINV = "the pseudo-inverse A^+ of a blur is not a per-thread preimage (it is an FFT or an SVD): DDNM does not take ('blur', kernel)"


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
    that can be refused without a device.  par: the mask's channel count / the down-sampling factor / 0 / 0 (the kernel of a blur is
    ``operator[1]``, held to ``blur_kernel``'s rule here).  With ``name``, ``y`` is held to the shape of A's image under that name."""
    if not isinstance(operator, (tuple, list)) or not operator or operator[0] not in OPERATORS:
        raise ValueError(f"operator must be ('mask', mask), ('down', f), ('gray',) or ('blur', kernel), got {operator!r}")
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
    elif kind == "blur":
        blur_kernel(operator[1], H, W)
        par, mask, mshape = 0, None, (B, C, H, W)
    else:
        par, mask, mshape = mask_channels(operator[1], (B, C, H, W)), operator[1], (B, C, H, W)
    if name is not None and (not torch.is_tensor(y) or tuple(y.shape) != mshape):
        raise ValueError(f"{name} must have shape {mshape}, the image of shape {tuple(shape)} under {kind!r}, got "
                         f"{tuple(getattr(y, 'shape', ()))}")
    return kind, par, mask, mshape


def blur_kernel(kernel, H, W):
    """the rule of the kernel of ``("blur", kernel)`` on H x W images: a 2-D floating tensor (Kh, Kw), both sides odd and at most
    ``BLUR_KMAX``, every tap finite, the radii (Kh-1)/2 <= H-1 and (Kw-1)/2 <= W-1 (the reflect boundary needs them inside the image).
    Returns (Kh, Kw)."""
    if not torch.is_tensor(kernel) or kernel.dim() != 2 or not kernel.dtype.is_floating_point:
        raise ValueError(f"the kernel of the 'blur' operator must be a 2-D floating tensor (Kh, Kw), got "
                         f"{tuple(kernel.shape) if torch.is_tensor(kernel) else kernel!r}"
                         f"{' of ' + str(kernel.dtype) if torch.is_tensor(kernel) else ''}")
    kh, kw = (int(v) for v in kernel.shape)
    if kh % 2 != 1 or kw % 2 != 1 or kh > BLUR_KMAX or kw > BLUR_KMAX:
        raise ValueError(f"the kernel of the 'blur' operator has odd sides of at most {BLUR_KMAX} taps, got {kh} x {kw}")
    if not bool(torch.isfinite(kernel).all()):
        raise ValueError("the kernel of the 'blur' operator has a tap that is not finite")
    if kh // 2 > H - 1 or kw // 2 > W - 1:
        raise ValueError(f"the radii {kh // 2}, {kw // 2} of the 'blur' operator's kernel do not fit a {H} x {W} image (at most H - 1, W - 1)")
    return kh, kw


def gaussian_kernel(size, std):
    """the (size, size) fp32 Gaussian blur kernel of the DPS experiments: taps exp(-d^2 / (2 std^2)) at the distances d from the centre in
    fp64, their outer product, divided by its fp64 sum, rounded to fp32 once.  ``size`` odd, 1 ... ``BLUR_KMAX``; ``std`` finite, > 0."""
    if isinstance(size, bool) or not isinstance(size, numbers.Integral) or size < 1 or size > BLUR_KMAX or size % 2 != 1:
        raise ValueError(f"size must be an odd integer in 1 ... {BLUR_KMAX}, got {size!r}")
    if isinstance(std, bool) or not isinstance(std, numbers.Real) or not (std > 0.0 and std < float("inf")):
        raise ValueError(f"std must be finite and > 0, got {std!r}")
    d = torch.arange(int(size), dtype=torch.float64) - (int(size) - 1) / 2
    g = torch.exp(-(d * d) / (2.0 * float(std) ** 2))
    k = torch.outer(g, g)
    return (k / k.sum()).to(torch.float32)


def dps_measure(x, operator):
    """A x of an image batch ``x`` (B, C, H, W) with plain torch operations on ``x``'s device: M (.) x for ``("mask", mask)``, the mean
    over f x f blocks for ``("down", f)``, the channel mean (B, 1, H, W) for ``("gray",)``, the depthwise cross-correlation with the
    kernel after reflect padding for ``("blur", kernel)``.  Not hot path: it makes the measurement a caller hands to ``p_sample_dps``
    (adding the measurement noise is the caller's)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"x must be a (B, C, H, W) tensor, got shape {tuple(getattr(x, 'shape', ()))}")
    kind, par, mask, _ = parse_operator(operator, tuple(x.shape))
    if kind == "mask":
        return mask.to(device=x.device, dtype=x.dtype) * x
    if kind == "down":
        return F.avg_pool2d(x, par)
    if kind == "blur":
        k = operator[1].to(device=x.device, dtype=x.dtype)
        C, (kh, kw) = x.shape[1], k.shape
        return F.conv2d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2), mode="reflect"), k.expand(C, 1, kh, kw), groups=C)
    return x.mean(dim=1, keepdim=True)


def ddnm_pinv(y, operator, shape):
    """A^+ y for a measurement batch ``y`` of images of ``shape`` = (B, C, H, W), with plain torch operations on ``y``'s device: y / M
    where M > 0 and 0 elsewhere for ``("mask", mask)``, every measurement element spread over its f x f block for ``("down", f)`` and
    over the C channels for ``("gray",)`` (both means: A^+ copies).  The companion of ``dps_measure``: A A^+ y = y on the range of A.
    Not hot path."""
    kind, par, mask, mshape = parse_operator(operator, tuple(shape), y, "y")
    if kind == "blur":
        raise NotImplementedError(f"ddnm_pinv: {NO_PINV}")
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
