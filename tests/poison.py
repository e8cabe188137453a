"""Poison for memory a kernel must not read (tests/test_poisoned_memory_gpu.py, tests/test_poisoned_step_gpu.py; DESIGN.md, "Memory a
kernel may not read").  0 x 3.0 is 0, 0 x NaN is not: a masked K tail that is read and multiplied by zero, a split-K slab that is summed
without having been written, a pitch column that reaches a sum -- each passes on finite leftovers and shows on NaN.  No GPU code here;
the device-independent helpers are checked by tests/test_poison_cpu.py."""
import torch

NAN = float("nan")
SENTINEL = -777.0            # finite value for the pitch columns of DESTINATIONS: a kernel that writes them changes it, one that reads them gets no NaN
# workspace tags of v_diffusion._hip.workspace whose contents are floats written and consumed inside ONE call (read from the host code of
# every entry that takes them: nothing in them is meant to survive a call).  The metric scratch (knn, knn_hits, kid, is) is not audited.
FLOAT_TAGS = ("splitk", "planes", "planes_v", "wgrad43", "dgrad_planes", "wgrad", "gn", "colsum", "sumsq")


def pitched(x_nchw, ld, pad=NAN, device="cuda"):
    """NCHW tensor -> NHWC tensor on `device` with pixel pitch ld; columns [C, ld) hold `pad` (NaN: the poisoned twin of the nhwc() helpers)"""
    n, c, h, w = x_nchw.shape
    assert ld >= c
    out = torch.full((n, h, w, ld), pad, dtype=x_nchw.dtype)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return out.to(device)


def pitched_rows(x, ld, pad=NAN, device="cuda"):
    """[rows][cols] matrix -> [rows][ld] on `device`, columns [cols, ld) hold `pad`"""
    rows, cols = x.shape
    assert ld >= cols
    out = torch.full((rows, ld), pad, dtype=x.dtype)
    out[:, :cols] = x
    return out.to(device)


def poison_workspaces(H, tags, value=NAN):
    """Fill every cached scratch buffer of H._ws_cache (keys (device, stream, tag)) whose tag is in `tags` with `value` -- the WHOLE buffer,
    on every stream, after a device synchronisation -- and return the set of tags found.  The caller asserts that the tag of the entry
    under test is among them, so a case cannot pass without having poisoned anything."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    found = set()
    for key, buf in H._ws_cache.items():
        if key[2] in tags:
            buf.fill_(value)
            found.add(key[2])
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return found


def same_bits(a, b):
    """bitwise equality of two fp32 tensors (compared as int32: NaN equals the same NaN, -0.0 differs from 0.0)"""
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        return False
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _free_blocks(device):
    """[(bytes, in the small pool?, stream handle)] of the allocator's free blocks on `device`, largest first"""
    index = torch.device(device).index
    index = torch.cuda.current_device() if index is None else index
    out = [(b["size"], seg["segment_type"] == "small", int(seg.get("stream", 0) or 0)) for seg in torch.cuda.memory_snapshot()
           if seg["device"] == index for b in seg["blocks"] if b["state"] == "inactive"]
    return sorted(out, reverse=True)


def _fill_holes(device, rounds=8):
    """NaN tensors of exactly the sizes of the allocator's free blocks, largest first (best fit then serves each from a block of its own
    size): the free pieces inside segments that live tensors keep from being released.  A block is reused only on the stream it was
    allocated on (a scratch buffer that grew on the engine's side stream leaves one behind), so each is requested under that stream; a
    piece of the small pool above 1 MiB is taken in parts (a request above 1 MiB would go to the large pool).  Returns (the tensors, the
    free blocks left)."""
    held = []
    for _ in range(rounds):
        free = _free_blocks(device)
        if not free:
            break
        for nb, small, handle in free:
            floats = min(nb, 1 << 20) // 4 if small else nb // 4
            if handle:
                with torch.cuda.stream(torch.cuda.ExternalStream(handle, device=device)):
                    held.append(torch.full((floats,), NAN, device=device))
            else:
                held.append(torch.full((floats,), NAN, device=device))
    return held, _free_blocks(device)


def poison_allocator(nbytes, device="cuda", small_blocks=300, probe_floats=(1 << 16, 1 << 19)):
    """Leave the caching allocator holding nothing but NaN: empty its cache; fill the free pieces that remain inside segments with live
    tensors (the parameters share theirs with the first run's temporaries); allocate NaN-filled tensors adding up to `nbytes` (what the
    first run peaked at) -- one large block of whole 2 MiB pieces plus `small_blocks` blocks between 512 B and 1 MiB for the small pool --
    and fill what they left free of their segments; free everything.  The engine's next torch.empty is then served NaN.  Returns "" when it
    took -- no free block was left unfilled, and fresh torch.empty tensors of `probe_floats` floats (a typical activation, a large one) are
    all NaN -- else what went wrong."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held, _ = _fill_holes(device)
    g = torch.Generator().manual_seed(0)
    sizes = [128 * int(s) for s in torch.randint(1, 2049, (small_blocks,), generator=g)]       # floats: 512 B ... 1 MiB in whole 512-byte granules
    held += [torch.full((s,), NAN, device=device) for s in sizes]
    big = max(int(nbytes) - 4 * sum(sizes), 16 << 20)            # >= 10 MiB: a segment of its own, rounded up to whole 2 MiB pieces
    held.append(torch.full(((big + (2 << 20) - 1) // (2 << 20) * (2 << 20) // 4,), NAN, device=device))
    more, left = _fill_holes(device)
    torch.cuda.synchronize()
    del held, more
    if left:
        return f"{len(left)} free blocks could not be filled (bytes, small pool, stream): {left[:8]}"
    for n in probe_floats:
        probe = torch.empty(n, device=device)
        nans = int(torch.isnan(probe).sum())
        del probe
        if nans != n:
            return f"a fresh torch.empty of {n} floats holds {n - nans} values that are not NaN"
    return ""
