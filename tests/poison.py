"""Poison for memory a kernel must not read, guard bands for memory it must not write (tests/test_poisoned_memory_gpu.py,
tests/test_memory_bounds_gpu.py, tests/test_poisoned_step_gpu.py; DESIGN.md, "Memory a kernel may not read").  0 x 3.0 is 0, 0 x NaN is
not: a masked K tail that is read and multiplied by zero, a split-K slab that is summed without having been written, a pitch column that
reaches a sum -- each passes on finite leftovers and shows on NaN.  A store one row, one tile or one image past a tensor lands in whatever
the allocator put there and shows nowhere: Banded puts memory the test owns on both sides of every tensor, ExactWorkspace hands the
wrappers scratch of exactly the size they asked for.  No GPU code here; the device-independent helpers are checked by
tests/test_poison_cpu.py."""
import contextlib

import torch

NAN = float("nan")
SENTINEL = -777.0            # finite value for the pitch columns of DESTINATIONS: a kernel that writes them changes it, one that reads them gets no NaN
# workspace tags of v_diffusion._hip.workspace whose contents are floats written and consumed inside ONE call (read from the host code of
# every entry that takes them: nothing in them is meant to survive a call).  The metric scratch (knn, knn_hits, kid, is) is not audited.
FLOAT_TAGS = ("splitk", "planes", "planes_v", "wgrad43", "dgrad_planes", "wgrad", "gn", "colsum", "sumsq")


# ------------------------------------------------------------------------------------------------ guard bands
# A banded tensor is a view into the middle of one larger allocation: a band before it, a band behind it, both owned by the test.  The
# band is a CONDITION on what the test can observe, not a measurement: it holds a whole image of the tensor and 256 of its rows, so a
# kernel that runs one row, one tile (the largest row tile is 256) or one image past either end lands in the band and changes it.
BAND_ROWS = 256
BAND_FLOOR = 1 << 16          # elements; flat tensors have neither rows nor images
BAND_BYTES = 512              # bands are whole multiples of this (128 floats): the real part keeps the allocator's 512-byte alignment, so
#                               the kernel form an entry picks from the alignment of its operands is the one it picks for a plain tensor
WS_BAND_BYTES = 1 << 20       # bands of an exact-size scratch buffer: the floor of _hip.workspace, i.e. what a small request owns today

_ledger = []                  # every Banded made since the last forget_bands(): twice() and the bounds tests check and clear it
_shift = [0]                  # elements every new Banded is moved off its 512-byte line unless it says otherwise: shifted()


@contextlib.contextmanager
def shifted(elems):
    """every Banded made inside (pitched(), pitched_rows(), on_device(), banded(), ...) starts `elems` elements behind a 512-byte line: 4
    floats give the 16-byte-aligned bases of channel slices of a wider buffer.  Scratch buffers stay where they are."""
    _shift.append(int(elems))
    try:
        yield
    finally:
        _shift.pop()


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def band_elems(real_shape, itemsize=4, floor=BAND_FLOOR):
    """elements of ONE band of a tensor of `real_shape` (last axis = the pitch; axes 1.. = one image): at least an image, BAND_ROWS rows
    and `floor` elements, rounded up to whole BAND_BYTES"""
    shape = tuple(int(s) for s in real_shape)
    pitch = shape[-1] if shape else 1
    image = _numel(shape[1:]) if len(shape) >= 2 else 0
    need = max(image, BAND_ROWS * pitch if len(shape) >= 2 else 0, int(floor), 1)
    gran = BAND_BYTES // itemsize
    return -(-need // gran) * gran


class Banded:
    """`real` (shape `real_shape`, filled with `fill` unless that is None) between two bands of `band_fill`.  shift: elements by which the
    real part is moved off its 512-byte line (the front band grows by them, the back band keeps its size; None: what shifted() set)."""
    made = 0

    def __init__(self, real_shape, fill, band_fill, dtype=torch.float32, device="cuda", shift=None, floor=BAND_FLOOR, check=True):
        real_shape = tuple(int(s) for s in real_shape)
        item = torch.empty((), dtype=dtype).element_size()
        shift = _shift[-1] if shift is None else int(shift)
        self.band, self.shift, self.band_fill, self.check = band_elems(real_shape, item, floor), shift, band_fill, check
        n = _numel(real_shape)
        self.lo = self.band + self.shift
        self.whole = torch.full((self.lo + n + self.band,), band_fill, dtype=dtype, device=device)
        Banded.made += 1
        self.serial = Banded.made                               # position in the order of creation (survives forget_bands())
        self.real = self.whole[self.lo:self.lo + n].view(real_shape)
        if fill is not None:
            self.real.fill_(fill)
        _ledger.append(self)

    def bands(self):
        return self.whole[:self.lo], self.whole[self.lo + self.real.numel():]

    def damage(self):
        """"" when both bands still hold band_fill, else where they do not"""
        out = []
        for name, b in zip(("front", "back"), self.bands()):
            bad = ~torch.isnan(b) if isinstance(self.band_fill, float) and self.band_fill != self.band_fill else b != self.band_fill
            k = int(bad.sum())
            if k:
                idx = bad.nonzero().flatten()
                first, last = int(idx[0]), int(idx[-1])
                where = (f"{len(b) - last} .. {len(b) - first} elements before the tensor" if name == "front"
                         else f"{first} .. {last + 1} elements behind its end")
                out.append(f"{k} elements of the {name} band changed, {where}")
        return "; ".join(out)

    def intact(self):
        return not self.damage()


def banded(real_shape, fill, band_fill=SENTINEL, **kw):
    """the real part of a new Banded (its record is kept in the ledger: bands_damage())"""
    return Banded(real_shape, fill, band_fill, **kw).real


def banded_like(x, band_fill, device="cuda", shift=None, check=False):
    """a banded copy on `device` of the CPU tensor x (built on the host, one transfer); sources: the bands hold the run's pad value"""
    x = x.contiguous()
    b = Banded(x.shape, None, band_fill, dtype=x.dtype, device="cpu", shift=shift, check=check)
    b.real.copy_(x)
    if torch.device(device).type != "cpu":
        b.whole = b.whole.to(device)
        b.real = b.whole[b.lo:b.lo + x.numel()].view(x.shape)
    return b.real


def on_device(x, device="cuda"):
    """a small source (bias, weights, labels) on `device` between NaN bands (bands of the largest value for integer types)"""
    return banded_like(x, NAN if x.dtype.is_floating_point else torch.iinfo(x.dtype).max, device)


def bands_damage(clear=True):
    """damage of every checked Banded in the ledger as one string ("" = all intact); the ledger is emptied unless clear is False"""
    out = [f"{tuple(b.real.shape)}: {d}" for b in _ledger if b.check for d in (b.damage(),) if d]
    if clear:
        _ledger.clear()
    return " | ".join(out)


def forget_bands():
    _ledger.clear()


def pitched(x_nchw, ld, pad=NAN, device="cuda", shift=None):
    """NCHW tensor -> banded NHWC tensor on `device` with pixel pitch ld; columns [C, ld) AND both bands hold `pad` (NaN: the poisoned twin
    of the nhwc() helpers): the halo rows above the first image and below the last are the run's pad value"""
    n, c, h, w = x_nchw.shape
    assert ld >= c
    out = torch.full((n, h, w, ld), pad, dtype=x_nchw.dtype)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return banded_like(out, pad, device, shift)


def pitched_rows(x, ld, pad=NAN, device="cuda", shift=None):
    """[rows][cols] matrix -> banded [rows][ld] on `device`, columns [cols, ld) and both bands hold `pad`"""
    rows, cols = x.shape
    assert ld >= cols
    out = torch.full((rows, ld), pad, dtype=x.dtype)
    out[:, :cols] = x
    return banded_like(out, pad, device, shift)


class ExactWorkspace:
    """Stand-in for v_diffusion._hip.workspace (install with monkeypatch.setattr(_hip, "workspace", ...): the wrappers look the name up
    on every call).  Same (device, stream, tag) keying; the buffer handed out is EXACTLY nbytes rounded up to 16, NaN-filled on every
    request, between two SENTINEL bands of at least 1 MiB (the floor of the real workspace: at the shapes of the tests that range is
    owned by the scratch today).  requests: [(tag, nbytes)] in order.  Every buffer ever handed out stays alive and checked.
    force: {tag: bytes} -- requests of that tag get exactly that many bytes (a multiple of 4) whatever they ask for: the boundary of an
    entry's own check, and one float below it; only: {tag: k} -- no more than the k-th request of the tag (from 0) is forced."""

    def __init__(self, stream_of=None, force=None, only=None):
        self.requests, self.cache, self.all, self.force, self.only = [], {}, [], dict(force or {}), dict(only or {})
        self.stream_of = stream_of or (lambda device: torch.cuda.current_stream(device).cuda_stream)

    def __call__(self, nbytes, device, tag="default"):
        nth = sum(1 for t, _ in self.requests if t == tag)
        forced = tag in self.force and self.only.get(tag, nth) == nth
        floats = self.force[tag] // 4 if forced else (int(nbytes) + 15) // 16 * 4
        self.requests.append((tag, int(nbytes)))
        key = (device, self.stream_of(device), tag)
        b = self.cache.get(key)
        if b is None or b.real.numel() != floats:
            b = Banded((floats,), None, SENTINEL, device=device, shift=0, floor=WS_BAND_BYTES // 4, check=False)
            _ledger.remove(b)
            self.cache[key] = b
            self.all.append(b)
        b.real.fill_(NAN)
        return b.real

    def tags(self):
        return {t for t, _ in self.requests}

    def damage(self):
        return " | ".join(f"scratch of {4 * b.real.numel()} bytes: {d}" for b in self.all for d in (b.damage(),) if d)

    def intact(self):
        return not self.damage()


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
