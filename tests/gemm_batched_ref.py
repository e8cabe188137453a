"""fp64 / fp32 references of the eight batched vd_gemm forms the UNet engine launches (v_diffusion/engine.py: _attn_fwd, _attn_bwd,
_film_fwd, _film_bwd), in plain torch on CPU tensors: the yardstick of tests/test_gemm_batched_gpu.py.

Every contraction is one ``einsum`` over LOGICAL tensors -- [B][nh][L][hd] heads, [B][nh][L][L] maps, [nb][...] FiLM stacks -- that are
generated in that shape.  The packed device layouts (the [B][L][3 nh hd] projection row, the [B][L][nh hd] output row, padded pitches, guard
rows) exist only in ``pack_heads`` / ``pack_rows`` and their inverses, which move data with explicit slices: no stride tuple of a launch is
used to compute an expected value.  ``unpack_heads_strided`` is the one strided view, checked against a reshape/permute formulation by
tests/test_gemm_batched_cpu.py.

Operands of batch entry z are scaled by 2^((z % 5) - 2) (exact in binary floating point): entries differ in magnitude, so an entry computed
from another entry's operands is off by a power of two, not by rounding."""
import torch

F64 = torch.float64
SENTINEL = 7.0
GUARD_ROWS = 256            # rows appended behind the last image / entry of every buffer
PAD = 4                     # floats added to every row pitch


def entry_scale(z):
    return 2.0 ** ((z % 5) - 2)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=F64).float()


def _scale_entries(x):
    """x: [n0][n1]... -> entry z = i0 * n1 + i1 scaled by entry_scale(z)"""
    n0, n1 = x.shape[:2]
    s = torch.tensor([entry_scale(z) for z in range(n0 * n1)], dtype=x.dtype).reshape(n0, n1, *([1] * (x.dim() - 2)))
    return x * s


# ------------------------------------------------------------------------------------------------ packed layouts
def pack_heads(x, pitch, col0, buf=None, rows_extra=GUARD_ROWS, fill=None):
    """x [B][nh][L][hd] -> columns col0 + h*hd ... of a [B*L + rows_extra][pitch] buffer (row b*L + l); a new buffer is filled with ``fill``
    (a float, or None for finite junk)"""
    B, nh, L, hd = x.shape
    if buf is None:
        buf = junk(B * L + rows_extra, pitch) if fill is None else torch.full((B * L + rows_extra, pitch), float(fill))
    for b in range(B):
        for h in range(nh):
            buf[b * L:(b + 1) * L, col0 + h * hd: col0 + (h + 1) * hd] = x[b, h]
    return buf


def unpack_heads(buf, B, nh, L, hd, col0):
    """inverse of pack_heads: [B][nh][L][hd], by slices"""
    out = torch.empty(B, nh, L, hd, dtype=buf.dtype)
    for b in range(B):
        for h in range(nh):
            out[b, h] = buf[b * L:(b + 1) * L, col0 + h * hd: col0 + (h + 1) * hd]
    return out


def unpack_heads_strided(buf, B, nh, L, hd, col0):
    """the same as ONE strided view of the buffer (no copy)"""
    pitch = buf.shape[1]
    return buf.as_strided((B, nh, L, hd), (L * pitch, hd, pitch, 1), buf.storage_offset() + col0)


def heads_mask(B, nh, L, hd, pitch, col0, entries=None, rows_extra=GUARD_ROWS):
    """bool [B*L + rows_extra][pitch]: the elements a launch over the first ``entries`` (default all) batch entries may write"""
    m = torch.zeros(B * L + rows_extra, pitch, dtype=torch.bool)
    n = B * nh if entries is None else entries
    for z in range(n):
        b, h = divmod(z, nh)
        m[b * L:(b + 1) * L, col0 + h * hd: col0 + (h + 1) * hd] = True
    return m


def pack_rows(x, pitch, buf=None, rows_extra=GUARD_ROWS, fill=None):
    """x [n0][n1][R][C] (or [n][R][C]) -> entry-major rows of a [n*R + rows_extra][pitch] buffer, columns 0 .. C-1"""
    x3 = x.reshape(-1, x.shape[-2], x.shape[-1])
    n, R, Cc = x3.shape
    if buf is None:
        buf = junk(n * R + rows_extra, pitch) if fill is None else torch.full((n * R + rows_extra, pitch), float(fill))
    for z in range(n):
        buf[z * R:(z + 1) * R, :Cc] = x3[z]
    return buf


def unpack_rows(buf, shape):
    """inverse of pack_rows: ``shape`` = the logical [..., R][C] shape"""
    R, Cc = shape[-2:]
    n = 1
    for s in shape[:-2]:
        n *= s
    out = torch.empty(n, R, Cc, dtype=buf.dtype)
    for z in range(n):
        out[z] = buf[z * R:(z + 1) * R, :Cc]
    return out.reshape(*shape)


def rows_mask(n, R, Cc, pitch, entries=None, rows_extra=GUARD_ROWS):
    m = torch.zeros(n * R + rows_extra, pitch, dtype=torch.bool)
    m[: (n if entries is None else entries) * R, :Cc] = True
    return m


def junk(rows, cols):
    """finite, deterministic filler of source padding: large enough that reading it would show"""
    i = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)
    return 50.0 + (i % 17.0)


# ------------------------------------------------------------------------------------------------ attention forms 1-6
ATTN_FORMS = {  # form: (einsum over logical tensors, A, B, destination kind)
    1: ("bnld,bnmd->bnlm", "q", "k", "map"),        # S  = Q K^T
    2: ("bnlm,bnmd->bnld", "P", "v", "o"),          # O  = P V
    3: ("bnlm,bnld->bnmd", "P", "dO", "dv"),        # dV = P^T dO
    4: ("bnld,bnmd->bnlm", "dO", "v", "map"),       # dP = dO V^T
    5: ("bnlm,bnmd->bnld", "dS", "k", "dq"),        # dQ = dS K
    6: ("bnlm,bnld->bnmd", "dS", "q", "dk"),        # dK = dS^T Q
}


def attn_operands(B, nh, L, hd, seed=0):
    """logical operands, entry-scaled: q, k, v, dO [B][nh][L][hd]; P, dS [B][nh][L][L]; c0_* = the random destinations of the accumulate runs"""
    g = torch.Generator().manual_seed(4242 + seed + 13 * B + 7 * nh + L + 3 * hd)
    d = {n: _scale_entries(_randn(g, B, nh, L, hd)) for n in ("q", "k", "v", "dO")}
    d.update({n: _scale_entries(_randn(g, B, nh, L, L)) for n in ("P", "dS")})
    d["c0_map"] = _randn(g, B, nh, L, L)
    d["c0_head"] = _randn(g, B, nh, L, hd)
    return d


def attn_products(d):
    """{form: (fp64 product, torch fp32 product)} without alpha / accumulation"""
    out = {}
    for f, (eq, a, b, _) in ATTN_FORMS.items():
        out[f] = (torch.einsum(eq, d[a].double(), d[b].double()), torch.einsum(eq, d[a], d[b]))
    return out


# ------------------------------------------------------------------------------------------------ FiLM forms 7, 8
def film_operands(nb, B, E, c2, seed=0):
    """ta [B][E] (shared by every entry); W [nb][c2][E], bias [nb][c2], dfilm [nb][B][c2], R [nb][B][c2] entry-scaled; c0_* random destinations"""
    g = torch.Generator().manual_seed(977 + seed + 11 * nb + 5 * B + E + 3 * c2)
    sc = lambda x: _scale_entries(x.unsqueeze(1)).squeeze(1)
    d = dict(ta=_randn(g, B, E), W=sc(_randn(g, nb, c2, E)), bias=sc(_randn(g, nb, c2)), df=sc(_randn(g, nb, B, c2)), R=sc(_randn(g, nb, B, c2)))
    d["c0_fwd"] = _randn(g, nb, B, c2)
    d["c0_bwd"] = _randn(g, nb, B, E)
    return d


def film_products(d):
    """{7: film[i] = ta W_i^T, 8: P[i] = dfilm[i] W_i} as (fp64, fp32), without bias / residual / alpha"""
    return {7: (torch.einsum("be,ice->ibc", d["ta"].double(), d["W"].double()), torch.einsum("be,ice->ibc", d["ta"], d["W"])),
            8: (torch.einsum("ibc,ice->ibe", d["df"].double(), d["W"].double()), torch.einsum("ibc,ice->ibe", d["df"], d["W"]))}


def compose(prod, alpha, bias=None, R=None, c0=None):
    """alpha * product (+ bias) (+ R) (+ c0) in the dtype of ``prod``: the expected destination of a launch"""
    out = prod * alpha
    for t in (bias, R, c0):
        if t is not None:
            out = out + t.to(prod.dtype)
    return out
