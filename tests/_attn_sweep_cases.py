"""Shared by tests/test_attn_sweep_host.py and tests/test_gpu_attention_sweep.py: the sweep over EVERY token count the attention
kernels take (csrc/attention.hip, attention_bwd.hip: N = 1 .. 640; csrc/attention_skip.hip: per-image lengths 1 .. 256) -- the
domains, seeded inputs, a float64 reference in plain torch ops and a restatement of the two dispatch functions that labels a length
with the instantiations it runs.  Nothing here needs a GPU; every function works on whatever device its tensors live on.

The existing attention tests pick about twenty lengths; inside each instantiation correctness depends on where N falls within a
16-key tile, a 32-key k-step, a query tile and a key block, so the sweep runs all of them."""
import collections
import math
import random

import torch

from _skip_attn_cases import expand_rows, weighted_attention_f64  # noqa: F401  (the varlen reference: ONE restatement, theirs)

B, H, HD = 3, 2, 64
SCALE = HD ** -0.5
DTYPES = (torch.float16, torch.bfloat16)
FULL_NS = range(1, 641)
CHUNKS = tuple(range(lo, lo + 64) for lo in range(1, 641, 64))       # ten consecutive chunks of 64 lengths
VARLEN_LENS = range(1, 257)
VARLEN_MAX = 256
VARLEN_BATCH = 64
RESIDUES_GUARDED = (0, 1, 7, 8, 15)           # N mod 16 at which the guard-band test must run in every bucket (it runs every N)

# NaN bit patterns with a payload no kernel produces: what poisons neighbours and pre-fills caller-owned output buffers
NAN16 = {torch.float16: 0x7DA5, torch.bfloat16: 0x7FA5}
NAN32 = 0x7FC0A5A5


def dtype_name(dt) -> str:
    return {torch.float16: "f16", torch.bfloat16: "bf16"}[dt]


def seed(N: int, dt) -> int:
    """one seed per (N, dtype): a failing case is named by it"""
    return 10 * N + DTYPES.index(dt)


def inputs(N: int, dt, batch: int = B, heads: int = H):
    """qkv [B, N, 3, H, 64] and dout [B, N, H*64] in ``dt`` on the CPU, drawn as tests/test_gpu_attention_long.py::_inputs and
    tests/test_gpu_dense.py::test_attention_backward_matches_float64_autograd draw them (so their bars apply unchanged)."""
    g = torch.Generator().manual_seed(seed(N, dt))
    qkv = (torch.randn(batch, N, 3, heads, HD, generator=g) * 1.2).to(dt)
    dout = (torch.randn(batch, N, heads * HD, generator=g) * 0.5).to(dt)
    return qkv, dout


def reference(qkv: torch.Tensor, dout: torch.Tensor, scale: float = SCALE) -> dict:
    """float64, on the dtype-rounded inputs, closed form: out [B, N, H*64] = softmax(q k^T scale) v, lse [B, H, N] in the log2 domain
    (as the kernels store it), dqkv [B, N, 3, H, 64] (dV = P^T dO; dS = P (dP - rowsum(dO O)); dQ = scale dS K; dK = scale dS^T Q)."""
    Bq, N, _, Hq, hd = qkv.shape
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4).unbind(0)                   # [B, H, N, hd]
    do = dout.double().reshape(Bq, N, Hq, hd).transpose(1, 2)                 # [B, H, N, hd]
    s = q @ k.transpose(-2, -1) * scale
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    den = e.sum(dim=-1, keepdim=True)
    p = e / den
    o = p @ v
    lse = (m + torch.log(den)).squeeze(-1) / math.log(2.0)
    dv = p.transpose(-2, -1) @ do
    ds = p * (do @ v.transpose(-2, -1) - (do * o).sum(dim=-1, keepdim=True))
    dq = ds @ k * scale
    dk = ds.transpose(-2, -1) @ q * scale
    dqkv = torch.stack((dq, dk, dv), dim=0).permute(1, 3, 0, 2, 4).contiguous()         # [B, N, 3, H, hd]
    return {"out": o.transpose(1, 2).reshape(Bq, N, Hq * hd), "lse": lse, "dqkv": dqkv}


def reference_autograd(qkv: torch.Tensor, dout: torch.Tensor, scale: float = SCALE) -> torch.Tensor:
    """dqkv by float64 autograd through torch.softmax: what the closed form above is checked against."""
    Bq, N, _, Hq, hd = qkv.shape
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.permute(2, 0, 3, 1, 4).unbind(0)
    (torch.softmax(q @ k.transpose(-2, -1) * scale, -1) @ v).transpose(1, 2).reshape(Bq, N, Hq * hd).backward(dout.double())
    return qr.grad


def varlen_reference(img: torch.Tensor, mult: int, scale: float = 0.125) -> torch.Tensor:
    """One compact image [len, 3, H, 64] -> float64 [len, H, 64]: the last key counts ``mult`` times when mult > 0."""
    return torch.stack([weighted_attention_f64(img[:, 0, h], img[:, 1, h], img[:, 2, h], scale, mult)
                        for h in range(img.shape[2])], dim=1)


# ---- the two dispatch functions, restated (labels for the error report only: no length is ever skipped by them) ----
Bucket = collections.namedtuple("Bucket", "fwd bwd")


def bucket(N: int, bwd_waves: int = 8) -> Bucket:
    """attention.hip::attn_dispatch and attention_bwd.hip::bwd_dispatch on nkt = ceil(N / 16)."""
    if not 1 <= N <= 640:
        raise ValueError(N)
    nkt = (N + 15) // 16
    if nkt in (4, 8, 13, 16):
        fwd = f"attn_fwd<{nkt},exact>"
    elif nkt < 16:
        fwd = f"attn_fwd<{next(t for t in (4, 8, 13, 16) if nkt < t)},masked>"
    else:
        fwd = f"attn_fwd_long<{next(t for t in (20, 30, 37, 40) if nkt <= t)}>"
    if nkt > 16:
        bwd = "attn_bwd_dq+dkv"
    elif nkt <= 4:
        bwd = "attn_bwd<4,4>"
    else:
        bwd = f"attn_bwd<{next(t for t in (8, 13, 16) if nkt <= t)},{bwd_waves}>"
    return Bucket(fwd, bwd)


def buckets(bwd_waves: int = 8) -> dict:
    """bucket -> the lengths that take it, over the whole domain, in order"""
    out = collections.OrderedDict()
    for N in FULL_NS:
        out.setdefault(bucket(N, bwd_waves), []).append(N)
    return out


# ---- varlen sweep: every length with mult in {0, 1, 256 - len}, mixed into batches of 64 images with unowned rows between them ----
def varlen_cases():
    """[(len, mult)]: 768 images in a fixed mixed order"""
    cases = [(L, m) for L in VARLEN_LENS for m in (0, 1, VARLEN_MAX - L)]
    random.Random(20).shuffle(cases)
    return cases


def varlen_batches():
    """[(lens, mults, row_start, rows)] per batch of 64 images: image i starts 1 + i % 3 unowned rows after its predecessor's end
    (and after row 0), and two unowned rows close the buffer."""
    cases, out = varlen_cases(), []
    for lo in range(0, len(cases), VARLEN_BATCH):
        lens, mults, rs, r = [], [], [], 0
        for i, (L, m) in enumerate(cases[lo:lo + VARLEN_BATCH]):
            r += 1 + i % 3
            rs.append(r)
            lens.append(L)
            mults.append(m)
            r += L
        out.append((lens, mults, rs, r + 2))
    return out


def varlen_inputs(batch_index: int, rows: int, dt, heads: int = H) -> torch.Tensor:
    """compact qkv [rows, 3, H, 64] in ``dt`` on the CPU, unit normal as tests/test_gpu_skip_attention.py::_varlen_cases draws it
    (VARLEN_BAR is stated for that), one seed per (batch, dtype)"""
    g = torch.Generator().manual_seed(1000 + 10 * batch_index + DTYPES.index(dt))
    return torch.randn(rows, 3, heads, HD, generator=g).to(dt)
