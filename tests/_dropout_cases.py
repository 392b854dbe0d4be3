"""THE mask rule of the counter-based dropout kernels (include/slimmoe.h, csrc/dropout.hip), restated in numpy, and the case table of
tests/test_dropout_host.py and tests/test_gpu_dropout.py.

Philox4x32-10 with the Random123 constants.  A call owns a key (k, c) (two 64-bit words).  Elements are numbered row-major over the
logical [rows, cols] tensor (cols % 8 == 0); element e lies in block b = first_block + e // 8 (mod 2^64); block b's Philox key is
(lo32 k, hi32 k), its counter (lo32 b, hi32 b, lo32 c, hi32 c); of the four output words r0..r3, element 8 b + 2 j + h draws
u = (r_j >> 16 h) & 0xffff and is kept iff u < thr16, thr16 = round((1 - p) * 65536) (ties to even).  Kept values are multiplied by
scale = f32(65536 / thr16) (0 when nothing is kept), then by row_scale[row] when given; a dropped element is SELECTED to +0.0;
dropout_add then adds the f32 residual.  f32 arithmetic, one rounding per operation, one round-to-nearest-even into the output dtype.
Nothing here imports the package under test."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF

# Random123 known-answer vectors (kat_vectors: philox4x32 10): (counter, key, result)
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (or scalars) of 32-bit words held in uint64; one round maps (c0, c1, c2, c3) to
    (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key then moves on by the Weyl increments."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    m32 = np.uint64(MASK32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def params(p: float):
    """(thr16, scale as np.float32) of a drop probability."""
    thr16 = int(np.rint((1.0 - float(p)) * 65536.0))
    thr16 = min(65536, max(0, thr16))
    return thr16, np.float32(65536.0 / thr16 if thr16 else 0.0)


def draws(key, n: int, first_block: int = 0) -> np.ndarray:
    """The 16-bit draws u of elements 0..n-1 (n % 8 == 0) under ``key`` = (k, c), ints of either sign."""
    assert n % 8 == 0
    k, c = int(key[0]) & MASK64, int(key[1]) & MASK64
    nb = n // 8
    b = (np.arange(nb, dtype=np.uint64) + np.uint64(int(first_block) & MASK64))     # wraps mod 2^64
    r = philox4x32_10(b & np.uint64(MASK32), b >> np.uint64(32), c & MASK32, c >> 32, k & MASK32, k >> 32)
    u = np.empty((nb, 8), dtype=np.uint32)
    for j in range(4):
        u[:, 2 * j] = (r[j] & np.uint64(0xffff)).astype(np.uint32)
        u[:, 2 * j + 1] = ((r[j] >> np.uint64(16)) & np.uint64(0xffff)).astype(np.uint32)
    return u.reshape(-1)


def mask(key, n: int, p: float, first_block: int = 0) -> np.ndarray:
    """bool [n]: element kept."""
    return draws(key, n, first_block) < np.uint32(params(p)[0])


def key_of(t: torch.Tensor):
    """(k, c) of a key tensor int64 [2]."""
    k, c = t.detach().cpu().tolist()
    return k, c


def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().float().contiguous().view(-1).numpy()      # 16-bit -> f32 is exact


def _term(x: torch.Tensor, key, p, row_scale, first_block):
    cols = x.shape[-1]
    v = _f32(x)
    thr16, scale = params(p)
    with np.errstate(all="ignore"):
        t = v * scale                                                    # f32 * f32, rounded once
        if row_scale is not None:
            t = (t.reshape(-1, cols) * _f32(row_scale).reshape(-1, 1)).reshape(-1)
    return np.where(mask(key, v.size, p, first_block), t, np.float32(0.0)).astype(np.float32)


def dropout(x: torch.Tensor, key, p: float, out_dtype=None, row_scale=None, first_block: int = 0) -> torch.Tensor:
    """The kernel's result for ``x`` (any of f32 / f16 / bf16, CPU or GPU) as a CPU tensor of ``out_dtype``."""
    t = _term(x, key, p, row_scale, first_block)
    return torch.from_numpy(t).reshape(x.shape).to(out_dtype or x.dtype)  # torch's cast: round to nearest even


def dropout_add(h: torch.Tensor, residual: torch.Tensor, key, p: float, row_scale=None) -> torch.Tensor:
    t = _term(h, key, p, row_scale, 0)
    with np.errstate(all="ignore"):
        return torch.from_numpy(_f32(residual) + t).reshape(h.shape)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit equality, a NaN matching any NaN (the payload a conversion leaves in a NaN is not part of the rule)."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    eq = (got.view(it) == want.view(it)) | (torch.isnan(got) & torch.isnan(want))
    return bool(eq.all())


# ---- the case table ---------------------------------------------------------------------------------------------------------------
GRID_CAP = 4096                       # workgroups (csrc/dropout.hip DROP_MAX_BLOCKS), 256 lanes x 8 elements each per trip
SHAPES = [(1, 8), (1, 2040), (1, 2048), (1, 2056), (3, 192), (7, 768), (257, 3072), (1000, 1024)]
CAP_BLOCKS = [GRID_CAP * 256 - 1, GRID_CAP * 256 + 1, 2 * GRID_CAP * 256 + 3]     # 8-element units: below, past, past twice the cap
PS = [0.1, 0.5, 1.0]
FIRST_BLOCKS = [0, 2 ** 32 - 3]       # the second: the counter's high word changes inside a small tensor
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
PAIRS = [(a, b) for a in DTYPES for b in DTYPES]
STAT_KEYS = [(1, 2), (-1, 2 ** 40 + 7), (0, 0)]
STAT_PS = [0.1, 0.5, 0.9]
PARAM_CASES = [(0.0, 65536, 1.0), (0.05, 62259, 65536.0 / 62259), (0.1, 58982, 65536.0 / 58982), (0.5, 32768, 2.0),
               (1.0 - 2.0 ** -17, 0, 0.0), (1.0, 0, 0.0)]
