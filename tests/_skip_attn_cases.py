"""Shared by tests/test_skip_attention_host.py and tests/test_gpu_skip_attention.py: the case tables, a float64 restatement of the
weighted-key attention the skip-aware attention half rests on, and the host plan smoe_skip_plan is held to bit for bit.

The identity ("Skip-aware attention half"): with a hard gate a bypassed token's operand row is exactly zero, so its
q / k / v are the qkv bias.  Per image with n entering and m = N - n bypassed tokens, attention over the N keys equals attention over
the n entering keys plus ONE key whose probability counts m times, and the m bypassed queries all get one output row."""
import numpy as np
import torch

PATTERNS = ("none", "all", "first", "last", "alternating", "share0.1", "share0.5", "share0.9")
PLAN_B = (1, 3, 5)
PLAN_N = (1, 16, 17, 197, 256)
VARLEN_LENS = (1, 2, 15, 16, 17, 63, 64, 65, 197, 198, 208, 256)


def bypass_pattern(name: str, B: int, N: int, seed: int = 0) -> np.ndarray:
    """bool [B, N]: True = the token bypasses attention."""
    byp = np.zeros((B, N), dtype=bool)
    if name == "none":
        pass
    elif name == "all":
        byp[:] = True
    elif name == "first":
        byp[:, 0] = True
    elif name == "last":
        byp[:, N - 1] = True
    elif name == "alternating":
        byp[:, 1::2] = True
    elif name.startswith("share"):
        rng = np.random.default_rng(1000 * seed + 7 * B + N)
        byp = rng.random((B, N)) < float(name[5:])
    elif name == "all_next_to_none":          # an all-bypassed image beside a none-bypassed one (B >= 2)
        byp[0::2] = True
    else:
        raise ValueError(name)
    return byp


def mask_from_bypass(byp: np.ndarray) -> torch.Tensor:
    """The gate's mask as smoe_gate_ln_router writes it: f32 [B*N, 2], channel 0 = bypassed, channel 1 = entering, exactly 0 / 1."""
    b = torch.from_numpy(byp.reshape(-1).astype(np.float32))
    return torch.stack((b, 1.0 - b), dim=1).contiguous()


def host_plan(byp: np.ndarray) -> dict:
    """What smoe_skip_plan must write, vectorised numpy."""
    B, N = byp.shape
    T = B * N
    ent = ~byp
    n = ent.sum(axis=1).astype(np.int64)
    m = (N - n).astype(np.int32)
    length = (n + (m > 0)).astype(np.int32)
    row_start = (np.cumsum(length) - length).astype(np.int32)
    R = int(length.sum())
    gather = np.zeros(T, dtype=np.int64)
    row_map = np.full(T, T, dtype=np.int64)
    rep_row = np.where(byp, T + np.arange(B)[:, None], -1).astype(np.int32).reshape(-1)
    for b in range(B):
        toks = np.flatnonzero(ent[b]) + b * N
        s = int(row_start[b])
        gather[s:s + toks.size] = toks
        row_map[s:s + toks.size] = toks
        if m[b] > 0:
            gather[s + toks.size] = b * N + int(np.argmax(byp[b]))
            row_map[s + toks.size] = T + b
    return {"row_start": row_start, "len": length, "mult": m, "gather": gather, "row_map": row_map,
            "offsets": np.array([0, R], dtype=np.int32), "rep_row": rep_row}


def brute_plan(byp: np.ndarray) -> dict:
    """The same plan, one token at a time."""
    B, N = byp.shape
    T = B * N
    out = {"row_start": [], "len": [], "mult": [], "gather": [0] * T, "row_map": [T] * T, "rep_row": [-1] * T}
    r = 0
    for b in range(B):
        out["row_start"].append(r)
        first, m = None, 0
        for t in range(N):
            if byp[b, t]:
                m += 1
                first = t if first is None else first
                out["rep_row"][b * N + t] = T + b
            else:
                out["gather"][r] = b * N + t
                out["row_map"][r] = b * N + t
                r += 1
        if m:
            out["gather"][r] = b * N + first
            out["row_map"][r] = T + b
            r += 1
        out["len"].append(r - out["row_start"][-1])
        out["mult"].append(m)
    out["offsets"] = [0, r]
    return {k: np.asarray(v) for k, v in out.items()}


def attention_f64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
    """Plain softmax(q k^T scale) v, [n, hd] operands, float64."""
    s = (q.double() @ k.double().T) * scale
    return torch.softmax(s, dim=-1) @ v.double()


def weighted_attention_f64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, mult: int) -> torch.Tensor:
    """softmax(q k^T scale) v where the LAST key counts ``mult`` times (mult = 0: a plain key like every other)."""
    s = (q.double() @ k.double().T) * scale
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    if mult > 0:
        p[:, -1] = p[:, -1] * mult
    return (p / p.sum(dim=-1, keepdim=True)) @ v.double()


def expand_rows(n: int, m: int):
    """Row indices that turn a compact image (n entering rows, then the representative when m > 0) into its expanded form: the n
    entering rows followed by m copies of the representative."""
    return list(range(n)) + [n] * m


def varlen_batches():
    """(lens, mults, N) per batch: every len of VARLEN_LENS mixed within batches, mult in {0, 1, N - n}.  N is the token count the
    images expand to (len = n + (mult > 0), n + mult = N for the N - n cases; the other mults stand for what they say)."""
    a = [(1, 0), (2, 1), (15, 0), (16, 1), (17, 0), (63, 1), (64, 0), (65, 1)]                # lens <= 65: mult 0 / 1
    b = [(197, 0), (198, 1), (208, 0), (256, 1), (64, 0), (17, 1)]
    c = [(L, 256 - (L - 1)) for L in (1, 2, 15, 16, 17, 63, 64, 65, 197, 198, 208, 256)]      # mult = N - n with N = 256
    d = [(L, 197 - (L - 1)) for L in (1, 16, 65, 197)] + [(197, 0)]                            # ... and N = 197 (nkt 13)
    return [a, b, c, d]
