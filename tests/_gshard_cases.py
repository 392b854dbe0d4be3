"""The GShard gate's rule ("GShardGate") as a plain CPU restatement in float64, and the case table the host and
the GPU tests share.

Entry counts of the kernels under test (csrc/gshard.hip) -- the sizes at which they change path:

    kernel                  per wave        per workgroup
    gshard_count / _rank    256 entries     1024 entries   (128 / 512 tokens: T = 127, 128, 129 and 511, 512, 513 straddle them)
    gshard_aux_partial      --              256 rows       (T = 511, 512, 513 and 1500: 2, 2, 3 and 6 chunks, the last one ragged)
    gshard_gate_bwd         64 rows         256 rows       (one thread per row: no row crosses a boundary)

Regimes of the table (seed 7; test_gshard_host.py asserts them):
  * T >= 127: every cell in which the capacity can bind at all -- rate 0.5; or an expert-0 offset of 2 with (rate 1.2, E >= 8) or
    (rate 4.0, E = 32) -- has entries dropped by the capacity, more than 75 entries kept, and, with ``u``, entries dropped by random
    routing.  (E = 2 routes every token to both experts, T entries each, and cap = ceil(rate T) >= T from rate 1 on; E = 8 at rate
    4.0 has cap = T: there no capacity drop exists, whatever the logits are.)
  * T in {1, 2} with E >= 8 and rate <= 1.2: cap = 0, everything is dropped.
"""
import itertools
import math

import torch

TS = (1, 2, 127, 128, 129, 511, 512, 513, 1500)
ES = (2, 8, 32)
RATES = (0.5, 1.2, 4.0)
OFFSETS = (0.0, 2.0)
SEED = 7


def capacity(rate: float, T: int, E: int) -> int:
    """rule 3: cap = (ceil(rate * T) * 2) // E"""
    return (int(math.ceil(rate * T)) * 2) // E


class Case:
    def __init__(self, T, E, rate, offset, with_u):
        self.T, self.E, self.rate, self.offset, self.with_u = T, E, rate, offset, with_u
        self.cap = capacity(rate, T, E)
        g = torch.Generator().manual_seed(SEED + 1000003 * T + 7919 * E + int(10 * rate) * 101 + int(offset) * 13)
        self.logits = torch.randn(T, E, generator=g)
        self.logits[:, 0] += offset
        u = torch.rand(T, generator=g)
        self.u = u if with_u else None
        self.dscore = torch.randn(T, 2, generator=g)
        # the router's outputs, as the NAIVE top-2 router emits them (f32 logits; random: no ties)
        val, self.idx = torch.topk(self.logits, 2, dim=1)
        self.score = torch.softmax(val, dim=-1)

    @property
    def id(self):
        return f"T{self.T}-E{self.E}-r{self.rate}-o{int(self.offset)}-{'u' if self.with_u else 'nou'}"


def table(Ts=TS):
    return [Case(T, E, r, o, w) for T, E, r, o, w in itertools.product(Ts, ES, RATES, OFFSETS, (True, False))]


# ---- rules 3 + 4 ------------------------------------------------------------------------------------------------------------------
def prune(idx, score, u, E, cap):
    """(idx_out i64 [T, 2], top1_counts i64 [E], dropped-by-capacity mask [T, 2], dropped-by-random mask [T, 2]), vectorised: the
    capacity rank of a flat entry = how many earlier flat entries named its expert (a one-hot cumulative sum)."""
    T = idx.shape[0]
    flat = idx.reshape(-1)
    valid = (flat >= 0) & (flat < E)
    safe = torch.where(valid, flat, torch.zeros_like(flat))
    onehot = torch.nn.functional.one_hot(safe, E) * valid.unsqueeze(1)
    rank = (onehot.cumsum(0) - onehot).gather(1, safe.unsqueeze(1)).squeeze(1)
    by_cap = valid & (rank >= cap) if cap >= 0 else torch.zeros_like(valid)
    by_rand = torch.zeros_like(valid)
    if u is not None:
        # the compare is in f32 and exact: 2 * score is a power-of-two scaling
        second = (2.0 * score[:, 1].float()) < u.float()
        by_rand = torch.stack([torch.zeros_like(second), second], 1).reshape(-1) & valid & ~by_cap
    keep = valid & ~by_cap & ~by_rand
    out = torch.where(keep, flat, torch.full_like(flat, -1)).reshape(T, 2)
    first = idx[:, 0]
    ok = (first >= 0) & (first < E)
    top1 = torch.bincount(first[ok], minlength=E)[:E]
    return out, top1, by_cap.reshape(T, 2), by_rand.reshape(T, 2)


def prune_walk(idx, score, u, E, cap):
    """rules 3 + 4 entry by entry, as the issue words them."""
    T = idx.shape[0]
    seen = [0] * E
    out = [[-1, -1] for _ in range(T)]
    top1 = [0] * E
    for t in range(T):
        for j in range(2):
            e = int(idx[t, j])
            if not 0 <= e < E:
                continue
            if j == 0:
                top1[e] += 1
            keep = cap < 0 or seen[e] < cap
            seen[e] += 1                      # an entry uses its slot whether random routing drops it afterwards or not
            if keep and j == 1 and u is not None and bool(torch.tensor(2.0, dtype=torch.float32) * score[t, 1].float() < u[t].float()):
                keep = False
            if keep:
                out[t][j] = e
    return torch.tensor(out, dtype=torch.int64).reshape(T, 2), torch.tensor(top1, dtype=torch.int64)


# ---- rule 2 and the backward formulas, float64 ------------------------------------------------------------------------------------
def aux64(logits, top1, num_expert):
    """(aux, coef [E]) in float64; coef[e] = d aux / d softmax(logits)[t, e] = num_expert^2 top1[e] / (E T^2)."""
    T, E = logits.shape
    p = torch.softmax(logits.double(), dim=1)
    c = top1.double() / max(T, 1)
    aux = (c * p.mean(0)).mean() * num_expert ** 2 if T > 0 else torch.zeros((), dtype=torch.float64)
    return aux, num_expert ** 2 * top1.double() / (E * max(T, 1) ** 2)


def gate_bwd64(logits, idx, idx_out, score, dscore, coef, coef_scale=1.0):
    """dlogits [T, E] in float64 by the formulas of smoe_gshard_gate_bwd."""
    l = logits.double()
    T, E = l.shape
    dl = torch.zeros_like(l)
    if coef is not None:
        p = torch.softmax(l, dim=1)
        c = coef.double().unsqueeze(0)
        dl = coef_scale * p * (c - (p * c).sum(1, keepdim=True))
    if dscore is not None:
        s = score.double()
        ds = dscore.double() * (idx_out >= 0)
        inner = (s * ds).sum(1, keepdim=True)
        dl = dl.scatter_add(1, idx, s * (ds - inner))
    return dl


def objective64(logits, idx, idx_out, top1, num_expert, w_score, w_aux):
    """sum(score * w_score over the kept entries) + w_aux * aux as a differentiable float64 function of ``logits`` (autograd checks
    gate_bwd64)."""
    l = logits.double()
    score = torch.softmax(l.gather(1, idx), dim=-1)
    T, E = l.shape
    m = torch.softmax(l, dim=1).mean(0)
    aux = ((top1.double() / T) * m).mean() * num_expert ** 2
    return (score * w_score.double() * (idx_out >= 0)).sum() + w_aux * aux


# ---- f32 emulation of the kernels' arithmetic, in their summation order ------------------------------------------------------------
AUX_ROWS = 256   # rows per workgroup of gshard_aux_partial


def aux_emulated(logits, top1, num_expert):
    """(aux, coef) as smoe_gshard_aux computes them: f32 row softmax (max, exp, 1 / sum), column sums per 256-row chunk with thread
    (row of the pass, column) adding every rpp-th row, the rpp partial sums in order, the chunks four-way interleaved, in f32."""
    f = torch.float32
    T, E = logits.shape
    l = logits.to(f)
    scale = torch.tensor(float(num_expert) * float(num_expert), dtype=f) / torch.tensor(float(E), dtype=f)
    Tf = torch.tensor(float(max(T, 1)), dtype=f)
    rpp = 256 // E
    partial = []
    for r0 in range(0, T, AUX_ROWS):
        rows = l[r0:r0 + AUX_ROWS]
        m = rows.max(1, keepdim=True).values
        ex = torch.exp(rows - m)
        s = torch.zeros(rows.shape[0], dtype=f)
        for e in range(E):
            s = s + ex[:, e]
        p = ex * (1.0 / s).unsqueeze(1)
        red = torch.zeros(rpp, E, dtype=f)
        for r in range(rows.shape[0]):
            red[r % rpp] = red[r % rpp] + p[r]
        a = torch.zeros(E, dtype=f)
        for q in range(rpp):
            a = a + red[q]
        partial.append(a)
    acc = [torch.zeros(E, dtype=f) for _ in range(4)]
    n = len(partial)
    c = 0
    while c + 3 < n:
        for q in range(4):
            acc[q] = acc[q] + partial[c + q]
        c += 4
    while c < n:
        acc[0] = acc[0] + partial[c]
        c += 1
    colsum = (acc[0] + acc[1]) + (acc[2] + acc[3])
    ce = top1.to(f) / Tf
    term = ce * (colsum / Tf)
    a = torch.zeros((), dtype=f)
    for e in range(E):
        a = a + term[e]
    return a * scale, scale * ce / Tf


def gate_bwd_emulated(logits, idx, idx_out, score, dscore, coef, coef_scale=None):
    """dlogits as smoe_gshard_gate_bwd computes it, in f32 and in its order (fused multiply-adds written as separate operations: the
    difference is part of what the measured error covers)."""
    f = torch.float32
    l = logits.to(f)
    T, E = l.shape
    s = score.to(f)
    if dscore is not None:
        ds = dscore.to(f) * (idx_out >= 0)
    else:
        ds = torch.zeros(T, 2, dtype=f)
    inner = s[:, 1] * ds[:, 1] + s[:, 0] * ds[:, 0]
    g = s * (ds - inner.unsqueeze(1))
    out = torch.zeros(T, E, dtype=f)
    if coef is not None:
        cs = torch.tensor(1.0, dtype=f) if coef_scale is None else coef_scale.to(f).reshape(())
        m = l.max(1, keepdim=True).values
        ex = torch.exp(l - m)
        ssum = torch.zeros(T, dtype=f)
        dot = torch.zeros(T, dtype=f)
        for e in range(E):
            ssum = ssum + ex[:, e]
            dot = dot + ex[:, e] * coef[e].to(f)
        inv = 1.0 / ssum
        dot = dot * inv
        p = ex * inv.unsqueeze(1)
        out = cs * (p * (coef.to(f).unsqueeze(0) - dot.unsqueeze(1)))
    add0 = torch.zeros(T, E, dtype=f).scatter_(1, idx[:, :1], g[:, :1])
    add1 = torch.zeros(T, E, dtype=f).scatter_(1, idx[:, 1:], g[:, 1:])
    return (out + add0) + add1


def ulp32(x: float) -> float:
    """the spacing of f32 at |x| (one unit in the last place)"""
    x = abs(float(x))
    return 2.0 ** -149 if x < 2.0 ** -126 else 2.0 ** (math.floor(math.log2(x)) - 23)


def bar(emulated_err: float, ref_abs_max: float) -> float:
    """the project's rule for an f32 kernel against float64: 3 x the error the same arithmetic makes in a host emulation, and never
    below one f32 ulp of the largest reference value (an emulation that happens to be exact says nothing about an ulp)."""
    return max(3.0 * emulated_err, ulp32(ref_abs_max))


# ---- rule 5: the whole operator in float64 ------------------------------------------------------------------------------------------
def ffn64(x, w1, b1, w2, b2, e):
    h = torch.nn.functional.gelu(x.double() @ w1[e].double().t() + b1[e].double())
    return h @ w2[e].double().t() + b2[e].double()


def moe64(x, idx_out, score, w1, b1, w2, b2, residual=None):
    """out[t] = sum over the KEPT entries of score[t, j] * expert_{idx_out[t, j]}(x[t]) (+ residual[t]); scores not renormalised."""
    T, d = x.shape
    out = torch.zeros(T, w2.shape[1], dtype=torch.float64) if residual is None else residual.double().clone()
    for e in range(w1.shape[0]):
        for j in range(2):
            rows = (idx_out[:, j] == e).nonzero().squeeze(1)
            if rows.numel():
                out = out.index_add(0, rows, score[rows, j].double().unsqueeze(1) * ffn64(x[rows], w1, b1, w2, b2, e))
    return out
