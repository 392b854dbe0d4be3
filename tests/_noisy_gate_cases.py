"""The noisy top-k gate's rule ("NoisyGate") as a plain CPU restatement in float64 -- autograd over it is the gradient
oracle --, an f32 host emulation of the kernels' arithmetic (its error against float64 is what the GPU bars are taken from) and
the case table the host and the GPU tests share.  The emulation is f32 THROUGHOUT, in the kernels' formulas and summation order: the
bar of an all-f32 kernel.  The kernels themselves compute in f64 between their f32 inputs and outputs (csrc/noisy_gate.hip says
why), so they sit well inside it; the emulation is not loosened to match.

Row counts of the kernels under test (csrc/noisy_gate.hip) -- the sizes at which they change path:

    kernel                  per wave     per workgroup
    noisy_gate_rows         64 rows      256 rows = one chunk of column partials  (T = 63, 64, 65 and 255, 256, 257 straddle them)
    noisy_gate_finish       --           adds the chunks in order                 (T = 257: 2 chunks; T = 1500: 6, the last one ragged)
    noisy_gate_bwd          64 rows      256 rows                                 (one thread per row: no row crosses a boundary)

Regimes (the logits2 = [clean | raw] of a case):
    plain   Gaussian clean and raw
    sat     raw shifted to -8: sigma close to 0.01, Phi saturates
    lin     raw shifted to +25: softplus' linear branch (raw > 20)
    zero    raw = 0 (w_noise = 0)
    offset  expert 0's clean logit + 2: importance and load unbalanced
Rows are tie-free by construction: a row's eps is redrawn until all pairwise gaps of its float64 noisy values exceed
MARGIN * max(1, |value|); test_noisy_gate_host.py asserts that for every row of every case.
"""
import itertools
import math

import torch

TS = (1, 2, 63, 64, 65, 255, 256, 257, 1500)
EKS = ((2, 1), (8, 1), (8, 2), (8, 4), (32, 1), (32, 2), (32, 4))
REGIMES = ("plain", "sat", "lin", "zero", "offset")
SEED = 11
MARGIN = 1e-4
NOISE_EPS = 1e-2
CHUNK = 256      # rows per workgroup of noisy_gate_rows = rows per chunk of the column partials


def sigma64(raw):
    """softplus(raw) + noise_epsilon, torch's softplus: beta 1, threshold 20"""
    return torch.where(raw > 20.0, raw, torch.log1p(torch.exp(torch.clamp(raw, max=20.0)))) + NOISE_EPS


def noisy64(logits2, eps, training=True):
    l = logits2.double()
    E = l.shape[1] // 2
    clean, raw = l[:, :E], l[:, E:]
    if not training:
        return clean, raw, torch.zeros_like(clean), clean
    sigma = sigma64(raw)
    e = torch.zeros_like(clean) if eps is None else eps.double()
    return clean, raw, sigma, clean + e * sigma


def min_margin(values):
    """per row: min over pairs of |a - b| / max(1, |a|, |b|)"""
    v = values.double()
    gap = (v.unsqueeze(2) - v.unsqueeze(1)).abs()
    scale = torch.maximum(v.abs().unsqueeze(2), v.abs().unsqueeze(1)).clamp(min=1.0)
    ratio = gap / scale
    ratio = ratio + torch.eye(v.shape[1], dtype=torch.float64).unsqueeze(0) * 1e30
    return ratio.reshape(v.shape[0], -1).min(1).values


class Case:
    def __init__(self, T, E, k, regime):
        self.T, self.E, self.k, self.regime = T, E, k, regime
        g = torch.Generator().manual_seed(SEED + 1000003 * T + 7919 * E + 101 * k + 13 * REGIMES.index(regime))
        clean = torch.randn(T, E, generator=g)
        raw = torch.randn(T, E, generator=g)
        if regime == "sat":
            raw = raw - 8.0
        elif regime == "lin":
            raw = raw + 25.0
        elif regime == "zero":
            raw = torch.zeros(T, E)
        elif regime == "offset":
            clean[:, 0] += 2.0
        self.logits2 = torch.cat((clean, raw), 1).contiguous()
        eps = torch.randn(T, E, generator=g)
        for _ in range(200):
            bad = (min_margin(noisy64(self.logits2, eps)[3]) <= MARGIN).nonzero().squeeze(1)
            if bad.numel() == 0:
                break
            eps[bad] = torch.randn(bad.numel(), E, generator=g)
        else:
            raise AssertionError("could not make the rows tie-free")
        self.eps = eps
        self.dscore = torch.randn(T, k, generator=g)
        self.scale = float((0.01 * (1.0 + torch.rand((), generator=g))).float())      # d loss / d aux, an f32 value

    @property
    def id(self):
        return f"T{self.T}-E{self.E}-k{self.k}-{self.regime}"


def table(Ts=TS):
    return [Case(T, E, k, r) for T, (E, k), r in itertools.product(Ts, EKS, REGIMES)]


# ---- the rule, float64 -------------------------------------------------------------------------------------------------------------
def cv2(v):
    return v.var(unbiased=True) / (v.mean() ** 2 + 1e-10)


def forward64(logits2, eps, k, training=True):
    """dict(idx, score, vk, vk1, next, imp, load, aux, noisy) in float64, differentiable w.r.t. ``logits2`` when that is a float64
    leaf.  Ties -> lowest expert id (a stable descending sort)."""
    clean, raw, sigma, noisy = noisy64(logits2, eps, training)
    E = clean.shape[1]
    val, order = torch.sort(noisy, dim=1, descending=True, stable=True)
    idx = order[:, :k]
    score = torch.softmax(val[:, :k], dim=-1)
    imp = torch.zeros(E, dtype=torch.float64).scatter_add(0, idx.reshape(-1), score.reshape(-1))
    vk, vk1 = val[:, k - 1], val[:, k]
    if training:
        thr = torch.where(noisy > vk1.unsqueeze(1), vk1.unsqueeze(1), vk.unsqueeze(1))
        load = (0.5 * (1.0 + torch.erf((clean - thr) / sigma / math.sqrt(2.0)))).sum(0)
    else:
        load = torch.zeros(E, dtype=torch.float64)
    aux = cv2(imp) + (cv2(load) if training else 0.0)
    return dict(idx=idx, score=score, vk=vk, vk1=vk1, next=order[:, k], imp=imp, load=load, aux=aux, noisy=noisy)


def forward_literal(logits2, eps, k, training=True):
    """The rule row by row and expert by expert, as the issue words it (plain Python floats: float64)."""
    T, E2 = logits2.shape
    E = E2 // 2
    idx, score, imp, load = [], [], [0.0] * E, [0.0] * E
    for t in range(T):
        clean = [float(logits2[t, e]) for e in range(E)]
        raw = [float(logits2[t, E + e]) for e in range(E)]
        if training:
            sigma = [(r if r > 20.0 else math.log1p(math.exp(r))) + NOISE_EPS for r in raw]
        else:
            sigma = [0.0] * E
        noisy = [clean[e] + (float(eps[t, e]) if eps is not None else 0.0) * sigma[e] for e in range(E)]
        order = sorted(range(E), key=lambda e: (-noisy[e], e))
        top = order[:k + 1]
        m = noisy[top[0]]
        ex = [math.exp(noisy[e] - m) for e in top[:k]]
        sc = [v / sum(ex) for v in ex]
        idx.append(top[:k]); score.append(sc)
        for j in range(k):
            imp[top[j]] += sc[j]
        if training:
            vk, vk1 = noisy[top[k - 1]], noisy[top[k]]
            for e in range(E):
                thr = vk1 if noisy[e] > vk1 else vk
                load[e] += 0.5 * (1.0 + math.erf((clean[e] - thr) / sigma[e] / math.sqrt(2.0)))
    def cv(v):
        mean = sum(v) / E
        var = sum((a - mean) ** 2 for a in v) / (E - 1)
        return var / (mean * mean + 1e-10)
    aux = cv(imp) + (cv(load) if training else 0.0)
    return (torch.tensor(idx, dtype=torch.int64).reshape(T, k), torch.tensor(score, dtype=torch.float64).reshape(T, k),
            torch.tensor(imp, dtype=torch.float64), torch.tensor(load, dtype=torch.float64), aux)


def coefs64(imp, load, training=True):
    """(d aux / d imp [E], d aux / d load [E]) by autograd over cv2"""
    out = []
    for v, on in ((imp, True), (load, training)):
        if not on:
            out.append(torch.zeros_like(v))
            continue
        leaf = v.detach().clone().requires_grad_(True)
        cv2(leaf).backward()
        out.append(leaf.grad)
    return out


def backward64(logits2, eps, k, dscore, scale, training=True):
    """dlogits2 [T, 2E] of sum(score * dscore) + scale * aux by float64 autograd over the restatement (``dscore`` / ``scale`` None:
    that term is left out)."""
    leaf = logits2.double().clone().requires_grad_(True)
    r = forward64(leaf, eps, k, training)
    obj = torch.zeros((), dtype=torch.float64)
    if dscore is not None:
        obj = obj + (r["score"] * dscore.double()).sum()
    if scale is not None:
        obj = obj + float(scale) * r["aux"]
    if not obj.requires_grad:
        return torch.zeros_like(leaf)
    obj.backward()
    return leaf.grad


# ---- f32 emulation of the kernels' arithmetic, in their summation order ------------------------------------------------------------
F = torch.float32


def _sigma32(raw):
    return torch.where(raw > 20.0, raw, torch.log1p(torch.exp(torch.clamp(raw, max=20.0)))) + torch.tensor(NOISE_EPS, dtype=F)


def _wave_sum(rows):
    """[64, C] -> [C]: the xor butterfly of wave_sum (lane 0's value)"""
    lanes = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        rows = rows + rows[lanes ^ m]
    return rows[0]


def _seq_sum(cols):
    acc = torch.zeros(cols.shape[1:], dtype=F)
    for q in range(cols.shape[0]):
        acc = acc + cols[q]
    return acc


def fwd_emulated(logits2, eps, k, training=True):
    """dict(score, keep, imp, load, aux, coef_imp, coef_load, idx, next) as smoe_noisy_gate_fwd computes them, in f32 (fused
    multiply-adds written as separate operations: the difference is part of what the measured error covers)."""
    l = logits2.to(F)
    T, E = l.shape[0], l.shape[1] // 2
    clean, raw = l[:, :E], l[:, E:]
    if training:
        sigma = _sigma32(raw)
        noisy = clean + (eps.to(F) if eps is not None else torch.zeros(T, E, dtype=F)) * sigma
    else:
        sigma, noisy = torch.zeros_like(clean), clean
    val, order = torch.sort(noisy, dim=1, descending=True, stable=True)
    idx = order[:, :k]
    ex = torch.exp(val[:, :k] - val[:, :1])
    ssum = torch.zeros(T, dtype=F)
    for j in range(k):
        ssum = ssum + ex[:, j]
    score = ex * (1.0 / ssum).unsqueeze(1)
    vk, vk1 = val[:, k - 1], val[:, k]
    ci = torch.zeros(T, E, dtype=F)
    for j in range(k):
        ci = ci + torch.zeros(T, E, dtype=F).scatter_(1, idx[:, j:j + 1], score[:, j:j + 1])
    if training:
        thr = torch.where(noisy > vk1.unsqueeze(1), vk1.unsqueeze(1), vk.unsqueeze(1))
        cl = 0.5 * (1.0 + torch.erf((clean - thr) / sigma * torch.tensor(0.70710678118654752, dtype=F)))
    else:
        cl = torch.zeros(T, E, dtype=F)
    cols = torch.cat((ci, cl), 1)
    pad = (-T) % CHUNK
    cols = torch.cat((cols, torch.zeros(pad, 2 * E, dtype=F)), 0).reshape(-1, CHUNK // 64, 64, 2 * E)
    chunks = []
    for c in range(cols.shape[0]):
        chunks.append(_seq_sum(torch.stack([_wave_sum(cols[c, w]) for w in range(CHUNK // 64)])))
    col = _seq_sum(torch.stack(chunks)) if chunks else torch.zeros(2 * E, dtype=F)
    out = dict(idx=idx, score=score, keep=torch.stack((vk, vk1), 1), next=order[:, k], imp=col[:E], load=col[E:])
    aux = torch.zeros((), dtype=F)
    Ef = torch.tensor(float(E), dtype=F)
    E1 = torch.tensor(float(E - 1), dtype=F)
    for name, vec in (("imp", col[:E]), ("load", col[E:])):
        mean = _seq_sum(vec.reshape(E, 1)).reshape(()) / Ef
        var = _seq_sum(((vec - mean) * (vec - mean)).reshape(E, 1)).reshape(()) / E1
        den = mean * mean + torch.tensor(1e-10, dtype=F)
        out["coef_" + name] = (2.0 * (vec - mean) / E1 * den - var * (2.0 * mean / Ef)) / (den * den)
        aux = aux + var / den if name == "load" else var / den
    out["aux"] = aux
    return out


def bwd_emulated(logits2, eps, k, fwd, dscore, scale, training=True):
    """dlogits2 as smoe_noisy_gate_bwd computes it from the forward's outputs ``fwd`` (f32 tensors: idx, score, keep, next, coef_imp,
    coef_load), in f32."""
    l = logits2.to(F)
    T, E = l.shape[0], l.shape[1] // 2
    clean, raw = l[:, :E], l[:, E:]
    e32 = eps.to(F) if eps is not None else torch.zeros(T, E, dtype=F)
    idx, s = fwd["idx"], fwd["score"].to(F)
    g = dscore.to(F).clone() if dscore is not None else torch.zeros(T, k, dtype=F)
    cs = torch.tensor(0.0 if scale is None else float(scale), dtype=F)
    if scale is not None:
        g = cs * fwd["coef_imp"].to(F)[idx] + g
    inner = torch.zeros(T, dtype=F)
    for j in range(k):
        inner = s[:, j] * g[:, j] + inner
    gn = s * (g - inner.unsqueeze(1))
    dn = torch.zeros(T, E, dtype=F)
    for j in range(k):
        dn = dn + torch.zeros(T, E, dtype=F).scatter_(1, idx[:, j:j + 1], gn[:, j:j + 1])
    dclean, draw = dn.clone(), torch.zeros(T, E, dtype=F)
    if training:
        dsp = torch.where(raw > 20.0, torch.ones_like(raw), 1.0 / (1.0 + torch.exp(-raw)))
        dsig = dn * e32
        if scale is not None:
            sg = _sigma32(raw)
            noisy = clean + e32 * sg
            vk, vk1 = fwd["keep"][:, :1].to(F), fwd["keep"][:, 1:].to(F)
            inside = noisy > vk1
            z = (clean - torch.where(inside, vk1, vk)) / sg
            a = cs * fwd["coef_load"].to(F).unsqueeze(0) * (torch.tensor(0.3989422804014327, dtype=F) * torch.exp(-0.5 * z * z)) / sg
            dclean = dclean + a
            dsig = -a * z + dsig
            zero = torch.zeros_like(a)
            sum_in = _seq_sum(torch.where(inside, a, zero).t().reshape(E, T, 1)).reshape(T)
            sum_out = _seq_sum(torch.where(inside, zero, a).t().reshape(E, T, 1)).reshape(T)
        draw = dsig * dsp
        if scale is not None:
            for who, amount in ((fwd["next"].reshape(T, 1).long(), sum_in), (idx[:, k - 1:k], sum_out)):
                dclean = dclean - torch.zeros(T, E, dtype=F).scatter_(1, who, amount.unsqueeze(1))
                draw = draw - torch.zeros(T, E, dtype=F).scatter_(1, who, (amount * e32.gather(1, who).squeeze(1)
                                                                           * dsp.gather(1, who).squeeze(1)).unsqueeze(1))
    return torch.cat((dclean, draw), 1)


def ulp32(x):
    """the spacing of f32 at |x| (one unit in the last place), elementwise for a tensor"""
    x = torch.as_tensor(x, dtype=torch.float64).abs().clamp(min=2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(x)) - 23)


def within_bar(got, ref, emulated, per_row=True):
    """(ok, worst error / bar ratio).  The bar of an f32 kernel against float64: 3 x the largest error the host emulation of the same
    arithmetic makes on this case, and never below one f32 ulp at the row's scale (per_row: the largest |reference| of the row;
    else -- the [E] sums, a scalar -- of the whole tensor)."""
    ref = ref.double()
    err = (got.double() - ref).abs()
    emu = float((emulated.double() - ref).abs().max()) if ref.numel() else 0.0
    if ref.numel() == 0:
        return True, 0.0
    if per_row and ref.dim() == 2:
        floor = ulp32(ref.abs().max(1, keepdim=True).values)
    else:
        floor = ulp32(ref.abs().max())
    bar = torch.clamp(floor, min=3.0 * emu)
    ratio = float((err / bar).max())
    return ratio <= 1.0, ratio


# ---- the whole operator in float64 ---------------------------------------------------------------------------------------------------
def ffn64(x, w1, b1, w2, b2, e):
    h = torch.nn.functional.gelu(x.double() @ w1[e].double().t() + b1[e].double())
    return h @ w2[e].double().t() + b2[e].double()


def moe64(x, idx, score, w1, b1, w2, b2, residual=None):
    """out[t] = sum_j score[t, j] * expert_{idx[t, j]}(x[t]) (+ residual[t]); scores not renormalised, nothing dropped."""
    out = torch.zeros(x.shape[0], w2.shape[1], dtype=torch.float64) if residual is None else residual.double().clone()
    for e in range(w1.shape[0]):
        for j in range(idx.shape[1]):
            rows = (idx[:, j] == e).nonzero().squeeze(1)
            if rows.numel():
                out = out.index_add(0, rows, score[rows, j].double().unsqueeze(1) * ffn64(x[rows], w1, b1, w2, b2, e))
    return out
