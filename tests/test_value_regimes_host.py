"""Value regimes: the inputs, float64 references, f32 / 16-bit EMULATIONS and bars for LayerNorm rows and attention heads that are
not benign Gaussian data -- rows with a common offset, outlier channels, a variance near eps or of zero; attention rows whose running
maximum climbs at every key chunk, whose dominant key sits next to the padding, that are flat, peaked or offset by hundreds.
tests/test_gpu_value_regimes.py imports this module and holds the kernels to the bars; nothing here needs a GPU or the library.

The bars come from EMULATIONS of the kernels' arithmetic written in torch on the CPU, never from what the kernels give.

LayerNorm, forward, per row (u = 2^-24, float64 mu, sig = sqrt(var + eps), yhat = (x - mu) / sig):

    bar = LN_C u (|mu| / sig + max |yhat| + 1) max |gamma|        (+ the half ulp of a 16-bit store, see ln_elem_bar)

The leading term is the f32 mean's rounding error, which shifts every normalised value by delta / sig.  LN_C = 3 x the worst
error / (bar at LN_C = 1) of `ln_emulate_two_pass` -- f32, summed as csrc/smoe_common.h wave_row_stats sums: 8 serial adds per lane
and 512-element slab, then the 6-step xor butterfly, the squares by FMA -- over every class and width; that worst is 2.80 (off300,
d 192), 3 x it 8.41, so LN_C = 8.5.  Error / bar at LN_C = 8.5, worst row of the 64, for d = 192 / 384 / 768 / 1024:

    class     two-pass emulation               one-pass emulation (E[x^2] - E[x]^2, same summation order)
    benign    0.14    0.16    0.20    0.17     0.19     0.20     0.20     0.17
    off30     0.17    0.19    0.19    0.12     15       14       17       12
    off300    0.33    0.24    0.27    0.24     2.0e2    1.9e2    2.8e2    2.4e2
    off3000   0.30    0.23    0.26    0.16     2.1e6    1.9e6    1.9e6    1.9e6
    negoff    0.26    0.31    0.32    0.19     2.1e4    2.0e4    2.2e4    2.4e4
    out1e3    0.17    0.22    0.12    0.15     0.15     0.26     0.19     0.13
    out1e4    0.12    0.21    0.15    0.12     0.16     0.19     0.16     0.15
    tiny      0.29    0.27    0.23    0.21     3.4e2    2.9e2    2.9e2    2.8e2
    const     0       0       0       0        0        0        0        0

so a one-pass statistic is out by 190 bars and more on off300 / off3000 / negoff / tiny (by 12 on off30) while the two-pass form
stays inside a third of one.  (The outlier classes do not tell the two apart: their mean is small against their deviation.  They are
there for max |yhat| = sqrt(d), for the routers' error bound, and they saturate the token-skip gate, see below.)

LayerNorm, backward, per class (relative L2 of dx, dgamma, dbeta against float64 autograd, each class a call of its own):

    bar = 2e-6 (tests/test_gpu_dense.py) + LN_C u max_rows(|mu| / sig)

`ln_bwd_emulate` (f32, statistics in two passes as csrc/dense_bwd.hip takes them: 4 adds per lane and 256-element slab, butterfly),
worst of the three quantities / bar: benign 0.07-0.08 (bar 2.1e-6), off30 0.04-0.08 (1.8e-5), off300 0.08-0.10 (1.7e-4), off3000
0.08-0.12 (1.6e-3), negoff 0.08-0.12 (8e-3), out1e3 0.07-0.08, out1e4 0.07-0.13 (2.0e-6), tiny 0.11-0.19 (3.8e-4), const 0.00.

The token-skip gate behind the LayerNorm (smoe_gate_ln_bwd, smoe_skip_gate_bwd): dz = -<g_f, xn> p (1 - p) and the gate's weight
gradient sum_t dz_t xn_t, relative L2.  GATE_DZ_BAR = 2.2e-6 = 3 x the worst error of `gate_dz_emulate` (f32 dot products, p (1 - p)
as e / (1 + e)^2 with e = exp(-|z|)): 7.1e-7, on out1e3 at d 768, where the outlier channel puts the logit at 5.1-5.5 in every row;
1.0e-7 to 3.5e-7 everywhere else.  The form p (1 - p) with 1 - p subtracted from the rounded p reaches 6.5e-6 there (3e-7 elsewhere):
that is what both kernels computed until these tests, and what they were changed for.

smoe_gate_ln_bwd's dx, dgamma, dbeta are held to the LayerNorm backward's bar on upstream gradients of its own (`gate_grads`), and the
same emulation check runs on exactly those: `ln_bwd_emulate` of dL/dxn = g_f keep + g_out + dz w, worst / bar: benign 0.08, off30
0.08, off300 0.12, off3000 0.11, negoff 0.12, out1e3 0.07, out1e4 0.16, tiny 0.17, const 0.00.  In the outlier classes g_out carries a
common offset of 0.2: with zero-mean gradients the outlier channel's column sum dgamma[7] is 64 equal-sized terms of random sign,
and the draw first used (out1e3, d 1024) left 0.58 of a sum of magnitudes of 366 -- the emulation then sits at 0.82 (f32 g_f) / 1.04
(f16) of the bar and the MI355X kernel measured 0.73 / 1.41: a column sum that cancels is an input the bar has no term for.

Attention, per (class, N, dtype) and per (image, head): bar = max(the project's bar for the quantity, 3 x the error of `attn_emulate`
against float64) where the emulation is f32 arithmetic with the kernels' rounding points (csrc/attention.hip, attention_bwd.hip): P
rounded to 16 bit relative to the (running) maximum before it meets V and the all-ones row sum, key chunks of 160 with an unconditional
exp2((m_old - m_new) c) rescale for N > 256, `out` rounded to 16 bit before rowsum(dO o out), lse = m c + log2 l in f32, p = exp2(s c -
lse), P and dS rounded to 16 bit before the three gradient products, f32 accumulation, 16-bit stores.  The project's bars: out max
|diff| <= tol max(1, max |ref|), tol 2e-3 f16 / 1.5e-2 bf16 (test_gpu_parity.py); lse 2e-3 / 2e-2 absolute; dq / dk / dv relative L2
4e-3 / 2e-2 and max |diff| <= 2e-2 / 1e-1 max |ref| for N <= 256 (test_gpu_dense.py), 9.4e-4 / 7.6e-3 and 2.4e-3 / 1.7e-2 above
(test_gpu_attention_long.py).  No bar may exceed 10 x the SHORT kernel's bar of its quantity (attn_cap), at any N: the long kernels'
tightened bars are 3 x a measurement on benign data and the peaked classes exceed 10 x them by construction -- dS = P o (dP - delta)
cancels where one key carries the row, and dq = dS K multiplies what the 16-bit dS lost by keys of magnitude 0.25 N (asc) or 150
(offset).  `asc` is toned down for that cap: its slope is 0.25 per key, not 0.35 (at 0.35 its bf16 dq needs 3 x 7.9e-2 relative L2
and 3 x 0.35 max at N = 640, past the cap of 0.2 / 1.0; at 0.25, 0.82 of it); a chunk of 160 keys still raises the running maximum
by 58 log2 units.  `desc` keeps 0.35.  The emulation's errors, worst head and worst N of each class (profiles/r11_value_regimes.md
has every N):

    class    dt    out      lse      dq L2    dk L2    dv L2    dq max   dk max   dv max
    benign   f16   3.8e-04  1.2e-04  3.3e-04  3.1e-04  3.1e-04  7.5e-04  6.8e-04  6.1e-04
    benign   bf16  2.9e-03  1.0e-03  2.6e-03  2.4e-03  2.4e-03  5.2e-03  3.8e-03  5.5e-03
    asc      f16   3.7e-04  2.6e-04  6.8e-03  4.0e-04  3.1e-04  2.5e-02  6.1e-04  4.5e-04
    asc      bf16  3.0e-03  2.2e-03  5.4e-02  4.0e-03  2.6e-03  2.7e-01  7.5e-03  3.3e-03
    desc     f16   3.9e-04  2.5e-04  3.9e-04  4.5e-04  3.3e-04  6.4e-04  9.8e-04  5.1e-04
    desc     bf16  2.9e-03  2.1e-03  3.2e-03  3.6e-03  2.5e-03  7.1e-03  5.3e-03  4.2e-03
    peaked   f16   4.2e-04  3.0e-04  8.5e-04  8.3e-04  2.6e-04  8.0e-04  1.1e-03  4.2e-04
    peaked   bf16  3.4e-03  2.0e-03  6.6e-03  6.4e-03  2.1e-03  9.3e-03  8.2e-03  3.7e-03
    uniform  f16   6.1e-05  3.3e-07  3.0e-04  0        3.5e-04  4.3e-04  0        5.8e-04
    uniform  bf16  4.8e-04  3.3e-07  2.4e-03  0        2.8e-03  3.9e-03  0        4.2e-03
    offset   f16   3.6e-04  1.3e-04  6.1e-03  3.1e-04  3.1e-04  2.7e-02  4.8e-04  5.1e-04
    offset   bf16  3.3e-03  1.0e-03  4.6e-02  2.4e-03  2.4e-03  1.9e-01  4.2e-03  6.3e-03
"""
import functools
import math

import pytest
import torch

EPS = 1e-6
U = 2.0 ** -24
ROWS = 64
DIMS = (192, 384, 768, 1024)
LN_CLASSES = ("benign", "off30", "off300", "off3000", "negoff", "out1e3", "out1e4", "tiny", "const")
ONE_PASS_MUST_FAIL = ("off300", "off3000", "negoff", "tiny")
LN_C = 8.5
LN_BWD_BASE = 2e-6


# --------------------------------------------------------------------------------------------------------------- LayerNorm: inputs
@functools.lru_cache(maxsize=None)
def ln_rows(cls, d):
    """[ROWS, d] f32 rows of one class; a fixed seed per (class, d).  Shared between tests: never written to."""
    g = torch.Generator().manual_seed(1000 * LN_CLASSES.index(cls) + d)
    r = torch.randn(ROWS, d, generator=g)
    if cls == "benign":
        x = r * 1.7 + 0.3
    elif cls in ("off30", "off300", "off3000"):
        x = r + float(cls[3:])
    elif cls == "negoff":
        x = 0.05 * r - 700.0
    elif cls == "out1e3":
        x = r.clone()
        x[:, 7] = 1e3
    elif cls == "out1e4":
        x = r.clone()
        x[:, 3::97] = 3e2
        x[:, 7] = 1e4
    elif cls == "tiny":
        x = 1 + 1e-3 * r
    elif cls == "const":
        x = torch.full((ROWS, d), 2.5)
    else:
        raise KeyError(cls)
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def ln_params(d):
    g = torch.Generator().manual_seed(77 + d)
    return (1 + 0.2 * torch.randn(d, generator=g)).float(), (0.1 * torch.randn(d, generator=g)).float()


@functools.lru_cache(maxsize=None)
def ln_dy(cls, d, dt=torch.float32):
    g = torch.Generator().manual_seed(5000 + 1000 * LN_CLASSES.index(cls) + d)
    return (torch.randn(ROWS, d, generator=g) * 0.1).to(dt)


# ----------------------------------------------------------------------------------------------------- LayerNorm: float64 and bars
def ln_f64(x, gamma, beta):
    """float64 statistics and output of rows x (any float dtype: read as they are): dict(mu, sig, yhat, y), mu / sig [R]"""
    xd = x.double()
    mu = xd.mean(-1)
    xc = xd - mu[:, None]
    sig = ((xc * xc).mean(-1) + EPS).sqrt()
    yhat = xc / sig[:, None]
    return dict(mu=mu, sig=sig, yhat=yhat, y=yhat * gamma.double() + beta.double())


def ln_row_bar(ref, gamma, c=LN_C):
    """[R] float64: c u (|mu| / sig + max |yhat| + 1) max |gamma|"""
    return c * U * (ref["mu"].abs() / ref["sig"] + ref["yhat"].abs().amax(-1) + 1) * float(gamma.abs().max())


_STORE = {torch.float32: (0.0, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25), torch.bfloat16: (2.0 ** -8, 0.0), None: (0.0, 0.0)}


def ln_elem_bar(ref, gamma, odt=torch.float32, c=LN_C):
    """[R, d] float64: the row bar, plus for a 16-bit output the half ulp of the store of a value inside the row bar of the
    reference: 2^-11 (f16) / 2^-8 (bf16) relative, 2^-25 absolute for f16's subnormals."""
    rb = ln_row_bar(ref, gamma, c)[:, None]
    rel, ab = _STORE[odt]
    return rb + rel * (ref["y"].abs() + rb) + ab


def ln_ratio(got, ref, gamma, odt=torch.float32, c=LN_C):
    """[R]: per row the worst |got - ref| / bar (inf where got is not finite)"""
    g = got.detach().double().cpu()
    r = ((g - ref["y"]).abs() / ln_elem_bar(ref, gamma, odt, c)).amax(-1)
    return torch.where(torch.isfinite(g).all(-1), r, torch.full_like(r, math.inf))


def ln_bwd_f64(x, dy, gamma, beta):
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (x.shape[-1],), gr, br, EPS).backward(dy.double())
    return xr.grad, gr.grad, br.grad


def ln_bwd_bar(x, gamma, beta):
    ref = ln_f64(x, gamma, beta)
    return LN_BWD_BASE + LN_C * U * float((ref["mu"].abs() / ref["sig"]).max())


def rel_l2(got, ref):
    return float((got.detach().double().cpu() - ref.double()).norm() / ref.double().norm().clamp(min=1e-30))


# ------------------------------------------------------------------------------------------------------- LayerNorm: f32 emulations
def _fma(a, b, c):
    """f32 fma: the product of two f32 is exact in float64; one rounding to f64 of the sum, far below the one to f32"""
    return (a.double() * b.double() + c.double()).float()


def _butterfly(s):
    """s [R, 64] f32 -> [R]: s += shfl_xor(s, m) for m = 32 .. 1 (every lane ends with the same value)"""
    lanes = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ m]
    return s[:, 0]


def _slabs(x, per_lane):
    """x [R, d] f32 -> ([R, NI, 64, per_lane], valid [NI, 64]): lane l's elements [per_lane l + 64 per_lane i, + per_lane) of slab i,
    zeros past d; valid = the lane's chunk starts inside the row (d is a multiple of per_lane)"""
    R, d = x.shape
    slab = 64 * per_lane
    NI = -(-d // slab)
    xp = torch.zeros(R, NI * slab)
    xp[:, :d] = x
    valid = (torch.arange(NI * 64) * per_lane < d).reshape(NI, 64)
    return xp.reshape(R, NI, 64, per_lane), valid


def _wave_sum8(v):
    """wave_row_stats' first sum: per lane s += v[i][q] serially over slabs and the 8 elements, then the butterfly"""
    s = torch.zeros(v.shape[0], 64)
    for i in range(v.shape[1]):
        for q in range(v.shape[3]):
            s = s + v[:, i, :, q]
    return _butterfly(s)


def _wave_stats(x, one_pass=False):
    """(mean, rstd) [R] f32 of rows x as csrc/smoe_common.h wave_row_stats computes them; one_pass: var = E[x^2] - E[x]^2 with the
    squares summed in the same order (the variant the kernels must NOT be)"""
    d = x.shape[1]
    inv_d = torch.tensor(1.0 / d, dtype=torch.float32)
    v, valid = _slabs(x, 8)
    mean = _wave_sum8(v) * inv_d
    s2 = torch.zeros(x.shape[0], 64)
    for i in range(v.shape[1]):
        for q in range(8):
            a = v[:, i, :, q] if one_pass else v[:, i, :, q] - mean[:, None]
            s2 = torch.where(valid[i][None, :], _fma(a, a, s2), s2)
    s2 = _butterfly(s2)
    var = (s2 * inv_d - mean * mean).clamp(min=0.0) if one_pass else s2 * inv_d
    return mean, torch.rsqrt(var + torch.tensor(EPS, dtype=torch.float32))


def ln_emulate_two_pass(x, gamma, beta, one_pass=False):
    """f32 LayerNorm of f32 rows in wave_row_stats' order and wave_row_affine's form: fma((x - mean) rstd, gamma, beta)"""
    mean, rstd = _wave_stats(x.float(), one_pass)
    return _fma((x.float() - mean[:, None]) * rstd[:, None], gamma, beta)


def ln_emulate_one_pass(x, gamma, beta):
    return ln_emulate_two_pass(x, gamma, beta, one_pass=True)


def ln_bwd_emulate(x, dy, gamma):
    """f32 emulation of csrc/dense_bwd.hip layernorm_bwd_kernel: lane l holds elements [4 l + 256 j, + 4); mean from
    (x0 + x1) + (x2 + x3) per slab, the squares by FMA, both over the butterfly; then c1 = mean(g), c2 = mean(g xhat),
    dx = rstd (g - c1 - xhat c2); dgamma / dbeta summed row after row."""
    R, d = x.shape
    inv_d = torch.tensor(1.0 / d, dtype=torch.float32)
    xv, valid = _slabs(x.float(), 4)
    gv, _ = _slabs(dy.float(), 4)
    gm, _ = _slabs(gamma.float()[None, :], 4)
    s1 = torch.zeros(R, 64)
    for j in range(xv.shape[1]):
        s1 = s1 + ((xv[:, j, :, 0] + xv[:, j, :, 1]) + (xv[:, j, :, 2] + xv[:, j, :, 3]))
    mean = _butterfly(s1) * inv_d
    s2 = torch.zeros(R, 64)
    for j in range(xv.shape[1]):
        for i in range(4):
            dv = xv[:, j, :, i] - mean[:, None]
            s2 = torch.where(valid[j][None, :], _fma(dv, dv, s2), s2)
    rstd = torch.rsqrt(_butterfly(s2) * inv_d + torch.tensor(EPS, dtype=torch.float32))
    xh = torch.where(valid[None, :, :, None], (xv - mean[:, None, None, None]) * rstd[:, None, None, None], torch.zeros(()))
    g = gv * gm
    c1, c2 = torch.zeros(R, 64), torch.zeros(R, 64)
    for j in range(xv.shape[1]):
        for i in range(4):
            c1 = c1 + g[:, j, :, i]
            c2 = _fma(g[:, j, :, i], xh[:, j, :, i], c2)
    c1, c2 = _butterfly(c1) * inv_d, _butterfly(c2) * inv_d
    dx = rstd[:, None, None, None] * (g - c1[:, None, None, None] - xh * c2[:, None, None, None])
    dgam, dbet = torch.zeros(xv.shape[1:]), torch.zeros(xv.shape[1:])
    for t in range(R):
        dgam = _fma(gv[t], xh[t], dgam)
        dbet = dbet + gv[t]
    return dx.reshape(R, -1)[:, :d], dgam.reshape(-1)[:d], dbet.reshape(-1)[:d]


# ------------------------------------------------------------------------------------------- the token-skip gate behind a LayerNorm
GATE_DZ_BAR = 2.2e-6


@functools.lru_cache(maxsize=None)
def gate_params(d):
    g = torch.Generator().manual_seed(7 * d + 3)
    return torch.randn(d, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1


def gate_dz_f64(xn, g_f, w, b):
    """dz = -<g_f, xn> p (1 - p), p = sigmoid(<xn, w> + b), in float64 on the rows xn as they are"""
    z = xn.double() @ w.double() + b.double()
    return -(g_f.double() * xn.double()).sum(-1) * torch.sigmoid(z) * torch.sigmoid(-z)


def gate_dz_emulate(xn, g_f, w, b, subtract=False):
    """f32: both dot products, then p (1 - p) as e / (1 + e)^2 with e = exp(-|z|) -- or, `subtract`, as p (1 - p) from the rounded
    p = 1 / (1 + exp(-z)), the form the gate's backward kernels had: it cancels once the gate saturates"""
    xn = xn.float()
    z, dot = (xn * w).sum(-1) + b, (g_f.float() * xn).sum(-1)
    if subtract:
        p = 1 / (1 + torch.exp(-z))
        return -dot * p * (1 - p)
    e = torch.exp(-z.abs())
    return -dot * (e / ((1 + e) * (1 + e)))


GATE_THR = 0.55
G_OUT_OFFSET = {"out1e3": 0.2, "out1e4": 0.2}      # every other class: 0


@functools.lru_cache(maxsize=None)
def gate_grads(cls, d, gdt=torch.float32, g_out_offset=None):
    """(g_f [R, d] in gdt, g_out [R, d] f32): the two upstream gradients of one gated half.  In the outlier classes g_out carries a
    common offset of 0.2, as a residual stream's gradient may: there xhat = sqrt(d) in EVERY row of channel 7, so with zero-mean
    gradients dgamma[7] = sum_t dxn[t, 7] xhat[t, 7] is a sum of 64 equal-sized terms of random sign, which dominates |dgamma| --
    unless the draw leaves it near 0 (a few draws in a hundred), where ANY f32 sum misses a
    relative bar: test_a_cancelling_column_sum_is_outside_the_bar_for_any_f32_sum.  The other classes keep zero-mean
    gradients (an offset there multiplies the common error of a row's xhat into every column: `tiny` reaches 0.41 of the bar at 0.2).
    test_gate_ln_backward_emulation_is_inside_a_third_of_the_bar holds every (class, d, dtype) drawn here to the emulation check."""
    g = torch.Generator().manual_seed(7 * d + 4)
    off = G_OUT_OFFSET.get(cls, 0.0) if g_out_offset is None else g_out_offset
    return (3 * ln_dy(cls, d)).to(gdt), torch.randn(ROWS, d, generator=g) * 0.2 + off


def gate_ln_bwd_f64(x, gamma, beta, w, b, g_f, g_out):
    """float64 autograd through LayerNorm and the reference's gate expressions (models/resMoE.py:69-77, 126-136; the formula of
    tests/test_gpu_gate.py): dict(dx, dgamma, dbeta, dgate_w, xn, dxn = dL/dxn, mask [R, 2] f32 = (skip, keep))"""
    d = x.shape[1]
    xr, gr, btr, wr, br = [t.double().requires_grad_(True) for t in (x, gamma, beta, w, b)]
    xn = torch.nn.functional.layer_norm(xr, (d,), gr, btr, EPS)
    xn.retain_grad()
    prob = torch.sigmoid(xn @ wr + br)[:, None]
    _prob = 1 - prob
    skip_tk = (prob > GATE_THR).double() + _prob.detach() - _prob
    tk = (prob <= GATE_THR).double() + prob.detach() - prob
    ((g_f.double() * (xn * tk)).sum() + (g_out.double() * (xn * tk + xn * skip_tk)).sum()).backward()
    mask = torch.cat([(prob > GATE_THR).float(), (prob <= GATE_THR).float()], dim=1).detach()
    return dict(dx=xr.grad, dgamma=gr.grad, dbeta=btr.grad, dgate_w=wr.grad, xn=xn.detach(), dxn=xn.grad, mask=mask)


def gate_bwd_bar(x, gamma, beta):
    """dz and the gate's weight gradient behind a LayerNorm: GATE_DZ_BAR + the LayerNorm term of ln_bwd_bar"""
    return ln_bwd_bar(x, gamma, beta) - LN_BWD_BASE + GATE_DZ_BAR


# -------------------------------------------------------------------------------------------------------------- attention: inputs
SCALE = 0.125
ATTN_CLASSES = ("benign", "asc", "desc", "peaked", "uniform", "offset")
ATTN_NS = (197, 256, 257, 300, 577, 640)
ATTN_DTYPES = (torch.float16, torch.bfloat16)
ATTN_H = 2
QUANTS = ("out", "lse", "dq_l2", "dk_l2", "dv_l2", "dq_max", "dk_max", "dv_max")
FWD_CHUNK = 160          # keys per chunk of attn_fwd_long_kernel (CH = 10 tiles of 16)
ASC_SLOPE, DESC_SLOPE = 0.25, 0.35
P_ZERO = 2.0 ** -160     # a float64 probability below this is exactly 0 in the kernels' f32 exp2


def _dn(dt):
    return {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[dt]


@functools.lru_cache(maxsize=None)
def attn_inputs(cls, N, dt):
    """(qkv [1, N, 3, H, 64], dout [1, N, H 64]) in 16 bit: the float64 reference reads these rounded values"""
    g = torch.Generator().manual_seed(10000 * ATTN_CLASSES.index(cls) + N)
    qkv = torch.randn(1, N, 3, ATTN_H, 64, generator=g) * 1.2
    do = torch.randn(1, N, ATTN_H * 64, generator=g) * 0.5
    j = torch.arange(N, dtype=torch.float32)[None, :, None]
    if cls in ("asc", "desc"):
        qkv[:, :, 0, :, 0] = 8.0
        qkv[:, :, 1, :, 0] = (ASC_SLOPE if cls == "asc" else -DESC_SLOPE) * j
    elif cls == "peaked":
        qkv[:, :, 0:2] *= 3.0
    elif cls == "uniform":
        qkv[:, :, 0] = 0.0
    elif cls == "offset":
        qkv[:, :, 0, :, 0] = 16.0
        qkv[:, :, 1, :, 0] = 150.0
    return qkv.to(dt), do.to(dt)


@functools.lru_cache(maxsize=None)
def attn_f64(cls, N, dt):
    """float64 out [1, N, H 64], lse [1, H, N] (log2 domain), dqkv [1, N, 3, H, 64], probs [1, H, N, N] of the class's inputs"""
    qkv, do = attn_inputs(cls, N, dt)
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.permute(2, 0, 3, 1, 4).unbind(0)
    s = q @ k.transpose(-2, -1) * SCALE
    p = torch.softmax(s, -1)
    out = (p @ v).transpose(1, 2).reshape(1, N, ATTN_H * 64)
    out.backward(do.double())
    lse = torch.logsumexp(s.detach(), -1) / math.log(2.0)
    return dict(out=out.detach(), lse=lse, dqkv=qr.grad, probs=p.detach())


# ----------------------------------------------------------------------------------------------------------- attention: emulation
def _r16(t, dt):
    return t.to(dt).float()


def attn_emulate(qkv, do, dt):
    """(out dt, lse f32, dqkv dt): f32 arithmetic with the kernels' rounding points (module docstring)"""
    B, N, _, H, _ = qkv.shape
    q, k, v = qkv.float().permute(2, 0, 3, 1, 4).unbind(0)                   # [B, H, N, 64]
    scale = torch.tensor(SCALE, dtype=torch.float32)
    c = scale * torch.tensor(1.4426950408889634, dtype=torch.float32)
    s = q @ k.transpose(-2, -1)
    chunk = N if N <= 256 else FWD_CHUNK
    m = torch.full((B, H, N), -math.inf)
    l = torch.zeros(B, H, N)
    o = torch.zeros(B, H, N, 64)
    for k0 in range(0, N, chunk):
        sc = s[..., k0:k0 + chunk]
        m_new = torch.maximum(m, sc.amax(-1))
        alpha = torch.exp2((m - m_new) * c)
        p16 = _r16(torch.exp2(_fma(sc, c, (-m_new * c)[..., None])), dt)
        o = o * alpha[..., None] + p16 @ v[..., k0:k0 + chunk, :]
        l = l * alpha + p16.sum(-1)
        m = m_new
    out = (o * (1.0 / l)[..., None]).transpose(1, 2).reshape(B, N, H * 64).to(dt)
    lse = _fma(m, c, torch.log2(l))
    # backward: delta from the 16-bit out, p from lse
    do4 = do.float().reshape(B, N, H, 64).transpose(1, 2)
    delta = (out.float().reshape(B, N, H, 64).transpose(1, 2) * do4).sum(-1)
    p = torch.exp2(_fma(s, c, -lse[..., None]))
    dp = do4 @ v.transpose(-2, -1)
    ds16 = _r16(p * (dp - delta[..., None]) * scale, dt)
    p16 = _r16(p, dt)
    dq, dk, dv = ds16 @ k, ds16.transpose(-2, -1) @ q, p16.transpose(-2, -1) @ do4
    dqkv = torch.stack((dq, dk, dv), 0).permute(1, 3, 0, 2, 4).to(dt)
    return out, lse, dqkv


def attn_errors(out, lse, dqkv, ref):
    """per head h: {quantity: error}.  out: max |diff| / max(1, max |ref|); lse: max |diff|; dq / dk / dv: relative L2 (_l2) and
    max |diff| / max |ref| (_max), each over the head's own elements"""
    N, H = out.shape[1], ATTN_H
    res = []
    o, r_o = out.detach().double().cpu().reshape(1, N, H, 64), ref["out"].reshape(1, N, H, 64)
    l, g = lse.detach().double().cpu(), dqkv.detach().double().cpu()
    for h in range(H):
        e = {"out": float((o[:, :, h] - r_o[:, :, h]).abs().max() / max(1.0, float(r_o[:, :, h].abs().max()))),
             "lse": float((l[:, h] - ref["lse"][:, h]).abs().max())}
        for i, nm in enumerate("qkv"):
            a, b = g[:, :, i, h], ref["dqkv"][:, :, i, h]
            e[f"d{nm}_l2"] = float((a - b).norm() / b.norm().clamp(min=1e-30))
            e[f"d{nm}_max"] = float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
        res.append(e)
    return res


def attn_existing_bar(quant, N, dt):
    """the bar the suite already holds benign data to (module docstring)"""
    f16 = dt == torch.float16
    if quant == "out":
        return 2e-3 if f16 else 1.5e-2
    if quant == "lse":
        return 2e-3 if f16 else 2e-2
    if N <= 256:
        return {"l2": 4e-3 if f16 else 2e-2, "max": 2e-2 if f16 else 1e-1}[quant[3:]]
    return {"l2": 9.4e-4 if f16 else 7.6e-3, "max": 2.4e-3 if f16 else 1.7e-2}[quant[3:]]


def attn_cap(quant, dt):
    """10 x the short kernel's bar of the quantity"""
    return 10 * attn_existing_bar(quant, 1, dt)


@functools.lru_cache(maxsize=None)
def attn_emulation_errors(cls, N, dt):
    """{quantity: the emulation's error against float64, worst head}"""
    qkv, do = attn_inputs(cls, N, dt)
    errs = attn_errors(*attn_emulate(qkv, do, dt), attn_f64(cls, N, dt))
    return {qn: max(e[qn] for e in errs) for qn in QUANTS}


def attn_bar(cls, N, dt):
    """{quantity: max(existing bar, 3 x emulation error)}"""
    em = attn_emulation_errors(cls, N, dt)
    return {qn: max(attn_existing_bar(qn, N, dt), 3 * em[qn]) for qn in QUANTS}


# --------------------------------------------------------------------------------------------------------------------- the tests
def _fmt(v):
    return f"{v:.2g}"


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cls", LN_CLASSES)
def test_two_pass_emulation_is_inside_a_third_of_the_bar(cls, d):
    x, (gamma, beta) = ln_rows(cls, d), ln_params(d)
    ref = ln_f64(x, gamma, beta)
    r = float(ln_ratio(ln_emulate_two_pass(x, gamma, beta), ref, gamma).max())
    print(f"two-pass {cls} d {d}: worst error / bar {r:.3g}")
    assert r <= 1 / 3
    for odt in (torch.float16, torch.bfloat16):          # ... and still inside the whole bar once a 16-bit store rounds it
        assert float(ln_ratio(ln_emulate_two_pass(x, gamma, beta).to(odt), ref, gamma, odt).max()) <= 1.0


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cls", ONE_PASS_MUST_FAIL)
def test_one_pass_emulation_is_outside_ten_bars(cls, d):
    """the bar discriminates: E[x^2] - E[x]^2 in f32, in the very same summation order, misses it by more than 10 x in EVERY row"""
    x, (gamma, beta) = ln_rows(cls, d), ln_params(d)
    r = ln_ratio(ln_emulate_one_pass(x, gamma, beta), ln_f64(x, gamma, beta), gamma)
    print(f"one-pass {cls} d {d}: error / bar worst row {float(r.max()):.3g}, best row {float(r.min()):.3g}")
    assert float(r.max()) > 10


@pytest.mark.parametrize("d", DIMS)
def test_constant_rows_give_beta_exactly(d):
    x, (gamma, beta) = ln_rows("const", d), ln_params(d)
    assert torch.equal(ln_emulate_two_pass(x, gamma, beta), beta.expand(ROWS, d))
    assert torch.equal(ln_f64(x, gamma, beta)["y"], beta.double().expand(ROWS, d))


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cls", LN_CLASSES)
def test_backward_emulation_is_inside_a_third_of_the_bar(cls, d):
    x, (gamma, beta), dy = ln_rows(cls, d), ln_params(d), ln_dy(cls, d)
    ref = ln_bwd_f64(x, dy, gamma, beta)
    errs = [rel_l2(a, b) for a, b in zip(ln_bwd_emulate(x, dy, gamma), ref)]
    bar = ln_bwd_bar(x, gamma, beta)
    print(f"backward {cls} d {d}: dx {errs[0]:.2e} dgamma {errs[1]:.2e} dbeta {errs[2]:.2e}  bar {bar:.2e}")
    assert max(errs) <= bar / 3


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cls", LN_CLASSES)
def test_gate_dz_emulation_is_inside_a_third_of_its_bar(cls, d):
    """... and the subtracting form is outside the bar where an outlier channel saturates the gate (z about 5 in every row)"""
    x, (gamma, beta), (w, b), g_f = ln_rows(cls, d), ln_params(d), gate_params(d), gate_grads(cls, d)[0]
    xn = ln_f64(x, gamma, beta)["y"].float()
    ref = gate_dz_f64(xn, g_f, w, b)
    e, e_sub = rel_l2(gate_dz_emulate(xn, g_f, w, b), ref), rel_l2(gate_dz_emulate(xn, g_f, w, b, subtract=True), ref)
    print(f"gate dz {cls} d {d}: e / (1 + e)^2 {e:.2e}   p (1 - p) {e_sub:.2e}")
    assert e <= GATE_DZ_BAR / 3
    if d == 768 and cls in ("out1e3", "out1e4"):
        assert e_sub > 2 * GATE_DZ_BAR


def _gate_ln_bwd_emulation_errors(cls, d, gdt, g_out_offset=None):
    x, (gamma, beta), (w, b) = ln_rows(cls, d), ln_params(d), gate_params(d)
    g_f, g_out = gate_grads(cls, d, gdt, g_out_offset)
    ref = gate_ln_bwd_f64(x, gamma, beta, w, b, g_f, g_out)
    got = ln_bwd_emulate(x, ref["dxn"].float(), gamma)          # the LayerNorm backward of the gate's dL/dxn, rounded to f32
    return [rel_l2(a, ref[k]) for a, k in zip(got, ("dx", "dgamma", "dbeta"))], ln_bwd_bar(x, gamma, beta)


@pytest.mark.parametrize("gdt", [torch.float32, torch.float16], ids=_dn)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cls", LN_CLASSES)
def test_gate_ln_backward_emulation_is_inside_a_third_of_the_bar(cls, d, gdt):
    """the emulation check of the LayerNorm backward on the very upstream gradients tests/test_gpu_value_regimes.py hands
    smoe_gate_ln_bwd (dL/dxn = g_f keep + g_out + dz w in float64, rounded to f32)"""
    errs, bar = _gate_ln_bwd_emulation_errors(cls, d, gdt)
    print(f"gate_ln_bwd emulation {cls} d {d} {_dn(gdt)}: dx {errs[0]:.2e} dgamma {errs[1]:.2e} dbeta {errs[2]:.2e}  bar {bar:.2e}")
    assert max(errs) <= bar / 3


def test_a_cancelling_column_sum_is_outside_the_bar_for_any_f32_sum():
    """Why g_out carries an offset.  With zero-mean g_out, out1e3 at d 1024 and an f16 g_f: the outlier channel's 64 terms
    dxn[t, 7] xhat[t, 7] (sum of magnitudes 366) cancel to 0.58, a condition number above 600, and the f32 emulation's dgamma is
    outside the bar (the MI355X kernel measured 2.85e-6 against 2.02e-6 there) -- an input the bar was not made for, whatever sums."""
    x, (gamma, beta), (w, b) = ln_rows("out1e3", 1024), ln_params(1024), gate_params(1024)
    g_f, g_out = gate_grads("out1e3", 1024, torch.float16, 0.0)
    ref = gate_ln_bwd_f64(x, gamma, beta, w, b, g_f, g_out)
    terms = ref["dxn"][:, 7] * ln_f64(x, gamma, beta)["yhat"][:, 7]
    assert float(terms.abs().sum() / terms.sum().abs()) > 600
    errs, bar = _gate_ln_bwd_emulation_errors("out1e3", 1024, torch.float16, 0.0)
    print(f"zero-mean g_out, out1e3 d 1024 f16: emulated dgamma {errs[1]:.2e}, bar {bar:.2e}")
    assert errs[1] > bar / 3


@pytest.mark.parametrize("dt", ATTN_DTYPES, ids=_dn)
@pytest.mark.parametrize("N", ATTN_NS)
@pytest.mark.parametrize("cls", ATTN_CLASSES)
def test_no_attention_bar_exceeds_ten_benign_bars(cls, N, dt):
    em, bar = attn_emulation_errors(cls, N, dt), attn_bar(cls, N, dt)
    print(f"{cls} N {N} {_dn(dt)}: " + "  ".join(f"{qn} {em[qn]:.1e}" for qn in QUANTS))
    for qn in QUANTS:
        assert math.isfinite(em[qn]), qn
        assert bar[qn] <= attn_cap(qn, dt), (qn, bar[qn], attn_cap(qn, dt))


def test_the_classes_are_what_they_claim():
    """asc: the last keys (the last two tiles, next to the padding) carry every row, each chunk of 160 keys raises the maximum by
    tens of log2 units and, from N = 577 on, early keys are below P_ZERO in every row; desc: the first keys do and late keys are; uniform: every probability 1 / N; offset: scores near 300; peaked: score deviation > 10"""
    for dt in ATTN_DTYPES:
        for N in (300, 577):
            p = attn_f64("asc", N, dt)["probs"]
            assert float(p[..., N - 32:].sum(-1).min()) > 0.9 and (N < 577 or int((p.amax(-2) < P_ZERO).sum()) > 0)
            p = attn_f64("desc", N, dt)["probs"]
            assert float(p[..., :32].sum(-1).min()) > 0.9 and (N < 577 or bool((p[..., N - 1] < P_ZERO).all()))
            p = attn_f64("uniform", N, dt)["probs"]
            assert float((p - 1.0 / N).abs().max()) < 1e-15
            qkv, _ = attn_inputs("offset", N, dt)
            q, k, _v = qkv.double().permute(2, 0, 3, 1, 4).unbind(0)
            s = q @ k.transpose(-2, -1) * SCALE
            assert 280 < float(s.min()) and float(s.max()) < 320
            qkv, _ = attn_inputs("peaked", N, dt)
            q, k, _v = qkv.double().permute(2, 0, 3, 1, 4).unbind(0)
            assert float((q @ k.transpose(-2, -1) * SCALE).std()) > 10
