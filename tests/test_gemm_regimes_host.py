"""Value regimes of the GEMM family and the token reductions: the inputs, float64 references, f32 / 16-bit EMULATIONS of the
kernels' arithmetic (written from csrc/) and the bars.  tests/test_gpu_gemm_regimes.py imports this module and holds the kernels to
the bars; nothing here needs a GPU or the library.  A bar is never taken from what a kernel returns.

Every contraction here takes operands that are exact in float64 (f16 / bf16 / f32) and accumulates in f32 (u = 2^-24).

OPERAND CLASSES (along the contracted dimension; `draw`):
    benign     a ~ N(0, 1), w ~ 0.05 N(0, 1), bias ~ 0.1 N(0, 1): the draw of tests/test_gpu_parity.py
    positive   |a|, |w|: nothing cancels, the accumulator grows over all of K -- a short accumulator shows, and the f32 error
               itself grows with the number of adds
    cancel     the second half of K repeats the first with w negated and moved by -1 / 0 / +1 unit in its last place:
               median sum |a| |w| / |sum a w| >= 1e3 (f16 3e5, bf16 3e3-2e4, f32 5e8-4e9)
    range      column k of a times 2^s_k, of w times 2^-s_k, s_k in [-6, 6].  Its unscaled twin `range0` is the benign draw with
               the magnitudes clamped into [2^-7, 16] (a) and [2^-7, 1] (w): the benign draw itself holds f16 subnormals
               (P(|w| < 2^-14) = 1e-3), so "no element leaves the normal range" needs the clamp.  float64(range) == float64(range0).
    subnormal  (f16 only) |a| < 2^-14 (multiples of 2^-24) against |w| in [2^8, 2^10]: ordinary normal outputs; a flush of 16-bit
               input subnormals gives zeros
    edge16     (16-bit stores only, `edge16_case`) one exact product per output, pre-store values over +-[3e4, 7e4] (f16: inf
               above 65520) / the top two binades (bf16), with exact ties: the store must be torch's .to(dtype) of the f32 value

BARS.  f32 store, per element:  |got - ref| <= C u (|A| |W|^T + |bias|),  C = C(class, K, operand type) = 3 x the worst
error / (u (|A| |W|^T + |bias|)) of TWO emulations taken together (`contraction_C`): f32 accumulation strictly sequential in k, and f32
accumulation of exact sums of blocks of the MFMA's K (32 for 16-bit operands: v_mfma_f32_16x16x32; 4 for f32 operands: 16x16x4).
The hardware's inner sum lies between the two WHEN BOTH ARE TAKEN OVER THE SAME OUTPUTS: C comes from 3.5 k outputs, the kernels are
measured on 148 k, and a worst case over 42 x as many outputs is larger -- for f32 operands the MI355X reads 1.1 to 2.0 x the
sequential figures below.  Like for like it IS the sequential emulation there: over all 148 k outputs at K = 64 the chain of FMAs
gives 5.05 / 9.53 / 2.66 / 4.08 (benign / positive / cancel / range), the MI355X's figures to the digit, where a product rounded
before the add gives 4.26 / 9.32 / 2.61 / 4.08 and exact blocks of 4 give 2.20 / 4.13 / 1.36 / 2.20: v_mfma_f32_16x16x4f32 is a chain
of FMAs in k order (`emulate_gemm_all`; the GPU module prints the comparison for f32 operands at K = 64).  The factor 3 is what
covers the larger sample, at 0.46-0.68 of the bar.  C is recomputed from the draws whenever it is used (the first 16 rows of every
group x 72 columns of the N = 72 draw, with and without its bias; the tests print it, profiles/r16_gemm_value_regimes.md has the
sequential and block figures apart):

    class      f16 operands: K 64 / 768 / 3072     bf16 operands            f32 operands (block 4)
    benign     10 / 13 / 9.3                       4.6 / 5.7 / 5.8          11 / 12 / 8.9
    positive   22 / 79 / 149                       12 / 61 / 149            22 / 82 / 171
    cancel     4.5 / 5.0 / 6.6                     2.6 / 2.9 / 3.7          5.4 / 5.6 / 5.1
    range      6.1 / 9.2 / 9.0                     3.2 / 3.6 / 7.5          9.6 / 10 / 7.5
    subnormal  4.4 / 7.1 / 5.8                     -                        -

(the sequential emulation sets every one of them: 1.5-4.3 on benign / range / cancel, 7-57 on positive, where it grows like the
square root of the number of adds; the block emulation stays at 0.3-0.9, positive 2-11, at block 32 and 0.9-2.3, positive 4-24, at
block 4.  bf16 operands sit lower at small K because sums of their 16-bit products are often exact in f32.)

16-bit store: the f32 bar plus half an ulp of the type at the reference (2^-11 f16, 2^-8 bf16 relative; 2^-25 absolute for f16's
subnormals) PER ROUNDING the epilogue performs.  csrc/gemm.hip rounds (staged and direct epilogues alike): (1) acc + bias (+GELU) to
the store type, (2) scale16 by row_scale, rounded again, (3) add16 of the residual, or mulgrad16 by gelu'(H), rounded again
(`chain_ref_bar` carries the error through exactly those points, `chain16` performs them).  With an f32 store the same chain is
two more f32 roundings.

GELU epilogues: the pre-activation's bar times max |gelu'| over the bar's interval, plus the error of the form: 3 x the worst
|f32 emulation of the same polynomial - float64 exact-erf GELU| over [-12, 12] (`gelu_form_error`) plus 4 u |gelu| (v_exp / v_rcp
are good to an ulp; beyond the interval only the relative term is left).  Measured here: gelu_erf 3.7e-7 on |v| < 10 (gemm.hip
quotes < 1e-6: holds), gelu_fast 3.63e-6 on [-6, 6] and on [-12, 12] (gemm.hip quotes 3.6e-6: holds to its two digits); gelu_grad
2.8e-7 on [-8, 8].

THE 20 x CONDITION.  On `benign` every new bar (its LARGEST element, the worst group) is at least 20 x below the bar the existing
test holds the same output to (`test_the_new_bars_are_20x_below_the_existing_ones`, `test_the_other_new_bars_against_the_existing_ones`):
    tests/test_gpu_parity.py grouped GEMM, tol max(1, max |ref|), tol 1e-3 / 8e-3      200-930 x (f16), 2.6e3-1.6e4 x (bf16)
    tests/test_gpu_backward.py wgrad_rows, tol 2e-3 / 1.5e-2 (against the split's C + 3)  318-365 x (f16), 4.2e3-4.9e3 x (bf16)
    ... gate_wgrad, 1e-5 max(1, max |ref|) sqrt(T), on that test's own N(0, 1) draws      57 / 218-293 / 448 x at T 1 / 257 / 5000
    ... group_colsum, tol 2e-3 / 2e-2 (16-bit rows)                                       1.2e3 / 1.2e4 x
Two existing bars are f32 bars already, and 20 x below them is below what an f32 sum can do.  The grouped GEMM's tol for f32
OPERANDS is 2e-5 = 336 u of an output of magnitude 1 to 14 whose sum of magnitudes is 2 to 100, and a sequential f32 sum needs
C = 9-12 u of that sum: the existing bar is 16 / 5.5 / 4.3 x the new one at K 64 / 768 / 3072.  group_colsum's tol for f32 rows is
1e-5 = 168 u of a column sum of about 4 sqrt(n) whose sum of magnitudes is 0.8 n, and the kernel's tree needs C = 4-5 u of that:
5.8 x at the 1500-row group.  4 x is asserted in those two places.  The other new bars have no existing max-norm bar to stand
against: gate_wgrad's bias column is not checked by the existing test, gate_dgrad, rowdot, gather_combine, switch_aux and grad_sumsq
are held to relative L2 or to their own float64 twins elsewhere.

MUTANTS (`test_mutants_are_outside_the_new_bar_and_inside_the_old`): each is outside the new bar on the named class; (a)-(d) are
inside the existing bar on `benign`; (e) is not, and (f) has no existing bar -- the arithmetic of each is beside it:
    (a) accumulator rounded to 16 bit once per 64-element K-step    positive K 768     inside the old bar (0.85-0.89 of it)
    (b) f32 store passed through a 16-bit rounding                  benign K 768       inside
    (c) bf16 store by truncation                                    benign K 768       inside (the old test has f32 stores only)
    (d) bias rounded to the operand type                            benign K 64        inside
    (e) the last K element dropped                                  positive K 768     OUTSIDE the old bar too: one product of
        Gaussian data is 0.03 typical and 0.5 at worst over the output, the old bar is 6e-3 -- what passes the old bar is a dropped
        product below 6e-3, which the new bar (2e-5) still catches by 4e3 x: asserted with the product scaled by 2^-8 (`drop_scale`)
    (f) residual added before the combine scale                     benign K 768       no existing GEMM value test passes a residual, so there
        is nothing for it to be inside of; the difference is (1 - s) |residual|, of the output's own size

THE CONSISTENCY CHECK (GPU module): where a variant's f32-out and 16-bit-out forms share the main loop -- all of 0, 1, 4, 9, 10, 13,
14 do: one kernel template per variant, the store type is a template parameter of the epilogue only -- the 16-bit result equals
`chain16` of the kernel's own f32 store of acc + bias (+GELU), bit for bit.  Not for EPI_GELU_GRAD: gelu'(H) goes through v_exp /
v_rcp, which no CPU reproduces bit for bit; the bar stays there.

THE TOKEN REDUCTIONS, each emulated in its own summation order (csrc/backward.hip, dense_bwd.hip, dispatch.hip, optim.hip), bar =
3 x the emulation's worst error relative to the sum of magnitudes of the terms, and never below 2 u (`reduction_bar_c`):
    group_colsum   chunk of 256 rows x 16 waves, wave w rows w, w + 16, ..: a += (v0 + v1) + (v2 + v3) four rows at a time, a
                   16-leaf tree, chunks k, k + 4, .. of wave k % 4 in two chains, a 4-leaf tree
    gate_wgrad     chunk of 256 rows x 4 waves, wave w rows w, w + 4, .. by FMA, (s0 + s1) + (s2 + s3), chunks as above; the bias
                   column: plain adds, lane l chunks l, l + 64, .., xor butterfly
    gate_dgrad     E FMAs in expert order from 0
    rowdot         lane l elements [8 l + 512 i, + 8) by FMA, xor butterfly
    gather_combine fma(s1, y1, s0 y0) (+ residual)
    switch_aux     thread (rr, e): rows rr, rr + 64, .. and rr + 32, rr + 96, .. of a 1024-row chunk, a0 + a1, 32 partials in
                   order; chunks c % 4 in four chains, (a0 + a1) + (a2 + a3); frac (sum / kept); E terms in order
    grad_sumsq     thread t elements [8 t + 2048 i, + 8) of a 16384-block by FMA of (g mul)^2, xor butterfly, (r0 + r1) + (r2 +
                   r3); the block partials added in f32
"""
import functools
import math

import pytest
import torch

from test_value_regimes_host import _butterfly, _fma    # f32 fma through float64; s += shfl_xor(s, m), m = 32 .. 1, on [R, 64]

U = 2.0 ** -24
THIRD = 1 / 3 + 1e-12      # C is 3 x a worst ratio: that very ratio sits at a third, to rounding
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GROUPS = (1, 0, 127, 129, 321)           # 128-, 256- and 320-row tiles all see a full tile, a tail and an empty group
KS = (64, 768, 3072)
NS = (72, 256)
CLASSES = ("benign", "positive", "cancel", "range")
EMU_ROWS, EMU_COLS = 16, 72              # what the emulations run on: the first rows of every group, the first columns
WGRAD_ROWS = (1, 63, 65, 1000, 0, 2049)
WGRAD_R = ((72, 136), (256, 320))
_STORE = {F32: (U, 0.0), F16: (2.0 ** -11, 2.0 ** -25), BF16: (2.0 ** -8, 0.0)}
OLD_TOL = {F32: 2e-5, F16: 1e-3, BF16: 8e-3}     # tests/test_gpu_parity.py test_grouped_gemm_matches_fp64_reference


def _dn(dt):
    return {F16: "f16", BF16: "bf16", F32: "f32"}[dt]


def mfma_block(dt):
    return 4 if dt == F32 else 32


def classes_of(dt):
    return CLASSES + (("subnormal",) if dt == F16 else ())


# ------------------------------------------------------------------------------------------------------------------- the classes
def _nudge(t, g):
    """t moved by -1 / 0 / +1 unit in the last place of its own type (zeros stay)"""
    it = {2: torch.int16, 4: torch.int32}[t.element_size()]
    step = torch.randint(-1, 2, t.shape, generator=g).to(it)
    return torch.where(t == 0, t, (t.contiguous().view(it) + step).view(t.dtype))


def draw(cls, ra, rw, K, dt, seed):
    """(a [ra, K], w [rw, K]) in dt: one class along the contracted dimension K"""
    g = torch.Generator().manual_seed(seed)
    a, w = torch.randn(ra, K, generator=g), torch.randn(rw, K, generator=g) * 0.05
    if cls == "benign":
        pass
    elif cls == "positive":
        a, w = a.abs(), w.abs()
    elif cls == "cancel":
        h = K // 2
        a, w = a.to(dt), w.to(dt)
        a[:, h:2 * h] = a[:, :h]
        w[:, h:2 * h] = -_nudge(w[:, :h], g)
        a[:, 2 * h:] = 0            # an odd K (the weight gradients' row counts): the element left over is zero
        w[:, 2 * h:] = 0
    elif cls in ("range", "range0"):
        sgn = lambda t: torch.where(t >= 0, 1.0, -1.0)      # noqa: E731
        a, w = (sgn(a) * a.abs().clamp(2.0 ** -7, 16.0)).to(dt), (sgn(w) * w.abs().clamp(2.0 ** -7, 1.0)).to(dt)
        if cls == "range":
            s = torch.randint(-6, 7, (K,), generator=g).float()
            a, w = a * torch.exp2(s).to(dt), w * torch.exp2(-s).to(dt)
    elif cls == "subnormal":
        assert dt == F16
        a = torch.randint(-1023, 1024, (ra, K), generator=g).float() * 2.0 ** -24
        w = torch.where(w >= 0, 1.0, -1.0) * (256 + 768 * torch.rand(rw, K, generator=g))
    else:
        raise KeyError(cls)
    return a.to(dt).contiguous(), w.to(dt).contiguous()


def _seed(cls, K, N):
    return 100003 * (CLASSES + ("subnormal", "range0")).index(cls) + 17 * K + N


@functools.lru_cache(maxsize=6)
def gemm_case(cls, K, N, dt):
    """dict(A [M, K] dt, W [E, N, K] dt, bias [E, N] f32, offsets i32 [E + 1], expert [M] i64).  Shared: never written to."""
    E, M = len(GROUPS), sum(GROUPS)
    a, w = draw(cls, M, E * N, K, dt, _seed(cls, K, N))
    g = torch.Generator().manual_seed(_seed(cls, K, N) + 1)
    bias = torch.randn(E, N, generator=g) * 0.1
    offsets = torch.tensor([0] + list(GROUPS), dtype=torch.int64).cumsum(0).to(torch.int32)
    expert = torch.repeat_interleave(torch.arange(E), torch.tensor(GROUPS))
    return dict(A=a, W=w.reshape(E, N, K), bias=bias, offsets=offsets, expert=expert)


@functools.lru_cache(maxsize=64)
def gemm_ref(cls, K, N, dt):
    """float64 (acc [M, N] = A W[e]^T without the bias, mag [M, N] = |A| |W[e]|^T, bias rows [M, N])"""
    c = gemm_case(cls, K, N, dt)
    M = c["A"].shape[0]
    acc, mag = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, N, dtype=torch.float64)
    for e in range(len(GROUPS)):
        lo, hi = int(c["offsets"][e]), int(c["offsets"][e + 1])
        if hi > lo:
            ad, wd = c["A"][lo:hi].double(), c["W"][e].double()
            acc[lo:hi], mag[lo:hi] = ad @ wd.t(), ad.abs() @ wd.abs().t()
    return acc, mag, c["bias"].double()[c["expert"]]


# -------------------------------------------------------------------------------------------------- the contraction's emulations
def emulate_acc(a, w, block, round_every=None, drop_last=False, drop_scale=1.0):
    """f32 [r, n] = sum_k a[r, k] w[n, k]: acc = f32(acc + the exact sum of `block` products), blocks in k order from 0 (block 1: a
    chain of FMAs).  The mutants: round_every = (elements, dtype): the accumulator rounded to dtype after every so many elements;
    drop_last: the last product (times drop_scale) is left out."""
    ad, wd = a.double(), w.double().clone()
    K = a.shape[1]
    if drop_last:
        full = ad[:, K - 1, None] * wd[None, :, K - 1]
        wd[:, K - 1] = 0
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, K, block):
        s = ad[:, k0, None] * wd[None, :, k0] if block == 1 else ad[:, k0:k0 + block] @ wd[:, k0:k0 + block].t()
        acc = (acc.double() + s).float()
        if round_every and (k0 + block) % round_every[0] == 0:
            acc = acc.to(round_every[1]).float()
    if drop_last and drop_scale != 1.0:
        acc = (acc.double() + full * (1 - drop_scale)).float()
    return acc


def emu_index(cls, K, N, dt):
    """(rows, cols): the first EMU_ROWS rows of every group and the first EMU_COLS columns"""
    c = gemm_case(cls, K, N, dt)
    rows = torch.cat([torch.arange(int(c["offsets"][e]), min(int(c["offsets"][e]) + EMU_ROWS, int(c["offsets"][e + 1])))
                      for e in range(len(GROUPS))])
    return rows, torch.arange(min(N, EMU_COLS))


def emulate_gemm(cls, K, N, dt, block, bias=True, bias_dt=None, **mutant):
    """f32 [rows, cols] of emu_index: acc + bias as the kernels add it (one f32 add behind the K loop)"""
    c = gemm_case(cls, K, N, dt)
    rows, cols = emu_index(cls, K, N, dt)
    out = torch.zeros(len(rows), len(cols))
    for e in range(len(GROUPS)):
        sel = c["expert"][rows] == e
        if bool(sel.any()):
            out[sel] = emulate_acc(c["A"][rows[sel]], c["W"][e][cols], block, **mutant)
    if bias:
        b = c["bias"][c["expert"][rows]][:, cols]
        out = out + (b.to(bias_dt).float() if bias_dt is not None else b)
    return out


def emulate_gemm_all(cls, K, N, dt, block):
    """f32 [M, N]: emulate_acc over EVERY output of the case (no bias): what the kernels are measured on.  Cheap at K = 64 only."""
    c = gemm_case(cls, K, N, dt)
    out = torch.zeros(c["A"].shape[0], N)
    for e in range(len(GROUPS)):
        lo, hi = int(c["offsets"][e]), int(c["offsets"][e + 1])
        if hi > lo:
            out[lo:hi] = emulate_acc(c["A"][lo:hi], c["W"][e], block)
    return out


def sub(t, idx):
    rows, cols = idx
    return t[rows][:, cols]


def f32_ratio(got, acc, mag, bias):
    """|got - (acc + bias)| / (u (mag + |bias|)), 0 where both are 0; inf where got is not finite"""
    ref = acc + (bias if bias is not None else 0)
    den = U * (mag + (bias.abs() if bias is not None else 0))
    err = (got.detach().double().cpu() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / den.clamp(min=1e-300))
    return torch.where(torch.isfinite(got.detach().double().cpu()), r, torch.full_like(r, math.inf))


@functools.lru_cache(maxsize=None)
def contraction_C(cls, K, dt):
    """(C, sequential worst, block worst): C = 3 x the worst ratio of the two emulations, on the N = 72 draw with and without
    its bias"""
    N = NS[0]
    idx = emu_index(cls, K, N, dt)
    acc, mag, bias = [sub(t, idx) for t in gemm_ref(cls, K, N, dt)]
    seq, blk = [max(float(f32_ratio(emulate_gemm(cls, K, N, dt, b, bias=wb), acc, mag, bias if wb else None).max()) for wb in (True, False))
                for b in (1, mfma_block(dt))]
    return 3 * max(seq, blk), seq, blk


# ---------------------------------------------------------------------------------------------------------------- GELU and chains
def gelu64(v):
    v = v.double()
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad64(v):
    v = v.double()
    return 0.5 * (1 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def _c(x):
    return torch.tensor(x, dtype=torch.float32)


def _erf_poly(v):
    """(p ex, ex) of csrc/gemm.hip gelu_erf / gelu_grad: Abramowitz-Stegun 7.1.26 in f32"""
    z = v.abs() * _c(0.70710678118654752440)
    t = 1.0 / _fma(_c(0.3275911), z, _c(1.0))
    p = _fma(t, _c(1.061405429), _c(-1.453152027))
    for cf in (1.421413741, -0.284496736, 0.254829592):
        p = _fma(p, t, _c(cf))
    p = p * t
    return p, torch.exp2(z * z * _c(-1.4426950408889634))


def gelu_erf_emulate(v):
    v = v.float()
    p, ex = _erf_poly(v)
    return _fma(_c(0.5) * v.abs(), _fma(-p, ex, _c(1.0)), _c(0.5) * v)


def gelu_fast_emulate(v):
    v = v.float()
    v2 = v * v
    p = _fma(v2, _c(-3.28856595e-06), _c(8.92457392e-05))
    for cf in (3.55226046e-04, -1.05218634e-01, -2.30204797e+00):
        p = _fma(p, v2, _c(cf))
    return v * (1.0 / (1.0 + torch.exp2(v * p)))


def gelu_grad_emulate(v):
    v = v.float()
    p, ex = _erf_poly(v)
    cdf = 0.5 + 0.5 * torch.copysign(_fma(-p, ex, _c(1.0)), v)
    return _fma(v * _c(0.3989422804014327), ex, cdf)


_FORMS = {"erf": (gelu_erf_emulate, gelu64), "fast": (gelu_fast_emulate, gelu64), "grad": (gelu_grad_emulate, gelu_grad64)}


@functools.lru_cache(maxsize=None)
def gelu_form_error(form, lim=12.0):
    """the worst |f32 emulation - float64| of one form over [-lim, lim] (a grid of 2^20 + 1 points and every f16 value inside)"""
    grid = torch.cat([torch.linspace(-lim, lim, 2 ** 20 + 1), torch.arange(-2 ** 15, 2 ** 15).to(torch.int16).view(F16).float()])
    grid = grid[torch.isfinite(grid) & (grid.abs() <= lim)]
    emu, exact = _FORMS[form]
    return float((emu(grid).double() - exact(grid)).abs().max())


def _h(x, err, dt):
    """half an ulp of dt at a value within err of x"""
    rel, ab = _STORE[dt]
    return rel * (x.abs() + err) + ab


def chain_ref_bar(acc, mag, bias, C, odt, gelu=None, scale=None, residual=None, hgrad=None):
    """(float64 reference, per-element bar) of one epilogue: acc + bias (-> GELU of form gelu) -> store type -> x scale -> + residual
    | x gelu'(hgrad), each rounded to odt where the kernels round.  scale [M, 1], residual / hgrad [M, N] as the kernel reads them."""
    ref = acc + (bias if bias is not None else 0)
    err = C * U * (mag + (bias.abs() if bias is not None else 0))
    if gelu:
        slope = torch.maximum(gelu_grad64(ref).abs(), torch.maximum(gelu_grad64(ref - err).abs(), gelu_grad64(ref + err).abs())) + err
        ref = gelu64(ref)
        err = err * slope + 3 * gelu_form_error(gelu) + 4 * U * ref.abs()
    if odt != F32:
        err = err + _h(ref, err, odt)
    if scale is not None:
        s = scale.double()
        ref, err = ref * s, err * s.abs()
        err = err + _h(ref, err, odt)
    if residual is not None:
        ref = ref + residual.double()
        err = err + _h(ref, err, odt)
    if hgrad is not None:
        gp = gelu_grad64(hgrad)
        err = err * gp.abs() + ref.abs() * 3 * gelu_form_error("grad", 8.0) + 2 * U * (ref * gp).abs()
        ref = ref * gp
        err = err + _h(ref, err, odt)
    return ref, err


def chain16(v32, odt, scale=None, residual=None, hgrad=None):
    """the epilogue's roundings behind the f32 value acc + bias (+GELU): OutPack::write4, scale16, add16 / mulgrad16"""
    y = v32.float().to(odt)
    if scale is not None:
        y = (y.float() * scale.float()).to(odt)
    if residual is not None:
        y = (y.float() + residual.float()).to(odt)
    if hgrad is not None:
        y = (y.float() * gelu_grad_emulate(hgrad.float())).to(odt)
    return y


def worst(got, ref, bar):
    """worst |got - ref| / bar (inf if got is not finite where ref is)"""
    g = got.detach().double().cpu()
    r = torch.where(g == ref, torch.zeros_like(ref), (g - ref).abs() / bar.clamp(min=1e-300))
    r = torch.where(torch.isfinite(g) | ~torch.isfinite(ref), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


@functools.lru_cache(maxsize=None)
def epilogue_inputs(N, odt):
    """(row_map [M] i64 permutation, row_scale [M] f32 in [0, 1] by OUTPUT row, residual [M, N] odt of the output's magnitude,
    H [M, N] odt saved pre-activations in [-6, 6] with +-0 and the saturated ends)"""
    M = sum(GROUPS)
    g = torch.Generator().manual_seed(4242 + N)
    row_map = torch.randperm(M, generator=g)
    scale = torch.rand(M, generator=g)
    scale[:4] = torch.tensor([0.0, 1.0, 0.5, 2.0 ** -20])
    residual = (torch.randn(M, N, generator=g) * 1.5).to(odt)
    H = torch.rand(M, N, generator=g) * 12 - 6
    H[:, 0], H[:, 1], H[:, 2], H[:, 3] = 0.0, -0.0, 6.0, -6.0
    return row_map, scale, residual, H.to(odt)


@functools.lru_cache(maxsize=None)
def edge16_case(dt):
    """(A [M, 64] dt, W [1, N, 64] dt, pre [M, N] f32): A has one non-zero a_m per row (at k = m % 64), W[n, :] = w_n, so
    pre[m, n] = a_m w_n is ONE exact product (22 / 16 significant bits) -- f16: over +-[3e4, 7e4], past 65520 (inf) on a tenth of
    it; bf16: over the top two binades, [2^126, 2^128).  pre[0, 0] is an exact tie between two finite neighbours, pre[1, 1] the
    largest finite value (f16) / a value that rounds to inf (bf16), pre[2, 2] (f16) the tie 65520 between 65504 and inf."""
    M, N, K = 320, 72, 64
    g = torch.Generator().manual_seed(99)
    if dt == F16:
        a, w = 128 + 128 * torch.rand(M, generator=g), 234.5 + 38.5 * torch.rand(N, generator=g)
        a[:3] = torch.tensor([192.0, 255.875, 252.0])
        w[:3] = torch.tensor([256.25, 256.0, 260.0])     # 192 x 256.25 = 49200: between 49184 and 49216; 252 x 260 = 65520
    else:
        a, w = 2.0 ** 56 * (128 + 53 * torch.rand(M, generator=g)), 2.0 ** 57 * (64 + 117 * torch.rand(N, generator=g))
        a[:2] = 2.0 ** 56 * torch.tensor([160.0, 181.0])
        w[:2] = 2.0 ** 57 * torch.tensor([130.0, 181.0])   # 160 x 130 = 162.5 x 128: a tie; 181 x 181 = 32761 > 32704: inf in bf16
    sa, sw = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0), torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    a, w = (a * sa).to(dt), (w * sw).to(dt)
    A = torch.zeros(M, K, dtype=dt)
    A[torch.arange(M), torch.arange(M) % K] = a
    W = w[:, None].expand(N, K).contiguous()[None]
    pre = (a.double()[:, None] * w.double()[None, :])
    assert torch.equal(pre.float().double(), pre), "every product is exact in f32"
    return A, W, pre.float()


# -------------------------------------------------------------------------------------------------------- weight gradients (rows)
@functools.lru_cache(maxsize=8)
def wgrad_case(cls, R1, R2, dt, rows=WGRAD_ROWS):
    """dict(P [n, R1], Q [n, R2] token-major in dt, offsets i32): class `cls` along the ROWS of every group"""
    P, Q = [], []
    for i, n in enumerate(rows):
        a, w = draw(cls, R1, R2, n, dt, _seed(cls, n, R1 + i)) if n else (torch.zeros(R1, 0, dtype=dt), torch.zeros(R2, 0, dtype=dt))
        P.append(a.t())
        Q.append(w.t())
    offsets = torch.tensor([0] + list(rows), dtype=torch.int64).cumsum(0).to(torch.int32)
    return dict(P=torch.cat(P).contiguous(), Q=torch.cat(Q).contiguous(), offsets=offsets)


@functools.lru_cache(maxsize=8)
def wgrad_ref(cls, R1, R2, dt, rows=WGRAD_ROWS):
    """float64 (out [G, R1, R2], mag)"""
    c = wgrad_case(cls, R1, R2, dt, rows)
    out = torch.zeros(len(rows), R1, R2, dtype=torch.float64)
    mag = torch.zeros_like(out)
    for e in range(len(rows)):
        lo, hi = int(c["offsets"][e]), int(c["offsets"][e + 1])
        p, q = c["P"][lo:hi].double(), c["Q"][lo:hi].double()
        out[e], mag[e] = p.t() @ q, p.abs().t() @ q.abs()
    return out, mag


@functools.lru_cache(maxsize=None)
def wgrad_C(cls, dt, rows=WGRAD_ROWS):
    """3 x the worst ratio of the sequential and the block-32 emulation over the groups' row counts (first 16 x 72 outputs of the
    (72, 136) draw).  The kernel pads a group's rows with zeros to its K-step: exact."""
    R1, R2 = WGRAD_R[0]
    c = wgrad_case(cls, R1, R2, dt, rows)
    out, mag = wgrad_ref(cls, R1, R2, dt, rows)
    w = 0.0
    for e, n in enumerate(rows):
        if n:
            lo = int(c["offsets"][e])
            a, b = c["P"][lo:lo + n, :EMU_ROWS].t(), c["Q"][lo:lo + n, :EMU_COLS].t()
            for block in (1, 32):
                w = max(w, float(f32_ratio(emulate_acc(a, b, block), out[e, :EMU_ROWS, :EMU_COLS], mag[e, :EMU_ROWS, :EMU_COLS], None).max()))
    return 3 * w


# ------------------------------------------------------------------------------------------------------------ the token reductions
def _tree4(r):
    return (r[0] + r[1]) + (r[2] + r[3])


def _two_chains(parts, stride):
    """group_colsum_final / gate_wgrad_final: wave w adds chunks w, w + 4, ..: a0 gets k, a1 gets k + 4, k += 8; then the 4-leaf tree"""
    nc = len(parts)
    zero = torch.zeros_like(parts[0]) if nc else None
    red = []
    for wv in range(stride):
        a0, a1 = zero.clone(), zero.clone()
        k = wv
        while k + stride < nc:
            a0, a1 = a0 + parts[k], a1 + parts[k + stride]
            k += 2 * stride
        if k < nc:
            a0 = a0 + parts[k]
        red.append(a0 + a1)
    return _tree4(red)


def colsum_emulate(src, offsets):
    """f32 [G, C]: csrc/backward.hip group_colsum_partial_kernel + group_colsum_final_kernel"""
    x = src.float()
    out = torch.zeros(len(offsets) - 1, x.shape[1])
    for e in range(len(offsets) - 1):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        parts = []
        for r0 in range(lo, hi, 256):
            r1 = min(r0 + 256, hi)
            red = []
            for wv in range(16):
                a = torch.zeros(x.shape[1])
                r = r0 + wv
                while r + 48 < r1:
                    a = a + ((x[r] + x[r + 16]) + (x[r + 32] + x[r + 48]))
                    r += 64
                while r < r1:
                    a = a + x[r]
                    r += 16
                red.append(a)
            parts.append(_tree4([_tree4(red[4 * q:4 * q + 4]) for q in range(4)]))
        if parts:
            out[e] = _two_chains(parts, 4)
    return out


def gate_wgrad_emulate(dl, x):
    """(dWg f32 [E, C], dbg f32 [E]): gate_wgrad_partial_kernel + gate_wgrad_final_kernel"""
    T, E = dl.shape
    xf = x.float()
    parts, bparts = [], []
    for r0 in range(0, T, 256):
        r1 = min(r0 + 256, T)
        red, bred = [], []
        for wv in range(4):
            acc, bacc = torch.zeros(E, xf.shape[1]), torch.zeros(E)
            for r in range(r0 + wv, r1, 4):
                acc = _fma(dl[r][:, None], xf[r][None, :], acc)
                bacc = bacc + dl[r]
            red.append(acc)
            bred.append(bacc)
        parts.append((red[0] + red[1]) + (red[2] + red[3]))
        bparts.append(_tree4(bred))
    lanes = torch.zeros(E, 64)
    for k, b in enumerate(bparts):
        lanes[:, k % 64] = lanes[:, k % 64] + b
    return _two_chains(parts, 4), _butterfly(lanes)


def gate_dgrad_emulate(dl, w):
    acc = torch.zeros(dl.shape[0], w.shape[1])
    for e in range(w.shape[0]):
        acc = _fma(dl[:, e, None], w[e][None, :], acc)
    return acc


def _lanes8(v):
    """v [n, d] -> [n, NI, 64, 8]: lane l holds elements [8 l + 512 i, + 8), zeros past d"""
    n, d = v.shape
    NI = -(-d // 512)
    p = torch.zeros(n, NI * 512)
    p[:, :d] = v.float()
    return p.reshape(n, NI, 64, 8)


def rowdot_emulate(dout, y, inv_pos, k):
    a, b = _lanes8(dout.float()[torch.arange(len(inv_pos)) // k]), _lanes8(y.float()[inv_pos.clamp(min=0)])
    acc = torch.zeros(len(inv_pos), 64)
    for i in range(a.shape[1]):
        for q in range(8):
            acc = _fma(a[:, i, :, q], b[:, i, :, q], acc)
    return torch.where(inv_pos >= 0, _butterfly(acc), torch.zeros(()))


def gather_combine_emulate(y, inv_pos, score, T, k, residual=None):
    acc = torch.zeros(T, y.shape[1])
    for j in range(k):
        slot = inv_pos.reshape(T, k)[:, j]
        acc = torch.where((slot >= 0)[:, None], _fma(score.reshape(T, k)[:, j, None], y.float()[slot.clamp(min=0)], acc), acc)
    return acc + residual if residual is not None else acc


def switch_aux_emulate(probs, counts):
    """(aux f32 [], coef f32 [E]): switch_aux_partial_kernel + switch_aux_final_kernel"""
    T, E = probs.shape
    rpp = 256 // E
    parts = []
    for r0 in range(0, T, 1024):
        r1 = min(r0 + 1024, T)
        acc = torch.zeros(E)
        for rr in range(rpp):
            a0, a1 = torch.zeros(E), torch.zeros(E)
            r = r0 + rr
            while r + rpp < r1:
                a0, a1 = a0 + probs[r], a1 + probs[r + rpp]
                r += 2 * rpp
            if r < r1:
                a0 = a0 + probs[r]
            acc = acc + (a0 + a1)
        parts.append(acc)
    a = [torch.zeros(E) for _ in range(4)]
    c = 0
    while c + 3 < len(parts):
        for q in range(4):
            a[q] = a[q] + parts[c + q]
        c += 4
    for p in parts[c:]:
        a[0] = a[0] + p
    kept = torch.tensor(float(max(int(counts.sum()), 1)))
    frac = counts.float() / kept
    term = frac * (_tree4(a) / kept)
    acc = torch.zeros(())
    for q in range(E):
        acc = acc + term[q]
    return _c(float(E)) * acc, _c(float(E)) * frac / kept


def sumsq_emulate(g, mul):
    """f32 [n_blocks]: csrc/optim.hip sumsq_block"""
    n = g.numel()
    nb = -(-n // 16384)
    p = torch.zeros(nb * 16384)
    p[:n] = g.float() * _c(mul)
    v = p.reshape(nb, 8, 256, 8)                       # [block, trip, thread, element]
    acc = torch.zeros(nb, 256)
    for i in range(8):
        for q in range(8):
            acc = _fma(v[:, i, :, q], v[:, i, :, q], acc)
    red = _butterfly(acc.reshape(nb * 4, 64)).reshape(nb, 4)
    return (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])


def reduction_bar_c(emulated, ref, mag):
    """C of a reduction's bar C u mag: 3 x the emulation's worst error / (u mag), at least 2"""
    err = (emulated.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * mag).clamp(min=1e-300))
    return max(2.0, 3 * float(r.max()))


COLSUM_GROUPS = (1500, 0, 512, 513, 1)
COLSUM_C = 72


@functools.lru_cache(maxsize=None)
def colsum_case(cls, dt):
    """(src [n, C] dt, offsets i32, ref f64 [G, C], mag, C of the bar): class `positive` / `cancel` along every group's rows"""
    cols = [draw(cls, COLSUM_C, 1, n, dt, 31 * n + 7)[0].t() if n else torch.zeros(0, COLSUM_C, dtype=dt) for n in COLSUM_GROUPS]
    if cls == "cancel":      # a column that cancels: the second half of the rows is the negated first half, moved in its last place
        g = torch.Generator().manual_seed(5)
        cols = [torch.cat([c[:len(c) // 2], -_nudge(c[:len(c) // 2].contiguous(), g), c[2 * (len(c) // 2):]]) for c in cols]
    src = torch.cat(cols).contiguous()
    offsets = torch.tensor([0] + list(COLSUM_GROUPS), dtype=torch.int64).cumsum(0).to(torch.int32)
    ref = torch.stack([src[int(offsets[e]):int(offsets[e + 1])].double().sum(0) for e in range(len(COLSUM_GROUPS))])
    mag = torch.stack([src[int(offsets[e]):int(offsets[e + 1])].double().abs().sum(0) for e in range(len(COLSUM_GROUPS))])
    return src, offsets, ref, mag, reduction_bar_c(colsum_emulate(src, offsets), ref, mag)


GATE_E, GATE_D = 8, 192
GATE_TS = (1, 257, 5000)


@functools.lru_cache(maxsize=None)
def gate_case(T, xdt, dl_scale=0.01):
    """dl [T, E] f32 (0.01 N(0, 1): a softmax backward's magnitudes; 1.0: the draw of tests/test_gpu_backward.py), x [T, d] xdt,
    w [E, d] f32 + float64 references, magnitudes, bar C"""
    g = torch.Generator().manual_seed(T + 1)
    dl, x, w = torch.randn(T, GATE_E, generator=g) * dl_scale, torch.randn(T, GATE_D, generator=g).to(xdt), torch.randn(GATE_E, GATE_D, generator=g) * 0.1
    r = dict(dl=dl, x=x, w=w)
    r["dw"], r["dw_mag"] = dl.double().t() @ x.double(), dl.double().abs().t() @ x.double().abs()
    r["db"], r["db_mag"] = dl.double().sum(0), dl.double().abs().sum(0)
    r["dx"], r["dx_mag"] = dl.double() @ w.double(), dl.double().abs() @ w.double().abs()
    edw, edb = gate_wgrad_emulate(dl, x)
    r["C_dw"], r["C_db"] = reduction_bar_c(edw, r["dw"], r["dw_mag"]), reduction_bar_c(edb, r["db"], r["db_mag"])
    r["C_dx"] = reduction_bar_c(gate_dgrad_emulate(dl, w), r["dx"], r["dx_mag"])
    return r


@functools.lru_cache(maxsize=None)
def combine_case(ydt):
    """k = 2, d = 768, T = 300 tokens, 600 entries into 700 slots, every seventh entry dropped (inv_pos = -1)"""
    T, k, d, S = 300, 2, 768, 700
    g = torch.Generator().manual_seed(12)
    y, dout = torch.randn(S, d, generator=g).to(ydt), (torch.randn(T, d, generator=g) * 0.1)
    inv = torch.randperm(S, generator=g)[:T * k].clone()
    inv[::7] = -1
    score = torch.rand(T * k, generator=g)
    keep = (inv >= 0)
    yg = y.double()[inv.clamp(min=0)] * keep[:, None]
    dd = dout.double()[torch.arange(T * k) // k]
    r = dict(T=T, k=k, y=y, dout=dout, inv=inv, score=score)
    r["dot"], r["dot_mag"] = (dd * yg).sum(-1), (dd.abs() * yg.abs()).sum(-1)
    r["mix"] = (score.double()[:, None] * yg).reshape(T, k, d).sum(1)
    r["mix_mag"] = (score.double()[:, None] * yg.abs()).reshape(T, k, d).sum(1)
    r["C_dot"] = reduction_bar_c(rowdot_emulate(dout, y, inv, k), r["dot"], r["dot_mag"])
    r["C_mix"] = reduction_bar_c(gather_combine_emulate(y, inv, score, T, k), r["mix"], r["mix_mag"])
    return r


@functools.lru_cache(maxsize=None)
def switch_aux_case():
    """T = 5000, E = 8: probabilities of a peaked softmax, counts = the top-1 histogram minus some dropped tokens"""
    T, E = 5000, 8
    g = torch.Generator().manual_seed(8)
    probs = torch.softmax(torch.randn(T, E, generator=g) * 4, -1)
    counts = torch.bincount(probs.argmax(-1), minlength=E).to(torch.int32)
    counts[3] -= 17
    kept = float(counts.sum())
    colsum = probs.double().sum(0)
    aux = E * ((counts.double() / kept) * (colsum / kept)).sum()
    coef = E * counts.double() / kept / kept
    e_aux, e_coef = switch_aux_emulate(probs, counts)
    return dict(probs=probs, counts=counts, aux=aux, coef=coef, C_aux=reduction_bar_c(e_aux, aux, aux.abs()),
                C_coef=reduction_bar_c(e_coef, coef, coef.abs()))


SUMSQ_N = 3 * 16384 + 5
SUMSQ_INV_SCALE = 2.0 ** -16
SUMSQ_REGIMES = {"small": (1e-3, (F32, F16, BF16)),         # a gradient vector near 1e-3
                 "floor": (2.0 ** -44, (F32, BF16)),        # (g 2^-16)^2 about 2^-120: the bottom of f32's normal range (f16 cannot hold it)
                 "top16": (4.0e4, (F32, F16, BF16))}        # near the top of f16


@functools.lru_cache(maxsize=None)
def sumsq_case(regime, dt):
    """(g [n] dt, float64 sum of (g inv_scale)^2, C of the bar relative to it)"""
    g = torch.Generator().manual_seed(len(regime))
    grad = (SUMSQ_REGIMES[regime][0] * (0.5 + torch.rand(SUMSQ_N, generator=g)) * torch.where(torch.rand(SUMSQ_N, generator=g) < 0.5, -1.0, 1.0)).to(dt)
    ref = ((grad.double() * SUMSQ_INV_SCALE) ** 2).sum()
    emu = sumsq_emulate(grad, SUMSQ_INV_SCALE).sum()
    return grad, ref, reduction_bar_c(emu, ref, ref)


# --------------------------------------------------------------------------------------------------------------------- the tests
ALL_DT = (F16, BF16, F32)
CASES = [(c, K, dt) for dt in ALL_DT for c in classes_of(dt) for K in KS]
cases = pytest.mark.parametrize("cls,K,dt", CASES, ids=[f"{c}-K{K}-{_dn(dt)}" for c, K, dt in CASES])


@cases
def test_honest_emulations_are_inside_a_third_of_the_bar(cls, K, dt):
    """both emulations against the f32 bar; and behind the 16-bit stores, the GELU forms and the scale / residual chain against
    theirs (those bars have terms of their own, which no emulation's error went into)"""
    N = NS[0]
    C, seq, blk = contraction_C(cls, K, dt)
    print(f"{cls} K {K} {_dn(dt)}: sequential {seq:.3g}  block {mfma_block(dt)} {blk:.3g}  C {C:.3g}")
    idx = emu_index(cls, K, N, dt)
    acc, mag, bias = [sub(t, idx) for t in gemm_ref(cls, K, N, dt)]
    row_map, scale, residual, H = epilogue_inputs(N, F32)
    for block in (1, mfma_block(dt)):
        for with_bias in (True, False):
            v = emulate_gemm(cls, K, N, dt, block, bias=with_bias)
            b = bias if with_bias else None
            assert worst(v, *chain_ref_bar(acc, mag, b, C, F32)) <= THIRD
            for odt in (F32,) if dt == F32 else (F32, dt):
                s, res, h = sub(scale[:, None].expand(-1, N), idx), sub(residual, idx).to(odt), sub(H, idx).to(odt)
                form = "erf" if block == 1 else "fast"
                emu = _FORMS[form][0]
                assert worst(chain16(v, odt), *chain_ref_bar(acc, mag, b, C, odt)) <= THIRD + (odt != F32) * 2 / 3
                assert worst(chain16(emu(v), odt), *chain_ref_bar(acc, mag, b, C, odt, gelu=form)) <= THIRD + (odt != F32) * 2 / 3
                assert worst(chain16(v, odt, s, res), *chain_ref_bar(acc, mag, b, C, odt, scale=s, residual=res)) <= 1.0
                assert worst(chain16(v, odt, hgrad=h), *chain_ref_bar(acc, mag, b, C, odt, hgrad=h)) <= 1.0


def test_the_sequential_emulation_over_every_output_is_inside_the_bar():
    """f32 operands, K = 64: the chain of FMAs over all 148 k outputs the kernels are measured on (it is what the MI355X returns
    there, module docstring) against a C that came from 3.5 k of them: the factor 3 covers the larger sample"""
    for cls in CLASSES:
        acc, mag, _bias = gemm_ref(cls, 64, NS[1], F32)
        C, seq, _blk = contraction_C(cls, 64, F32)
        full = float(f32_ratio(emulate_gemm_all(cls, 64, NS[1], F32, 1), acc, mag, None).max())
        print(f"{cls} K 64 f32: sequential over 3.5 k outputs {seq:.3g}, over 148 k {full:.3g}, C {C:.3g}")
        assert seq <= full <= 0.6 * C


def test_the_classes_are_what_they_claim():
    for dt in ALL_DT:
        fi = torch.finfo(dt)
        for K in KS:
            a, w = draw("positive", 8, 8, K, dt, 1)
            assert float(a.min()) >= 0 and float(w.min()) >= 0
            a, w = draw("cancel", 64, 64, K, dt, 2)
            cond = (a.double().abs() @ w.double().abs().t()) / (a.double() @ w.double().t()).abs().clamp(min=1e-300)
            print(f"cancel K {K} {_dn(dt)}: median sum |a||w| / |sum a w| {float(cond.median()):.3g}")
            assert float(cond.median()) >= 1e3
            assert torch.equal(a[:, K // 2:], a[:, :K // 2]) and float((w[:, K // 2:].double() + w[:, :K // 2].double()).abs().max()) > 0
            a, w = draw("range", 64, 64, K, dt, 3)
            a0, w0 = draw("range0", 64, 64, K, dt, 3)
            for t in (a, w, a0, w0):
                assert float(t.float().abs().min()) >= fi.smallest_normal and float(t.float().abs().max()) < fi.max
            assert float((a.double() / a0.double()).log2().abs().max()) == 6.0
            assert torch.equal((a.double() * w.double()), (a0.double() * w0.double())), "every product is the twin's, exactly"
            ref, ref0 = a.double() @ w.double().t(), a0.double() @ w0.double().t()
            assert float((ref - ref0).abs().max()) <= 2.0 ** -50 * float((a0.double().abs() @ w0.double().abs().t()).max())
        if dt == F16:
            a, w = draw("subnormal", 64, 64, 768, dt, 4)
            assert float(a.float().abs().max()) < 2.0 ** -14 and float(w.float().abs().min()) >= 256 and float(w.float().abs().max()) <= 1024
            out = (a.double() @ w.double().t()).abs()
            assert float(out.median()) > 2.0 ** -10, "the outputs are ordinary normal numbers"
            assert float((a.float() != 0).float().mean()) > 0.99
        if dt != F32:
            A, W, pre = edge16_case(dt)
            st = pre.to(dt)
            assert int(torch.isfinite(st).sum()) > 100 and bool(torch.isfinite(pre).all())
            if dt == F16:
                assert 2.99e4 <= float(pre.abs().min()) and float(pre.abs().max()) <= 7e4 and int(torch.isinf(st).sum()) > 100
                assert float(pre[0, 0].abs()) == 49200.0 and float(st[0, 0].abs()) == 49216.0, "a tie goes to the even neighbour"
                assert float(st[1, 1].abs()) == 65504.0 and float(pre[2, 2].abs()) == 65520.0 and bool(torch.isinf(st[2, 2]))
            else:
                assert 2.0 ** 126 <= float(pre.abs().min()) and float(pre.abs().max()) < 2.0 ** 128
                assert float(pre[0, 0].abs()) == 20800 * 2.0 ** 113 and float(st[0, 0].float().abs()) == 20736 * 2.0 ** 113
                assert bool(torch.isinf(st[1, 1])) and int(torch.isinf(st).sum()) >= 1
            assert int(((A != 0).sum(1) == 1).all())


def _old_bar(cls, K, N, dt):
    acc, _mag, bias = gemm_ref(cls, K, N, dt)
    return OLD_TOL[dt] * max(1.0, float((acc + bias).abs().max()))


@pytest.mark.parametrize("dt", ALL_DT, ids=_dn)
@pytest.mark.parametrize("K", KS)
def test_the_new_bars_are_20x_below_the_existing_ones(K, dt):
    """benign: the largest element of the new f32 bar against tests/test_gpu_parity.py's tol max(1, max |ref|) of the same output
    (module docstring: 20 x cannot hold for f32 operands, whose existing tol is 2e-5; 4 x is asserted there)"""
    for N in NS:
        acc, mag, bias = gemm_ref("benign", K, N, dt)
        new = float(chain_ref_bar(acc, mag, bias, contraction_C("benign", K, dt)[0], F32)[1].max())
        old = _old_bar("benign", K, N, dt)
        print(f"benign K {K} N {N} {_dn(dt)}: existing bar {old:.3g}  new bar (largest element) {new:.3g}  ratio {old / new:.3g}")
        assert old >= (4 if dt == F32 else 20) * new


OLD_WGRAD_TOL = {F16: 2e-3, BF16: 1.5e-2}                # tests/test_gpu_backward.py test_grouped_wgrad_rows_matches_per_expert_matmul
OLD_COLSUM_TOL = {F16: 2e-3, BF16: 2e-2, F32: 1e-5}      # ... test_group_colsum_many_chunks_and_empty_groups
OLD_GATE_WGRAD_TOL = 1e-5                                # ... test_gate_wgrad_matches_matmul: tol max(1, max |ref|) sqrt(T)


def test_the_other_new_bars_against_the_existing_ones():
    """module docstring, THE 20 x CONDITION: the weight gradients, the router's weight gradient and the column sums, on benign
    data (a N(0, 1), w 0.05 N(0, 1); gate_wgrad: the existing test's own N(0, 1) draws), group by group as the existing tests compare"""
    low = {}
    for dt in (F16, BF16):
        for R in WGRAD_R:
            ref, mag = wgrad_ref("benign", R[0], R[1], dt)
            C = wgrad_C("benign", dt) + 3                        # the split's bar, the wider of the two
            r = min(OLD_WGRAD_TOL[dt] * max(1.0, float(ref[e].abs().max())) / (C * U * float(mag[e].max()))
                    for e, n in enumerate(WGRAD_ROWS) if n)
            low[f"wgrad_rows {R[0]} x {R[1]} {_dn(dt)}"] = (r, 20)
    for T in GATE_TS:
        for xdt in (F32, F16):
            g = gate_case(T, xdt, 1.0)
            old = OLD_GATE_WGRAD_TOL * max(1.0, float(g["dw"].abs().max())) * T ** 0.5
            low[f"gate_wgrad T {T} x {_dn(xdt)}"] = (old / (g["C_dw"] * U * float(g["dw_mag"].max())), 20)
    for dt in ALL_DT:
        _src, _offsets, ref, mag, C = colsum_case("benign", dt)
        r = min(OLD_COLSUM_TOL[dt] * max(1.0, float(ref[e].abs().max())) / (C * U * float(mag[e].max()))
                for e, n in enumerate(COLSUM_GROUPS) if n)
        low[f"group_colsum {_dn(dt)}"] = (r, 4 if dt == F32 else 20)
    for k, (r, need) in low.items():
        print(f"benign {k}: existing bar / new bar (largest element, worst group) {r:.3g}  (asserted: {need})")
    for k, (r, need) in low.items():
        assert r >= need, (k, r, need)


MUTANTS = [(m, dt) for m in "abcdef" for dt in (F16, BF16) if (m, dt) != ("c", F16)]      # (c) is about the bf16 store


@pytest.mark.parametrize("m,dt", MUTANTS, ids=[f"{m}-{_dn(dt)}" for m, dt in MUTANTS])
def test_mutants_are_outside_the_new_bar_and_inside_the_old(m, dt):
    """module docstring, MUTANTS"""
    N = NS[0]
    blockK = mfma_block(dt)

    def run(cls, K, odt=F32, **kw):
        idx = emu_index(cls, K, N, dt)
        acc, mag, bias = [sub(t, idx) for t in gemm_ref(cls, K, N, dt)]
        C = contraction_C(cls, K, dt)[0]
        post = kw.pop("post", lambda v: v)
        got = post(emulate_gemm(cls, K, N, dt, blockK, **kw))
        ref, bar = chain_ref_bar(acc, mag, bias, C, odt)
        new = worst(got, ref, bar)
        old = float((got.double() - ref).abs().max()) / _old_bar(cls, K, N, dt)
        return new, old

    if m == "a":
        new, _ = run("positive", 768, round_every=(64, dt))
        _, old = run("benign", 768, round_every=(64, dt))
    elif m == "b":
        new, old = run("benign", 768, post=lambda v: v.to(dt).float())
    elif m == "c":
        trunc = lambda v: (v.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)      # noqa: E731
        new, old = run("benign", 768, odt=BF16, post=trunc)
    elif m == "d":
        new, old = run("benign", 64, bias_dt=dt)
    elif m == "e":
        new, _ = run("positive", 768, drop_last=True)
        new_b, old_b = run("benign", 768, drop_last=True)
        print(f"mutant e {_dn(dt)}: a whole dropped product on benign: {new_b:.3g} new bars, {old_b:.3g} old bars")
        assert new > 1 and old_b > 1, "a whole dropped product of Gaussian data is outside BOTH bars"
        new2, old = run("benign", 768, drop_last=True, drop_scale=2.0 ** -8)
        assert new2 > 1
    elif m == "f":
        idx = emu_index("benign", 768, N, dt)
        acc, mag, bias = [sub(t, idx) for t in gemm_ref("benign", 768, N, dt)]
        _rm, scale, residual, _H = epilogue_inputs(N, F32)
        s, res = sub(scale[:, None].expand(-1, N), idx), sub(residual, idx)
        v = emulate_gemm("benign", 768, N, dt, blockK)
        ref, bar = chain_ref_bar(acc, mag, bias, contraction_C("benign", 768, dt)[0], F32, scale=s, residual=res)
        assert worst(chain16(v, F32, s, res), ref, bar) <= 1.0
        new, old = worst((v + res) * s, ref, bar), 0.0
    print(f"mutant {m} {_dn(dt)}: {new:.3g} x the new bar, {old:.3g} x the existing bar")
    assert new > 1, "outside the new bar"
    assert old <= 1, "inside the existing bar"


def test_gelu_form_errors_are_what_gemm_hip_quotes():
    erf10, fast6, fast12, grad = gelu_form_error("erf", 10.0), gelu_form_error("fast", 6.0), gelu_form_error("fast"), gelu_form_error("grad", 8.0)
    print(f"gelu_erf |v| < 10: {erf10:.3g} (quoted < 1e-6)   gelu_fast [-6, 6]: {fast6:.3g} (quoted 3.6e-6)  [-12, 12]: {fast12:.3g}"
          f"   gelu_grad [-8, 8]: {grad:.3g}")
    assert erf10 < 1e-6
    assert fast6 <= 3.6e-6 * 1.02
    assert fast12 <= 2 * fast6 and gelu_form_error("erf") < 1e-6


@pytest.mark.parametrize("dt", (F16, BF16), ids=_dn)
@pytest.mark.parametrize("cls", CLASSES)
def test_weight_gradient_emulations(cls, dt):
    C = wgrad_C(cls, dt)
    print(f"wgrad rows {cls} {_dn(dt)}: C {C:.3g}")
    assert 0 < C < (150 if cls == "positive" else 15), "an emulation that changes silently shows here"


@pytest.mark.parametrize("dt", ALL_DT, ids=_dn)
@pytest.mark.parametrize("cls", ("positive", "cancel"))
def test_colsum_emulation_and_a_cancelling_column(cls, dt):
    """the bar is relative to the column's sum of magnitudes, which a cancelling column is fair against (what it is NOT fair
    against: a bar relative to the result, test_value_regimes_host.py test_a_cancelling_column_sum_is_outside_the_bar_for_any_f32_sum)"""
    src, offsets, ref, mag, C = colsum_case(cls, dt)
    print(f"group_colsum {cls} {_dn(dt)}: C {C:.3g}")
    assert C < 8
    if cls == "cancel":
        assert float((mag[0] / ref[0].abs().clamp(min=1e-300)).median()) > 1e3


def test_reduction_emulations():
    for T in GATE_TS:
        for xdt in (F32, F16):
            r = gate_case(T, xdt)
            print(f"gate T {T} x {_dn(xdt)}: C dWg {r['C_dw']:.3g}  dbg {r['C_db']:.3g}  dx {r['C_dx']:.3g}")
            assert max(r["C_dw"], r["C_db"]) < 6 and r["C_dx"] < 15
    for ydt in (F16, F32):
        r = combine_case(ydt)
        print(f"rowdot / gather_combine y {_dn(ydt)}: C {r['C_dot']:.3g} / {r['C_mix']:.3g}")
        assert r["C_dot"] < 20 and r["C_mix"] <= 8, "a few u of sum |score| |y|"
    r = switch_aux_case()
    print(f"switch_aux: C aux {r['C_aux']:.3g} coef {r['C_coef']:.3g}")
    assert r["C_aux"] < 8 and r["C_coef"] <= 4.5
    for regime, (_, dts) in SUMSQ_REGIMES.items():
        for dt in dts:
            grad, ref, C = sumsq_case(regime, dt)
            print(f"grad_sumsq {regime} {_dn(dt)}: sum {float(ref):.3g}  C {C:.3g}")
            assert C < (15 if dt == F16 else 5) and (regime != "floor" or 2.0 ** -126 < float(ref) < 2.0 ** -100)
