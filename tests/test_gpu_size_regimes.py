"""Every kernel that carries 32-bit address arithmetic, across the sizes at which an address stops fitting in 32 bits.

THE TABLE (B = bytes, el = elements; "rerouted" = the library or its Python wrapper picks other code there, "enforced" = an error)

entry point                      the 32-bit quantity (where the code says so)                       boundary                      sizes run here
-------------------------------  -----------------------------------------------------------------  ----------------------------  ----------------------------------------
smoe_grouped_gemm 9-14, A        a_src: byte offset of a row of A (gemm_persistent.h setup)         m_rows_max K 2 = 2^32 B:      1a  M = 524,287 (persistent), K = 4,096, N = 256
                                                                                                    rerouted to 4-8 (gemm.hip)    1b  M = 526,005 (one workgroup per tile)
smoe_grouped_gemm_gelu_keep      the same                                                           returns -1 there              1b  the wrapper's two-step form
smoe_grouped_gemm 9-14, W        w_src: byte offset of a row of W                                   E N K 2 = 2^32 B: rerouted    1c  E N K = 7 x 65,536 x 4,096 (3.5 GiB: one
                                                                                                                                      more expert is 4 GiB) and 8 x 65,544 x 4,096
smoe_grouped_gemm 9-13, 16-bit   per-tile buffer descriptor from a 64-bit base (direct store)      none (64-bit base)            1d  out 526,005 x 4,096 (4.01 GiB), K = 64;
  direct-store epilogue                                                                                                               EPI_NONE, EPI_GELU, gelu_keep; 9 == 14
smoe_grouped_gemm 9, f32 out     buffer descriptor over all of out                                  out_rows N 4 = 2^31 B:        1e  out_rows 524,287 / 524,288, N = 1,024; f16, bf16
                                                                                                    rerouted to flat addressing   1f  out_rows 1,048,909 (4.00 GiB + 333 rows)
smoe_grouped_gemm 9-14, a_gather a_src of the UN-PERMUTED A, whose row count the ABI never sees     A.numel() 2 = 2^32 B: the     1g  A 525,288 x 4,096, 640 gathered rows,
  (and smoe_expert_ffn's X)                                                                         caller's duty; ops.grouped_       a_div 1 and 2, variants 9, 10, 14; group_end
                                                                                                    gemm reroutes to 4-8              raises; ops.expert_ffn returns None; f16, bf16
smoe_grouped_gemm, group_end     persistent kernel only                                             operands of 4 GiB: enforced   1h  A 524,287 x 4,096 runs, 524,288 raises; f16, bf16
smoe_grouped_wgrad_rows          a_rowoff / w_rowoff: ELEMENT offsets (gemm.hip MODE 2)             n_rows R1 = 2^32 el: caller's 1i  n_rows R1 = 2^32 - R1 (token-major) and
                                                                                                    duty; ops.grouped_wgrad_rows      2^32 (K-major), R1 = 4,096, R2 = 8
                                                                                                    reroutes to smoe_grouped_wgrad
smoe_gelu                        (int64_t) i                                                        none                          f16 n = 2^32 + 104, bf16 n = 2^31 + 104
smoe_cast                        (int64_t) i                                                        none                          f32 -> f16 n = 2^31 + 5, f16 -> bf16 n = 2^32 + 5
smoe_scatter_rows[_fill]         s * (int64_t) d                                                    none                          2^21 + 77 slots x 1,024, plain / fill / scale
smoe_gather_combine              t * (int64_t) d, slot * (int64_t) d                                none                          2^21 + 77 tokens x 1,024, k = 2, residual
smoe_gather_combine_ln           the same                                                           none                          2^21 + 77 tokens x 1,024, k = 1
smoe_rowdot                      slot * (int64_t) d                                                 none                          2^21 + 77 entries x 1,024, k = 2
smoe_layernorm                   t * (int64_t) d                                                    none                          d = 1,024: 2^21 + 77 rows; d = 192: 11,185,810 rows
smoe_layernorm_rows              t * row_stride                                                     none                          2^21 + 77 rows, row stride 1,032
smoe_patchify_cast               o / row_len                                                        none                          2,731 images 3 x 512 x 512, 16 x 16 patches
smoe_gate_dgrad                  t * (int64_t) d                                                    none                          2^21 + 77 rows x 1,024, E = 4, f16 out
smoe_router_topk                 t * (int64_t) d                                                    none                          2,796,302 rows x 768, E = 8, k = 2
smoe_ln_router_topk              t * (int64_t) d                                                    none                          2,796,302 x 768, E = 8, k = 2; 2^21 + 77 x 1,024, E = 32
smoe_gate_ln_router              t * (int64_t) d                                                    none                          2,796,302 rows x 768, E = 8, k = 1
smoe_embed_ln                    t * (int64_t) d                                                    none                          1,048,653 images of one patch, d = 1,024
smoe_layernorm_bwd               t * (int64_t) d                                                    none                          2^21 + 77 rows x 1,024, dy f16
smoe_gate_ln_bwd                 t * (int64_t) d                                                    none                          2^21 + 77 rows x 1,024, g_f f16, no g_out
smoe_attention_fwd / _bwd        (int64_t) b * N * tok_stride                                       none                          B = 43,700, N = 16, H = 16: qkv 2^31 + 458,752 el
smoe_soft_ce_bwd                 gridDim.y = B (loss.hip)                                           B = 65,535: enforced          B = limit + 3, C = 8
smoe_soft_ce_fwd                 gridDim.x = B                                                      B = 2^31: enforced            B = limit + 3, C = 8 (runs, float64)
smoe_transpose_cast              gridDim.y = R / 64, gridDim.z = B                                  65,535 each: enforced         R = 64 (limit + 1), C = 64
smoe_transpose_pad               gridDim.y = Lp / 64                                                65,535: enforced (NEW here)   Lp / 64 = 65,535 (runs) and limit + 2
smoe_group_colsum                gridDim.y = chunks of 256 rows + E                                 65,535: enforced              256 (limit + 1) rows, C = 64
smoe_gate_wgrad                  gridDim.y = chunks of 256 rows                                     65,535: enforced              256 (limit + 1) rows, C = 64, E = 4

limit = the smaller of hipDeviceAttributeMaxGridDimY / Z of the device, read through hipDeviceGetAttribute: 65,536 on an MI355X (the
library caps at 65,535).

Left out, and why:
  * the optimizer, EMA and sumsq launches: no parameter tensor approaches 2^31 elements, and the four f32 streams of one step at that
    size need more than 32 GiB.
  * the four dispatch plans, smoe_ep_pack_headers, the loss and the Mixup kernels: their ABI rejects n >= 2^31 (per sample: C H W >=
    2^31; the padded plan also E slot_rows >= 2^31); test_entry_points_that_refuse_2p31_say_so asserts those rejections with pointers
    that are never dereferenced.  smoe_ep_unpack_headers takes no row count at all (see that test).

Method.  Inputs are i.i.d. normal values filled in place in chunks (no periodic pattern: a read displaced by 2^31 or 2^32 lands on
other numbers); outputs are NaN-filled or poisoned.  Assertion A: the large run equals, bit for bit, the same entry point on pieces
that lie below every boundary (GEMMs: pieces cut at multiples of 1,280 rows = lcm(256, 320) from each group's first row, explicit
plan variants 10 / 5).  Assertion B: a float64 reference written with torch ops on windows of 640 rows -- the first, the last and one
centred on every byte / element offset 2^31 and 2^32 that the tensor contains -- or on the whole output where that is small.
Copies and casts are compared with torch over the whole tensor.
Bars.  Where the existing test of a kernel has a bar within 3 x of the error measured at these shapes, it is used and named.  Most are
set for other K / d / row counts and are wider than that here; then the bar is worked out where it is used and the test says how it
differs from the existing one: a 16-bit output is held to the half ulp of its store (store_bar), an f32 output to a count of the
roundings that reach it or, where such a count is far from the error, to 3 x the error measured on an MI355X.

MEASURED on an MI355X (maxGridSize y, z = 65,536, 65,536; 0 skips).  Largest error / bar per group of rows of the table:
  grouped GEMM, 16-bit out (store_bar; 1a, 1b, 1c, 1d, 1g, 1h)   0.80, f16 and bf16 alike: half an ulp of the store at max |ref| is attained
                                                     (K = 4,096: max |diff| 3.9e-3 f16 / 3.1e-2 bf16 at |value| in [8, 16)); 1d 0.77 - 0.80
  gelu_keep's gelu(H) in its two-step form (1b)      0.376 (two roundings: 2.13 half ulps allowed, one attained)
  grouped GEMM, K = 64, f32 out (1e, 1f)             0.32 - 0.37 of 6 x 2^-24 S (f16 0.373, bf16 0.354)
  wgrad rows (1i)                                    max |diff| / max |ref| <= 1.25e-5 (f16 and bf16, both paths): 0.35 of WGRAD_BAR
  gelu 0.97; gather_combine 0.998 (the 16-bit store's half ulp is the bound); gather_combine_ln out 0.64, xn 0.80; rowdot 0.335
  layernorm 0.80 (d = 1,024 and d = 192); embed_ln 0.80; layernorm_rows 0.34 (max |diff| 1.34e-7 max |ref|); gate_dgrad 0.42
  layernorm_bwd: relative L2 dx 6.28e-8, dgamma 4.48e-7, dbeta 1.11e-7 (LNB_BARS: 0.35, 0.34, 0.34)
  gate_ln_bwd: relative L2 dx 7.57e-8, dz 1.32e-7, dgamma 4.19e-7, dbeta 4.03e-7, dgate_w 4.55e-7; the scalar sums 2.02e-7, 7.60e-8
               (GLNB_BARS: 0.34, 0.34, 0.52, 0.50, 0.57; 0.34, 0.35)
  routers: logits 7.15e-7, scores 2.38e-7; fused LayerNorm 9.69e-7, its scores 5.36e-7 (ROUTER_BARS: 0.34, 0.34, 0.33, 0.34)
  attention: out 0.91; lse 2.97e-4, dq / dk / dv relative L2 3.45e-4, max |diff| / max |ref| 5.45e-4 (ATTN_BARS: 0.34, 0.34, 0.34)
  soft_ce_fwd at B = 65,539: row error 1.04e-6 (0.35), mean 4.86e-8 (0.34)
No bar above is more than 3 x the largest error measured for it, except store bounds that are attained.
Copies, casts, scatters, the f32 embedding stream, routing indices and every assertion A: bit-exact.
Wall time of the module: 53 tests in 20 s in one process (each test about 5 s at the most, most under 0.5 s).
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import moe_oracle as mo  # noqa: E402
from slim_switch_moe_vit_amd import _lib, ops  # noqa: E402
from test_gpu_launch_regimes import (BF16, DEV, F16, F32, HALF_ULP, TINY, dgen, nans, pieces, poison, rel,  # noqa: E402
                                     same_bits, worst)

G31, G32 = 2 ** 31, 2 ** 32
GIB = 2 ** 30
T_BIG = 2 ** 21 + 77          # rows of 1,024: 2^31 + 78,848 elements; 16-bit rows cross 2^31 B at row 2^20 and 2^32 B at row 2^21
STEP = 1280                   # lcm of the two tile heights
MANTISSA = {F16: 11, BF16: 8}


def store_bar(ref: torch.Tensor, dt, roundings: float = 1.0) -> float:
    """The bar of the 16-bit outputs of the GEMM, LayerNorm and attention here: max |diff| <= 1.25 x `roundings` x half an ulp of dt at max |ref|.  The kernels compute in
    f32 and round once on the store, so half an ulp at the largest magnitude is attained; the quarter on top is for the f32 error
    that carries a value across a rounding boundary (worst-case operation counts are not used: at K = 4,096 they are 8 x the store's
    half ulp, and a bar may be at most 3 x the measured error).  This is tighter than the existing tests' tol x max(1, max |ref|)
    (tol 1e-3 f16 / 8e-3 bf16 for the GEMM, 2e-3 for LayerNorm, 2e-3 for attention), which it replaces in this module."""
    top = float(ref.abs().max())
    return 1.25 * roundings * 2.0 ** (math.floor(math.log2(top)) - MANTISSA[dt])


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    torch.cuda.empty_cache()


def need(gib: float) -> None:
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB free on the device, {gib} GiB needed")


def randn_(t: torch.Tensor, seed: int, scale: float = 1.0, shift: float = 0.0) -> torch.Tensor:
    """i.i.d. normal values written in place, 2^28 elements at a time"""
    flat, g = t.view(-1), dgen(seed)
    for a in range(0, flat.numel(), 1 << 28):
        flat[a:a + (1 << 28)].normal_(shift, scale, generator=g)
    return t


def empty(shape, dt) -> torch.Tensor:
    return torch.empty(shape, dtype=dt, device=DEV)


def i32(v) -> torch.Tensor:
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def windows(rows: int, geometries, W: int = 640):
    """Row ranges of W rows: the first, the last, and one centred on every offset 2^31 / 2^32 (in bytes and in elements) of every
    (elements per row, bytes per element) geometry given -- the operands and outputs that share these rows."""
    centres = [W // 2, rows - W // 2]
    for row_elems, esize in geometries:
        for c in (G31, G32):
            if rows * row_elems > c:
                centres.append(c // row_elems)
            if rows * row_elems * esize > c:
                centres.append(c // (row_elems * esize))
    out = set()
    for c in centres:
        lo = max(0, min(c - W // 2, rows - W))
        out.add((lo, min(rows, lo + W)))
    return sorted(out)


def gelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def equal_in_chunks(got: torch.Tensor, ref_of, n: int, step: int = 1 << 27) -> None:
    """got[a:b] == ref_of(a, b) bit for bit over all of [0, n)"""
    for a in range(0, n, step):
        b = min(n, a + step)
        assert same_bits(got[a:b], ref_of(a, b)), f"[{a}:{b}) differs from torch"


# ================================================================================================ 1. grouped GEMM regimes
def _gemm_operands(M, K, N, E, dt, seed):
    A = randn_(empty((M, K), dt), seed)
    W = randn_(empty((E, N, K), dt), seed + 1, 0.05)          # the scales of test_grouped_gemm_matches_fp64_reference
    bias = randn_(empty((E, N), F32), seed + 2, 0.1)
    return A, W, bias


def _gemm_rows64(A, W, bias, groups, experts, lo, hi, epi=ops.EPI_NONE):
    """float64 of rows [lo, hi): NaN where no group owns the row"""
    ref = torch.full((hi - lo, W.shape[1]), float("nan"), dtype=torch.float64, device=DEV)
    for (a, b), e in zip(groups, experts):
        s, t = max(a, lo), min(b, hi)
        if s < t:
            ref[s - lo:t - lo] = A[s:t].double() @ W[e].double().t() + bias[e].double()
    return gelu64(ref) if epi == ops.EPI_GELU else ref


def _gemm_anchor(name, got, A, W, bias, groups, experts, epi, wins, dt, roundings=1.0):
    """assertion B at store_bar (test_grouped_gemm_matches_fp64_reference's bar is 3.4 - 4 x the error at these shapes); returns
    error / bar"""
    err, top = 0.0, torch.zeros((), dtype=torch.float64, device=DEV)
    for lo, hi in wins:
        ref = _gemm_rows64(A, W, bias, groups, experts, lo, hi, epi)
        live = ~torch.isnan(ref[:, 0])
        g_ = got[lo:hi][live].double()
        assert not bool(torch.isnan(g_).any()), f"{name}: NaN (an unwritten row?) in rows [{lo}, {hi})"
        err = max(err, float((g_ - ref[live]).abs().max()))
        top = torch.maximum(top, ref[live].abs().max())
    ratio = err / store_bar(top, dt, roundings)
    print(f"{name}: max |diff| {err:.3e}, max |ref| {float(top):.2f}, error / bar = {ratio:.3f} over {len(wins)} windows")
    assert ratio <= 1.0, (name, err, float(top))
    return ratio


def _gemm_pieces_equal(name, big, A, W, bias, groups, experts, epi, variant, step):
    """assertion A: every group's rows in pieces of `step` rows (a multiple of both tile heights) as one-group GEMMs"""
    for (a, b), e in zip(groups, experts):
        for s in range(a, b, step):
            t = min(b, s + step)
            o = nans((t - s, W.shape[1]), big.dtype)
            ops.grouped_gemm(A[s:t], W[e:e + 1], bias[e:e + 1], i32([0, t - s]), epi, out=o, variant=variant)
            assert same_bits(o, big[s:t]), f"{name}: rows [{s}, {t}) differ from the GEMM of that piece alone"
            del o


def _piece_rows(*row_bytes) -> int:
    return ((G31 - 1) // max(row_bytes)) // STEP * STEP


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("M,cuts", [(524287, (0, 150001, 400000, 524287)), (524288 + 1717, (0, 100000, 525000, 524288 + 1717))],
                         ids=["1a-below-4GiB", "1b-past-4GiB"])
def test_gemm_operand_A_on_both_sides_of_4GiB(M, cuts, dt):
    """1a: persistent kernel, the middle group straddles row 262,144 (2 GiB).  1b: the same plan in the one-workgroup-per-tile family,
    the middle group straddles rows 262,144 and 524,288 (4 GiB = 2^31 elements).  Variants 9 == 4 and 10 == 5 bit for bit; variant
    10 == the persistent kernel on pieces; float64 on the windows.  bf16: variants 9 == 4 and float64 only.
    1b: smoe_grouped_gemm_gelu_keep returns -1 and the wrapper gives EPI_NONE + smoe_gelu, bit for bit."""
    need(8)
    K, N, E = 4096, 256, 3
    A, W, bias = _gemm_operands(M, K, N, E, dt, M % 1000)
    offsets, groups, experts = i32(cuts), list(zip(cuts[:-1], cuts[1:])), list(range(E))
    wins = windows(M, [(K, 2), (N, 2)])
    outs = {}
    for v in ((9, 4, 10, 5) if dt == F16 else (9, 4)):
        outs[v] = ops.grouped_gemm(A, W, bias, offsets, ops.EPI_NONE, out=nans((M, N), dt), variant=v)
    assert same_bits(outs[9], outs[4]), "variant 9 differs from variant 4"
    _gemm_anchor(f"A {M} x {K} {dt} variant 9", outs[9], A, W, bias, groups, experts, ops.EPI_NONE, wins, dt)
    if dt == F16:
        assert same_bits(outs[10], outs[5]), "variant 10 differs from variant 5"
        _gemm_anchor(f"A {M} x {K} {dt} variant 10", outs[10], A, W, bias, groups, experts, ops.EPI_NONE, wins, dt)
        _gemm_pieces_equal("variant 10", outs[10], A, W, bias, groups, experts, ops.EPI_NONE, 10, _piece_rows(K * 2, N * 2))
    if M * K * 2 >= G32:
        pre_ref = outs[9]
        pre0, act0 = nans((M, N), dt), nans((M, N), dt)
        rc = _lib.load().smoe_grouped_gemm_gelu_keep(A.data_ptr(), W.data_ptr(), bias.data_ptr(), offsets.data_ptr(), None, None, E, E, M, K, N,
                                                     ops.dtype_code(dt), pre0.data_ptr(), act0.data_ptr(), ops._stream(A))
        assert rc == -1, "an A of 4 GiB is outside the fused two-store epilogue: -1 expected"
        assert bool(torch.isnan(pre0).all()) and bool(torch.isnan(act0).all()), "-1 must come back before anything is written"
        del pre0, act0
        poison(M * N * 2, M * N * 2)
        pre, act = ops.grouped_gemm_gelu_keep(A, W, bias, offsets)
        assert same_bits(pre, pre_ref), "gelu_keep's H differs from EPI_NONE"
        assert same_bits(act, ops.gelu(pre_ref)), "gelu_keep's gelu(H) differs from smoe_gelu of EPI_NONE"
        # gelu(H) of the ROUNDED H against gelu in float64 of the float64 GEMM: H's half ulp through a slope of at most 1.13, then the
        # store's own half ulp
        _gemm_anchor(f"gelu_keep {dt}", act, A, W, bias, groups, experts, ops.EPI_GELU, wins, dt, roundings=2.13)


@pytest.mark.parametrize("E,N,dt", [(7, 65536, F16), (8, 65544, F16), (8, 65544, BF16)], ids=["below-f16", "past-f16", "past-bf16"])
def test_gemm_operand_W_on_both_sides_of_4GiB(E, N, dt):
    """1c: two groups of one row each on the first and the last expert.  `below`: (E + 1) N K 2 = 2^32, so the last expert ends
    N K 2 bytes under 4 GiB (persistent kernel); `past`: 4 GiB + 32 KiB (one workgroup per tile).  Float64 on all of the (small)
    output; variants 9 == 4, 10 == 5; variant 10 == the persistent kernel on each expert's own 512 MiB of W."""
    need(6)
    K = 4096
    assert (E * N * K * 2 >= G32) == (E == 8) and (E == 8 or (E + 1) * N * K * 2 == G32)
    A, W, bias = _gemm_operands(2, K, N, E, dt, E)
    offsets, ge, experts = i32([0, 1, 2]), i32([0, E - 1]), [0, E - 1]
    outs = {v: ops.grouped_gemm(A, W, bias, offsets, ops.EPI_NONE, out=nans((2, N), dt), variant=v, group_expert=ge) for v in (9, 4, 10, 5)}
    assert same_bits(outs[9], outs[4]) and same_bits(outs[10], outs[5])
    for r, e in enumerate(experts):
        ref = torch.cat([W[e, c:c + 8192].double() @ A[r].double() + bias[e, c:c + 8192].double() for c in range(0, N, 8192)])
        for v in (9, 10):
            err, bar = float((outs[v][r].double() - ref).abs().max()), store_bar(ref, dt)
            print(f"W {E} x {N} x {K} {dt} variant {v} expert {e}: max |diff| {err:.3e}, error / bar = {err / bar:.3f}")
            assert err <= bar, (v, e, err, bar)
        o = ops.grouped_gemm(A[r:r + 1], W[e:e + 1], bias[e:e + 1], i32([0, 1]), ops.EPI_NONE, out=nans((1, N), dt), variant=10)
        assert same_bits(o[0], outs[10][r]), f"expert {e}: differs from the GEMM on that expert's weights alone"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_gemm_16bit_output_past_4GiB(dt):
    """1d: K = 64, so that the direct-store epilogue is all there is; out is 526,005 x 4,096 (4.01 GiB), the middle group straddles
    the output's 2 GiB and 4 GiB.  EPI_NONE and EPI_GELU: variant 10 == pieces, float64 windows, 9 == 14; gelu_keep: == pieces, windows.
    bf16: EPI_NONE only."""
    need(14)
    K, N, E = 64, 4096, 3
    M = 524288 + 1717
    cuts = (0, 100000, 525000, M)
    A, W, bias = _gemm_operands(M, K, N, E, dt, 41)
    offsets, groups, experts = i32(cuts), list(zip(cuts[:-1], cuts[1:])), list(range(E))
    wins, step = windows(M, [(N, 2)]), _piece_rows(N * 2)
    for epi, name in ((ops.EPI_NONE, "none"), (ops.EPI_GELU, "gelu")):
        if dt == BF16 and epi != ops.EPI_NONE:
            continue
        o10 = ops.grouped_gemm(A, W, bias, offsets, epi, out=nans((M, N), dt), variant=10)
        _gemm_anchor(f"out {M} x {N} {dt} {name} variant 10", o10, A, W, bias, groups, experts, epi, wins, dt)
        _gemm_pieces_equal(f"{name} variant 10", o10, A, W, bias, groups, experts, epi, 10, step)
        del o10
        o9 = ops.grouped_gemm(A, W, bias, offsets, epi, out=nans((M, N), dt), variant=9)
        o14 = ops.grouped_gemm(A, W, bias, offsets, epi, out=nans((M, N), dt), variant=14)
        assert same_bits(o9, o14), f"{name}: variant 9 (direct store) differs from variant 14 (staged)"
        _gemm_anchor(f"out {M} x {N} {dt} {name} variant 9", o9, A, W, bias, groups, experts, epi, wins, dt)
        del o9, o14
    if dt == F16:
        poison(M * N * 2, M * N * 2)
        pre, act = ops.grouped_gemm_gelu_keep(A, W, bias, offsets)
        _gemm_anchor("gelu_keep H", pre, A, W, bias, groups, experts, ops.EPI_NONE, wins, dt)
        _gemm_anchor("gelu_keep gelu(H)", act, A, W, bias, groups, experts, ops.EPI_GELU, wins, dt)      # (gelu of the f32 H here)
        for (a, b), e in zip(groups, experts):
            for s in range(a, b, step):
                t = min(b, s + step)
                poison((t - s) * N * 2, (t - s) * N * 2)
                p_, a_ = ops.grouped_gemm_gelu_keep(A[s:t], W[e:e + 1], bias[e:e + 1], i32([0, t - s]))
                assert same_bits(p_, pre[s:t]) and same_bits(a_, act[s:t]), f"gelu_keep rows [{s}, {t}) differ from that piece alone"
                del p_, a_


F32_OUT_ROUNDINGS = 6


@pytest.mark.parametrize("inplace,dt", [(False, F16), (True, F16), (False, BF16)], ids=["residual-f16", "residual-in-place-f16", "residual-bf16"])
@pytest.mark.parametrize("out_rows", [524287, 524288, 1048576 + 333], ids=["1e-below-2GiB", "1e-at-2GiB", "1f-past-4GiB"])
def test_gemm_f32_output_on_both_sides_of_2GiB_and_past_4GiB(out_rows, inplace, dt):
    """1e / 1f: 2,000 GEMM rows stored through row_map, with row_scale and a residual, to the first rows, the last rows and the rows
    around every 2 GiB / 4 GiB offset of an f32 output of out_rows x 1,024.  Below 2 GiB variant 9 stores through buffer descriptors,
    from 2 GiB on with flat addresses: variants 9, 14 and 4 give the same bits everywhere; rows no slot maps to keep their bytes; the
    mapped rows equal the same GEMM stored into a compact 2,000-row output (assertion A) and float64 (assertion B, all 2,000 rows, at a
    bound worked out below: test_grouped_gemm_matches_fp64_reference's bar is set for 16-bit stores, 10,000 x the error of an f32 one)."""
    need(20)
    K, N, E, M = 64, 1024, 3, 2000
    cuts = (0, 900, 901, M)
    A, W, bias = _gemm_operands(M, K, N, E, dt, out_rows % 997)
    offsets, groups, experts = i32(cuts), list(zip(cuts[:-1], cuts[1:])), list(range(E))
    cand = torch.cat([torch.arange(lo, hi, device=DEV) for lo, hi in windows(out_rows, [(N, 4)], W=1024)]).unique()
    assert cand.numel() >= M and int(cand[0]) == 0 and int(cand[-1]) == out_rows - 1
    g = dgen(out_rows)
    inner = cand[1:-1][torch.randperm(cand.numel() - 2, generator=g, device=DEV)[:M - 2]]
    row_map = torch.cat([cand[:1], cand[-1:], inner])[torch.randperm(M, generator=g, device=DEV)].contiguous()
    assert row_map.unique().numel() == M
    row_scale = torch.rand(out_rows, generator=g, device=DEV) * 0.75 + 0.25
    res0 = randn_(empty((out_rows, N), F32), out_rows % 991)

    def run(variant, rmap, scale, res, rows):
        out = res.clone() if inplace else nans((rows, N), F32)
        return ops.grouped_gemm(A, W, bias, offsets, ops.EPI_NONE, out=out, variant=variant, row_map=rmap, row_scale=scale,
                                residual=out if inplace else res)
    o9 = run(9, row_map, row_scale, res0, out_rows)
    for v in (14, 4):
        assert same_bits(run(v, row_map, row_scale, res0, out_rows), o9), f"variant {v} differs from variant 9"
    expect = res0.clone() if inplace else nans((out_rows, N), F32)
    expect[row_map] = o9[row_map]
    assert same_bits(expect, o9), "a row that no slot maps to was written"
    del expect
    small = run(9, torch.arange(M, device=DEV), row_scale[row_map].contiguous(), res0[row_map].contiguous(), M)
    assert same_bits(small, o9[row_map]), "the mapped rows differ from the same GEMM stored to a compact output"
    prod = _gemm_rows64(A, W, bias, groups, experts, 0, M)
    ref = res0[row_map].double() + row_scale[row_map].double()[:, None] * prod
    # An f32 store leaves only the accumulation.  The products of 16-bit operands are exact in f32.  The kernel issues
    # mfma_f32_16x16x32, so two instructions cover K = 64; how one instruction rounds inside is not documented, and two roundings
    # each are allowed here (4).  The bias and the scaled add onto the residual bring F32_OUT_ROUNDINGS = 6, each within 2^-24 of a
    # partial result whose magnitude never exceeds S = |residual| + scale (sum |a w| + |bias|): |error| <= 6 x 2^-24 S.  Largest
    # error / bound measured: see MEASURED.  (One rounding per product, (K + 3) 2^-24 S, would be 30 x the measured error.)
    mag = res0[row_map].double().abs() + row_scale[row_map].double()[:, None] * torch.cat(
        [A[a:b].double().abs() @ W[e].double().abs().t() + bias[e].double().abs() for (a, b), e in zip(groups, experts)])
    w = worst((o9[row_map].double() - ref).abs(), F32_OUT_ROUNDINGS * 2.0 ** -24 * mag)
    print(f"f32 out {out_rows} x {N} {dt} in place {inplace}: error / bound = {w:.3f}")
    assert w <= 1.0, w


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_gemm_gathered_rows_of_an_A_past_4GiB(dt):
    """1g (finding 1): the persistent kernel's byte offsets are taken from the UN-PERMUTED A, whose row count smoe_grouped_gemm never
    learns: 640 gathered rows pass its 4 GiB check whatever A's size, and row 524,288 + i of a [525,288, 4,096] A would be read as
    row i.  ops.grouped_gemm sends such an A to the same plan in variants 4-8; float64 on every row, for a_div 1 and 2."""
    need(6)
    rows, K, N, E, M = 525288, 4096, 256, 2, 640
    A, W, bias = _gemm_operands(rows, K, N, E, dt, 17)
    src = torch.linspace(0, rows - 1, M, device=DEV).round().long()
    assert int(src[0]) == 0 and int(src[-1]) == rows - 1 and int((src >= 524288).sum()) >= 1 and src.unique().numel() == M
    src = src[torch.randperm(M, generator=dgen(3), device=DEV)]
    offsets, groups = i32([0, 320, M]), [(0, 320), (320, M)]
    ref = _gemm_rows64(A[src], W, bias, groups, [0, 1], 0, M, ops.EPI_GELU)
    base = {}
    for a_div in (1, 2):
        a_gather = (src * a_div + (torch.arange(M, device=DEV) % a_div)).contiguous()
        for v in (9, 10, 14, 5):
            out = ops.grouped_gemm(A, W, bias, offsets, ops.EPI_GELU, out=nans((M, N), dt), variant=v, a_gather=a_gather, a_div=a_div)
            err, bar = float((out.double() - ref).abs().max()), store_bar(ref, dt)
            print(f"gathered A past 4 GiB {dt}, a_div {a_div} variant {v}: max |diff| {err:.3e}, error / bar = {err / bar:.3f}")
            assert err <= bar, (a_div, v, err, bar)
            assert same_bits(out, base.setdefault(v == 9 or v == 14, out)), "variants of one plan differ"
        with pytest.raises(RuntimeError, match="under 4 GiB"):
            ops.grouped_gemm(A, W, bias, i32([0, 320]), ops.EPI_GELU, out=nans((M, N), dt), variant=9, a_gather=a_gather, a_div=a_div,
                             group_end=i32([300, M]))
    W2 = randn_(empty((E, 64, N), dt), 5, 0.05)
    assert ops.expert_ffn(A, W, bias, W2, None, offsets, nans((M, 64), F32), a_gather=src.contiguous()) is None, \
        "an X of 4 GiB with a_gather is outside the fused launch: None (= issue the two GEMMs) expected"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_gemm_separate_row_ranges_below_4GiB_and_refused_at_4GiB(dt):
    """1h: group_end on an A one row under 4 GiB -- rows between the ranges hold NaN in A and a sentinel in out, neither matters /
    changes (the property of test_grouped_gemm_separate_row_ranges_touch_only_their_rows), float64 on the windows; at 4 GiB the
    documented error."""
    need(6)
    M, K, N, E = 524287, 4096, 256, 3
    A, W, bias = _gemm_operands(M, K, N, E, dt, 23)
    starts, ends = (0, 150001, 400000), (149000, 399000, M)
    groups = list(zip(starts, ends))
    A[149000:150001] = float("nan")
    A[399000:400000] = float("nan")
    for v in (9, 10):
        out = torch.full((M, N), 7.0, dtype=dt, device=DEV)
        ops.grouped_gemm(A, W, bias, i32(starts), ops.EPI_NONE, out=out, variant=v, group_end=i32(ends))
        assert bool((out[149000:150001] == 7.0).all()) and bool((out[399000:400000] == 7.0).all()), "padding rows were written"
        _gemm_anchor(f"group_end variant {v}", out, A, W, bias, groups, [0, 1, 2], ops.EPI_NONE,
                     windows(M, [(K, 2)]) + [(148700, 149340), (399700, 400340)], dt)
        del out
    del A
    A4 = empty((524288, K), dt)      # never read: the call is refused before any launch
    with pytest.raises(_lib.SlimMoEError, match="group_end"):
        ops.grouped_gemm(A4, W, bias, i32(starts), ops.EPI_NONE, out=nans((524288, N), dt), variant=9, group_end=i32((149000, 399000, 524288)))


# The products of 16-bit operands are exact in f32 for f16 and bf16 alike, so one bar serves both: what is left is the f32 accumulation
# of k = 300,000 - 400,000 products of magnitude 0.25 into sums of magnitude sqrt(k) / 4 = 150.  A worst-case count (k 2^-24 of the sum
# of magnitudes) is 1,000 x the error; the bar is 3 x the largest max |diff| / max(1, max |ref|) measured on an MI355X (see MEASURED).
WGRAD_BAR = 3.6e-5


def _wgrad64(P, Q, cuts):
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc = torch.zeros((P.shape[1], Q.shape[1]), dtype=torch.float64, device=DEV)
        for s in range(a, b, 32768):
            t = min(b, s + 32768)
            acc += P[s:t].double().t() @ Q[s:t].double()
        out.append(acc)
    return torch.stack(out)


@pytest.mark.parametrize("n_rows,dt", [(2 ** 20 - 1, F16), (2 ** 20 - 1, BF16), (2 ** 20, F16)], ids=["token-major-f16", "token-major-bf16", "k-major-f16"])
def test_wgrad_rows_on_both_sides_of_2p32_elements(n_rows, dt):
    """1i (finding 2): R1 = 4,096, so P has 2^32 - 4,096 elements (the token-major kernel: 32-bit element offsets, whose last K-tile
    computes offsets past 2^32 for the rows behind the last range -- those rows read the zero page) or 2^32 (ops.grouped_wgrad_rows
    takes the K-major path).  Float64 per expert on all of out.  The contraction runs over 300,000 - 400,000 rows, a length no other
    wgrad test comes near, so the bar is WGRAD_BAR and not that of test_grouped_wgrad_rows_matches_per_expert_matmul (2e-3 f16, 1.5e-2
    bf16: 170 x and 1,250 x the error here).  Below 2^32 the two paths agree to that test's 1e-3 max(1, max |ref|)."""
    need(20)
    R1, R2 = 4096, 8
    cuts = (0, 300001, 700030, n_rows)
    assert (n_rows - cuts[2]) % 64 and (cuts[1] - cuts[0]) % 64 and (n_rows * R1 >= G32) == (n_rows == 2 ** 20)
    P = randn_(empty((n_rows, R1), dt), 7, 0.5)
    Q = randn_(empty((n_rows, R2), dt), 8, 0.5)
    offsets = i32(cuts)
    poison(3 * R1 * R2 * 4)
    got = ops.grouped_wgrad_rows(P, Q, offsets)
    ref = _wgrad64(P, Q, cuts)
    for e in range(3):
        err, bar = float((got[e].double() - ref[e]).abs().max()), WGRAD_BAR * max(1.0, float(ref[e].abs().max()))
        print(f"wgrad rows n = {n_rows} {dt} expert {e}: max |diff| {err:.3e}, error / bar = {err / bar:.4f}")
        assert err <= bar, (e, err, bar)
    if n_rows * R1 < G32 and dt == F16:
        offp, Lp = ops.pad_offsets(offsets), ops.padded_len(n_rows, 3)
        PT = ops.transpose_pad(P, offsets, offp, Lp)
        del P
        old = ops.grouped_wgrad(PT, ops.transpose_pad(Q, offsets, offp, Lp), offp)
        assert float((got.double() - old.double()).abs().max()) <= 1e-3 * max(1.0, float(old.abs().max())), "token-major and K-major paths disagree"


# ================================================================================================ 2. row and elementwise kernels
def _flat_windows(n, esize):
    return windows(n, [(1, esize)], W=640 * 1024)


@pytest.mark.parametrize("dt,n", [(F16, G32 + 104), (BF16, G31 + 104)], ids=["f16-2p32", "bf16-2p31"])
def test_gelu_past_2p31_and_2p32_elements(dt, n):
    """(n % 8 == 0 is smoe_gelu's contract: 13 units of 8 past the boundary.)  The bar of test_gelu_on_both_sides_of_its_grid_cap on
    windows of 655,360 elements; == pieces of under 2^29 elements."""
    need(20)
    x = randn_(empty((n,), dt), 1, 2.0)
    poison(n * 2)
    got = ops.gelu(x)
    w = 0.0
    for lo, hi in _flat_windows(n, 2):
        ref = gelu64(x[lo:hi])
        bound = 2e-6 + 1e-5 * ref.abs() + HALF_ULP[dt] * ref.abs() + TINY[dt]
        w = max(w, worst((got[lo:hi].double() - ref).abs(), bound))
    print(f"gelu {dt} n = {n}: max err / bar = {w:.3f}")
    assert w <= 1.0, w
    for a, b in pieces(n, 1 << 29, 8):
        assert same_bits(ops.gelu(x[a:b]), got[a:b]), f"gelu [{a}, {b}) differs from gelu of that piece alone"


@pytest.mark.parametrize("sd,dd,n", [(F32, F16, G31 + 5), (F16, BF16, G32 + 5)], ids=["f32-f16-2p31", "f16-bf16-2p32"])
def test_cast_past_2p31_and_2p32_elements(sd, dd, n):
    """bit-equal to torch's round-to-nearest cast over the whole tensor, and to smoe_cast of pieces"""
    need(20)
    x = randn_(empty((n,), sd), 2, 3.0)
    poison(n * 2)
    got = ops.cast(x, dd)
    equal_in_chunks(got, lambda a, b: x[a:b].to(dd), n)
    for a, b in pieces(n, 1 << 28, 8):
        assert same_bits(ops.cast(x[a:b], dd), got[a:b])


@pytest.mark.parametrize("mode", ["plain", "fill", "scale"])
def test_scatter_rows_past_2p31_elements(mode):
    """bit-equal to torch over the whole buffer (a copy; with the combine's scale one f32 multiplication in front of the store), as
    test_scatter_rows_on_both_sides_of_its_grid_cap; == the slots scattered in pieces"""
    need(12)
    n, k, d = T_BIG, 2, 1024
    T = n // k + 4
    x = randn_(empty((T, d), F16), 3)
    g = dgen(n)
    pos = torch.randperm(T * k, generator=g, device=DEV)[:n].contiguous()
    pos[3::7] = -1
    scale = torch.rand(T * k, generator=g, device=DEV) * 0.75 + 0.25

    def run(p_, out):
        return ops.scatter_rows(x, p_, k, F16, out=out, zero_fill=mode == "fill", scale=scale if mode == "scale" else None)
    got = run(pos, torch.full((n, d), 7.0, dtype=F16, device=DEV))

    def ref_of(a, b):
        p_ = pos[a:b]
        src = x[p_.clamp(min=0) // k].float()
        if mode == "scale":
            src = src * scale[p_.clamp(min=0)][:, None]
        return torch.where((p_ >= 0)[:, None], src.to(F16), torch.tensor(0.0 if mode == "fill" else 7.0, dtype=F16, device=DEV))
    equal_in_chunks(got, ref_of, n, 1 << 18)
    again = torch.full((n, d), 7.0, dtype=F16, device=DEV)
    for a, b in pieces(n, 1 << 19):
        run(pos[a:b].clone(), again[a:b])
    assert same_bits(again, got)


def _combine_rows64(y, inv, score, res, k, lo, hi):
    iv = inv[lo * k:hi * k]
    yy = torch.where((iv >= 0)[:, None], y[iv.clamp(min=0)].double(), torch.zeros((), dtype=torch.float64, device=DEV))
    terms = (score[lo * k:hi * k].double()[:, None] * yy).reshape(hi - lo, k, -1)
    return terms.sum(1) + res[lo:hi].double(), terms.abs().sum(1) + res[lo:hi].double().abs()


def _combine_inputs(T, k, d, rdt, seed):
    y = randn_(empty((T * k + 5, d), F16), seed)
    g = dgen(seed + 1)
    inv = torch.randperm(T * k + 5, generator=g, device=DEV)[:T * k].contiguous()
    inv[2::5] = -1
    score = torch.rand(T * k, generator=g, device=DEV)
    res = randn_(empty((T, d), rdt), seed + 2)
    return y, inv, score, res


def _compact(y, inv_piece):
    """the rows of y that a piece reads, as an operand of their own (below every boundary), and the piece's indices into it"""
    live = inv_piece >= 0
    yc = y[inv_piece.clamp(min=0)]
    return yc, torch.where(live, torch.arange(inv_piece.numel(), device=DEV), torch.full_like(inv_piece, -1))


def test_gather_combine_past_2p31_elements():
    """k = 2 with a residual, f16 in and out.  Windows: float64 inside the bound of test_gather_combine_on_both_sides_of_its_grid_cap,
    (k + 2) 2^-24 S + half an ulp of the store; == tokens combined in pieces from compacted copies of their rows."""
    need(24)
    T, k, d = T_BIG, 2, 1024
    y, inv, score, res = _combine_inputs(T, k, d, F16, 11)
    got = ops.gather_combine(y, inv, score, T, k, F16, residual=res, out=nans((T, d), F16))
    w = 0.0
    for lo, hi in windows(T, [(d, 2)]):
        ref, mag = _combine_rows64(y, inv, score, res, k, lo, hi)
        w = max(w, worst((got[lo:hi].double() - ref).abs(), (k + 2) * 2.0 ** -24 * mag + HALF_ULP[F16] * ref.abs() + TINY[F16] + 1e-30))
    print(f"gather_combine T = {T}: max err / bound = {w:.3f}")
    assert w <= 1.0, w
    for a, b in pieces(T, 1 << 18):
        yc, ic = _compact(y, inv[a * k:b * k])
        part = ops.gather_combine(yc, ic, score[a * k:b * k].clone(), b - a, k, F16, residual=res[a:b], out=nans((b - a, d), F16))
        assert same_bits(part, got[a:b]), f"tokens [{a}, {b}) differ from the combine of that piece alone"
        del yc, part


def test_gather_combine_ln_past_2p31_elements():
    """k = 1, f32 stream + f16 LayerNorm image.  Windows: out inside the combine's bound, xn at store_bar (the 2e-3 max(1, max |ref|)
    of test_gather_combine_ln_on_both_sides_of_its_grid_cap is 6 x the error at d = 1,024); both == pieces."""
    need(30)
    T, k, d = T_BIG, 1, 1024
    y, inv, score, res = _combine_inputs(T, k, d, F32, 13)
    g = dgen(5)
    w_, b_ = 1 + 0.2 * torch.randn(d, generator=g, device=DEV), 0.1 * torch.randn(d, generator=g, device=DEV)
    out, xn = ops.gather_combine_ln(y, inv, score, T, k, res, w_, b_, 1e-6, F16, out=nans((T, d), F32), xn=nans((T, d), F16))
    wo = wn = 0.0
    for lo, hi in windows(T, [(d, 4), (d, 2)]):
        ref, mag = _combine_rows64(y, inv, score, res, k, lo, hi)
        wo = max(wo, worst((out[lo:hi].double() - ref).abs(), (k + 2) * 2.0 ** -24 * mag + 1e-30))
        ref_xn = torch.nn.functional.layer_norm(out[lo:hi].double(), (d,), w_.double(), b_.double(), 1e-6)
        e, bar = float((xn[lo:hi].double() - ref_xn).abs().max()), store_bar(ref_xn, F16)
        wn = max(wn, e / bar)
    print(f"gather_combine_ln T = {T}: out max err / bound = {wo:.3f}, xn max err / bar = {wn:.3f}")
    assert wo <= 1.0 and wn <= 1.0, (wo, wn)
    for a, b in pieces(T, 1 << 18):
        yc, ic = _compact(y, inv[a * k:b * k])
        po, pn = ops.gather_combine_ln(yc, ic, score[a * k:b * k].clone(), b - a, k, res[a:b], w_, b_, 1e-6, F16)
        assert same_bits(po, out[a:b]) and same_bits(pn, xn[a:b]), f"tokens [{a}, {b}) differ from that piece alone"
        del yc, po, pn


ROWDOT_ROUNDINGS = 1.5


def test_rowdot_past_2p31_elements():
    """y has 2^31 + 88,064 elements.  Float64 on every entry (the output is small); == entries computed in pieces from compacted rows.
    bar_rowdot of tests/test_gpu_nonfinite.py counts every operation of a lane, (16 FMAs + 6 adds) 2^-24 S with S = sum |dout y|: at
    d = 1,024 that is 40 x the error, because a row's 1,024 roundings do not line up.  The bar here is ROWDOT_ROUNDINGS 2^-24 S, 3 x
    the largest error / (2^-24 S) measured on an MI355X (see MEASURED)."""
    need(12)
    n, k, d = T_BIG, 2, 1024
    T = (n + k - 1) // k
    dout = randn_(empty((T, d), F16), 21)
    y = randn_(empty((n + 9, d), F16), 22)
    inv = torch.randperm(n + 9, generator=dgen(23), device=DEV)[:n].contiguous()
    inv[1::6] = -1
    poison(4 * n)
    got = ops.rowdot(dout, y, inv, k)
    w = 0.0
    for a in range(0, n, 1 << 17):
        b = min(n, a + (1 << 17))
        iv = inv[a:b]
        prod = dout[torch.arange(a, b, device=DEV) // k].double() * y[iv.clamp(min=0)].double()
        live = iv >= 0
        ref = torch.where(live, prod.sum(-1), torch.zeros((), dtype=torch.float64, device=DEV))
        mag = torch.where(live, prod.abs().sum(-1), torch.zeros((), dtype=torch.float64, device=DEV))
        w = max(w, worst((got[a:b].double() - ref).abs(), ROWDOT_ROUNDINGS * 2.0 ** -24 * mag + 1e-30))
        assert bool((got[a:b][~live] == 0).all())
    print(f"rowdot n = {n}: max err / bound = {w:.3f}")
    assert w <= 1.0, w
    for a, b in pieces(n, 1 << 19, k):
        yc, ic = _compact(y, inv[a:b])
        assert same_bits(ops.rowdot(dout[a // k:(b + k - 1) // k], yc, ic, k), got[a:b])
        del yc


@pytest.mark.parametrize("d,T", [(1024, T_BIG), (192, G31 // 192 + 1000)], ids=["wave-per-row-d1024", "16-lanes-per-row-d192"])
def test_layernorm_past_2p31_elements(d, T):
    """f16 in, f16 out; windows at store_bar (test_layernorm_kernel_matches_reference_layernorm's 2e-3 max(1, max |ref|) for a 16-bit
    output is 6 - 7 x the error here); == rows normalised in pieces"""
    need(10)
    x = randn_(empty((T, d), F16), d, 3.0, 1.0)
    g = dgen(d)
    w, b = 1 + 0.3 * torch.randn(d, generator=g, device=DEV), 0.2 * torch.randn(d, generator=g, device=DEV)
    poison(T * d * 2)
    got = ops.layernorm(x, w, b, 1e-6, F16)
    worst_ = 0.0
    for lo, hi in windows(T, [(d, 2)]):
        ref = torch.nn.functional.layer_norm(x[lo:hi].double(), (d,), w.double(), b.double(), 1e-6)
        worst_ = max(worst_, float((got[lo:hi].double() - ref).abs().max()) / store_bar(ref, F16))
    print(f"layernorm d = {d} T = {T}: max err / bar = {worst_:.3f}")
    assert worst_ <= 1.0, worst_
    for lo, hi in pieces(T, (1 << 29) // d):
        assert same_bits(ops.layernorm(x[lo:hi], w, b, 1e-6, F16), got[lo:hi])


LN_F32_BAR = 4e-7


def test_layernorm_rows_past_2p31_elements():
    """rows 1,032 floats apart; windows at LN_F32_BAR max(1, max |ref|), 3 x the error measured on an MI355X (the f32 bar of
    test_layernorm_kernel_matches_reference_layernorm, 2e-6, is 14 x the error at d = 1,024); == smoe_layernorm's bits on the gathered rows
    (the assertion of test_wave_per_row_embedding_stage_on_both_sides_of_its_grid_cap) and == pieces"""
    need(20)
    T, d, stride = T_BIG, 1024, 1032
    buf = randn_(empty((T, stride), F32), 31, 2.0)
    g = dgen(32)
    w, b = 1 + 0.3 * torch.randn(d, generator=g, device=DEV), 0.2 * torch.randn(d, generator=g, device=DEV)
    poison(T * d * 4)
    got = ops.layernorm_rows(buf, stride, T, d, w, b, 1e-6)
    worst_ = 0.0
    for lo, hi in windows(T, [(d, 4), (stride, 4)]):
        ref = torch.nn.functional.layer_norm(buf[lo:hi, :d].double(), (d,), w.double(), b.double(), 1e-6)
        worst_ = max(worst_, float((got[lo:hi].double() - ref).abs().max()) / (LN_F32_BAR * max(1.0, float(ref.abs().max()))))
        assert same_bits(got[lo:hi], ops.layernorm(buf[lo:hi, :d].contiguous(), w, b, 1e-6, F32))
    print(f"layernorm_rows T = {T}: max err / bar = {worst_:.3f}")
    assert worst_ <= 1.0, worst_
    for lo, hi in pieces(T, 1 << 18):
        assert same_bits(ops.layernorm_rows(buf[lo:hi], stride, hi - lo, d, w, b, 1e-6), got[lo:hi])


def test_patchify_cast_past_2p31_elements():
    """2,731 images of 3 x 512 x 512 (2^31 + 2.1 M floats) in 16 x 16 patches, f16: bit-equal to the torch patch gather + cast over
    the whole output (test_patchify_cast_on_both_sides_of_its_grid_cap's assertion), and to images cut in pieces"""
    need(16)
    B, C, H, Wd, p = 2731, 3, 512, 512, 16
    assert B * C * H * Wd > G31
    img = randn_(empty((B, C, H, Wd), F32), 33, 1.5)
    poison(2 * img.numel())
    got = ops.patchify_cast(img, p, p, F16)
    per = (H // p) * (Wd // p)

    def ref_of(im):
        n = im.shape[0]
        return im.reshape(n, C, H // p, p, Wd // p, p).permute(0, 2, 4, 1, 3, 5).reshape(n * per, C * p * p).to(F16)
    for a in range(0, B, 128):
        b = min(B, a + 128)
        assert same_bits(got[a * per:b * per], ref_of(img[a:b])), f"images [{a}, {b}) differ from torch"
    for a, b in pieces(B, 600):
        assert same_bits(ops.patchify_cast(img[a:b], p, p, F16), got[a * per:b * per])


def test_gate_dgrad_past_2p31_elements():
    """f16 out; == rows in pieces.  Windows in relative L2 at 2^-11 x 1.02: every element is an f32 sum of E = 4 products rounded once
    to f16, so no element, and hence no L2 norm, is off by more than half an ulp (the 2 % is for the f32 sum); the 1e-3 of
    test_gate_dgrad_streaming_kernel_matches_matmul is 5 x the error here."""
    need(8)
    T, E, d = T_BIG, 4, 1024
    dl = randn_(empty((T, E), F32), 41)
    w = randn_(empty((E, d), F32), 42, 0.1)
    poison(T * d * 2)
    got = ops.gate_dgrad(dl, w, F16)
    worst_ = 0.0
    for lo, hi in windows(T, [(d, 2)]):
        worst_ = max(worst_, rel(got[lo:hi], dl[lo:hi].double() @ w.double()) / (1.02 * HALF_ULP[F16]))
    print(f"gate_dgrad T = {T}: max relative L2 / bar = {worst_:.3f}")
    assert worst_ <= 1.0, worst_
    for lo, hi in pieces(T, 1 << 19):
        assert same_bits(ops.gate_dgrad(dl[lo:hi], w, F16), got[lo:hi])


# max |diff| against the oracle / F.layer_norm in float64; "ln" and "ln scores" are the fused LayerNorm + router's
ROUTER_BARS = {"logits": 2.1e-6, "scores": 7e-7, "ln": 2.9e-6, "ln scores": 1.6e-6}


def test_router_topk_past_2p31_elements():
    """d = 768, E = 8, k = 2 on f32 rows; on the windows the assertions of test_router_naive_matches_oracle: indices bit-exact against the
    oracle, logits and scores in max |diff| at ROUTER_BARS (that test's 1e-5 and 5e-6 are 14 x and 21 x the error here; these are 3 x
    the error measured on an MI355X, see MEASURED); indices and scores == rows routed in pieces"""
    need(12)
    d, E, k = 768, 8, 2
    T = G31 // d + 100
    x = randn_(empty((T, d), F32), 51)
    g = dgen(52)
    wg, bg = torch.randn(E, d, generator=g, device=DEV) * 0.05, torch.randn(E, generator=g, device=DEV) * 0.1
    poison(8 * T * k, 4 * T * k, 4 * T * E)
    idx, score, logits, _ = ops.router_topk(x, wg, bg, k, ops.GATE_NAIVE, want_logits=True)
    for lo, hi in windows(T, [(d, 4)]):
        o_idx, o_score, o_logits = mo.naive_gate(x[lo:hi].cpu(), wg.cpu(), bg.cpu(), k)
        assert torch.equal(idx[lo:hi].cpu(), o_idx), f"routing of rows [{lo}, {hi}) differs from the oracle"
        e_l, e_s = float((logits[lo:hi].cpu() - o_logits).abs().max()), float((score[lo:hi].cpu() - o_score).abs().max())
        print(f"router_topk rows [{lo}, {hi}): max |diff| logits {e_l:.2e}, scores {e_s:.2e} (bars {ROUTER_BARS})")
        assert e_l <= ROUTER_BARS["logits"] and e_s <= ROUTER_BARS["scores"], (e_l, e_s)
    for lo, hi in pieces(T, 1 << 19):
        p_idx, p_score, _, _ = ops.router_topk(x[lo:hi], wg, bg, k, ops.GATE_NAIVE, want_logits=True)
        assert torch.equal(p_idx, idx[lo:hi]) and same_bits(p_score, score[lo:hi])


def test_embed_ln_past_2p31_elements():
    """d = 1,024, one patch per image: 2 B = 2^21 + 154 rows.  The f32 stream bit-equal to cat(cls, tokens) + pos_embed over the whole
    tensor, its 16-bit LayerNorm at store_bar on the windows (the assertions of
    test_wave_per_row_embedding_stage_on_both_sides_of_its_grid_cap, whose 2e-3 max(1, max |ref|) is 6 x the error here); both ==
    images embedded in pieces."""
    need(18)
    d, P = 1024, 1
    B = T_BIG // 2 + 39
    tok = randn_(empty((B * P, d), F16), 71)
    g = dgen(72)
    cls, pos = torch.randn(1, 1, d, generator=g, device=DEV), torch.randn(1, P + 1, d, generator=g, device=DEV)
    w, b = 1 + 0.3 * torch.randn(d, generator=g, device=DEV), 0.2 * torch.randn(d, generator=g, device=DEV)
    poison(B * (P + 1) * d * 4, B * (P + 1) * d * 2)
    x32, xn = ops.embed_ln(tok, cls, pos, B, P, ln=(w, b, 1e-6))
    assert x32.numel() > G31
    equal_in_chunks(x32, lambda lo, hi: torch.cat((cls.expand(hi - lo, -1, -1), tok[lo:hi].reshape(hi - lo, P, d).float()), dim=1) + pos, B, 1 << 16)
    rows, xr, worst_ = x32.reshape(-1, d), xn.reshape(-1, d), 0.0
    for lo, hi in windows(2 * B, [(d, 4), (d, 2)]):
        ref = torch.nn.functional.layer_norm(rows[lo:hi].double(), (d,), w.double(), b.double(), 1e-6)
        worst_ = max(worst_, float((xr[lo:hi].double() - ref).abs().max()) / store_bar(ref, F16))
    print(f"embed_ln rows = {2 * B}: xn max err / bar = {worst_:.3f}")
    assert worst_ <= 1.0, worst_
    for lo, hi in pieces(B, 1 << 18):
        px, pn = ops.embed_ln(tok[lo:hi], cls, pos, hi - lo, P, ln=(w, b, 1e-6))
        assert same_bits(px, x32[lo:hi]) and same_bits(pn.reshape(-1, d), xr[2 * lo:2 * hi])
        del px, pn


LNB_BARS = {"dx": 1.8e-7, "dgamma": 1.3e-6, "dbeta": 3.3e-7}


def test_layernorm_bwd_past_2p31_elements():
    """x f32, dy f16, d = 1,024.  dx on the windows, dgamma and dbeta over all rows, against float64 of LayerNorm's backward in relative
    L2; dx == rows in pieces.  test_layernorm_backward_matches_float64_autograd's 2e-6 (set at d = 192 and a few thousand rows) is 4 - 30
    x the errors at this shape: the bars are LNB_BARS, each 3 x the error measured on an MI355X (see MEASURED)."""
    need(26)
    T, d, eps = T_BIG, 1024, 1e-6
    x = randn_(empty((T, d), F32), 81, 2.0, 0.5)
    dy = randn_(empty((T, d), F16), 82, 0.1)
    w = 1 + 0.3 * torch.randn(d, generator=dgen(83), device=DEV)
    poison(4 * T * d, 8 * d)
    dx, dw, db = ops.layernorm_bwd(x, dy, w, eps)

    def rows64(lo, hi):
        xd, gy = x[lo:hi].double(), dy[lo:hi].double()
        mu = xd.mean(-1, keepdim=True)
        rstd = ((xd - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
        xh, gw = (xd - mu) * rstd, gy * w.double()
        return rstd * (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True)), (gy * xh).sum(0), gy.sum(0)
    dw64, db64 = torch.zeros(d, dtype=torch.float64, device=DEV), torch.zeros(d, dtype=torch.float64, device=DEV)
    for lo in range(0, T, 1 << 16):
        _, a_, b_ = rows64(lo, min(T, lo + (1 << 16)))
        dw64 += a_
        db64 += b_
    e_x = max(rel(dx[lo:hi], rows64(lo, hi)[0]) for lo, hi in windows(T, [(d, 4), (d, 2)]))
    e_w, e_b = rel(dw, dw64), rel(db, db64)
    print(f"layernorm_bwd T = {T}: relative L2 dx {e_x:.2e}, dgamma {e_w:.2e}, dbeta {e_b:.2e} (bars {LNB_BARS})")
    assert e_x <= LNB_BARS["dx"] and e_w <= LNB_BARS["dgamma"] and e_b <= LNB_BARS["dbeta"], (e_x, e_w, e_b)
    for lo, hi in pieces(T, 1 << 18):
        assert same_bits(ops.layernorm_bwd(x[lo:hi], dy[lo:hi], w, eps)[0], dx[lo:hi])


GLNB_BARS = {"dx": 2.2e-7, "dz": 3.9e-7, "dgamma": 8e-7, "dbeta": 8e-7, "dgate_w": 8e-7, "dgate_b": 6e-7, "sum dz": 2.2e-7}


def test_gate_ln_bwd_past_2p31_elements():
    """x f32, g_f f16, d = 1,024, no g_out.  dx and dz over ALL rows, dgamma, dbeta and the gate's weight / bias gradients, against
    float64 autograd through LayerNorm and the reference's gate expressions, accumulated over chunks of 65,536 rows; the formula and
    the metrics of test_gate_ln_backward_in_one_pass_matches_float64_autograd_of_the_reference_formula (relative L2; the two scalar sums
    relative to max(1, |db|)); dx and dz == rows in pieces.  That test's 8e-7 stays for the three column sums (1.7 - 2 x the error
    here); for dx, dz and the scalar sums (its 1e-5) it is 6 - 130 x the error at this shape: GLNB_BARS, each 3 x the error measured on
    an MI355X (see MEASURED)."""
    need(26)
    T, d, thr, eps, CH = T_BIG, 1024, 0.55, 1e-6, 1 << 16
    x = randn_(empty((T, d), F32), 85, 1.7, 0.3)
    g_f = randn_(empty((T, d), F16), 86, 0.3)
    g = dgen(87)
    gam, bet = 1.0 + 0.2 * torch.randn(d, generator=g, device=DEV), 0.1 * torch.randn(d, generator=g, device=DEV)
    w, b = torch.randn(d, generator=g, device=DEV) * 0.03, torch.randn(1, generator=g, device=DEV) * 0.1
    gr, btr, wr, br = [t.double().requires_grad_(True) for t in (gam, bet, w, b)]

    def forward(lo, hi, xr):
        xn = torch.nn.functional.layer_norm(xr, (d,), gr, btr, eps)
        z = xn @ wr + br
        return xn, z, torch.sigmoid(z)[:, None]
    mask = empty((T, 2), F32)
    with torch.no_grad():
        for lo in range(0, T, CH):
            hi = min(T, lo + CH)
            prob = forward(lo, hi, x[lo:hi].double())[2]
            mask[lo:hi] = torch.cat([(prob > thr).float(), (prob <= thr).float()], dim=1)
    assert 0 < int(mask[:, 0].sum()) < T
    poison(4 * T * d, 4 * (3 * d + 4), 4 * T)
    dx, dg, db_, dgw, dgb, dz = ops.gate_ln_bwd(x, g_f, None, gam, bet, eps, w, b, mask, want_dz=True)
    num = {"dx": 0.0, "dz": 0.0}
    den = {"dx": 0.0, "dz": 0.0}
    for lo in range(0, T, CH):
        hi = min(T, lo + CH)
        xr = x[lo:hi].double().requires_grad_(True)
        xn, z, prob = forward(lo, hi, xr)
        z.retain_grad()
        tk = (prob <= thr).double() + prob.detach() - prob
        (g_f[lo:hi].double() * (xn * tk)).sum().backward()
        for nm, got, ref in (("dx", dx[lo:hi], xr.grad), ("dz", dz[lo:hi], z.grad)):
            num[nm] += float((got.double() - ref).pow(2).sum())
            den[nm] += float(ref.pow(2).sum())
        del xr, xn, z, prob, tk
    errs = {nm: (num[nm] / den[nm]) ** 0.5 for nm in num}
    errs.update(dgamma=rel(dg, gr.grad), dbeta=rel(db_, btr.grad), dgate_w=rel(dgw, wr.grad))
    scale = max(1.0, abs(float(br.grad)))
    e_b, e_z = abs(float(dgb) - float(br.grad)) / scale, abs(float(dz.double().sum()) - float(br.grad)) / scale
    print(f"gate_ln_bwd T = {T}: relative L2 " + ", ".join(f"{k_} {e:.2e}" for k_, e in errs.items())
          + f"; gate bias gradient {e_b:.2e}, sum of dz {e_z:.2e} (bars {GLNB_BARS})")
    assert all(e <= GLNB_BARS[nm] for nm, e in errs.items()), errs
    assert e_b <= GLNB_BARS["dgate_b"] and e_z <= GLNB_BARS["sum dz"], (e_b, e_z)
    for lo, hi in pieces(T, 1 << 18):
        r = ops.gate_ln_bwd(x[lo:hi], g_f[lo:hi], None, gam, bet, eps, w, b, mask[lo:hi], want_dz=True)
        assert same_bits(r[0], dx[lo:hi]) and same_bits(r[5], dz[lo:hi])
        del r


@pytest.mark.parametrize("d,E,k,T", [(768, 8, 2, G31 // 768 + 100), (1024, 32, 1, T_BIG)], ids=["d768-E8", "d1024-E32"])
def test_ln_router_topk_past_2p31_elements(d, E, k, T):
    """On the windows the assertions of test_layernorm_router_on_both_sides_of_its_grid_cap: the fused LayerNorm against F.layer_norm,
    routing equal to the oracle's on the very same normalised rows, scores; bars ROUTER_BARS "ln" and "ln scores" (that test's 1e-5
    and 5e-6 are 10 x the error here); over the whole tensor the
    16-bit image is the rounding of the f32 one; indices, scores and the 16-bit image == rows in pieces."""
    need(24)
    x = randn_(empty((T, d), F32), d + E, 1.7, 0.3)
    g = dgen(E)
    lw, lb = 1 + 0.2 * torch.randn(d, generator=g, device=DEV), 0.1 * torch.randn(d, generator=g, device=DEV)
    wg, bg = torch.randn(E, d, generator=g, device=DEV) * 0.1, torch.randn(E, generator=g, device=DEV) * 0.1
    poison(2 * T * d, 4 * T * d, 8 * T * k, 4 * T * k)
    xn16, xn32, idx, score, _, _ = ops.ln_router_topk(x, lw, lb, 1e-6, wg, bg, k, ops.GATE_NAIVE, want_xn32=True)
    equal_in_chunks(xn16, lambda lo, hi: xn32[lo:hi].half(), T, 1 << 18)
    for lo, hi in windows(T, [(d, 4), (d, 2)]):
        ref_ln = torch.nn.functional.layer_norm(x[lo:hi].double(), (d,), lw.double(), lb.double(), 1e-6)
        e_n = float((xn32[lo:hi].double() - ref_ln).abs().max())
        o_idx, o_score, _ = mo.naive_gate(xn32[lo:hi].cpu(), wg.cpu(), bg.cpu(), k)
        assert torch.equal(idx[lo:hi].cpu(), o_idx), f"routing of rows [{lo}, {hi}) differs from the oracle"
        e_s = float((score[lo:hi].cpu() - o_score).abs().max())
        print(f"ln_router_topk d = {d} rows [{lo}, {hi}): max |diff| LayerNorm {e_n:.2e}, scores {e_s:.2e} (bars {ROUTER_BARS})")
        assert e_n <= ROUTER_BARS["ln"] and e_s <= ROUTER_BARS["ln scores"], (e_n, e_s)
    del xn32
    for lo, hi in pieces(T, 1 << 19):
        p16, _, p_idx, p_score, _, _ = ops.ln_router_topk(x[lo:hi], lw, lb, 1e-6, wg, bg, k, ops.GATE_NAIVE)
        assert same_bits(p16, xn16[lo:hi]) and torch.equal(p_idx, idx[lo:hi]) and same_bits(p_score, score[lo:hi])
        del p16


def test_gate_ln_router_past_2p31_elements():
    """d = 768, E = 8, k = 1.  On the windows the assertions of test_gate_layernorm_router_on_both_sides_of_its_grid_cap (LayerNorm
    within ROUTER_BARS "ln" in place of that test's 1e-5, decisions and routing equal to the oracle's on the kernel's own normed rows,
    the k = 1 scores equal to the oracle's); over the whole tensor the 16-bit image =
    the masked rows and the device counter = the number of skipped tokens; mask, indices and the image == rows in pieces."""
    need(24)
    d, E, k = 768, 8, 1
    T = G31 // d + 100
    x = randn_(empty((T, d), F32), 91, 1.5, 0.2)
    g = dgen(92)
    lw, lb = 1 + 0.2 * torch.randn(d, generator=g, device=DEV), 0.1 * torch.randn(d, generator=g, device=DEV)
    gw, gb = torch.randn(1, d, generator=g, device=DEV) * 0.05, torch.full((1,), 0.1, device=DEV)
    wg, bg = torch.randn(E, d, generator=g, device=DEV) * 0.1, torch.randn(E, generator=g, device=DEV) * 0.1
    thr = torch.tensor(0.55, device=DEV)

    def run(rows):
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        r = ops.gate_ln_router(rows, gw, gb, thr, ln=(lw, lb, 1e-6), wg=wg, bg=bg, k=k, xn16_dtype=F16, want_xn32=True, want_mask=True,
                               skip_count=cnt)
        return r, cnt
    poison(2 * T * d, 4 * T * d, 8 * T * k, 8 * T)
    r, cnt = run(x)
    skipped = int(r["mask"][:, 0].sum())
    assert int(cnt.item()) == skipped and 0 < skipped < T, (int(cnt.item()), skipped, T)
    for lo in range(0, T, 1 << 18):      # (value equality, as that test: a masked row is +0 here, x * 0 is +-0)
        hi = min(T, lo + (1 << 18))
        assert torch.equal(r["xn16"][lo:hi], (r["xn32"][lo:hi] * r["mask"][lo:hi, 1:2]).half()), f"xn16 rows [{lo}, {hi})"
    for lo, hi in windows(T, [(d, 4), (d, 2)]):
        xn = r["xn32"][lo:hi].cpu()
        ref_ln = torch.nn.functional.layer_norm(x[lo:hi].double(), (d,), lw.double(), lb.double(), 1e-6)
        e_n = float((xn.double() - ref_ln.cpu()).abs().max())
        print(f"gate_ln_router rows [{lo}, {hi}): max |diff| LayerNorm {e_n:.2e} (bar {ROUTER_BARS['ln']})")
        assert e_n <= ROUTER_BARS["ln"], e_n
        m = mo.skip_gate(xn[None], gw.cpu(), gb.cpu(), float(thr))[0]
        assert torch.equal(r["mask"][lo:hi].cpu(), m)
        o_idx, o_score, _ = mo.naive_gate(xn * m[:, 1:2], wg.cpu(), bg.cpu(), k)
        e_s = float((r["score"][lo:hi].cpu() - o_score).abs().max())
        assert torch.equal(r["idx"][lo:hi].cpu(), o_idx) and e_s == 0.0, e_s
    for lo, hi in pieces(T, 1 << 19):
        p, _ = run(x[lo:hi])
        assert same_bits(p["xn16"], r["xn16"][lo:hi]) and torch.equal(p["mask"], r["mask"][lo:hi]) and torch.equal(p["idx"], r["idx"][lo:hi])
        del p


ATTN_BARS = {"lse": 8.8e-4, "L2": 1e-3, "max": 1.6e-3}


def test_attention_forward_and_backward_past_2p31_elements():
    """N = 16, H = 16, head dim 64, B = 43,700: qkv has 2^31 + 458,752 elements (43,700 x 16 heads of trivial work).  Windows of 16
    batch elements (first, last, around the 2 GiB / 4 GiB = 2^31-element offsets of qkv) against float64 autograd; out, lse and dqkv ==
    batch elements in pieces.  The metrics are those of test_attention_kernel_matches_reference_attention (out: max |diff|) and
    test_attention_backward_matches_float64_autograd (lse: max |diff|; dq, dk, dv: relative L2 and max |diff| / max |ref|); their bars
    (2e-3 max(1, max |ref|), 2e-3, 4e-3, 2e-2) are set for N up to 640 and are 6 - 30 x the error at N = 16.  Here: out at store_bar, the
    rest at ATTN_BARS, each 3 x the error measured on an MI355X (see MEASURED)."""
    need(14)
    B, N, H, scale = 43700, 16, 16, 64 ** -0.5
    qkv = randn_(empty((B, N, 3, H, 64), F16), 95, 1.2)
    do = randn_(empty((B, N, H * 64), F16), 96, 0.5)
    assert qkv.numel() > G31
    poison(do.numel() * 2, B * H * N * 4)
    out, lse = ops.attention(qkv, B, N, H, 64, scale, want_lse=True)
    poison(qkv.numel() * 2)
    dqkv = ops.attention_bwd(qkv, out, do, lse, B, N, H, 64, scale)
    for lo, hi in windows(B, [(N * 3 * H * 64, 2), (N * H * 64, 2)], W=16):
        qr = qkv[lo:hi].double().requires_grad_(True)
        q, k_, v = qr.permute(2, 0, 3, 1, 4).unbind(0)
        s_ = q @ k_.transpose(-2, -1) * scale
        o_ref = (torch.softmax(s_, -1) @ v).transpose(1, 2).reshape(hi - lo, N, H * 64)
        o_ref.backward(do[lo:hi].double())
        lse_ref = torch.logsumexp(s_.detach(), -1) / math.log(2.0)
        e_o = float((out[lo:hi].double() - o_ref.detach()).abs().max()) / store_bar(o_ref.detach(), F16)
        e_l = float((lse[lo:hi].double() - lse_ref).abs().max()) / ATTN_BARS["lse"]
        errs = []
        for i in range(3):
            got, ref = dqkv[lo:hi, :, i].double(), qr.grad[:, :, i]
            errs += [rel(got, ref) / ATTN_BARS["L2"], float((got - ref).abs().max()) / (ATTN_BARS["max"] * float(ref.abs().max()))]
        print(f"attention batches [{lo}, {hi}): error / bar: out {e_o:.3f}, lse {e_l:.3f}, dq dk dv (L2, max) " + " ".join(f"{e:.3f}" for e in errs))
        assert max([e_o, e_l] + errs) <= 1.0, (lo, hi, e_o, e_l, errs)
    for lo, hi in pieces(B, 20000):
        po, pl = ops.attention(qkv[lo:hi], hi - lo, N, H, 64, scale, want_lse=True)
        assert same_bits(po, out[lo:hi]) and same_bits(pl, lse[lo:hi])
        assert same_bits(ops.attention_bwd(qkv[lo:hi], po, do[lo:hi], pl, hi - lo, N, H, 64, scale), dqkv[lo:hi])


def test_entry_points_that_refuse_2p31_say_so():
    """The four dispatch plans, the header kernels, the loss and the Mixup kernels reject a count of 2^31 (per sample: C H W) before
    any launch: one call each with pointers that are never dereferenced.  smoe_dispatch_plan_padded also rejects E slot_rows = 2^31
    with few entries.  smoe_ep_unpack_headers takes no row count (its row positions come from the caller's i32 table local_base, so
    W x rows per block < 2^31 is the caller's duty): the call here is the size it does reject, more than 8,192 groups."""
    lib, fake, big = _lib.load(), 4096, 1 << 40

    def refused(rc, word):
        assert rc != 0 and rc != -1 and word in lib.smoe_last_error(), (rc, lib.smoe_last_error())
    refused(lib.smoe_dispatch_plan(fake, G31, 8, -1, fake, fake, fake, fake, fake, fake, big, None), b"out of range")
    refused(lib.smoe_dispatch_plan_hist(fake, G31, 8, -1, fake, 256, fake, fake, fake, fake, fake, fake, big, None), b"out of range")
    refused(lib.smoe_dispatch_plan_padded(fake, G31, 8, 1, 1, fake, fake, fake, fake, fake, fake, None, fake, big, None), b"out of range")
    refused(lib.smoe_dispatch_plan_padded(fake, 100, 8, 1, G31 // 8, fake, fake, fake, fake, fake, fake, None, fake, big, None),
            b"E * slot_rows out of range")
    refused(lib.smoe_dispatch_plan_slots(fake, G31, 8, -1, fake, 0, fake, fake, fake, fake, fake, fake, None, fake, big, None), b"out of range")
    refused(lib.smoe_ep_pack_headers(fake, fake, fake, 2, 64, G31, fake, None), b"t_rows")
    refused(lib.smoe_ep_unpack_headers(fake, 8193, 1, fake, 64, 8, fake, fake, None, None), b"smoe_ep_unpack_headers: bad sizes")
    refused(lib.smoe_soft_ce_fwd(fake, 0, fake, None, 0.0, G31, 8, fake, fake, fake, fake, fake, None), b"smoe_soft_ce_fwd")
    refused(lib.smoe_mixup_target(fake, fake, fake, 1.0, 0.0, G31, 8, fake, None), b"smoe_mixup_target")
    refused(lib.smoe_mixup_images(fake, 2, 2048, 1024, 1024, fake, fake, fake, None), b"2^31")


# ================================================================================================ 3. gridDim.y / gridDim.z
def grid_limit() -> int:
    """The smaller of the current device's maxGridSize[1] and [2].  torch's device properties do not carry them, so they are read
    through hipDeviceGetAttribute: hipDeviceAttributeMaxGridDimY = 30 and ...Z = 31 in the hipDeviceAttribute_t of ROCm 6 and 7's
    hip_runtime_api.h (the CUDA-compatible block of the enum, counted from hipDeviceAttributeCudaCompatibleBegin = 0).  A header that
    renumbered them would show here as a value that is no grid limit: the assertion below."""
    hip = ctypes.CDLL("libamdhip64.so")
    vals = []
    for attr in (30, 31):
        v = ctypes.c_int(0)
        assert hip.hipDeviceGetAttribute(ctypes.byref(v), attr, torch.cuda.current_device()) == 0
        assert 65535 <= v.value < 2 ** 31, f"attribute {attr} = {v.value} is not a grid limit"
        vals.append(v.value)
    print(f"maxGridSize y, z = {vals}")
    return min(vals)


def right_or_refused(call, check, *limit_words):
    """Past the grid limit a launcher may walk the dimension with a stride (then `check` compares with float64) or refuse with a
    SlimMoEError that names its limit -- never return success with output it did not write."""
    try:
        got = call()
    except _lib.SlimMoEError as e:
        assert any(w in str(e) for w in limit_words), f"the refusal does not name the limit: {e}"
        print(f"refused: {e}")
        return
    torch.cuda.synchronize()
    check(got)


SOFT_CE_ROW_BAR, SOFT_CE_MEAN_BAR = 3e-6, 1.45e-7


def test_soft_ce_past_the_grid_row_limit():
    """B = limit + 3, C = 8.  Forward (one workgroup per row on gridDim.x): per-row loss against float64 at the bar of
    test_soft_ce_shapes_both_target_forms_and_run_to_run_identity (tests/test_gpu_mixup_loss.py _bars: 3 x the error of torch's f32
    composition on these inputs), and at most SOFT_CE_ROW_BAR; the mean of 65,539 rows at SOFT_CE_MEAN_BAR (the rows' errors average
    out: the row bar is 70 x the mean's error); both 3 x the error measured on an MI355X (see MEASURED).  Backward (gridDim.y = B):
    right at that test's gradient bar, or refused naming 65,535."""
    from test_gpu_mixup_loss import _bars
    B, C = grid_limit() + 3, 8
    g = dgen(B)
    logits = torch.randn(B, C, generator=g, device=DEV) * 2
    target = torch.softmax(torch.randn(B, C, generator=g, device=DEV), dim=-1)
    r64, g64, bar_row, bar_grad, _ = _bars(logits, target)
    poison(16 * B, 4)
    loss, rows = ops.soft_ce_fwd(logits, target=target)
    e_r, e_m = float((rows[0].double() - r64).abs().max()), abs(float(loss) - float(r64.mean()))
    print(f"soft_ce_fwd B = {B}: max row error {e_r:.2e} (bars {bar_row:.2e}, {SOFT_CE_ROW_BAR:.1e}), error of the mean {e_m:.2e} (bar {SOFT_CE_MEAN_BAR:.1e})")
    assert e_r <= min(bar_row, SOFT_CE_ROW_BAR) and e_m <= SOFT_CE_MEAN_BAR, (e_r, e_m, bar_row)
    gsc = torch.ones((), device=DEV)

    def check(dl):
        assert float((dl.double() - g64).abs().max()) <= bar_grad
    poison(4 * B * C)
    right_or_refused(lambda: ops.soft_ce_bwd(logits, rows, gsc, target=target), check, "65535")


def test_transpose_cast_past_the_grid_row_limit():
    """R = 64 (limit + 1), C = 64: bit-equal to torch's transpose + cast, or refused naming the limit"""
    R, C = 64 * (grid_limit() + 1), 64
    src = randn_(empty((1, R, C), F32), 61)
    poison(2 * R * C)
    def check(got):
        assert same_bits(got, src.transpose(1, 2).to(F16).contiguous())
    right_or_refused(lambda: ops.transpose_cast(src, F16), check, "65535")


def _transpose_pad_case(n):
    src = randn_(empty((n, 64), F16), 62)
    offsets = i32([0, n])
    offp, Lp = ops.pad_offsets(offsets), ops.padded_len(n, 1)
    poison(2 * 64 * Lp)
    return src, Lp, (lambda: ops.transpose_pad(src, offsets, offp, Lp))


def test_transpose_pad_at_and_past_the_grid_row_limit():
    """Lp / 64 = 65,535 (the last size that fits the grid's second dimension): bit-equal to torch's transpose with zero padding;
    Lp / 64 = limit + 2: refused, naming 65,535."""
    n = 64 * 65534
    src, Lp, call = _transpose_pad_case(n)
    assert Lp // 64 == 65535
    got = call()
    assert same_bits(got[:, :n], src.t().contiguous()) and bool((got[:, n:] == 0).all())
    del got, src
    n = 64 * (grid_limit() + 1)
    src, Lp, call = _transpose_pad_case(n)

    def check(got):
        assert same_bits(got[:, :n], src.t().contiguous()) and bool((got[:, n:] == 0).all())
    right_or_refused(call, check, "65535")


def test_group_colsum_and_gate_wgrad_past_the_grid_row_limit():
    """256 (limit + 1) rows of 64 columns: more 256-row chunks than gridDim.y holds.  Right against float64, or refused naming 65,535."""
    n, C, E = 256 * (grid_limit() + 1), 64, 4
    x = randn_(empty((n, C), F16), 63)
    cuts = (0, n // 3, n // 3, n - 7, n)
    poison(4 * E * C)

    def check_colsum(got):      # the bar of test_group_colsum_many_chunks_and_empty_groups (f16: 2e-3 max(1, max |ref|))
        for e, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            ref = x[a:b].double().sum(0)
            assert float((got[e].double() - ref).abs().max()) <= 2e-3 * max(1.0, float(ref.abs().max()))
    right_or_refused(lambda: ops.group_colsum(x, i32(cuts)), check_colsum, "65535")
    dl = randn_(empty((n, E), F32), 64)

    def check_wgrad(got):       # the bar of test_gate_wgrad_matches_matmul
        ref = dl.double().t() @ x.double()
        assert float((got.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())) * n ** 0.5
    poison(4 * E * C)
    right_or_refused(lambda: ops.gate_wgrad(dl, x), check_wgrad, "65535")
