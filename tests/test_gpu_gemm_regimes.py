"""Value regimes: the GEMM family and the token reductions against float64 and the bars of tests/test_gemm_regimes_host.py (which
owns the inputs, the references, the emulations the bars come from, and the argument for each bar).  The fifth regime family,
next to test_gpu_value_regimes.py (LayerNorm, attention).  What a benign input and a bar of tol max(1, max |ref|) cannot tell
apart and these can: a partial sum kept in 16 bits, an f32 store that went through a 16-bit rounding, a 16-bit store that truncates
or saturates, a bias rounded to 16 bits, a dropped small product, a combine scale applied on the wrong side of the residual, a flush
of 16-bit input subnormals.

    entry point                          classes                              shapes                        checked
    ops.grouped_gemm, variants 0 (f32,   benign positive cancel range,        rows [1, 0, 127, 129, 321],   f32 store and operand-typed store, with and
    f16, bf16), 1 4 9 10 13 14 (16 bit)  subnormal (f16)                      K 64 768 3072, N 72 256       without bias, EPI_NONE and EPI_GELU: per-element
                                                                                                            bar; 16-bit store = chain16(own f32 store) bitwise
    ... row_map + row_scale + residual   the same                             the same                      bar; 16-bit: the bits of the rounding chain
    ... EPI_GELU_GRAD                    the same                             the same                      bar (H in [-6, 6] with +-0 and the ends)
    ... edge16                           one exact product per output         [320, 64] x [72, 64]          f32 store exact; 16-bit store = .to(dtype) bitwise
    ops.grouped_gemm_gelu_keep           benign positive subnormal            K 64 768, N 72 256            both outputs: bar, and the bits of variant 9's
    ops.grouped_wgrad_rows, _split (4),  benign positive cancel range         rows [1, 63, 65, 1000, 0,     per-element bar (the split: + 3 u for its piece sum);
    transpose_pad + grouped_wgrad        along the rows                       2049], R (72, 136) (256, 320) the swapped path on a shape that prefers it
    ops.group_colsum                     benign positive cancel, along rows       [1500, 0, 512, 513, 1] x 72   relative to the column's sum of magnitudes
    ops.gate_wgrad (+ bias), gate_dgrad  a softmax backward's magnitudes      T 1 257 5000, E 8, d 192      relative to the sum of magnitudes
    ops.rowdot, ops.gather_combine       k 2, d 768, dropped entries                                        the same; dropped entries give exact zeros
    ops.switch_aux                       a peaked softmax                     T 5000, E 8                   aux and coef
    smoe_grad_sumsq, _multi              1e-3, 2^-44 (floor of f32), 4e4      n 3 x 16384 + 5, 2^-16        the block partials' sum, relative to float64

Every test prints `REGIME <entry> <case>: worst error / bar`; profiles/r16_gemm_value_regimes.md holds the tables."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from slim_switch_moe_vit_amd import _lib, ops, optim  # noqa: E402
import test_gemm_regimes_host as gh  # noqa: E402

DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
VARIANTS = (0, 1, 4, 9, 10, 13, 14)
M = sum(gh.GROUPS)


def _variants(dt):
    """variants >= 1 take 16-bit operands and K % 64 == 0 (every K here is a multiple of 64)"""
    return VARIANTS if dt != F32 else (0,)


def _form(variant):
    return "erf" if variant == 0 else "fast"


def _dev(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


@functools.lru_cache(maxsize=2)
def _case(cls, K, N, dt):
    c = gh.gemm_case(cls, K, N, dt)
    A = torch.cat([c["A"], torch.full((7, K), 3.0, dtype=dt)])      # rows past offsets[E] exist and must not be touched
    return (*_dev(A, c["W"], c["bias"], c["offsets"]), *gh.gemm_ref(cls, K, N, dt), gh.contraction_C(cls, K, dt)[0])


def _report(entry, case, r):
    print(f"REGIME {entry} {case}: worst error / bar {r:.3f}")
    assert r <= 1.0, (entry, case, r)
    return r


GEMM_CASES = [(c, K, N, dt) for dt in gh.ALL_DT for c in gh.classes_of(dt) for K in gh.KS for N in gh.NS]
gemm_cases = pytest.mark.parametrize("cls,K,N,dt", GEMM_CASES, ids=[f"{c}-K{K}-N{N}-{gh._dn(dt)}" for c, K, N, dt in GEMM_CASES])


@gemm_cases
def test_grouped_gemm_stores(cls, K, N, dt):
    A, W, bias, offsets, acc, mag, brow, C = _case(cls, K, N, dt)
    for variant in _variants(dt):
        w32, w16, raw = 0.0, 0.0, 0.0
        for b, bref in ((bias, brow), (None, None)):
            for epi, form in ((ops.EPI_NONE, None), (ops.EPI_GELU, _form(variant))):
                out32 = torch.full((M + 7, N), 7.0, dtype=F32, device=DEV)
                ops.grouped_gemm(A, W, b, offsets, epi, out=out32, variant=variant)
                assert bool((out32[M:] == 7.0).all()), "rows past the last group stay untouched"
                w32 = max(w32, gh.worst(out32[:M], *gh.chain_ref_bar(acc, mag, bref, C, F32, gelu=form)))
                if b is None and form is None:
                    raw = float(gh.f32_ratio(out32[:M], acc, mag, None).max())
                if dt != F32:
                    out16 = ops.grouped_gemm(A, W, b, offsets, epi, dt, variant=variant)
                    w16 = max(w16, gh.worst(out16[:M], *gh.chain_ref_bar(acc, mag, bref, C, dt, gelu=form)))
                    assert torch.equal(out16[:M].cpu(), gh.chain16(out32[:M].cpu(), dt)), \
                        (variant, epi, "the 16-bit store is the rounding of the f32 store")
        case = f"{cls} K {K} N {N} {gh._dn(dt)} variant {variant}"
        _report("grouped_gemm/f32-store", case, w32)
        print(f"REGIME grouped_gemm/f32-store-raw {case}: no bias, no epilogue: {raw:.3g} u of |A| |W|^T (C {C:.3g})")
        if dt != F32:
            _report("grouped_gemm/16-bit-store", case, w16)
        if dt == F32 and K == 64:   # like for like: the chain of FMAs over the very same outputs (a note, not a requirement)
            emu = gh.emulate_gemm_all(cls, K, N, dt, 1)
            plain = ops.grouped_gemm(A, W, None, offsets, ops.EPI_NONE, F32, variant=variant)[:M].cpu()
            print(f"REGIME grouped_gemm/f32-operands-model {case}: sequential FMA emulation over the same outputs "
                  f"{float(gh.f32_ratio(emu, acc, mag, None).max()):.3g} u; {int((emu != plain).sum())} of {emu.numel()} outputs differ from it")
        if cls == "subnormal":      # (a flush is 1e4 bars out as it is; this names it)
            plain = ops.grouped_gemm(A, W, None, offsets, ops.EPI_NONE, F32, variant=variant)[:M]
            assert float((plain == 0).float().mean()) < 0.01, "16-bit input subnormals are not flushed to zero"


@gemm_cases
def test_grouped_gemm_combine_scale_then_residual(cls, K, N, dt):
    """out[row_map[m]] = residual[row_map[m]] + row_scale[row_map[m]] (A[m] W^T + bias): a permutation, scales in [0, 1] (0, 1,
    2^-20 among them), a residual of the output's magnitude -- the scale comes BEFORE the residual, each step rounded to the store"""
    A, W, bias, offsets, acc, mag, brow, C = _case(cls, K, N, dt)
    for odt in (F32,) if dt == F32 else (F32, dt):
        row_map, scale, residual, _H = gh.epilogue_inputs(N, odt)
        s, res = scale[row_map][:, None], residual[row_map]
        for variant in _variants(dt):
            w = 0.0
            for b, bref in ((bias, brow), (None, None)):
                out = torch.full((M, N), 7.0, dtype=odt, device=DEV)
                ops.grouped_gemm(A, W, b, offsets, ops.EPI_NONE, out=out, row_map=row_map.to(DEV), row_scale=scale.to(DEV),
                                 residual=residual.to(DEV), variant=variant)
                got = out.cpu()[row_map]
                w = max(w, gh.worst(got, *gh.chain_ref_bar(acc, mag, bref, C, odt, scale=s, residual=res)))
                if odt != F32:
                    plain = ops.grouped_gemm(A, W, b, offsets, ops.EPI_NONE, F32, variant=variant)[:M].cpu()
                    assert torch.equal(got, gh.chain16(plain, odt, s, res)), (variant, "round, scale16, add16: in that order")
            _report("grouped_gemm/scale+residual", f"{cls} K {K} N {N} {gh._dn(dt)} -> {gh._dn(odt)} variant {variant}", w)


@gemm_cases
def test_grouped_gemm_gelu_grad_epilogue(cls, K, N, dt):
    """out = (A W^T + bias) gelu'(H): saved pre-activations H in [-6, 6] with +-0 and the saturated ends in the first columns"""
    A, W, bias, offsets, acc, mag, brow, C = _case(cls, K, N, dt)
    for odt in (F32,) if dt == F32 else (F32, dt):
        H = gh.epilogue_inputs(N, odt)[3]
        ref, bar = gh.chain_ref_bar(acc, mag, brow, C, odt, hgrad=H)
        for variant in _variants(dt):
            out = ops.grouped_gemm(A, W, bias, offsets, ops.EPI_GELU_GRAD, odt, residual=torch.cat([H, H[:7]]).to(DEV), variant=variant)
            _report("grouped_gemm/gelu-grad", f"{cls} K {K} N {N} {gh._dn(dt)} -> {gh._dn(odt)} variant {variant}", gh.worst(out[:M], ref, bar))


@pytest.mark.parametrize("dt", (F16, BF16), ids=gh._dn)
@pytest.mark.parametrize("variant", VARIANTS)
def test_grouped_gemm_16_bit_store_rounds_to_nearest_even_and_overflows_to_inf(variant, dt):
    """one exact product per output over the top of the store type's range: no saturating and no truncating convert"""
    A, W, pre = gh.edge16_case(dt)
    offsets = torch.tensor([0, A.shape[0]], dtype=torch.int32)
    out32 = ops.grouped_gemm(*_dev(A, W), None, offsets.to(DEV), ops.EPI_NONE, F32, variant=variant)
    assert torch.equal(out32.cpu(), pre), "one product per output: the f32 store is exact"
    out16 = ops.grouped_gemm(*_dev(A, W), None, offsets.to(DEV), ops.EPI_NONE, dt, variant=variant)
    want = pre.to(dt)
    bad = int((out16.cpu().view(torch.int16) != want.view(torch.int16)).sum())
    print(f"REGIME grouped_gemm/edge16 {gh._dn(dt)} variant {variant}: {bad} of {want.numel()} stores differ from .to({gh._dn(dt)}); "
          f"{int(torch.isinf(want).sum())} are inf")
    assert bad == 0


KEEP_CASES = [(c, K, N, dt) for dt in (F16, BF16) for c in ("benign", "positive", "subnormal") if c in gh.classes_of(dt)
              for K, N in ((64, 72), (768, 256))]


@pytest.mark.parametrize("cls,K,N,dt", KEEP_CASES, ids=[f"{c}-K{K}-N{N}-{gh._dn(dt)}" for c, K, N, dt in KEEP_CASES])
def test_grouped_gemm_gelu_keep(cls, K, N, dt):
    A, W, bias, offsets, acc, mag, brow, C = _case(cls, K, N, dt)
    pre, act = ops.grouped_gemm_gelu_keep(A, W, bias, offsets)
    case = f"{cls} K {K} N {N} {gh._dn(dt)}"
    _report("gelu_keep/pre", case, gh.worst(pre[:M], *gh.chain_ref_bar(acc, mag, brow, C, dt)))
    _report("gelu_keep/gelu", case, gh.worst(act[:M], *gh.chain_ref_bar(acc, mag, brow, C, dt, gelu="fast")))
    for epi, got in ((ops.EPI_NONE, pre), (ops.EPI_GELU, act)):
        out32 = ops.grouped_gemm(A, W, bias, offsets, epi, F32, variant=9)
        assert torch.equal(got[:M].cpu(), gh.chain16(out32[:M].cpu(), dt)), "the bits of the production variant's f32 store, rounded"


# ================================================================================================================ weight gradients
WGRAD_CASES = [(c, R, dt) for dt in (F16, BF16) for c in gh.CLASSES for R in gh.WGRAD_R]


@pytest.mark.parametrize("cls,R,dt", WGRAD_CASES, ids=[f"{c}-R{R[0]}x{R[1]}-{gh._dn(dt)}" for c, R, dt in WGRAD_CASES])
def test_grouped_wgrad_rows_split_and_k_major(cls, R, dt):
    c = gh.wgrad_case(cls, R[0], R[1], dt)
    ref, mag = gh.wgrad_ref(cls, R[0], R[1], dt)
    C = gh.wgrad_C(cls, dt)
    P, Q, offsets = _dev(c["P"], c["Q"], c["offsets"])
    case = f"{cls} R {R[0]} x {R[1]} {gh._dn(dt)}"
    bar = C * gh.U * mag
    _report("grouped_wgrad_rows", case, gh.worst(ops.grouped_wgrad_rows(P, Q, offsets), ref, bar))
    S = 4
    split = ops.grouped_wgrad_rows_split(P, Q, offsets, S)
    _report("grouped_wgrad_rows_split", case, gh.worst(split, ref, (C + S - 1) * gh.U * mag))     # S - 1 more adds of at most u mag each
    offs_pad = ops.pad_offsets(offsets)
    Lp = ops.padded_len(P.shape[0], len(gh.WGRAD_ROWS))
    kmajor = ops.grouped_wgrad(ops.transpose_pad(P, offsets, offs_pad, Lp), ops.transpose_pad(Q, offsets, offs_pad, Lp), offs_pad)
    _report("transpose_pad+grouped_wgrad", case, gh.worst(kmajor, ref, bar))
    assert float(ops.grouped_wgrad_rows(P, Q, offsets)[4].abs().max()) == 0.0, "an empty group's gradient is zero"


@pytest.mark.parametrize("dt", (F16, BF16), ids=gh._dn)
def test_grouped_wgrad_rows_swapped_path(dt, monkeypatch):
    """32 groups x [64, 2304]: 288 tiles of 256 rows = two rounds on 256 CUs, transposed 256 tiles of 320 rows = one: computed as
    Q^T P and transposed back by smoe_transpose_cast"""
    rows, R1, R2 = (40,) * 32, 64, 2304
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert ops._wgrad_rounds(len(rows), R2, R1, cus) + 0.15 < ops._wgrad_rounds(len(rows), R1, R2, cus), "the shape prefers the swap"
    calls = []
    real = ops.transpose_cast
    monkeypatch.setattr(ops, "transpose_cast", lambda src, d: (calls.append(tuple(src.shape)), real(src, d))[1])
    for cls in ("benign", "positive"):
        c = gh.wgrad_case(cls, R1, R2, dt, rows)
        ref, mag = gh.wgrad_ref(cls, R1, R2, dt, rows)
        P, Q, offsets = _dev(c["P"], c["Q"], c["offsets"])
        n = len(calls)
        got = ops.grouped_wgrad_rows(P, Q, offsets)
        assert calls[n:] == [(len(rows), R2, R1)], "the swap was taken"
        bar = gh.wgrad_C(cls, dt, rows) * gh.U * mag
        _report("grouped_wgrad_rows/swapped", f"{cls} {gh._dn(dt)}", gh.worst(got, ref, bar))
        _report("grouped_wgrad_rows/unswapped", f"{cls} {gh._dn(dt)}", gh.worst(ops.grouped_wgrad_rows(P, Q, offsets, allow_swap=False), ref, bar))
        assert calls[n:] == [(len(rows), R2, R1)]


# ============================================================================================================ the token reductions
@pytest.mark.parametrize("dt", gh.ALL_DT, ids=gh._dn)
@pytest.mark.parametrize("cls", ("benign", "positive", "cancel"))
def test_group_colsum(cls, dt):
    src, offsets, ref, mag, C = gh.colsum_case(cls, dt)
    got = ops.group_colsum(*_dev(src, offsets))
    _report("group_colsum", f"{cls} {gh._dn(dt)}", gh.worst(got, ref, C * gh.U * mag))
    assert float(got[1].abs().max()) == 0.0, "an empty group sums to zero"
    # a note, not a requirement: a reordered sum inside the bar is fine, and then the host module's emulation wants the new order
    print(f"REGIME group_colsum {cls} {gh._dn(dt)}: {int((got.cpu() != gh.colsum_emulate(src, offsets)).sum())} of {got.numel()} sums differ "
          "from the emulation's bits")


@pytest.mark.parametrize("xdt", (F32, F16), ids=gh._dn)
@pytest.mark.parametrize("T", gh.GATE_TS)
def test_gate_wgrad_and_dgrad(T, xdt):
    r = gh.gate_case(T, xdt)
    dl, x, w = _dev(r["dl"], r["x"], r["w"])
    dw, db = ops.gate_wgrad(dl, x, want_bias=True)
    case = f"T {T} x {gh._dn(xdt)}"
    _report("gate_wgrad/dWg", case, gh.worst(dw, r["dw"], r["C_dw"] * gh.U * r["dw_mag"]))
    _report("gate_wgrad/dbg", case, gh.worst(db, r["db"], r["C_db"] * gh.U * r["db_mag"]))
    assert torch.equal(ops.gate_wgrad(dl, x), dw)
    for odt in (F32, F16):
        dx = ops.gate_dgrad(dl, w, odt)
        bar = r["C_dx"] * gh.U * r["dx_mag"]
        if odt != F32:
            bar = bar + gh._h(r["dx"], bar, odt)
        _report("gate_dgrad", f"T {T} -> {gh._dn(odt)}", gh.worst(dx, r["dx"], bar))


@pytest.mark.parametrize("ydt", (F16, F32), ids=gh._dn)
def test_rowdot_and_gather_combine(ydt):
    r = gh.combine_case(ydt)
    y, dout, inv, score = _dev(r["y"], r["dout"], r["inv"], r["score"])
    dot = ops.rowdot(dout, y, inv, r["k"])
    _report("rowdot", f"y {gh._dn(ydt)}", gh.worst(dot, r["dot"], r["C_dot"] * gh.U * r["dot_mag"]))
    assert float(dot[inv < 0].abs().max()) == 0.0, "dropped entries give exact zeros"
    mix = ops.gather_combine(y, inv, score, r["T"], r["k"], F32)
    _report("gather_combine", f"y {gh._dn(ydt)}", gh.worst(mix, r["mix"], r["C_mix"] * gh.U * r["mix_mag"]))
    both = (r["inv"].reshape(r["T"], r["k"]) < 0).all(1)
    assert not bool(both.any()) or float(mix.cpu()[both].abs().max()) == 0.0


def test_switch_aux():
    r = gh.switch_aux_case()
    aux, coef = ops.switch_aux(*_dev(r["probs"], r["counts"]))
    _report("switch_aux/aux", "T 5000 E 8", gh.worst(aux, r["aux"], r["C_aux"] * gh.U * r["aux"].abs()))
    _report("switch_aux/coef", "T 5000 E 8", gh.worst(coef, r["coef"], r["C_coef"] * gh.U * r["coef"].abs()))


SUMSQ_CASES = [(rg, dt) for rg, (_, dts) in gh.SUMSQ_REGIMES.items() for dt in dts]


@pytest.mark.parametrize("regime,dt", SUMSQ_CASES, ids=[f"{rg}-{gh._dn(dt)}" for rg, dt in SUMSQ_CASES])
def test_grad_sumsq(regime, dt):
    """the block partials added in f32, as optim.py adds them (one torch sum on the device), against float64: every term is >= 0"""
    grad, ref, C = gh.sumsq_case(regime, dt)
    lib = _lib.load()
    g = grad.to(DEV)
    nb = lib.smoe_grad_sumsq_blocks(g.numel())
    assert nb == 4
    partial = torch.full((nb,), -1.0, device=DEV)
    found = torch.zeros(1, device=DEV)
    inv = torch.tensor([gh.SUMSQ_INV_SCALE], device=DEV)
    _lib.check(lib.smoe_grad_sumsq(g.data_ptr(), ops.dtype_code(dt), g.numel(), inv.data_ptr(), partial.data_ptr(), found.data_ptr(),
                                   ops._stream(g)), "smoe_grad_sumsq")
    assert float(found.item()) == 0.0
    _report("grad_sumsq", f"{regime} {gh._dn(dt)}", gh.worst(partial.sum(), ref, C * gh.U * ref))
    print(f"REGIME grad_sumsq {regime} {gh._dn(dt)}: {int((partial.cpu() != gh.sumsq_emulate(grad, gh.SUMSQ_INV_SCALE)).sum())} of {nb} block "
          "partials differ from the emulation's bits (a note, not a requirement)")
    # the multi-tensor launch optim.py issues: a short tensor in front, so that this gradient's blocks sit behind another one's in
    # the block table -- the same partials for it, and the first tensor's own inside the bar
    g0 = g[:20000].clone()
    blk, nbs = optim._block_table([g0.numel(), g.numel()], torch.device(DEV))
    assert list(nbs) == [2, nb]
    ptrs = [g0.data_ptr(), g.data_ptr()]
    tab = torch.tensor([ptrs, ptrs, ptrs, ptrs, [g0.numel(), g.numel()]], dtype=torch.int64, device=DEV)
    multi = torch.full((sum(nbs),), -1.0, device=DEV)
    _lib.check(lib.smoe_grad_sumsq_multi(tab.data_ptr(), 2, blk.data_ptr(), sum(nbs), ops.dtype_code(dt), inv.data_ptr(), multi.data_ptr(),
                                         found.data_ptr(), ops._stream(g)), "smoe_grad_sumsq_multi")
    assert float(found.item()) == 0.0
    assert torch.equal(multi[2:], partial), "smoe_grad_sumsq_multi: the single-tensor launch's partials"
    ref0 = ((grad[:20000].double() * gh.SUMSQ_INV_SCALE) ** 2).sum()
    _report("grad_sumsq_multi", f"{regime} {gh._dn(dt)}", max(gh.worst(multi[2:].sum(), ref, C * gh.U * ref), gh.worst(multi[:2].sum(), ref0, C * gh.U * ref0)))
