"""The MoE layer and its kernels at widths off the four ViT widths (d = 192 / 384 / 768 / 1024), at expert counts past 32 and at
GEMM contraction lengths that are no multiple of 64: everything the library's argument checks accept and the other modules never launch.

  1  the generic router (csrc/router.hip) at every NCH = ceil(d / 256) from 3 to 8, weights in LDS and from global memory
  2  the row kernels and reductions past their first column trip / register chunk / workgroup-sized loop
  3  the grouped GEMM with f32 operands at K % 64 != 0 (where the library rewrites `variant` to 0)
  4  FMoETransformerMLP, eval and training, at such shapes against the oracle
  6  shapes just outside the envelope end in a RuntimeError that names the rule, and leave nothing behind

Case lists, inputs and float64 references live in tests/_offgrid_cases.py; tests/test_offgrid_host.py checks them on the CPU.  Every
bar is an existing bar of this project (named where it is used) or a rounding count written where it is used; each test prints its
worst error / bar ratio (pytest -s), test_worst_ratios_by_kernel_family the largest per kernel family."""
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import moe_oracle as mo  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import _lib, fmoe, ops  # noqa: E402
from _mp import dtype_factor, float_bar  # noqa: E402
import _offgrid_cases as oc  # noqa: E402
import test_gpu_launch_regimes as lr  # noqa: E402

DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DT_IDS = {F32: "f32", F16: "f16", BF16: "bf16"}
WORST = collections.defaultdict(float)      # kernel family -> largest error / bar ratio seen in this run


def note(family: str, what: str, ratio: float) -> float:
    WORST[family] = max(WORST[family], ratio)
    print(f"{family} {what}: error / bar = {ratio:.3f}")
    return ratio


def dev(*ts):
    out = [None if t is None else t.to(DEV) for t in ts]
    return out[0] if len(out) == 1 else out


# ================================================================================================ 1. generic router
@pytest.mark.parametrize("force_f64", [False, True], ids=["f32-pass", "all-f64"])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("d,E,k", oc.ROUTER_CASES)
def test_generic_router_at_every_chunk_count(d, E, k, dtype, force_f64):
    """idx bit-equal to the oracle; forced f64: the logits too; else inside router.hip's documented bound + one f32 ulp; scores
    within the 5e-6 of test_router_naive_matches_oracle"""
    x, wg, bg = oc.router_inputs(d, E, k, dtype)
    T = x.shape[0]
    lr.poison(8 * T * k, 4 * T * k, 4 * T * E)
    idx, score, logits, _ = ops.router_topk(*dev(x, wg, bg), k, ops.GATE_NAIVE, want_logits=True, force_f64=force_f64)
    o_idx, o_score, o_logits = mo.naive_gate(x.float(), wg, bg, k)
    assert torch.equal(idx.cpu(), o_idx), "routing indices must be bit-exact"
    if force_f64:
        assert lr.same_bits(logits.cpu(), o_logits), "f64-accumulated logits round to the same f32"
    else:
        ref = oc.router_logits64(x.float(), wg, bg)
        w = lr.worst((logits.cpu().double() - ref).abs(), oc.router_logit_bound(x.float(), wg, ref))
        assert note("router", f"d={d} E={E} k={k} {DT_IDS[dtype]} NCH={oc.router_nch(d)} lds={oc.router_weights_in_lds(d, E)}", w) <= 1.0
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
    if k == 1:
        assert bool((score == 1.0).all())


@pytest.mark.parametrize("d,E", oc.SWITCH_CASES)
def test_generic_router_switch_gate_with_noise(d, E):
    """test_router_switch_matches_oracle's assertions; the logits (stored before the noise is added) inside the router's bound"""
    x, wg, bg = oc.router_inputs(d, E, 1)
    noise = oc.switch_noise(d, E)
    T = x.shape[0]
    lr.poison(8 * T, 4 * T, 4 * T * E, 4 * T * E)
    idx, score, logits, probs = ops.router_topk(*dev(x, wg, bg), 1, ops.GATE_SWITCH, dev(noise), want_logits=True, want_probs=True)
    o_idx, o_score, o_p = mo.switch_gate(x, wg, bg, noise)
    assert torch.equal(idx.cpu(), o_idx)
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
    assert torch.allclose(probs.cpu(), o_p, rtol=0, atol=5e-6)
    ref = oc.router_logits64(x, wg, bg)
    assert note("router", f"switch d={d} E={E}", lr.worst((logits.cpu().double() - ref).abs(), oc.router_logit_bound(x, wg, ref))) <= 1.0


@pytest.mark.parametrize("d,E,k", oc.NEAR_TIE_CASES)
def test_generic_router_near_ties_take_the_redo_pass(d, E, k):
    """an exact and a one-ulp tie between experts (test_router_near_ties_take_the_f64_path_and_match_the_oracle's construction): the
    f32 pass cannot order them, the f64 redo pass of this NCH must, for every k the shape allows"""
    x, wg, bg = oc.near_tie_inputs(d, E)
    for kk in range(1, min(E, 4) + 1):
        idx, score, _, _ = ops.router_topk(*dev(x, wg, bg), kk, ops.GATE_NAIVE)
        o_idx, o_score, _ = mo.naive_gate(x, wg, bg, kk)
        assert torch.equal(idx.cpu(), o_idx), kk
        assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)


# ================================================================================================ 2. row kernels and reductions
ROWS = 37


@pytest.mark.parametrize("odt,bar", [(F32, 1e-6), (F16, 1e-3)], ids=["f32", "f16"])
@pytest.mark.parametrize("d,E", oc.DGRAD_CASES)
def test_gate_dgrad_second_column_trip(d, E, odt, bar):
    """dl @ w in float64 at the relative-L2 bars of test_gate_dgrad_streaming_kernel_matches_matmul"""
    g = oc.gen(d + E)
    dl, w = torch.randn(ROWS, E, generator=g), torch.randn(E, d, generator=g) * 0.1
    lr.poison(ROWS * d * lr.HALF_BYTES[odt])
    got = ops.gate_dgrad(*dev(dl, w), odt)
    e = lr.rel(got.cpu(), dl.double() @ w.double())
    assert note("gate_dgrad", f"E={E} d={d} {DT_IDS[odt]} ({oc.gate_dgrad_kernel(E)})", e / bar) <= 1.0, e


@pytest.mark.parametrize("want_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("C,E", oc.WGRAD_CASES)
def test_gate_wgrad_wide_and_narrow_rows(C, E, want_bias):
    """test_gate_wgrad_matches_matmul's bar, max |diff| <= 1e-5 max(1, max |ref|) sqrt(T), also for the bias column; two calls equal"""
    T = 150
    g = oc.gen(C + E)
    dl, x = torch.randn(T, E, generator=g), torch.randn(T, C, generator=g)
    lr.poison(4 * E * C, 4 * E)
    got = ops.gate_wgrad(*dev(dl, x), want_bias=want_bias)
    again = ops.gate_wgrad(*dev(dl, x), want_bias=want_bias)
    got, again = (got, again) if want_bias else ((got,), (again,))
    refs = (dl.double().t() @ x.double(), dl.double().sum(0))
    for name, gt, ag, ref in zip(("dw", "db"), got, again, refs):
        assert lr.same_bits(gt, ag), "two calls differ"
        bar = 1e-5 * max(1.0, float(ref.abs().max())) * T ** 0.5
        assert note("gate_wgrad", f"{name} C={C} E={E}", float((gt.cpu().double() - ref).abs().max()) / bar) <= 1.0


@pytest.mark.parametrize("mode", ["plain", "fill", "scale"])
@pytest.mark.parametrize("odt", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("d", oc.ROW_DIMS)
def test_scatter_rows_wide(d, odt, mode):
    """test_scatter_rows_on_both_sides_of_its_grid_cap's assertion: bit-equal to torch's copy (x scale) + round-to-nearest cast;
    unmapped slots keep the sentinel (plain, scale) or become zero rows (fill)"""
    n, k = 150, 2
    T = n // k + 3
    g = oc.gen(n + d)
    x = torch.randn(T, d, generator=g).to(F32 if odt != BF16 else F16)
    pos = torch.randperm(T * k, generator=g)[:n].contiguous()
    pos[3::7] = -1
    scale = torch.rand(T * k, generator=g) * 0.75 + 0.25
    xd, pd, sd = dev(x, pos, scale)
    got = ops.scatter_rows(xd, pd, k, odt, out=torch.full((n, d), 7.0, dtype=odt, device=DEV), zero_fill=mode == "fill",
                           scale=sd if mode == "scale" else None)
    src = xd[pd.clamp(min=0) // k].float()
    if mode == "scale":
        src = src * sd[pd.clamp(min=0)][:, None]
    ref = torch.where((pd >= 0)[:, None], src.to(odt), torch.tensor(0.0 if mode == "fill" else 7.0, dtype=odt, device=DEV))
    assert lr.same_bits(got, ref), f"smoe_scatter_rows {mode} -> {odt}, d={d}"


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("ydt,odt", [(F16, F32), (F32, F32), (BF16, BF16), (F16, F16)], ids=["f16-f32", "f32-f32", "bf16-bf16", "f16-f16"])
@pytest.mark.parametrize("k", oc.COMBINE_KS)
@pytest.mark.parametrize("d", oc.ROW_DIMS)
def test_gather_combine_wide(d, k, ydt, odt, with_res):
    """test_gather_combine_on_both_sides_of_its_grid_cap's bound: (k + 2) 2^-24 S + the output format's half ulp"""
    T = ROWS
    y, inv, score, res = oc.combine_inputs(T, k, d, ydt, odt)
    res = res if with_res else None
    got = ops.gather_combine(*dev(y, inv, score), T, k, odt, residual=dev(res), out=lr.nans((T, d), odt))
    ref, mag = oc.combine_ref(y, inv, score, res, T, k)
    w = lr.worst((got.cpu().double() - ref).abs(), lr._combine_bound(ref, mag, k, odt))
    assert note("gather_combine", f"d={d} k={k} {DT_IDS[ydt]}->{DT_IDS[odt]} res={with_res}", w) <= 1.0


@pytest.mark.parametrize("ddt,ydt", [(F16, F16), (F32, F32), (BF16, F32)], ids=["f16-f16", "f32-f32", "bf16-f32"])
@pytest.mark.parametrize("d", oc.ROW_DIMS)
def test_rowdot_wide(d, ddt, ydt):
    """test_rowdot_on_both_sides_of_its_grid_cap's bound with the FMA count of a lane written for any d: (d / 64 + 6) 2^-24 sum |a b|"""
    n, k = 150, 2
    dout, y, inv = oc.rowdot_inputs(n, k, d, ddt, ydt)
    lr.poison(4 * n)
    got = ops.rowdot(*dev(dout, y, inv), k)
    ref, mag = oc.rowdot_ref(dout, y, inv, k)
    w = lr.worst((got.cpu().double() - ref).abs(), oc.rowdot_fmas(d) * oc.U * mag + 1e-30)
    assert note("rowdot", f"d={d} {DT_IDS[ddt]} x {DT_IDS[ydt]}", w) <= 1.0
    assert bool((got.cpu()[inv < 0] == 0).all())


@pytest.mark.parametrize("with_dres", [False, True], ids=["plain", "dres"])
@pytest.mark.parametrize("dyt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("T", oc.LN_TS)
@pytest.mark.parametrize("d", oc.LN_DIMS)
def test_layernorm_backward_one_chunk_past_every_boundary(d, T, dyt, with_dres):
    """dx, dgamma, dbeta against the float64 closed form at LNB_BAR_D4 (relative L2 2e-6); two calls bit-identical"""
    x, w, b, dy, dres = oc.ln_inputs(T, d, dyt)
    dres = dres if with_dres else None
    args = (*dev(x, dy, w), oc.EPS, dev(dres))
    lr.poison(4 * T * d, 8 * d)
    dx, dw, db = ops.layernorm_bwd(*args)
    dx2, dw2, db2 = ops.layernorm_bwd(*args)
    assert lr.same_bits(dx, dx2) and lr.same_bits(dw, dw2) and lr.same_bits(db, db2), "two calls differ"
    ref = oc.ln_bwd_ref(x, w, dy, dres)
    errs = {n_: lr.rel(v.cpu(), ref[n_]) for n_, v in (("dx", dx), ("dw", dw), ("db", db))}
    print(f"layernorm_bwd d={d} T={T}: relative L2 " + ", ".join(f"{n_} {e:.2e}" for n_, e in errs.items()))
    assert note("layernorm_bwd", f"d={d} T={T} dy {DT_IDS[dyt]} dres={with_dres} NJ={oc.ln_nj(d)}", max(errs.values()) / lr.LNB_BAR_D4) <= 1.0, errs


@pytest.mark.parametrize("gdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("mode", oc.GATE_MODES)
@pytest.mark.parametrize("T", oc.LN_TS)
@pytest.mark.parametrize("d", oc.LN_DIMS)
def test_gate_layernorm_backward_one_chunk_past_every_boundary(d, T, mode, gdt):
    """every output against the float64 closed form of the kernel's stated formulas (checked against autograd of the reference's
    gate expressions in tests/test_offgrid_host.py) at GLNB_BAR_D4 (relative L2 8e-7) and the scalar bar 1e-5 relative to
    max(1, |db|) of test_gate_ln_backward_on_both_sides_of_its_grid_cap; two calls bit-identical"""
    x, gam, bet, w, b, g_f, g_out = oc.gate_ln_inputs(T, d, gdt)
    ref = oc.gate_ln_bwd_ref(x, gam, bet, w, b, g_f, g_out, mode)
    args = (*dev(x, g_f, g_out, gam, bet), oc.EPS, *dev(w, b, ref["mask"]))
    gate_on = {"off": False, "hard": True, "soft": 2}[mode]
    lr.poison(4 * T * d, 4 * (3 * d + 4), 4 * T)
    out = ops.gate_ln_bwd(*args, gate_on=gate_on, want_dz=True)
    again = ops.gate_ln_bwd(*args, gate_on=gate_on, want_dz=True)
    assert all(lr.same_bits(a, c) for a, c in zip(again, out)), "two calls differ"
    dx, dg, db_, dgw, dgb, dz = out
    errs = {"dx": lr.rel(dx.cpu(), ref["dx"]), "dgamma": lr.rel(dg.cpu(), ref["dgamma"]), "dbeta": lr.rel(db_.cpu(), ref["dbeta"])}
    if mode == "off":
        assert bool((dgw == 0).all()) and float(dgb) == 0.0 and bool((dz == 0).all()), "a disabled gate has no gradient"
        e_b = e_z = 0.0
    else:
        errs.update(dgate_w=lr.rel(dgw.cpu(), ref["dgate_w"]), dz=lr.rel(dz.cpu(), ref["dz"]))
        scale = max(1.0, abs(float(ref["dgate_b"])))
        e_b, e_z = abs(float(dgb) - float(ref["dgate_b"])) / scale, abs(float(dz.double().sum()) - float(ref["dgate_b"])) / scale
    print(f"gate_ln_bwd d={d} T={T} {mode}: relative L2 " + ", ".join(f"{n_} {e:.2e}" for n_, e in errs.items())
          + f"; gate bias gradient {e_b:.2e}, sum of dz {e_z:.2e}")
    what = f"d={d} T={T} {mode} g_f {DT_IDS[gdt]} NJ={oc.ln_nj(d)}"
    bars = {n_: oc.GLNB_MEASURED_BARS.get((d, T, gdt), {}).get(n_, lr.GLNB_BAR_D4) for n_ in errs}     # (one cancelling row: see there)
    assert note("gate_ln_bwd", what, max(e / bars[n_] for n_, e in errs.items())) <= 1.0, (errs, bars)
    assert note("gate_ln_bwd", what + " scalars", max(e_b, e_z) / lr.GLNB_SCALAR_BAR) <= 1.0, (e_b, e_z)


@pytest.mark.parametrize("ydt,ndt", [(F16, F16), (BF16, BF16)], ids=["f16", "bf16"])
@pytest.mark.parametrize("d,k", oc.COMBINE_LN_CASES)
def test_gather_combine_ln_one_chunk_past_every_boundary(d, k, ydt, ndt):
    """test_gather_combine_ln_on_both_sides_of_its_grid_cap's assertions: out bit for bit smoe_gather_combine's f32 rows and inside
    its bound; xn = LayerNorm of those rows against float64 at 2e-3 (f16; 8 x for bf16) x max(1, max |ref|)"""
    T = ROWS
    y, inv, score, res = oc.combine_inputs(T, k, d, ydt, F32, seed=1)
    g = oc.gen(d + k)
    w_, b_ = 1 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    yd, invd, sd, resd, wd, bd = dev(y, inv, score, res, w_, b_)
    out, xn = ops.gather_combine_ln(yd, invd, sd, T, k, resd, wd, bd, oc.EPS, ndt, out=lr.nans((T, d), F32), xn=lr.nans((T, d), ndt))
    assert lr.same_bits(out, ops.gather_combine(yd, invd, sd, T, k, F32, residual=resd, out=lr.nans((T, d), F32)))
    ref, mag = oc.combine_ref(y, inv, score, res, T, k)
    assert note("gather_combine_ln", f"out d={d} k={k}", lr.worst((out.cpu().double() - ref).abs(), lr._combine_bound(ref, mag, k, F32))) <= 1.0
    ref_xn = torch.nn.functional.layer_norm(out.cpu().double(), (d,), w_.double(), b_.double(), oc.EPS)
    e, bar = float((xn.cpu().double() - ref_xn).abs().max()), (2e-3 if ndt == F16 else 1.6e-2) * max(1.0, float(ref_xn.abs().max()))
    assert note("gather_combine_ln", f"xn d={d} k={k} {DT_IDS[ndt]} NJ={oc.combine_ln_nj(d)}", e / bar) <= 1.0, (e, bar)


@pytest.mark.parametrize("dtype,tol", [(F16, 2e-3), (F32, 1e-5)], ids=["f16", "f32"])
@pytest.mark.parametrize("C", oc.COLSUM_CS)
def test_group_colsum_off_grid_widths(C, dtype, tol):
    """test_group_colsum_many_chunks_and_empty_groups's bar and determinism, at C % 8 != 0 and C > 1024"""
    offsets = np.concatenate([[0], np.cumsum(oc.COLSUM_COUNTS)]).astype(np.int32)
    n = int(offsets[-1])
    src = (torch.randn(n + 5, C, generator=oc.gen(C)) * 0.5).to(dtype)      # rows past offsets[E] are ignored
    srcd, offd = dev(src, torch.from_numpy(offsets))
    lr.poison(4 * len(oc.COLSUM_COUNTS) * C)
    got = ops.group_colsum(srcd, offd)
    assert lr.same_bits(got, ops.group_colsum(srcd, offd))
    worst = 0.0
    for e, cnt in enumerate(oc.COLSUM_COUNTS):
        ref = src[offsets[e]:offsets[e + 1]].double().sum(0)
        worst = max(worst, float((got[e].cpu().double() - ref).abs().max()) / (tol * max(1.0, float(ref.abs().max()))))
        if cnt == 0:
            assert bool((got[e] == 0).all()), "an empty group sums to zero"
    assert note("group_colsum", f"C={C} {DT_IDS[dtype]}", worst) <= 1.0


@pytest.mark.parametrize("E", oc.SWITCH_BWD_ES)
def test_switch_gate_bwd_many_experts(E):
    """test_switch_gate_bwd_matches_autograd...'s bar, max |diff| <= 2e-6 max(1, max |ref|), with both terms and with either alone"""
    T = ROWS
    logits, idx, dscore, coef = oc.switch_bwd_inputs(T, E)
    probs = torch.softmax(logits, -1)
    for use_ds, use_cf in ((True, True), (True, False), (False, True)):
        ref = oc.switch_bwd_ref(logits, idx, dscore if use_ds else torch.zeros(T), coef if use_cf else torch.zeros(E))
        lr.poison(4 * T * E)
        got = ops.switch_gate_bwd(*dev(probs, idx), dev(dscore) if use_ds else None, dev(coef) if use_cf else None)
        e = float((got.cpu().double() - ref).abs().max()) / (2e-6 * max(1.0, float(ref.abs().max())))
        assert note("switch_gate_bwd", f"E={E} dscore={use_ds} coef={use_cf}", e) <= 1.0


@pytest.mark.parametrize("E", oc.PLAN_ES)
@pytest.mark.parametrize("n", oc.PLAN_NS)
def test_dispatch_plan_around_its_fused_form_and_past_the_workgroup_size(n, E):
    """bit-equal to the oracle, with and without a capacity of 3, on random ids and on ids that all name the last expert; the entry
    point is called on outputs pre-filled with a value no plan contains (test_dispatch_plan_tail_fill_on_both_sides_of_its_grid_cap)"""
    lib = _lib.load()
    for kind in ("random", "last"):
        ids = oc.plan_ids(n, E, kind)
        flat = torch.from_numpy(ids).to(DEV)
        for cap in oc.PLAN_CAPS:
            p = mo.dispatch_plan(ids, E, cap)
            ws_bytes = lib.smoe_dispatch_plan_workspace_bytes(n, E)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
            counts, offsets = (torch.full((m,), lr.NOT_A_PLAN, dtype=torch.int32, device=DEV) for m in (E, E + 1))
            pos, inv_pos, pruned = (torch.full((n,), lr.NOT_A_PLAN, dtype=torch.int64, device=DEV) for _ in range(3))
            _lib.check(lib.smoe_dispatch_plan(flat.data_ptr(), n, E, cap, counts.data_ptr(), offsets.data_ptr(), pos.data_ptr(),
                                              inv_pos.data_ptr(), pruned.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream(flat)),
                       "smoe_dispatch_plan")
            tag = (n, E, kind, cap)
            assert np.array_equal(counts.cpu().numpy(), p.counts), tag
            assert np.array_equal(offsets.cpu().numpy(), p.offsets), tag
            assert np.array_equal(pos.cpu().numpy(), p.pos), tag
            assert np.array_equal(inv_pos.cpu().numpy(), p.inv_pos), tag
            assert np.array_equal(pruned.cpu().numpy(), p.idx_pruned), tag


# ================================================================================================ 3. grouped GEMM, f32 operands, K % 64 != 0
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("gelu", [False, True], ids=["none", "gelu"])
@pytest.mark.parametrize("N", oc.GEMM_NS)
@pytest.mark.parametrize("K", oc.GEMM_KS)
def test_grouped_gemm_f32_operands_off_the_64_grid(K, N, gelu, with_bias):
    """variant 0 and variant 9 (which the library rewrites to 0 for these operands) are the same bits; both inside the 2e-5 x
    max(1, max |ref|) of test_grouped_gemm_matches_fp64_reference; rows past the last offset keep their sentinel"""
    A, W, bias, offsets = oc.gemm_inputs(K, N)
    bias = bias if with_bias else None
    M = int(offsets[-1])
    Ad, Wd, bd, offd = dev(A, W, bias, torch.from_numpy(offsets))
    outs = []
    for variant in (0, 9):
        out = torch.full((M + oc.GEMM_PAD, N), 7.0, dtype=F32, device=DEV)
        ops.grouped_gemm(Ad, Wd, bd, offd, ops.EPI_GELU if gelu else ops.EPI_NONE, out=out, variant=variant)
        outs.append(out)
    assert lr.same_bits(outs[0], outs[1]), "variant 9 with f32 operands must be variant 0"
    ref = oc.gemm_ref(A, W, bias, offsets, gelu)
    got = outs[0].cpu().double()
    e = float((got[:M] - ref).abs().max()) / (oc.GEMM_TOL * max(1.0, float(ref.abs().max())))
    assert note("grouped_gemm_f32", f"K={K} N={N} gelu={gelu} bias={with_bias}", e) <= 1.0
    assert bool((got[M:] == 7.0).all()), "rows past the last expert must stay untouched"


# ================================================================================================ 4. the layer
def _layer(d, h, E, k, params, switch=False, compute_dtype=None):
    x, wg, bg, w1, b1, w2, b2, _ = params
    kw = dict(gate="switch", capacity_factor=1.0) if switch else {}
    mod = sm.FMoETransformerMLP(E, d, h, torch.nn.GELU(), top_k=k, compute_dtype=compute_dtype, **kw).to(DEV)
    if switch:
        mod.gate.switch_eps = 0.0          # no jitter: oracle and device see the same logits
    with torch.no_grad():
        mod.gate.gate.weight.copy_(wg); mod.gate.gate.bias.copy_(bg)
        mod.experts.htoh4.weight.copy_(w1); mod.experts.htoh4.bias.copy_(b1)
        mod.experts.h4toh.weight.copy_(w2); mod.experts.h4toh.bias.copy_(b2)
    return mod


def _layer_case(case):
    d, h, E, k = case
    switch = case == oc.LAYER_SWITCH
    return d, h, E, k, switch, oc.layer_params(oc.LAYER_T, d, h, E, seed=d + E, skew=switch)


def _eval_against_oracle(mod, params, k, switch, what):
    x, wg, bg, w1, b1, w2, b2, _ = params
    T, E = x.shape[0], wg.shape[0]
    mod.eval()
    with torch.no_grad():
        out = mod(x.to(DEV))
    gate, cap = (mo.GATE_SWITCH, mo.switch_capacity(1.0, T, 1, E)) if switch else (mo.GATE_NAIVE, -1)
    r = mo.moe_forward(x, wg, bg, w1, b1, w2, b2, k, gate, cap, dtype=torch.float64)
    idx, _, counts, _, pos, _ = mod.last_plan
    assert torch.equal(idx.cpu(), r.idx), "routing indices differ from the oracle"
    assert np.array_equal(pos.cpu().numpy(), r.plan.pos), "permutation differs from the oracle"
    assert np.array_equal(counts.cpu().numpy(), r.plan.counts)
    max_abs, scale, rel_l2 = float_bar(out.cpu(), r.out)
    note("layer", what, max(max_abs / scale, rel_l2) / (1e-3 * dtype_factor()))
    return r


@pytest.mark.parametrize("case", oc.LAYER_CASES + [oc.LAYER_SWITCH], ids=lambda c: "d%d-h%d-E%d-k%d" % c)
def test_layer_eval_forward_off_the_grid(case):
    """idx, pos and counts bit-equal to mo.moe_forward; the output at _mp.float_bar"""
    d, h, E, k, switch, params = _layer_case(case)
    r = _eval_against_oracle(_layer(d, h, E, k, params, switch), params, k, switch, f"eval d={d} h={h} E={E} k={k}")
    if switch:
        assert (r.plan.idx_pruned < 0).sum() > 0, "the capacity must drop tokens"


def test_layer_eval_forward_f32_compute_reaches_the_f32_gemm():
    d, h, E, k = oc.LAYER_F32
    params = oc.layer_params(oc.LAYER_T, d, h, E, seed=d + E)
    _eval_against_oracle(_layer(d, h, E, k, params, compute_dtype=F32), params, k, False, f"eval f32 compute d={d} h={h}")


@pytest.mark.parametrize("case", oc.LAYER_CASES + [oc.LAYER_SWITCH], ids=lambda c: "d%d-h%d-E%d-k%d" % c)
def test_layer_training_step_off_the_grid(case, monkeypatch):
    """out and the seven gradients against float64 autograd through mo.moe_forward_diff at 2e-3 / 5e-3 x dtype_factor(), as
    test_naive_gate_backward_matches_autograd / test_cfg5_switch_capacity_aux_backward (the switch case with 3 x aux in the loss)"""
    d, h, E, k, switch, params = _layer_case(case)
    x, wg, bg, w1, b1, w2, b2, gout = params
    T = x.shape[0]
    mod = _layer(d, h, E, k, params, switch).train()
    calls = collections.Counter()
    for name in ("gate_dgrad", "gate_wgrad"):
        def spy(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    xg = x.to(DEV).requires_grad_(True)
    out = mod(xg)
    loss = (out * gout.to(DEV)).sum()
    if switch:
        aux = mod.gate.get_loss()
        loss = loss + 3.0 * aux
    loss.backward()
    leaves = [t.clone().requires_grad_(True) for t in (x, wg, bg, w1, b1, w2, b2)]
    if switch:
        ro, raux, plan = mo.moe_forward_diff(*leaves, 1, mo.GATE_SWITCH, mo.switch_capacity(1.0, T, 1, E))
        ((ro * gout.double()).sum() + 3.0 * raux).backward()
        assert (plan.idx_pruned < 0).sum() > 0
        assert abs(float(aux) - float(raux)) < 1e-4
    else:
        ro, _, plan = mo.moe_forward_diff(*leaves, k)
        (ro * gout.double()).sum().backward()
    assert np.array_equal(mod.last_plan[4].cpu().numpy(), plan.pos)
    e_out = lr.rel(out.detach().cpu(), ro.detach())
    assert note("layer", f"train out d={d} h={h} E={E} k={k}", e_out / (2e-3 * dtype_factor())) <= 1.0
    got = [xg.grad, mod.gate.gate.weight.grad, mod.gate.gate.bias.grad, mod.experts.htoh4.weight.grad,
           mod.experts.htoh4.bias.grad, mod.experts.h4toh.weight.grad, mod.experts.h4toh.bias.grad]
    for name, gt, rf in zip(["x", "wg", "bg", "w1", "b1", "w2", "b2"], got, leaves):
        if k == 1 and not switch and name in ("wg", "bg"):
            assert gt is None or float(gt.abs().max()) == 0.0      # top-1 naive gate: score == 1, no router gradient
            continue
        assert note("layer", f"train d{name} d={d} h={h} E={E} k={k}", lr.rel(gt.cpu(), rf.grad) / (5e-3 * dtype_factor())) <= 1.0, name
    if k > 1 or switch:
        # the router's backward: dx through the own streaming kernel at every E; the weight gradient through the own kernel up to
        # 16 experts and through torch above (autograd._GateLogits.backward)
        assert calls["gate_dgrad"] == 1, calls
        assert calls["gate_wgrad"] == (1 if E <= oc.GATE_WGRAD_MAX_E else 0), calls


def test_gate_logits_backward_branches_agree_at_33_experts():
    """ops.profile_begin records no router-backward launch, so the two branches of autograd._GateLogits.backward are called directly
    at the shape of the E = 33 layer case: the own kernels (gate_dgrad_any_kernel on its second column trip; gate_wgrad has no E > 16
    form and is refused) against the torch expressions of the other branch and against float64"""
    d, h, E, k = oc.LAYER_CASES[3]
    g = oc.gen(E)
    dl, w, x = torch.randn(oc.LAYER_T, E, generator=g), torch.randn(E, d, generator=g) * 0.05, torch.randn(oc.LAYER_T, d, generator=g)
    dld, wd, xd = dev(dl, w, x)
    own = ops.gate_dgrad(dld, wd, F32)
    torch_branch = dld @ wd.float()
    ref = dl.double() @ w.double()
    e_own, e_torch = lr.rel(own.cpu(), ref), lr.rel(torch_branch.cpu(), ref)
    print(f"gate logits backward E={E} d={d}: dx relative L2 own {e_own:.2e}, torch {e_torch:.2e}")
    assert note("gate_dgrad", f"E={E} d={d} against the torch branch", e_own / 1e-6) <= 1.0
    assert e_torch <= 1e-6                                                        # (hipBLASLt may use reduced-precision passes: not bit-equal)
    dw_torch = dld.t() @ xd.float()
    assert lr.rel(dw_torch.cpu(), dl.double().t() @ x.double()) <= 1e-5


# ================================================================================================ 5. one block through the Python seams
def _what(msgs):
    return {m.split(": shape")[0] for m in msgs}


@pytest.mark.parametrize("cfg", sorted(oc.BLOCK_CONFIGS))
def test_one_block_through_the_python_seams(cfg):
    """A one-block ViT whose widths leave some of the dense kernels: eval under fp16 autocast and one training step.  The recorded
    SlimMoEFallbackWarnings name exactly the seams the configuration is outside of (oc.BLOCK_CONFIGS says why), never the MoE half;
    the block's output, in eval and inside the training step, meets _mp.float_bar against mo.block_forward teacher-forced with the
    GPU's own routing."""
    import warnings
    from slim_switch_moe_vit_amd import resmoe, vit
    kw, expected = oc.BLOCK_CONFIGS[cfg]
    heads = kw["num_heads"]
    torch.manual_seed(0)
    model = sm.VisionTransformer(img_size=64, depth=1, num_classes=10, **kw)
    model = resmoe.patch_blocks_with_moe(model, 4, 2, False)
    g = oc.gen(17 + heads)
    blk = model.blocks[0]
    with torch.no_grad():
        blk.mlp.gate.gate.weight.copy_(torch.randn(blk.mlp.gate.gate.weight.shape, generator=g) * 0.1)
        blk.mlp.gate.gate.bias.zero_()
        for lin in (blk.mlp.experts.htoh4, blk.mlp.experts.h4toh):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.02)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.02)
    images = torch.randn(4, 3, 64, 64, generator=g)
    p = {n_: v.detach().clone() for n_, v in blk.state_dict().items()}
    model = model.to(DEV).eval()
    blk = model.blocks[0]

    def against_oracle(x_in, y, where):
        tr = []
        ref = mo.block_forward(x_in.detach().float().cpu(), p, heads, 2, False, forced_idx=blk.mlp.last_plan[0].cpu(), trace=tr)
        max_abs, scale, rel_l2 = float_bar(y.detach().float().cpu(), ref)
        print(f"block {cfg} {where}: max |diff| {max_abs:.2e} at scale {scale:.2f}, relative L2 {rel_l2:.2e}; routing against the oracle's own: {tr}")
        note("block", f"{cfg} {where}", max(max_abs / scale, rel_l2) / (1e-3 * dtype_factor()))

    vit._fallbacks_seen.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always", vit.SlimMoEFallbackWarning)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            logits = model(images.to(DEV))                       # every seam of the eval forward: embedding, block, final norm, head
            x0 = model._embed(images.to(DEV))
            y = blk(x0)                                          # (the model's own pass runs its last block's experts for the class rows only)
        assert bool(torch.isfinite(logits).all()) and tuple(logits.shape) == (4, 10)
        against_oracle(x0, y, "eval")
        model.train()
        seen = {}
        hook = blk.register_forward_hook(lambda m, a, out: seen.update(x=a[0], y=out))
        try:
            with torch.autocast("cuda", dtype=torch.float16):
                model(images.to(DEV)).float().sum().backward()
        finally:
            hook.remove()
        against_oracle(seen["x"], seen["y"], "training step")
    for n_, q in model.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), n_
    msgs = [str(w.message) for w in rec if issubclass(w.category, vit.SlimMoEFallbackWarning)]
    print(f"block {cfg}: fallbacks {sorted(msgs)}")
    assert _what(msgs) == set(expected), (sorted(msgs), expected)
    assert not any("MLP half" in n_ or "MoE" in n_ or "mlp" in n_.lower() for n_ in _what(msgs)), msgs      # the MoE half stays on its kernels


# ================================================================================================ 6. refusals
def test_layer_refusals_are_clean_and_not_sticky():
    """d = 200 with 16-bit operands (K % 64) and top_k = 5 end in a RuntimeError that carries the library's message; the next good
    call gives the oracle's result"""
    E = 8
    cd = F16 if fmoe.default_compute_dtype() == F32 else None      # 16-bit operands whatever SLIMMOE_COMPUTE_DTYPE says
    bad_d = sm.FMoETransformerMLP(E, 200, 256, torch.nn.GELU(), top_k=2, compute_dtype=cd).to(DEV).eval()
    bad_k = sm.FMoETransformerMLP(E, 256, 256, torch.nn.GELU(), top_k=5).to(DEV).eval()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"smoe_grouped_gemm: K=200 must be a multiple of 64"):
            bad_d(torch.randn(oc.ROWS_REFUSAL, 200, device=DEV))
        with pytest.raises(RuntimeError, match=r"smoe_router_topk: k=5 out of range"):
            bad_k(torch.randn(oc.ROWS_REFUSAL, 256, device=DEV))
    torch.cuda.synchronize()
    d, h, k = 256, 256, 2
    params = oc.layer_params(oc.ROWS_REFUSAL, d, h, E, seed=5)
    _eval_against_oracle(_layer(d, h, E, k, params), params, k, False, "eval after two refusals")


# ================================================================================================ summary
def test_worst_ratios_by_kernel_family():
    """prints (pytest -s) the largest error / bar ratio of each kernel family over the cases that ran before it in this process"""
    for fam in sorted(WORST):
        print(f"worst error / bar, {fam}: {WORST[fam]:.3f}")
    assert all(v <= 1.0 for v in WORST.values()), dict(WORST)
