"""Without a GPU: (a) every float64 reference of tests/_offgrid_cases.py against an independent formulation (torch autograd for
the LayerNorm and gate backward formulas, the oracle's differentiable layer, per-expert matmuls); (b) every case list against the form
of the kernel it claims to reach, recomputed from the launch rules -- a later edit of a list cannot drop a form silently; (c) the
restated launch constants against the sources; (d) shapes just outside the library's envelope are refused by the argument checks,
before any launch, with a message that names the rule."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import moe_oracle as mo
import slim_switch_moe_vit_amd as sm  # noqa: F401
from slim_switch_moe_vit_amd import _lib
import _offgrid_cases as oc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slim-switch-moe-vit_amd", "csrc")
F = torch.nn.functional


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-300))


# ------------------------------------------------------------------------------------------ (c) constants against the sources
def test_restated_launch_constants_are_the_sources():
    r = _src("router.hip")
    assert "constexpr int ROUTER_THREADS = 256;" in r and oc.ROUTER_WAVES == 256 // 64
    assert "(logit_bytes + w_bytes) <= 64 * 1024" in r and oc.ROUTER_LDS_LIMIT == 64 * 1024
    assert "(size_t)(ROUTER_WAVES + 1) * Epad * 4 + 15) & ~(size_t)15" in r
    assert "switch ((a.d + 255) / 256)" in r and "NCH_CASE(8);" in r and "NCH_CASE(9)" not in r
    assert "d % 8 == 0 && d <= 2048" in r and "E <= 4096" in r and "constexpr int ROUTER_MAX_K = 4;" in r
    r16 = _src("router16.hip")
    assert "if (E <= 8) return d == 192 || d == 384 || d == 768 || d == 1024;" in r16
    assert "return E <= 32 && (d == 768 || d == 1024);" in r16
    dp = _src("dispatch.hip")
    assert "constexpr int PLAN_FUSED_E = 64;" in dp and "constexpr int PLAN_THREADS = 256;" in dp and "PLAN_FUSED_MAX = 8192" in dp
    assert re.search(r"constexpr int PLAN_ITERS = 4;", dp) and oc.PLAN_CH == 256 * 4
    db = _src("dense_bwd.hip")
    assert db.count("const int nj = (d / 4 + 63) / 64;") == 2
    assert "const int nj = (d + 511) / 512;" in dp
    assert "if (E <= 8) hipLaunchKernelGGL((gate_dgrad_kernel<OT, 8>)" in db and "else if (E <= 16)" in db
    assert "int threads = ((nchunk < 256 ? nchunk : 256) + 63) / 64 * 64;" in db
    assert "if (K % 64 != 0 || smoe_dtype_size(ab_dtype) != 2) variant = 0;" in _src("gemm.hip")
    with open(os.path.join(os.path.dirname(CSRC), "autograd.py")) as fh:
        assert f"dl.shape[1] <= {oc.GATE_WGRAD_MAX_E} and" in fh.read()


# ------------------------------------------------------------------------------------------ (b) the lists reach what they claim
def test_router_cases_reach_every_chunk_count_and_both_weight_placements():
    every = oc.ROUTER_CASES + [(d, E, 1) for d, E in oc.SWITCH_CASES]
    for d, E, k in every:
        assert oc.router_is_generic(d, E, k), (d, E, k)
        assert d % 8 == 0 and d <= oc.ROUTER_MAX_D and E <= oc.ROUTER_MAX_E and 1 <= k <= min(E, oc.ROUTER_MAX_K)
    nch = {oc.router_nch(d) for d, _, _ in oc.ROUTER_CASES}
    assert nch >= set(range(3, 9)), nch
    assert oc.router_nch(520) == 3 and 520 - 2 * 256 == 8                      # the last chunk is 8 columns wide
    assert oc.router_nch(776) == 4 and 9 > 8 and ((9 + 7) & ~7) - 9 == 7       # E > 8: Epad 16, seven dead experts
    at8 = {oc.router_weights_in_lds(d, E) for d, E, _ in oc.ROUTER_CASES if oc.router_nch(d) == 8}
    assert at8 == {True, False}, "NCH 8 must run with its weights in LDS and from global memory"
    assert not oc.router_weights_in_lds(2048, 7) and oc.router_weights_in_lds(2040, 8)
    assert 8 * 2040 * 4 + 160 <= 65536 < 8 * 2048 * 4 + 160                    # the two sit right at the limit
    assert {oc.router_nch(d) for d, _ in oc.SWITCH_CASES} == {5, 8}
    assert {oc.router_weights_in_lds(d, E) for d, E, _ in oc.ROUTER_CASES if oc.router_nch(d) < 8} == {True, False}
    assert any(E > 64 for _, E, _ in oc.ROUTER_CASES), "more experts than lanes: the selection loop takes a second trip"
    assert {k for _, _, k in oc.ROUTER_CASES} == {1, 2, 3, 4}
    assert {oc.router_nch(d) for d, _, _ in oc.NEAR_TIE_CASES} == set(range(3, 9))
    assert all(c in oc.ROUTER_CASES for c in oc.NEAR_TIE_CASES)
    assert (oc.ROUTER_T + 3) // 4 == 10 and oc.ROUTER_T % 4 == 1               # nine full workgroups and one wave


def test_row_kernel_cases_reach_the_later_trips_and_every_register_chunk_count():
    assert {oc.gate_dgrad_kernel(E) for _, E in oc.DGRAD_CASES} == {"regs8", "regs16", "any"}
    assert all(oc.gate_dgrad_trips(d) == 2 and d % 4 == 0 for d, _ in oc.DGRAD_CASES)
    assert any(d % 8 for d, _ in oc.DGRAD_CASES), "a width gate_dgrad takes and the d % 8 kernels do not"
    assert any(d // 4 > 256 and E > 16 for d, E in oc.DGRAD_CASES)             # gate_dgrad_any_kernel past 256 column chunks
    assert {oc.ln_nj(d) for d in oc.LN_DIMS} == {1, 2, 3, 4}
    for j in (1, 2, 3):                                                        # one 4-column chunk past every boundary d = 256 j
        assert 256 * j + 4 in oc.LN_DIMS and oc.ln_nj(256 * j + 4) == j + 1
    assert 1020 in oc.LN_DIMS and oc.ln_nj(1020) == 4 and all(d % 4 == 0 and d <= 1024 for d in oc.LN_DIMS)
    assert any(d % 8 for d in oc.LN_DIMS)
    assert {oc.combine_ln_nj(d) for d, _ in oc.COMBINE_LN_CASES} == {1, 2} and {k for _, k in oc.COMBINE_LN_CASES} == {1, 3, 4}
    assert (520, 3) in oc.COMBINE_LN_CASES and oc.combine_ln_nj(520) == 2 and 520 - 512 == 8      # one 8-column chunk past the boundary
    assert all(d % 8 == 0 and d <= 1024 and d % 512 for d, _ in oc.COMBINE_LN_CASES)               # a partly filled last chunk everywhere
    assert all(d % 8 == 0 and d not in (192, 384, 768, 1024) for d in oc.ROW_DIMS) and max(oc.ROW_DIMS) > 1024
    assert 0 in oc.COLSUM_COUNTS and 1 in oc.COLSUM_COUNTS and any(C > 1024 for C in oc.COLSUM_CS) and any(C % 8 for C in oc.COLSUM_CS)
    assert all(E > 256 for E in oc.SWITCH_BWD_ES)
    assert all(C % 4 == 0 for C, _ in oc.WGRAD_CASES) and {E for _, E in oc.WGRAD_CASES} == {1, oc.GATE_WGRAD_MAX_E}


def test_plan_cases_sit_on_both_sides_of_the_fused_form_and_the_workgroup_size():
    for n in oc.PLAN_NS:
        fused = {E: oc.plan_is_fused(n, E) for E in oc.PLAN_ES}
        assert fused[64] and not fused[65] and fused[1] and fused[63], fused
    assert {(n + oc.PLAN_CH - 1) // oc.PLAN_CH for n in oc.PLAN_NS} == {1, 2}
    assert any(oc.PLAN_THREADS < E <= 1024 for E in oc.PLAN_ES) and any(E > 1024 for E in oc.PLAN_ES)   # histogram / scan loops: 2+ trips
    assert max(oc.PLAN_ES) == 8192 and min(oc.PLAN_ES) == 1
    for n in oc.PLAN_NS:
        for E in oc.PLAN_ES:
            ids = oc.plan_ids(n, E, "last")
            assert ids.min() == ids.max() == E - 1
            p = mo.dispatch_plan(oc.plan_ids(n, E, "random"), E, 3)
            if E <= 65:
                assert (p.idx_pruned < 0).sum() > n // 50, "a capacity of 3 must drop entries"


def test_gemm_and_layer_cases_reach_the_f32_override_and_the_python_seams():
    assert all(K % 32 == 0 and K % 64 != 0 for K in oc.GEMM_KS) and all(N % 8 == 0 for N in oc.GEMM_NS)
    assert 0 in oc.GEMM_COUNTS and 1 in oc.GEMM_COUNTS and max(oc.GEMM_COUNTS) > 128
    for d, h, E, k in oc.LAYER_CASES + [oc.LAYER_SWITCH]:
        assert d % 64 == 0 and h % 64 == 0 and d not in (192, 384, 768, 1024), (d, h)     # 16-bit GEMMs take them; off the grid
        assert oc.router_is_generic(d, E, k)
    d, h, E, k = oc.LAYER_CASES[3]
    assert E > oc.GATE_WGRAD_MAX_E and oc.gate_dgrad_kernel(E) == "any" and oc.gate_dgrad_trips(d) == 2 and k > 1
    assert {oc.router_nch(c[0]) for c in oc.LAYER_CASES} >= {1, 2, 3, 5, 8}
    d, h, E, k = oc.LAYER_F32
    assert d in oc.GEMM_KS and h in oc.GEMM_KS


def test_block_configurations_leave_exactly_the_seams_they_list():
    """the expected fallback names of oc.BLOCK_CONFIGS recomputed from the predicates the Python layer applies: ops.LN_DIMS (patch
    embedding tail, LayerNorms), K % 64 (dense.linear_supported) and the attention kernels' own answer"""
    from slim_switch_moe_vit_amd import ops
    lib = _lib.load()
    seen = set()
    for name, (kw, expected) in oc.BLOCK_CONFIGS.items():
        d, heads, ps = kw["embed_dim"], kw["num_heads"], kw["patch_size"]
        n_tok = (oc.BLOCK_IMG // ps) ** 2 + 1
        hd = d // heads
        assert d % heads == 0 and oc.BLOCK_IMG % ps == 0
        ln_off = d not in ops.LN_DIMS
        patch_off = ps % 4 != 0 or d not in ops.LN_DIMS
        attn_off = not (lib.smoe_attention_supported(n_tok, hd) and lib.smoe_attention_bwd_supported(n_tok, hd))
        linear_off = any(K % 64 for K in (d, 3 * ps * ps, 4 * d))            # qkv / proj / head, patch GEMM, expert GEMMs
        want = set()
        if patch_off:
            want.add("patch embedding")
        if attn_off:
            want |= {"attention", "attention (training)"}
        assert not linear_off, name
        assert want == set(expected), (name, want, expected)
        seen.add((ln_off, patch_off, attn_off))
    assert (True, True, False) in seen and (False, False, True) in seen, seen


# ------------------------------------------------------------------------------------------ (a) references
@pytest.mark.parametrize("T", oc.LN_TS)
@pytest.mark.parametrize("d", oc.LN_DIMS)
def test_layernorm_backward_reference_is_autograd(d, T):
    x, w, b, dy, dres = oc.ln_inputs(T, d)
    xr, wr, br = [t.double().requires_grad_(True) for t in (x, w, b)]
    (F.layer_norm(xr, (d,), wr, br, oc.EPS) * dy.double()).sum().backward()
    ref = oc.ln_bwd_ref(x, w, dy, dres)
    assert _rel(ref["dx"], xr.grad + dres.double()) < 1e-12 and _rel(ref["dw"], wr.grad) < 1e-12 and _rel(ref["db"], br.grad) < 1e-12
    assert _rel(oc.ln_bwd_ref(x, w, dy)["dx"], xr.grad) < 1e-12


@pytest.mark.parametrize("mode", oc.GATE_MODES)
@pytest.mark.parametrize("d,T", [(8, 1), (100, 37), (260, 37), (1020, 37)])
def test_gate_layernorm_backward_reference_is_autograd_of_the_gate_expressions(d, T, mode):
    """the reference's gate expressions (models/resMoE.py:59-85 as tests/test_gpu_launch_regimes.py and tests/_soft_gate_cases.py
    restate them): hard = straight-through estimator, soft = (1 - p, p), off = the mask (0, 1)"""
    x, gam, bet, w, b, g_f, g_out = oc.gate_ln_inputs(T, d)
    xr, gr, btr, wr, br = [t.double().requires_grad_(True) for t in (x, gam, bet, w, b)]
    xn = F.layer_norm(xr, (d,), gr, btr, oc.EPS)
    z = xn @ wr + br
    z.retain_grad()
    prob = torch.sigmoid(z)[:, None]
    if mode == "hard":
        _prob = 1 - prob
        skip_tk = (prob > oc.GATE_THR).double() + _prob.detach() - _prob
        tk = (prob <= oc.GATE_THR).double() + prob.detach() - prob
    elif mode == "soft":
        skip_tk, tk = 1 - prob, prob
    else:
        skip_tk, tk = torch.zeros_like(prob), torch.ones_like(prob) + 0.0 * prob
    ((g_f.double() * (xn * tk)).sum() + (g_out.double() * (xn * tk + xn * skip_tk)).sum()).backward()
    ref = oc.gate_ln_bwd_ref(x, gam, bet, w, b, g_f, g_out, mode)
    for name, want in (("dx", xr.grad), ("dgamma", gr.grad), ("dbeta", btr.grad), ("dgate_w", wr.grad), ("dgate_b", br.grad),
                       ("dz", z.grad)):
        if mode == "off" and name in ("dgate_w", "dgate_b", "dz"):
            assert float(ref[name].abs().max()) == 0.0 and float(want.abs().max()) == 0.0
        else:
            assert _rel(ref[name], want) < 1e-11, (name, _rel(ref[name], want))
    if mode == "hard":
        assert torch.equal(ref["mask"], torch.cat([(prob > oc.GATE_THR).float(), (prob <= oc.GATE_THR).float()], dim=1).detach().float())
        if T > 1:
            assert 0 < int(ref["mask"][:, 0].sum()) < T, "both decisions must occur"
    if mode == "soft":
        assert float((ref["mask"].double().sum(1) - 1).abs().max()) < 1e-6


def test_the_one_measured_gate_bar_belongs_to_the_one_cancelling_row():
    """GLNB_MEASURED_BARS: the case listed there is the only single-row case whose <g_f, xn> cancels badly (float64, so the same on
    every machine), the torch f32 evaluation of the same expressions misses the 8e-7 bar there as well, and nowhere else"""
    for d in oc.LN_DIMS:
        for gdt in (oc.F32, oc.F16):
            a = oc.gate_ln_inputs(1, d, gdt)
            x, gam, bet, w, b, g_f, g_out = a
            xhat, _ = oc._ln_stats(x)
            terms = g_f.double() * (xhat * gam.double() + bet.double())
            cond = float(terms.abs().sum() / terms.sum().abs())
            assert (cond > 200) == (d == 772), (d, cond)
            assert d == 772 or cond < 20, (d, cond)
    assert set(oc.GLNB_MEASURED_BARS) == {(772, 1, oc.F32)} and set(oc.GLNB_MEASURED_BARS[(772, 1, oc.F32)]) == {"dz", "dgate_w"}
    # the f32 evaluation the bar was measured with is the reference's own code: in float64 it must BE the reference
    a = oc.gate_ln_inputs(1, 772)
    r = oc.gate_ln_bwd_ref(*a, "soft")
    same = oc.gate_ln_bwd_ref(*a, "soft", dt=torch.float64, mask=r["mask"])
    assert all(_rel(same[n], r[n]) < 1e-7 for n in ("dx", "dgamma", "dbeta", "dgate_w", "dz"))      # (keep = the f32 mask's p)
    f32 = oc.gate_ln_bwd_ref(*a, "soft", dt=torch.float32, mask=r["mask"])
    assert f32["dz"].dtype == torch.float32 and _rel(f32["dx"], r["dx"]) < 2e-6


def test_combine_rowdot_switch_and_gemm_references_against_loops_and_autograd():
    T, k, d = 9, 3, 16
    y, inv, score, res = oc.combine_inputs(T, k, d, oc.F16, oc.F32)
    out, mag = oc.combine_ref(y, inv, score, res, T, k)
    for t in range(T):
        acc, m = res[t].double().clone(), res[t].double().abs()
        for j in range(k):
            if inv[t * k + j] >= 0:
                term = float(score[t * k + j]) * y[inv[t * k + j]].double()
                acc, m = acc + term, m + term.abs()
        assert torch.allclose(out[t], acc, rtol=1e-14, atol=0) and torch.allclose(mag[t], m, rtol=1e-14, atol=0)
    assert bool((inv < 0).any())
    dout, yy, inv2 = oc.rowdot_inputs(20, 2, 16, oc.F32, oc.F16)
    ref, s = oc.rowdot_ref(dout, yy, inv2, 2)
    for i in range(20):
        want = float(dout[i // 2].double() @ yy[inv2[i]].double()) if inv2[i] >= 0 else 0.0
        assert abs(float(ref[i]) - want) <= 1e-13 * max(1.0, float(s[i]))
    assert oc.rowdot_fmas(8) * 64 == 8 + 6 * 64 and oc.rowdot_fmas(1024) == 22        # d <= 1024: the 16 + 6 of tests/test_gpu_nonfinite.py
    logits, idx, dscore, coef = oc.switch_bwd_inputs(37, 257)
    l64 = logits.double().requires_grad_(True)
    p64 = torch.softmax(l64, -1)
    sel = idx >= 0
    ((dscore.double()[sel] * p64[sel, idx[sel]]).sum() + (p64 * coef.double()).sum()).backward()
    assert _rel(oc.switch_bwd_ref(logits, idx, dscore, coef), l64.grad) < 1e-12 and bool((~sel).any())
    for gelu in (False, True):
        A, W, bias, offsets = oc.gemm_inputs(96, 72)
        ref = oc.gemm_ref(A, W, bias, offsets, gelu)
        for e in range(len(oc.GEMM_COUNTS)):
            lo, hi = int(offsets[e]), int(offsets[e + 1])
            v = A[lo:hi].double() @ W[e].double().t() + bias[e].double()
            assert torch.allclose(ref[lo:hi], F.gelu(v) if gelu else v, rtol=1e-13, atol=1e-15)
        assert ref.shape[0] == sum(oc.GEMM_COUNTS) == A.shape[0] - oc.GEMM_PAD


def test_router_bound_and_ulp_helpers():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 1e-3], dtype=torch.float64)
    want = torch.tensor([float(torch.nextafter(torch.tensor(abs(t), dtype=torch.float32), torch.tensor(float("inf"))) - abs(t))
                         for t in v.float().tolist()], dtype=torch.float64)
    assert torch.equal(oc.f32_ulp(v.float().double()), want)
    for d, E, k in oc.ROUTER_CASES:
        x, wg, bg = oc.router_inputs(d, E, k)
        ref = oc.router_logits64(x, wg, bg)
        assert torch.equal(ref.float(), mo.router_logits(x, wg, bg))              # the oracle rounds the same float64 sums
        b = oc.router_logit_bound(x, wg, ref)
        # an f32 matmul in another summation order sits inside it, and it is no looser than the count of roundings it states
        assert float(((x @ wg.t() + bg).double() - ref).abs().div(b).max()) < 1.0
        row = x.double().norm(dim=1) * wg.double().norm(dim=1).max()
        assert float((b / row[:, None]).max()) <= (4 * oc.router_nch(d) + 7) * oc.U + 2.0 ** -22, (d, E)
    for d, E, k in oc.NEAR_TIE_CASES:
        x, wg, bg = oc.near_tie_inputs(d, E)
        lg = oc.router_logits64(x, wg, bg)
        gap = (lg[:, E - 1] - lg[:, 0]).abs()
        assert 0 < float(gap.max()) < 1e-7 and int((wg[E - 1] != wg[0]).sum()) == 1 and (d - 3) // 256 == oc.router_nch(d) - 1


@pytest.mark.parametrize("case", [oc.LAYER_CASES[0], oc.LAYER_SWITCH], ids=["naive", "switch"])
def test_layer_inputs_make_the_oracles_two_forms_agree(case):
    """moe_forward (the eval reference of section 4) against moe_forward_diff (its training reference), on section 4's own draws"""
    d, h, E, k = case
    switch = case is oc.LAYER_SWITCH
    x, wg, bg, w1, b1, w2, b2, _ = oc.layer_params(oc.LAYER_T, d, h, E, seed=d + E, skew=switch)
    gate, cap = (mo.GATE_SWITCH, mo.switch_capacity(1.0, oc.LAYER_T, 1, E)) if switch else (mo.GATE_NAIVE, -1)
    r = mo.moe_forward(x, wg, bg, w1, b1, w2, b2, k, gate, cap, dtype=torch.float64)
    ro, _, plan = mo.moe_forward_diff(x, wg, bg, w1, b1, w2, b2, k, gate, cap)
    # (moe_forward takes its combine weights from the f32 logits the routing contract rounds to: 2^-24 relative, not float64's)
    assert np.array_equal(plan.pos, r.plan.pos) and _rel(r.out, ro) < 4 * oc.U
    if switch:
        assert (plan.idx_pruned < 0).sum() > 0, "the skewed router must overflow the capacity"


# ------------------------------------------------------------------------------------------ (d) refusals
def test_shapes_outside_the_envelope_are_refused_before_any_launch():
    """Fake non-null pointers (never dereferenced: a check that let one of these through would fail to launch here and could not
    produce the message): the return is non-zero and smoe_last_error names the rule."""
    lib = _lib.load()
    cases = oc.refusal_calls(lib)
    assert len(cases) == 12
    for label, call, words in cases:
        rc = call()
        msg = lib.smoe_last_error()
        assert rc != 0, label
        assert all(w in msg for w in words), (label, msg)
