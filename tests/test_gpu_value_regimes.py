"""Value regimes: the LayerNorm family and the attention kernels on inputs that are NOT benign Gaussian data, against float64 and the
bars of tests/test_value_regimes_host.py (which owns the inputs, the references, the emulations the bars come from, and the
argument for each bar).  A fourth regime family next to test_gpu_nonfinite.py, test_gpu_launch_regimes.py and
test_gpu_size_regimes.py.  What a benign input cannot tell apart and these can: a variance taken in one pass (E[x^2] - E[x]^2), a
rescale of the online softmax that is thresholded, skipped or applied to the denominator only, a key mask that is wrong only when
the last valid key carries the row, stale LDS behind keys whose probability is exactly 0.

    entry point                          classes                       widths / lengths            checked
    ops.layernorm                        all 9 LayerNorm classes       d 192 384 768 1024          f32 in -> f32 f16 bf16, f16 in -> f32 f16: per-row bar
    ops.layernorm_rows (stride d + 8)    all 9                         d 192 384 768 1024          per-row bar; the bits of ops.layernorm
    ops.embed_ln, embed_ln2 form         all 9 (tokens + pos_embed,    d 192 384 768 1024          x32 = the f32 sum bit for bit; xn per-row bar (f16); the
                                         large, of opposite sign)                                  bits of ops.layernorm
    ops.gather_combine_ln (k = 2)        all 9 (two expert rows        d 192 384 768 1024          out = gather_combine bit for bit; xn per-row bar (f16);
                                         cancelling the residual)                                  d >= 768: the bits of ops.layernorm
    ops.ln_router_topk                   all 9                         E 4 8: every d              xn32 per-row bar; xn16 = xn32.half(); routing = the
                                                                       E 16 32: d 768 1024         oracle's on the kernel's own xn32
    ops.gate_ln_router                   all 9                         d 192 384 768 1024, E 4     the same, and the skip decisions = the oracle's
    ops.layernorm_bwd, ops.gate_ln_bwd   all 9, each its own call      d 192 384 768 1024          f32 and f16 dy: relative L2 per class; the gate's dz and
    (+ ops.skip_gate_bwd's dz)                                                                     weight gradient too (a saturated gate: out1e3, out1e4)
    ops.attention + ops.attention_bwd    all 6 attention classes       N 197 256 257 300 577 640   f16 bf16, per head: out lse dq dk dv against the bars;
                                                                                                   exact zeros, dense.AttentionFn's bits, determinism

The tests print what they measure; profiles/r11_value_regimes.md holds the tables."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import moe_oracle as mo  # noqa: E402
from slim_switch_moe_vit_amd import dense, ops  # noqa: E402
import test_value_regimes_host as vh  # noqa: E402

DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
R = vh.ROWS
LN_CASES = [(c, d) for c in vh.LN_CLASSES for d in vh.DIMS]
ln_cases = pytest.mark.parametrize("cls,d", LN_CASES, ids=[f"{c}-d{d}" for c, d in LN_CASES])


def _dev(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


def _assert_ln(got, rows, gamma, beta, odt, what):
    """`got` against the float64 LayerNorm of `rows` (read as they are) and the per-row bar; a constant row gives beta, rounded"""
    ref = vh.ln_f64(rows.cpu(), gamma, beta)
    r = float(vh.ln_ratio(got, ref, gamma, odt).max())
    print(f"{what} -> {vh._dn(odt)}: worst error / bar {r:.3f}")
    assert r <= 1.0, (what, odt, r)
    return r


# ====================================================================================================== LayerNorm forward family
@ln_cases
def test_layernorm(cls, d):
    x, (gamma, beta) = vh.ln_rows(cls, d), vh.ln_params(d)
    gd, bd = _dev(gamma, beta)
    for xin, outs in ((x, (F32, F16, BF16)), (x.half(), (F32, F16))):
        for odt in outs:
            got = ops.layernorm(xin.to(DEV), gd, bd, vh.EPS, odt)
            _assert_ln(got, xin, gamma, beta, odt, f"layernorm {cls} d {d} {vh._dn(xin.dtype)}")
            if cls == "const":
                assert torch.equal(got.cpu(), beta.to(odt).expand(R, d)), "variance 0: the output is beta"
    if d >= 768:     # one wave per row: the same bits whatever the store
        assert torch.equal(ops.layernorm(x.to(DEV), gd, bd, vh.EPS, F16), ops.layernorm(x.to(DEV), gd, bd, vh.EPS, F32).half())


@ln_cases
def test_layernorm_rows_with_a_row_stride(cls, d):
    x, (gamma, beta) = vh.ln_rows(cls, d), vh.ln_params(d)
    gd, bd = _dev(gamma, beta)
    stride = d + 8
    buf = torch.full((R, stride), 1e30)          # what lies between the rows must not reach the statistics
    buf[:, :d] = x
    got = ops.layernorm_rows(buf.to(DEV), stride, R, d, gd, bd, vh.EPS)
    _assert_ln(got, x, gamma, beta, F32, f"layernorm_rows {cls} d {d}")
    assert torch.equal(got, ops.layernorm(x.to(DEV), gd, bd, vh.EPS, F32)), "the bits of smoe_layernorm"


@pytest.mark.parametrize("dist", [False, True], ids=["embed_ln", "embed_ln2"])
@ln_cases
def test_embed_ln_of_large_parts_of_opposite_sign(cls, d, dist):
    """tokens = -+(256 + noise) in f16, pos_embed = class row - tokens (about class row +- 256): the f32 stream is their sum bit for
    bit (one rounding away from the class row) and its LayerNorm is inside the bar of THAT stream."""
    x, (gamma, beta) = vh.ln_rows(cls, d), vh.ln_params(d)
    gd, bd = _dev(gamma, beta)
    npre = 2 if dist else 1
    P = R - npre
    g = torch.Generator().manual_seed(d + npre)
    sign = -1.0 if float(x.mean()) >= 0 else 1.0                       # against the rows' own offset: pos_embed then has its sign
    part = (sign * (256 + 4 * torch.randn(R, d, generator=g))).half()  # [cls (, dist), tokens] before pos_embed
    pos = x - part.float()
    want = part.float() + pos
    assert float((want - x).abs().max()) <= 2.0 ** -23 * float(pos.abs().max())
    cls_tok, tok = part[0].float(), part[npre:].contiguous()
    x32, xn = ops.embed_ln(tok.to(DEV), cls_tok.to(DEV), pos.to(DEV), 1, P, ln=(gd, bd, vh.EPS),
                           dist_token=part[1].float().to(DEV) if dist else None)
    assert torch.equal(x32.cpu()[0], want)
    _assert_ln(xn[0], want, gamma, beta, F16, f"embed_ln{'2' if dist else ''} {cls} d {d}")
    assert torch.equal(xn[0], ops.layernorm(want.to(DEV), gd, bd, vh.EPS, F16)), "the bits of smoe_layernorm"


@ln_cases
def test_gather_combine_ln_of_expert_rows_that_cancel_the_residual(cls, d):
    """k = 2: residual = class row - (0.75 y0 + 0.5 y1) with y about -128: the combined f32 row is the class row to rounding at the
    residual's magnitude, bit for bit smoe_gather_combine's; its LayerNorm is inside the bar of THAT row."""
    x, (gamma, beta) = vh.ln_rows(cls, d), vh.ln_params(d)
    gd, bd = _dev(gamma, beta)
    g = torch.Generator().manual_seed(3 * d + 1)
    y = (-128 + 2 * torch.randn(2 * R, d, generator=g)).half()
    inv = torch.randperm(2 * R, generator=g)
    score = torch.tensor([0.75, 0.5]).repeat(R, 1)
    mix = (score[:, :, None].double() * y[inv].reshape(R, 2, d).double()).sum(1)
    res = (x.double() - mix).float()
    yd, invd, sd, resd = _dev(y, inv, score, res)
    out, xn = ops.gather_combine_ln(yd, invd, sd, R, 2, resd, gd, bd, vh.EPS, F16)
    assert torch.equal(out, ops.gather_combine(yd, invd, sd, R, 2, F32, residual=resd))
    assert float((out.cpu().double() - (res.double() + mix)).abs().max()) <= 3 * 2.0 ** -24 * float(res.abs().max() + mix.abs().max())
    _assert_ln(xn, out, gamma, beta, F16, f"gather_combine_ln {cls} d {d}")
    if d >= 768:
        assert torch.equal(xn, ops.layernorm(out, gd, bd, vh.EPS, F16)), "wave-per-row LayerNorms share their bits"


ROUTER_CASES = [(c, d, E, k) for c in vh.LN_CLASSES for d in vh.DIMS for E, k in ((4, 2), (8, 1), (16, 2), (32, 1)) if E <= 8 or d >= 768]


def _router_params(d, E):
    g = torch.Generator().manual_seed(11 * d + E)
    return torch.randn(E, d, generator=g) * 0.1, torch.randn(E, generator=g) * 0.1


@pytest.mark.parametrize("cls,d,E,k", ROUTER_CASES, ids=[f"{c}-d{d}-E{E}-k{k}" for c, d, E, k in ROUTER_CASES])
def test_ln_router_topk(cls, d, E, k):
    """E 4 / 8: the 16-lane kernel; E 16 / 32 (d >= 768): the matrix-core kernel"""
    assert ops.ln_router_supported(d, E, k)
    x, (gamma, beta) = vh.ln_rows(cls, d), vh.ln_params(d)
    wg, bg = _router_params(d, E)
    xn16, xn32, idx, score, _, _ = ops.ln_router_topk(x.to(DEV), *_dev(gamma, beta), vh.EPS, *_dev(wg, bg), k, ops.GATE_NAIVE,
                                                      want_xn32=True)
    _assert_ln(xn32, x, gamma, beta, F32, f"ln_router_topk {cls} d {d} E {E}")
    assert torch.equal(xn16, xn32.half())
    o_idx, o_score, _ = mo.naive_gate(xn32.cpu(), wg, bg, k)
    assert torch.equal(idx.cpu(), o_idx), "routing = the oracle's on the kernel's own normalised rows"
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
    if cls == "const":
        assert torch.equal(xn32.cpu(), beta.expand(R, d))


@ln_cases
def test_gate_ln_router(cls, d):
    E, k = 4, 1
    assert ops.gate_ln_router_supported(d, E, k)
    x, (gamma, beta) = vh.ln_rows(cls, d), vh.ln_params(d)
    wg, bg = _router_params(d, E)
    g = torch.Generator().manual_seed(5 * d + 2)
    gw, gb = torch.randn(1, d, generator=g) * 0.05, torch.full((1,), 0.1)
    thr = torch.tensor(0.55, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    r = ops.gate_ln_router(x.to(DEV), gw.to(DEV), gb.to(DEV), thr, ln=(*_dev(gamma, beta), vh.EPS), wg=wg.to(DEV), bg=bg.to(DEV), k=k,
                           xn16_dtype=F16, want_xn32=True, want_mask=True, skip_count=cnt)
    xn = r["xn32"].cpu()
    _assert_ln(xn, x, gamma, beta, F32, f"gate_ln_router {cls} d {d}")
    m = mo.skip_gate(xn[None], gw, gb, float(thr))[0]
    assert torch.equal(r["mask"].cpu(), m), "skip decisions = the oracle's on the kernel's own normalised rows"
    assert int(cnt.item()) == int(m[:, 0].sum())
    assert torch.equal(r["xn16"].cpu(), (xn * m[:, 1:2]).half())
    o_idx, o_score, _ = mo.naive_gate(xn * m[:, 1:2], wg, bg, k)
    assert torch.equal(r["idx"].cpu(), o_idx)
    assert torch.allclose(r["score"].cpu(), o_score, rtol=0, atol=5e-6)


# =========================================================================================================== LayerNorm backward
@pytest.mark.parametrize("dyt", [F32, F16], ids=["f32", "f16"])
@ln_cases
def test_layernorm_bwd(cls, d, dyt):
    x, (gamma, beta), dy = vh.ln_rows(cls, d), vh.ln_params(d), vh.ln_dy(cls, d, dyt)
    ref = vh.ln_bwd_f64(x, dy, gamma, beta)
    got = ops.layernorm_bwd(*_dev(x, dy, gamma), vh.EPS)
    errs = [vh.rel_l2(a, b) for a, b in zip(got, ref)]
    bar = vh.ln_bwd_bar(x, gamma, beta)
    print(f"layernorm_bwd {cls} d {d} dy {vh._dn(dyt)}: dx {errs[0]:.2e} dgamma {errs[1]:.2e} dbeta {errs[2]:.2e}  bar {bar:.2e}"
          f"  worst / bar {max(errs) / bar:.3f}")
    assert max(errs) <= bar, (errs, bar)


@pytest.mark.parametrize("gdt", [F32, F16], ids=["f32", "f16"])
@ln_cases
def test_gate_ln_bwd(cls, d, gdt):
    """the formula of test_gate_ln_backward_in_one_pass_matches_float64_autograd_of_the_reference_formula on one class's rows
    (vh.gate_ln_bwd_f64; the upstream gradients and why the outlier classes' g_out carries an offset: vh.gate_grads); an outlier
    channel saturates the gate (z about 5 in every row at d = 768), which p (1 - p) must survive."""
    x, (gamma, beta), (w, b) = vh.ln_rows(cls, d), vh.ln_params(d), vh.gate_params(d)
    g_f, g_out = vh.gate_grads(cls, d, gdt)
    ref = vh.gate_ln_bwd_f64(x, gamma, beta, w, b, g_f, g_out)
    mask = ref["mask"]
    dx, dg, db_, dgw, _dgb, dz = ops.gate_ln_bwd(*_dev(x, g_f, g_out, gamma, beta), vh.EPS, *_dev(w, b, mask), want_dz=True)
    errs = [vh.rel_l2(a, ref[k]) for a, k in ((dx, "dx"), (dg, "dgamma"), (db_, "dbeta"))]
    gerrs = [vh.rel_l2(dgw, ref["dgate_w"]), vh.rel_l2(dz, vh.gate_dz_f64(ref["xn"], g_f, w, b))]
    bar, gbar = vh.ln_bwd_bar(x, gamma, beta), vh.gate_bwd_bar(x, gamma, beta)
    print(f"gate_ln_bwd {cls} d {d} g_f {vh._dn(gdt)}: dx {errs[0]:.2e} dgamma {errs[1]:.2e} dbeta {errs[2]:.2e}  bar {bar:.2e}"
          f"  worst / bar {max(errs) / bar:.3f};  dgate_w {gerrs[0]:.2e} dz {gerrs[1]:.2e}  bar {gbar:.2e}  worst / bar {max(gerrs) / gbar:.3f}")
    assert max(errs) <= bar, (errs, bar)
    assert max(gerrs) <= gbar, (gerrs, gbar)
    # the same gate behind a LayerNorm of its own launch (smoe_skip_gate_bwd): dz of the rows it is given
    xn32 = ops.layernorm(*_dev(x, gamma, beta), vh.EPS, F32)
    _dxn, dz3 = ops.skip_gate_bwd(xn32, *_dev(g_f, g_out, w, b, mask))
    e3 = vh.rel_l2(dz3, vh.gate_dz_f64(xn32.cpu(), g_f, w, b))
    print(f"skip_gate_bwd {cls} d {d} g_f {vh._dn(gdt)}: dz {e3:.2e}  bar {vh.GATE_DZ_BAR:.2e}  ({e3 / vh.GATE_DZ_BAR:.3f})")
    assert e3 <= vh.GATE_DZ_BAR, e3


# ===================================================================================================================== attention
ATTN_CASES = [(c, N, dt) for c in vh.ATTN_CLASSES for N in vh.ATTN_NS for dt in vh.ATTN_DTYPES]
attn_cases = pytest.mark.parametrize("cls,N,dt", ATTN_CASES, ids=[f"{c}-N{N}-{vh._dn(dt)}" for c, N, dt in ATTN_CASES])
H = vh.ATTN_H


@functools.lru_cache(maxsize=None)
def _attn(cls, N, dt):
    qkv, do = _dev(*vh.attn_inputs(cls, N, dt))
    out, lse = ops.attention(qkv, 1, N, H, 64, vh.SCALE, want_lse=True)
    return qkv, do, out, lse, ops.attention_bwd(qkv, out, do, lse, 1, N, H, 64, vh.SCALE)


@attn_cases
def test_attention_forward_and_backward_inside_the_bars(cls, N, dt):
    _, _, out, lse, dqkv = _attn(cls, N, dt)
    bar = vh.attn_bar(cls, N, dt)
    for h, e in enumerate(vh.attn_errors(out, lse, dqkv, vh.attn_f64(cls, N, dt))):
        print(f"{cls} N {N} {vh._dn(dt)} head {h}: " + "  ".join(f"{qn} {e[qn]:.1e} ({e[qn] / bar[qn]:.2f} bar)" for qn in vh.QUANTS))
        for qn in vh.QUANTS:
            assert e[qn] <= bar[qn], (h, qn, e[qn], bar[qn])


@attn_cases
def test_attention_exact_zeros_and_the_same_bits_again(cls, N, dt):
    qkv, do, out, lse, dqkv = _attn(cls, N, dt)
    ref = vh.attn_f64(cls, N, dt)
    if cls == "uniform":
        assert float(dqkv[:, :, 1].abs().max()) == 0.0, "q = 0: dk = 0"
        assert float((lse.cpu().double() - torch.log2(torch.tensor(float(N), dtype=torch.float64))).abs().max()) <= 1e-6
        v_mean = qkv[:, :, 2].double().mean(1).reshape(1, 1, H * 64).cpu()
        assert float((out.cpu().double() - v_mean).abs().max()) <= vh.attn_bar(cls, N, dt)["out"] * max(1.0, float(v_mean.abs().max()))
    if cls in ("asc", "desc"):
        dead = ref["probs"][0].amax(-2) < vh.P_ZERO                   # [H, N]: the key is below P_ZERO in every row of its head
        assert N < 577 or int(dead.sum()) > 0
        for h in range(H):
            for i, nm in ((1, "dk"), (2, "dv")):
                assert float(dqkv[0, :, i, h][dead[h].to(DEV)].abs().max() if bool(dead[h].any()) else 0.0) == 0.0, (nm, h)
    qg = qkv.clone().requires_grad_(True)
    dense.AttentionFn.apply(qg, 1, N, H, 64, vh.SCALE).backward(do)
    assert torch.equal(qg.grad, dqkv)
    out2, lse2 = ops.attention(qkv, 1, N, H, 64, vh.SCALE, want_lse=True)
    assert torch.equal(out2, out) and torch.equal(lse2, lse)
    assert torch.equal(ops.attention_bwd(qkv, out, do, lse, 1, N, H, 64, vh.SCALE), dqkv)
