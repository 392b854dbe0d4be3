"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the C-ABI, against
the CPU oracle on the same seeded inputs, against the committed golden fixtures, and -- at BASELINE cfg-2
size -- through size-independent properties.

Bars: routing indices / counts / permutation bit-exact; float outputs within the tolerance written at
each assert (f32-exact MFMA path: 2e-5; f16 MFMA path: 1e-3 relative to the output scale)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import moe_oracle as mo  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402
from _mp import float_bar as _float_bar  # noqa: E402

DEV = "cuda:0"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mk(T, d, h, E, seed, wstd=0.02, skew=False):
    g = _gen(seed)
    x = torch.randn(T, d, generator=g)
    wg = torch.randn(E, d, generator=g) * 0.02
    bg = torch.zeros(E)
    if skew:
        bg[0] = 2.0
    w1 = torch.nn.init.trunc_normal_(torch.empty(E, h, d), std=wstd, a=-2, b=2, generator=g)
    w2 = torch.nn.init.trunc_normal_(torch.empty(E, d, h), std=wstd, a=-2, b=2, generator=g)
    b1 = torch.randn(E, h, generator=g) * 0.02
    b2 = torch.randn(E, d, generator=g) * 0.02
    return x, wg, bg, w1, b1, w2, b2


# ------------------------------------------------------------------------------------------ router
@pytest.mark.parametrize("T,d,E,k", [(1, 192, 4, 1), (777, 192, 4, 2), (5000, 768, 8, 1), (3000, 768, 8, 2),
                                     (2000, 1024, 32, 1), (513, 64, 3, 3), (1000, 384, 70, 2), (4001, 768, 16, 1),
                                     (1500, 1024, 12, 3), (2500, 768, 32, 2)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("force_f64", [False, True])
def test_router_naive_matches_oracle(T, d, E, k, dtype, force_f64):
    g = _gen(T + d + E)
    x = torch.randn(T, d, generator=g).to(dtype)
    wg = torch.randn(E, d, generator=g) * 0.05
    bg = torch.randn(E, generator=g) * 0.1
    idx, score, logits, _ = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), k, ops.GATE_NAIVE, want_logits=True,
                                            force_f64=force_f64)
    o_idx, o_score, o_logits = mo.naive_gate(x.float(), wg, bg, k)
    assert torch.equal(idx.cpu(), o_idx), "routing indices must be bit-exact"
    if force_f64:
        assert torch.equal(logits.cpu(), o_logits), "f64-accumulated logits round to the same f32"
    assert torch.allclose(logits.cpu(), o_logits, rtol=0, atol=1e-5)
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
    if k == 1:
        assert torch.all(score == 1.0)


@pytest.mark.parametrize("d,E,scale", [(1024, 32, 1.0), (768, 16, 1.0), (1024, 20, 40.0), (768, 32, 1e-3)])
def test_router_matrix_core_logits_stay_inside_the_error_bound(d, E, scale):
    """The 16- / 32-expert router accumulates its logits on the f32 matrix cores (csrc/router_mt_kernel.h), whose internal
    summation order is not documented.  Its redo list is only as rigorous as its bound: the f32 logits must sit well
    inside `4 (d / 16 + 6) 2^-24 |row| max|w_e|` of the f64 values (observed <= a quarter of it leaves the factor-4 margin)."""
    T = 4096
    g = _gen(d + E)
    x = (torch.randn(T, d, generator=g) * scale)
    wg = torch.randn(E, d, generator=g) * 0.05
    bg = torch.randn(E, generator=g) * 0.1
    _, _, logits, _ = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), 1, ops.GATE_NAIVE, want_logits=True)
    ref = x.double() @ wg.double().t() + bg.double()
    err = (logits.cpu().double() - ref).abs().max(dim=1).values
    bound = 4.0 * (d / 16 + 6) * 2.0 ** -24 * x.double().norm(dim=1) * wg.double().norm(dim=1).max()
    ratio = float((err / bound).max())
    print(f"d {d} E {E}: max |f32 - f64| / bound = {ratio:.4f}")
    assert ratio <= 0.25, ratio


@pytest.mark.parametrize("T", [1, 3, 16, 17, 33])
@pytest.mark.parametrize("d,E,k", [(768, 16, 2), (1024, 32, 1), (768, 27, 4)])
def test_router_matrix_core_partial_tiles_and_edges(T, d, E, k):
    """The 16-token tiles of the matrix-core router with fewer live tokens than slots, an expert count that is not a
    multiple of 16 (rows past E repeat the last expert's weights and must be masked everywhere), up to 4 choices; logits,
    probabilities and scores of every token against the oracle."""
    g = _gen(1000 * T + E)
    x = torch.randn(T, d, generator=g)
    wg = torch.randn(E, d, generator=g) * 0.05
    bg = torch.randn(E, generator=g) * 0.1
    idx, score, logits, _ = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), k, ops.GATE_NAIVE, want_logits=True)
    o_idx, o_score, _ = mo.naive_gate(x, wg, bg, k)
    assert torch.equal(idx.cpu(), o_idx)
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
    ref = x.double() @ wg.double().t() + bg.double()
    assert (logits.cpu().double() - ref).abs().max().item() <= 2e-5 * float(ref.abs().max())


@pytest.mark.parametrize("d,E", [(768, 16), (1024, 32)])
def test_router_matrix_core_zero_rows_near_ties_and_switch_probabilities(d, E):
    """(a) all-zero rows route by the biases, ties to the lowest id, without visiting the redo pass' arithmetic; (b) exact and
    near ties between experts in different 16-expert blocks and different lanes of the row go through the f64 matrix-core
    pass and come out as the oracle orders them; (c) the switch gate's probabilities, scores and noise handling."""
    g = _gen(31 + E)
    T = 2000
    x = torch.randn(T, d, generator=g)
    x[::7] = 0.0
    wg = torch.randn(E, d, generator=g) * 0.03
    wg[E - 1] = wg[2]                          # exact tie across blocks / lanes
    wg[9] = wg[1]; wg[9, 33] += 2e-9           # near ties far below the f32 accumulation error
    wg[E - 3] = wg[1]; wg[E - 3, d - 5] -= 4e-9
    bg = torch.zeros(E)
    bg[4] = bg[E - 2] = 0.5                    # zero rows: experts 4 and E - 2 tie on the bias -> 4 first
    for k in (1, 2, 3):
        idx, score, _, _ = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), k, ops.GATE_NAIVE)
        o_idx, o_score, _ = mo.naive_gate(x, wg, bg, k)
        assert torch.equal(idx.cpu(), o_idx), k
        assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
        assert torch.all(idx[::7, 0].cpu() == 4)
    noise = torch.rand(T, E, generator=g) * 0.2 + 0.9
    idx, score, _, probs = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), 1, ops.GATE_SWITCH, noise.to(DEV), want_probs=True)
    o_idx, o_score, o_p = mo.switch_gate(x, wg, bg, noise)
    assert torch.equal(idx.cpu(), o_idx)
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
    assert torch.allclose(probs.cpu(), o_p, rtol=0, atol=5e-6)


def test_router_zero_rows_route_by_bias_with_lowest_id_tie_break():
    x = torch.zeros(300, 192)
    wg = torch.randn(8, 192, generator=_gen(0))
    bg = torch.tensor([0.1, 0.9, 0.9, 0.2, 0.9, 0.0, 0.0, 0.0])
    idx, score, _, _ = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), 2, ops.GATE_NAIVE)
    assert torch.all(idx[:, 0] == 1) and torch.all(idx[:, 1] == 2)
    assert torch.allclose(score.cpu(), torch.full((300, 2), 0.5))


def test_router_near_ties_take_the_f64_path_and_match_the_oracle():
    """Experts whose logits differ by less than f32 summation noise: the f32 fast path must hand these
    tokens to the f64 re-do, which orders them exactly like the oracle."""
    T, d, E = 4096, 768, 8
    g = _gen(21)
    x = torch.randn(T, d, generator=g)
    wg = torch.randn(E, d, generator=g) * 0.02
    wg[5] = wg[2]                      # exact tie between experts 2 and 5 on every token
    wg[6] = wg[1]; wg[6, 17] += 3e-9   # near tie: gap ~3e-9 * |x|, far below f32 accumulation error
    wg[7] = wg[1]; wg[7, 400] -= 5e-9
    bg = torch.zeros(E)
    for k in (1, 2, 3):
        idx, score, _, _ = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), k, ops.GATE_NAIVE)
        o_idx, o_score, _ = mo.naive_gate(x, wg, bg, k)
        assert torch.equal(idx.cpu(), o_idx)
        assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)


@pytest.mark.parametrize("with_noise", [False, True])
def test_router_switch_matches_oracle(with_noise):
    T, d, E = 4000, 768, 8
    g = _gen(9)
    x, wg, bg = torch.randn(T, d, generator=g), torch.randn(E, d, generator=g) * 0.05, torch.zeros(E)
    noise = (torch.rand(T, E, generator=g) * 0.2 + 0.9) if with_noise else None
    idx, score, _, probs = ops.router_topk(x.to(DEV), wg.to(DEV), bg.to(DEV), 1, ops.GATE_SWITCH,
                                           noise.to(DEV) if with_noise else None, want_probs=True)
    o_idx, o_score, o_p = mo.switch_gate(x, wg, bg, noise)
    assert torch.equal(idx.cpu(), o_idx)
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)
    assert torch.allclose(probs.cpu(), o_p, rtol=0, atol=5e-6)


# The pass sequence of the router entry points (counter clear -> f32 pass -> f64 redo pass, or f64 over all tokens), pinned where
# the other tests do not reach: LayerNorm + forced f64, the kept workspace's invariant, and the clearing launch a plain C caller gets.
@pytest.mark.parametrize("T,d,E,k", [(333, 192, 4, 2),      # 16-lanes-per-token kernel
                                     (333, 768, 16, 2),     # matrix-core kernel
                                     (333, 768, 32, 1)])    # matrix-core kernel, f32 pass on two halves
def test_ln_router_forced_f64_writes_the_same_rows_and_routes_like_the_oracle(T, d, E, k):
    """Forced f64 with LayerNorm: the f32 pass still runs for its stores (xn16 / xn32 bit-equal to the normal call's), then every
    token goes through the f64 pass: idx and logits are the oracle's on the rows the kernel wrote."""
    g = _gen(T + d + E)
    x = torch.randn(T, d, generator=g)
    lw, lb = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    wg = torch.randn(E, d, generator=g) * 0.05
    bg = torch.randn(E, generator=g) * 0.1
    dev = [t.to(DEV) for t in (x, lw, lb)] + [1e-6] + [t.to(DEV) for t in (wg, bg)]
    n16, n32, _, _, _, _ = ops.ln_router_topk(*dev, k, ops.GATE_NAIVE, want_xn32=True, want_logits=True, force_f64=False)
    xn16, xn32, idx, score, logits, _ = ops.ln_router_topk(*dev, k, ops.GATE_NAIVE, want_xn32=True, want_logits=True, force_f64=True)
    assert torch.equal(xn32, n32) and torch.equal(xn16, n16), "the normalised rows do not depend on the routing mode"
    o_idx, o_score, o_logits = mo.naive_gate(xn32.cpu(), wg, bg, k)
    assert torch.equal(idx.cpu(), o_idx), "routing indices must be bit-exact"
    assert torch.equal(logits.cpu(), o_logits), "f64-accumulated logits round to the same f32"
    assert torch.allclose(score.cpu(), o_score, rtol=0, atol=5e-6)


_PASS_CASES = [("router", 64, 3), ("router", 192, 4), ("router", 768, 16), ("ln_router", 192, 4), ("ln_router", 768, 16),
               ("gate_router", 192, 4), ("gate", 192, 0)]   # generic, 16-lane, matrix-core launcher; gate + router, gate only


def _tie_planted(entry, d, E):
    """T = 512 inputs (on the device) whose redo list is not empty: the planted exact and near ties of
    test_router_near_ties_take_the_f64_path_and_match_the_oracle, and for the skip gate rows that sit on its threshold."""
    T = 512
    g = _gen(21 + d + E)
    x = torch.randn(T, d, generator=g)
    t = {"T": T, "k": min(2, max(E, 1))}
    if E:
        wg = torch.randn(E, d, generator=g) * 0.02
        wg[E - 1] = wg[0]                                    # exact tie on every token
        src, near = (0, 1) if E == 3 else (1, E - 2)
        wg[near] = wg[src]; wg[near, 17] += 3e-9             # near tie far below the f32 accumulation error
        t["wg"], t["bg"] = wg.to(DEV), torch.zeros(E, device=DEV)
    if entry != "router":
        lw, lb = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
        t["lw"], t["lb"] = lw.to(DEV), lb.to(DEV)
    if entry.startswith("gate"):
        # gate logit z = rstd <x - mean, lw gw> + <lb, gw> + gb.  Every fifth row loses its component along the centred lw gw, and
        # gb = -<lb, gw>: z ~ 0 = logit(threshold 0.5) up to rounding, far inside the f32 pass' error bound; zero rows likewise
        gw = torch.randn(d, generator=g) * 0.1
        g2 = (lw * gw).double()
        g2c = g2 - g2.mean()
        xc = x[::5].double() - x[::5].double().mean(1, keepdim=True)
        x[::5] = (x[::5].double() - ((xc @ g2) / (g2c @ g2c))[:, None] * g2c).float()
        x[::7] = 0.0
        gb = -(lb.double() @ gw.double()).float().reshape(1)
        t["gw"], t["gb"], t["thr"] = gw.to(DEV), gb.to(DEV), torch.tensor(0.5, device=DEV)
    t["x"] = x.to(DEV)
    return t


def _pass_call(entry, t):
    """The ops call of one case; its outputs as a list of tensors."""
    if entry == "router":
        return [o for o in ops.router_topk(t["x"], t["wg"], t["bg"], t["k"], ops.GATE_NAIVE, want_logits=True) if o is not None]
    if entry == "ln_router":
        r = ops.ln_router_topk(t["x"], t["lw"], t["lb"], 1e-6, t["wg"], t["bg"], t["k"], ops.GATE_NAIVE, want_xn32=True, want_logits=True)
        return [o for o in r if o is not None]
    r = ops.gate_ln_router(t["x"], t["gw"], t["gb"], t["thr"], ln=(t["lw"], t["lb"], 1e-6), wg=t.get("wg"), bg=t.get("bg"), k=t["k"],
                           xn16_dtype=torch.float16, want_xn32=True, want_mask=True)
    return [r[n] for n in ("xn16", "xn32", "idx", "idx_plan", "score", "mask") if r[n] is not None]


@pytest.mark.parametrize("entry,d,E", _PASS_CASES)
def test_router_calls_leave_the_kept_workspace_counters_zero(entry, d, E):
    """Every redo pass leaves both counter words of the kept workspace zero (ops._router_workspace relies on it in every forward):
    checked after each call on inputs with a non-empty redo list, and a second identical call returns the same bits."""
    t = _tie_planted(entry, d, E)
    ws = ops._router_workspace(torch.device(DEV), 1)
    assert ws is ops._router_ws[(0, ops._stream(t["x"]))]
    redo_list = ws[16:16 + 4 * t["T"]].view(torch.int32)
    redo_list.fill_(-1)                                      # (the list part carries no state between calls)
    first = _pass_call(entry, t)
    assert (redo_list >= 0).any(), "the planted ties must put tokens on the redo list, or the checks below are vacuous"
    assert not ws[:16].any(), ws[:16].tolist()
    second = _pass_call(entry, t)
    assert not ws[:16].any(), ws[:16].tolist()
    assert len(first) == len(second) and all(torch.equal(u, v) for u, v in zip(first, second))


@pytest.mark.parametrize("entry,d,E", _PASS_CASES)
def test_router_library_calls_clear_a_dirty_workspace_themselves(entry, d, E):
    """What a plain C caller gets: a private workspace full of 0xFF and no "kept zero" flag -> the call clears the counter words
    itself; every output bit-equal to the ops call's (kept workspace, no clearing launch), the counter words zero afterwards."""
    from slim_switch_moe_vit_amd import _lib
    t = _tie_planted(entry, d, E)
    want = _pass_call(entry, t)
    got = [torch.empty_like(o) for o in want]
    lib, p, x, T, k = _lib.load(), ops._ptr, t["x"], t["T"], t["k"]
    ws_bytes = lib.smoe_router_workspace_bytes(T)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    if entry == "router":
        idx, score, logits = got
        rc = lib.smoe_router_topk(p(x), ops.F32, p(t["wg"]), p(t["bg"]), None, T, d, E, k, ops.GATE_NAIVE, p(idx), p(score), p(logits),
                                  None, p(ws), ws_bytes, ops._stream(x))
    elif entry == "ln_router":
        xn16, xn32, idx, score, logits = got
        rc = lib.smoe_ln_router_topk(p(x), ops.F32, p(t["lw"]), p(t["lb"]), 1e-6, p(xn16), ops.F16, p(xn32), p(t["wg"]), p(t["bg"]), None,
                                     T, d, E, k, ops.GATE_NAIVE, p(idx), p(score), p(logits), None, None, p(ws), ws_bytes, ops._stream(x))
    else:
        xn16, xn32, mask = got[0], got[1], got[-1]
        idx, idx_plan, score = got[2:5] if E else (None, None, None)
        rc = lib.smoe_gate_ln_router(p(x), ops.F32, 1, p(t["lw"]), p(t["lb"]), 1e-6, p(t["gw"]), p(t["gb"]), p(t["thr"]), p(xn16), ops.F16,
                                     p(xn32), None, p(t.get("wg")), p(t.get("bg")), T, d, E, k, p(idx), p(idx_plan), p(score), p(mask),
                                     None, None, None, p(ws), ws_bytes, ops._stream(x))
    assert rc == 0, lib.smoe_last_error()
    assert not ws[:16].any(), ws[:16].tolist()
    assert all(torch.equal(u, v) for u, v in zip(got, want))


# ------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("n,E,cap", [(1, 4, -1), (63, 4, -1), (1024, 8, -1), (1025, 8, -1), (50432, 8, -1),
                                     (50432, 8, 6304), (20000, 32, 100), (5000, 300, -1), (4096, 1, -1),
                                     (100000, 16, 0)])
def test_dispatch_plan_bit_exact(n, E, cap):
    rng = np.random.default_rng(n + E)
    idx = rng.integers(-1 if n % 2 else 0, E, size=n).astype(np.int64)
    if E >= 8:
        idx[rng.random(n) < 0.3] = 0  # skew: expert 0 overloaded
    counts, offsets, pos, inv_pos, pruned = ops.dispatch_plan(torch.from_numpy(idx).to(DEV), E, cap, want_pruned=True)
    p = mo.dispatch_plan(idx, E, cap)
    assert np.array_equal(counts.cpu().numpy(), p.counts)
    assert np.array_equal(offsets.cpu().numpy(), p.offsets)
    assert np.array_equal(pos.cpu().numpy(), p.pos)
    assert np.array_equal(inv_pos.cpu().numpy(), p.inv_pos)
    assert np.array_equal(pruned.cpu().numpy(), p.idx_pruned)


def test_dispatch_plan_is_deterministic_and_handles_empty_experts():
    idx = torch.tensor([3, 3, 3, 0, 3, 0], dtype=torch.int64, device=DEV)  # experts 1, 2 empty
    a = ops.dispatch_plan(idx, 4)
    b = ops.dispatch_plan(idx, 4)
    assert a[0].tolist() == [2, 0, 0, 4] and a[1].tolist() == [0, 2, 2, 2, 6]
    assert a[2].tolist() == [3, 5, 0, 1, 2, 4]
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------ scatter / combine
@pytest.mark.parametrize("k", [1, 2, 3])
def test_scatter_then_gather_is_identity_on_kept_rows_and_zero_on_dropped(k):
    T, d, E = 3001, 192, 8
    g = _gen(k)
    x = torch.randn(T, d, generator=g)
    idx = torch.randint(0, E, (T, k), generator=g)
    counts, offsets, pos, inv_pos, pruned = ops.dispatch_plan(idx.to(DEV), E, capacity=300)
    buf = ops.scatter_rows(x.to(DEV), pos, k, torch.float32, zero_fill=True)
    p = mo.dispatch_plan(idx.numpy(), E, 300)
    kept = int(p.offsets[E])
    assert torch.equal(buf[:kept].cpu(), x[torch.from_numpy(p.pos[:kept]) // k]), "scatter is an exact row copy"
    score = torch.rand(T, k, generator=g)
    out = ops.gather_combine(buf, inv_pos, score.to(DEV), T, k, torch.float32).cpu()
    w = (score * torch.from_numpy(p.inv_pos.reshape(T, k) >= 0)).sum(-1, keepdim=True)
    assert torch.allclose(out, w * x, rtol=0, atol=1e-5)
    all_dropped = torch.from_numpy((p.inv_pos.reshape(T, k) < 0).all(-1))
    assert torch.all(out[all_dropped] == 0)
    # cast on scatter == torch's round-to-nearest cast
    b16 = ops.scatter_rows(x.to(DEV), pos, k, torch.float16, zero_fill=True)
    assert torch.equal(b16[:kept].cpu(), x[torch.from_numpy(p.pos[:kept]) // k].half())
    bb = ops.scatter_rows(x.to(DEV), pos, k, torch.bfloat16, zero_fill=True)
    assert torch.equal(bb[:kept].cpu(), x[torch.from_numpy(p.pos[:kept]) // k].bfloat16())


# ------------------------------------------------------------------------------------------ grouped GEMM
def _gemm_ref(A, W, bias, offsets, gelu):
    out = torch.zeros(A.shape[0], W.shape[1], dtype=torch.float64)
    for e in range(W.shape[0]):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        if hi > lo:
            v = A[lo:hi].double() @ W[e].double().t() + (bias[e].double() if bias is not None else 0)
            out[lo:hi] = torch.nn.functional.gelu(v) if gelu else v
    return out


@pytest.mark.parametrize("counts,K,N", [([128, 128], 64, 128), ([5, 0, 300, 1, 0, 77], 192, 768),
                                        ([1000, 3, 129, 127], 768, 192), ([0, 0, 0, 9], 128, 72),
                                        ([700, 650, 600, 800, 655, 690, 710, 640], 768, 3072)])
@pytest.mark.parametrize("cd,tol", [(torch.float32, 2e-5), (torch.float16, 1e-3), (torch.bfloat16, 8e-3)])
@pytest.mark.parametrize("gelu", [False, True])
# variants in the default matrix: 0 reference (register-staged; the f32-exact mode), 1 small-M dense GEMMs (classifier head),
# 4 one-workgroup-per-tile fallback (operands >= 4 GiB, > 63 groups), 9 production (persistent, direct-store epilogues),
# 10 / 13 forced 320-row tile without / with the deep schedule, 14 persistent with the LDS-staged epilogue (A/B reference).
# The other A/B structures (2, 3, 5-8, 11, 12) stay reachable through `variant=` but no longer run on every GPU test pass.
@pytest.mark.parametrize("variant", [0, 1, 4, 9, 10, 13, 14])
def test_grouped_gemm_matches_fp64_reference(counts, K, N, cd, tol, gelu, variant):
    if variant and (cd == torch.float32 or K % 64):
        pytest.skip("glds variants take 16-bit operands and K % 64 == 0")
    E = len(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    M = int(offsets[-1])
    g = _gen(M + K + N)
    A = torch.randn(M + 7, K, generator=g).to(cd)  # rows beyond offsets[E] exist but must not be touched
    W = (torch.randn(E, N, K, generator=g) * 0.05).to(cd)
    bias = torch.randn(E, N, generator=g) * 0.1
    out = torch.full((M + 7, N), 7.0, dtype=torch.float32, device=DEV)
    ops.grouped_gemm(A.to(DEV), W.to(DEV), bias.to(DEV), torch.from_numpy(offsets).to(DEV),
                     ops.EPI_GELU if gelu else ops.EPI_NONE, out=out, variant=variant)
    ref = _gemm_ref(A, W, bias, offsets, gelu)
    got = out.cpu().double()
    scale = max(1.0, float(ref.abs().max()))
    assert (got[:M] - ref[:M]).abs().max() <= tol * scale
    assert torch.all(got[M:] == 7.0), "rows past the last expert must stay untouched"


@pytest.mark.parametrize("variant", [0, 4, 9, 10, 14])
def test_grouped_gemm_gelu_epilogue_over_the_whole_input_range(variant):
    """The fused GELU (a fitted sigmoid form without a range clamp in the MFMA kernels, erf form in variant 0) must
    follow the exact-erf GELU from the saturated negative side to the saturated positive side: pre-activations
    from -6e4 to 6e4 are produced exactly (one non-zero product per output), f32 output (variant 9: the direct f32
    epilogue; 14: the staged one)."""
    vals = torch.tensor([0.0, 1e-3, 0.5, 1.0, 2.5, 4.0, 5.5, 7.9, 8.0, 8.1, 9.0, 12.0, 20.0, 64.0, 300.0, 4096.0,
                         60000.0], dtype=torch.float64)
    vals = torch.cat([vals, -vals])
    M, K, N = 320, 64, 64
    A = torch.zeros(M, K, dtype=torch.float16)
    for m in range(M):
        A[m, m % K] = vals[m % len(vals)].half()
    W = torch.eye(N, K, dtype=torch.float16)[None]   # out[m, n] = A[m, n]
    offsets = torch.tensor([0, M], dtype=torch.int32)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ops.grouped_gemm(A.to(DEV), W.to(DEV), None, offsets.to(DEV), ops.EPI_GELU, out=out, variant=variant)
    pre = A.double()
    ref = torch.nn.functional.gelu(pre)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    assert ((got - ref).abs() <= 1e-5 + 1e-5 * ref.abs()).all(), float((got - ref).abs().max())
    assert (got[pre <= -9.0] == 0).all() and (got[pre >= 9.0] == pre[pre >= 9.0]).all()


@pytest.mark.parametrize("variant,cd", [(0, torch.float32), (0, torch.float16), (1, torch.float16), (4, torch.float16),
                                        (4, torch.bfloat16), (9, torch.float16), (9, torch.bfloat16), (10, torch.float16),
                                        (10, torch.bfloat16), (11, torch.float16), (13, torch.float16), (13, torch.bfloat16),
                                        (14, torch.float16), (14, torch.bfloat16)])
def test_grouped_gemm_fused_combine_row_map(variant, cd):
    E, K, N, T = 4, 128, 64, 1000
    g = _gen(3)
    idx = torch.randint(0, E, (T, 1), generator=g)
    counts, offsets, pos, inv_pos, _ = ops.dispatch_plan(idx.to(DEV), E, capacity=200)
    A = torch.randn(T, K, generator=g)
    W = torch.randn(E, N, K, generator=g) * 0.05
    score = torch.rand(T, generator=g)
    out = torch.zeros(T, N, device=DEV)
    A, W = A.to(cd), W.to(cd)
    ops.grouped_gemm(A.to(DEV), W.to(DEV), None, offsets, ops.EPI_NONE, row_map=pos, row_scale=score.to(DEV), out=out,
                     variant=variant)
    p = mo.dispatch_plan(idx.numpy(), E, 200)
    ref = torch.zeros(T, N, dtype=torch.float64)
    y = _gemm_ref(A, W, None, p.offsets, False)
    kept = int(p.offsets[E])
    tok = torch.from_numpy(p.pos[:kept])
    ref[tok] = y[:kept] * score[tok, None].double()
    assert (out.cpu().double() - ref).abs().max() < (2e-5 if cd == torch.float32 else 1e-4)


@pytest.mark.parametrize("variant", [1, 4, 9, 10, 11, 12, 13, 14])
def test_grouped_gemm_variants_are_race_free_and_agree_bitwise(variant):
    """The staged variants hand tiles between waves through LDS DMA + barriers; a missing wait shows up as
    rare wrong tiles.  Same inputs, 15 launches, ragged groups, long K: every launch must be bit-identical
    to the register-staged variant 0 (same MFMA k-order, so equality is exact)."""
    counts = [3000, 1, 0, 2555, 777, 4096, 130, 1200]
    E, K, N = len(counts), 3072, 768
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), device=DEV)
    M = int(offsets[-1])
    g = _gen(variant)
    A = torch.randn(M, K, generator=g).half().to(DEV)
    W = (torch.randn(E, N, K, generator=g) * 0.05).half().to(DEV)
    ref = ops.grouped_gemm(A, W, None, offsets, ops.EPI_NONE, torch.float32, variant=0)
    for _ in range(15):
        got = ops.grouped_gemm(A, W, None, offsets, ops.EPI_NONE, torch.float32, variant=variant)
        assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------ whole operator
def _load_module(mod, wg, bg, w1, b1, w2, b2):
    with torch.no_grad():
        mod.gate.gate.weight.copy_(wg); mod.gate.gate.bias.copy_(bg)
        mod.experts.htoh4.weight.copy_(w1); mod.experts.htoh4.bias.copy_(b1)
        mod.experts.h4toh.weight.copy_(w2); mod.experts.h4toh.bias.copy_(b2)
    return mod.to(DEV).eval()


@pytest.mark.parametrize("E,k,skew", [(4, 1, False), (8, 2, False), (8, 1, True)])
@pytest.mark.parametrize("cd,tol", [(torch.float32, 3e-5), (torch.float16, 1e-3)])
def test_moe_module_matches_oracle_vit_tiny_dims(E, k, skew, cd, tol):
    """BASELINE cfg 1 operator shape: ViT-Ti (d 192, h 768), batch 8 x 197 tokens."""
    d, h, T = 192, 768, 8 * 197
    x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=E * 10 + k, skew=skew)
    mod = _load_module(sm.CustomizedMoEMLP(d, h, E, k, 0.0, compute_dtype=cd), wg, bg, w1, b1, w2, b2)
    with torch.no_grad():
        out = mod(x.reshape(8, 197, d).to(DEV))
    r = mo.moe_forward(x.reshape(8, 197, d), wg, bg, w1, b1, w2, b2, k)
    idx, score, counts, offsets, pos, inv_pos = mod.last_plan
    assert torch.equal(idx.cpu(), r.idx)
    assert np.array_equal(pos.cpu().numpy(), r.plan.pos) and np.array_equal(counts.cpu().numpy(), r.plan.counts)
    err = (out.cpu() - r.out).abs().max().item()
    assert err <= tol, f"expert outputs differ by {err}"


@pytest.mark.parametrize("k,gate,cap", [(1, "naive", None), (2, "naive", None), (1, "switch", 1.0)])
def test_forward_add_equals_residual_plus_forward(k, gate, cap):
    """forward_add(x, r) == r + forward(x) bit for bit (f32 output: same single add), incl. dropped tokens."""
    d, h, E, T = 192, 768, 8, 3000
    x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=31 + k, skew=(gate == "switch"))
    mod = sm.FMoETransformerMLP(E, d, h, torch.nn.GELU(), top_k=k, gate=gate, capacity_factor=cap)
    mod = _load_module(mod, wg, bg, w1, b1, w2, b2)
    r = torch.randn(T, d, generator=_gen(5)).to(DEV)
    with torch.no_grad():
        a = mod.forward_add(x.to(DEV), r)
        b = r + mod(x.to(DEV))
    assert torch.equal(a, b)


@pytest.mark.parametrize("d,h,E,k,gate", [(192, 768, 4, 1, "naive"), (768, 3072, 8, 1, "naive"), (384, 768, 8, 2, "naive"),
                                          (1024, 1024, 5, 1, "switch"), (768, 768, 16, 1, "naive"), (1024, 512, 13, 2, "naive"),
                                          (768, 768, 16, 1, "switch"), (1024, 1024, 32, 1, "naive"), (768, 768, 27, 2, "naive")])
def test_fused_layernorm_router_and_block_half(d, h, E, k, gate):
    """smoe_ln_router_topk + a_gather GEMM-1 + fused combine/residual == x + mlp(LayerNorm(x)):
    (a) the fused LayerNorm matches F.layer_norm, (b) routing equals the oracle's on the very same normalised rows,
    (c) the fused block half is bit-identical to the unfused kernels fed with those rows."""
    T = 3000
    g = _gen(d + E)
    x = torch.randn(T, d, generator=g) * 1.7 + 0.3
    ln = torch.nn.LayerNorm(d, eps=1e-6)
    with torch.no_grad():
        ln.weight.copy_(1 + 0.2 * torch.randn(d, generator=g)); ln.bias.copy_(0.1 * torch.randn(d, generator=g))
    _, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=3)
    wg = wg * 5
    mod = sm.FMoETransformerMLP(E, d, h, torch.nn.GELU(), top_k=k, gate=gate,
                                capacity_factor=1.0 if gate == "switch" else None)
    mod = _load_module(mod, wg, bg, w1, b1, w2, b2)
    ln = ln.to(DEV)
    xg = x.to(DEV)
    with torch.no_grad():
        xn16, xn32, idx, score, _, _ = ops.ln_router_topk(xg, ln.weight, ln.bias, ln.eps, wg.to(DEV), bg.to(DEV), k,
                                                          mod.gate.kind, want_xn32=True)
        ref_ln = torch.nn.functional.layer_norm(x, (d,), ln.weight.cpu(), ln.bias.cpu(), 1e-6)
        assert (xn32.cpu() - ref_ln).abs().max().item() < 1e-5
        assert torch.equal(xn16, xn32.half())
        if gate == "naive":
            o_idx, o_score, _ = mo.naive_gate(xn32.cpu(), wg, bg, k)
        else:
            o_idx, o_score, _ = mo.switch_gate(xn32.cpu(), wg, bg)
        assert torch.equal(idx.cpu(), o_idx)
        assert torch.allclose(score.cpu(), o_score, atol=5e-6)
        fused = mod.forward_norm_add(xg, ln)
        unfused = mod.forward_add(xn32, xg)
        assert torch.equal(mod.last_plan[0], idx)
        assert torch.equal(fused, unfused)


@pytest.mark.parametrize("d", [192, 384, 768, 1024])
@pytest.mark.parametrize("odt", [torch.float32, torch.float16])
def test_layernorm_kernel_matches_reference_layernorm(d, odt, golden_dir):
    g = _gen(d)
    x = torch.randn(777, d, generator=g) * 3 + 1
    w, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    got = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, odt).cpu()
    ref = torch.nn.functional.layer_norm(x.double(), (d,), w.double(), b.double(), 1e-6)
    tol = 2e-6 if odt == torch.float32 else 2e-3
    assert (got.double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())
    if d == 192:  # the reference's own manual LayerNorm outputs (models/layers.py:160-224)
        gd = np.load(os.path.join(golden_dir, "ref_layernorm_tiny.npz"))
        y = ops.layernorm(torch.from_numpy(gd["x"]).to(DEV), torch.from_numpy(gd["w"]).to(DEV),
                          torch.from_numpy(gd["b"]).to(DEV), 1e-6, torch.float32).cpu()
        assert (y - torch.from_numpy(gd["y"])).abs().max().item() < 1e-5


@pytest.mark.parametrize("B,N,H", [(3, 197, 12), (2, 197, 3), (1, 16, 2), (2, 50, 4), (1, 256, 2), (5, 1, 1), (2, 224, 3)])
@pytest.mark.parametrize("dt,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.5e-2)])
def test_attention_kernel_matches_reference_attention(B, N, H, dt, tol):
    """softmax(q k^T * scale) v of models/vision_transformer.py:248-280, from the fused qkv layout [B,N,3,H,64]."""
    g = _gen(B * 1000 + N + H)
    qkv = (torch.randn(B, N, 3, H, 64, generator=g) * 1.5).to(dt)
    got = ops.attention(qkv.to(DEV), B, N, H, 64, 64 ** -0.5).cpu().float()
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4).unbind(0)
    ref = (torch.softmax(q @ k.transpose(-2, -1) * 64 ** -0.5, -1) @ v).transpose(1, 2).reshape(B, N, H * 64)
    assert (got.double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("B,N,H", [(2, 577, 16), (1, 257, 2), (2, 300, 3), (1, 592, 2), (1, 640, 1), (3, 321, 4), (1, 480, 2)])
@pytest.mark.parametrize("dt,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.5e-2)])
def test_attention_kernel_long_sequences_online_softmax(B, N, H, dt, tol):
    """N > 256 (BASELINE cfg 4: ViT-L/16 @384 has N = 577): key chunks with an online softmax.  The second input makes
    the running maximum jump by > 40 between chunks (a spiked key in every chunk region, larger in later ones), so the
    rescale of the running output / denominator is exercised, not just present."""
    g = _gen(B * 1000 + N + H)
    for spike in (False, True):
        qkv = (torch.randn(B, N, 3, H, 64, generator=g) * 1.5)
        if spike:
            for j, pos in enumerate(range(5, N, 97)):
                qkv[:, pos, 1] = qkv[:, 3, 0] * (2.0 + 1.5 * j)      # key `pos` aligned with query 3, growing with pos
        qkv = qkv.to(dt)
        got = ops.attention(qkv.to(DEV), B, N, H, 64, 64 ** -0.5).cpu().float()
        q, k, v = qkv.double().permute(2, 0, 3, 1, 4).unbind(0)
        ref = (torch.softmax(q @ k.transpose(-2, -1) * 64 ** -0.5, -1) @ v).transpose(1, 2).reshape(B, N, H * 64)
        assert torch.isfinite(got).all()
        assert (got.double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()), spike


def test_attention_path_matches_reference_attention_golden(golden_dir):
    """The REFERENCE's own ``Attention`` outputs (models/layers.py:227-269 == models/vision_transformer.py:248-280;
    tests/golden/ref_attention_tiny.npz): (1) smoe_attention_fwd on the qkv the reference weights give, then the
    projection; (2) the product module ``vit.Attention`` under fp16 autocast with the residual add fused into the
    projection GEMM.  f16 operands: 2e-3 x scale."""
    from slim_switch_moe_vit_amd.vit import Attention
    g = np.load(os.path.join(golden_dir, "ref_attention_tiny.npz"))
    t = lambda k: torch.from_numpy(g[k])
    H = int(g["num_heads"])
    att = Attention(192, num_heads=H, qkv_bias=True)
    with torch.no_grad():
        att.qkv.weight.copy_(t("qkv_w")); att.qkv.bias.copy_(t("qkv_b"))
        att.proj.weight.copy_(t("proj_w")); att.proj.bias.copy_(t("proj_b"))
    att = att.to(DEV).eval()
    for xk, yk in (("xa", "ya"), ("xb", "yb")):
        x, ref = t(xk), t(yk)
        B, N, C = x.shape
        scale = max(1.0, float(ref.abs().max()))
        qkv = torch.nn.functional.linear(x, t("qkv_w"), t("qkv_b")).half().to(DEV)          # [B, N, 3*H*64]
        o = ops.attention(qkv, B, N, H, 64, 64 ** -0.5).float().cpu()
        y = torch.nn.functional.linear(o, t("proj_w"), t("proj_b"))
        assert (y - ref).abs().max().item() <= 2e-3 * scale, (y - ref).abs().max().item()
        res = torch.randn(B, N, C, generator=_gen(3)).to(DEV)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            out, added = att(x.to(DEV).half(), residual=res)
        assert added, "the fused projection + residual path must be the one that runs"
        assert ((out - res).cpu() - ref).abs().max().item() <= 2e-3 * scale


def test_moe_module_e1_equals_reference_mlp_golden(golden_dir):
    """E = 1: the HIP path reproduces the REFERENCE's own dense Mlp (models/layers.py:391-414) outputs."""
    g = np.load(os.path.join(golden_dir, "ref_mlp_tiny.npz"))
    t = lambda k: torch.from_numpy(g[k])
    for cd, tol in ((torch.float32, 2e-5), (torch.float16, 1e-3)):
        mod = _load_module(sm.CustomizedMoEMLP(192, 768, 1, 1, 0.0, compute_dtype=cd), torch.zeros(1, 192),
                           torch.zeros(1), t("fc1_w")[None], t("fc1_b")[None], t("fc2_w")[None], t("fc2_b")[None])
        with torch.no_grad():
            y = mod(t("x").to(DEV)).cpu()
        assert (y - t("y")).abs().max().item() <= tol


def test_moe_module_regression_vectors(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_moe_small.npz"))
    for name in ("naive_k2", "naive_k1"):
        T, k, gate, cap = [int(v) for v in g[f"{name}.meta"]]
        t = lambda key: torch.from_numpy(g[f"{name}.{key}"])
        mod = _load_module(sm.CustomizedMoEMLP(64, 128, 4, k, 0.0, compute_dtype=torch.float32), t("wg"), t("bg"),
                           t("w1"), t("b1"), t("w2"), t("b2"))
        with torch.no_grad():
            out = mod(t("x").to(DEV)).cpu()
        assert torch.equal(mod.last_plan[0].cpu(), t("idx"))
        assert torch.equal(mod.last_plan[4].cpu(), t("pos"))
        assert (out - t("out")).abs().max().item() < 3e-5


def test_moe_switch_gate_capacity_drops_and_aux_loss():
    d, h, E, T = 192, 768, 8, 4000
    x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=77, skew=True)
    mod = sm.FMoETransformerMLP(E, d, h, torch.nn.GELU(), top_k=1, gate="switch", capacity_factor=1.0,
                                compute_dtype=torch.float32)
    mod = _load_module(mod, wg, bg, w1, b1, w2, b2)
    with torch.no_grad():
        out = mod(x.to(DEV)).cpu()
    cap = mo.switch_capacity(1.0, T, 1, E)
    r = mo.moe_forward(x, wg, bg, w1, b1, w2, b2, 1, mo.GATE_SWITCH, cap)
    assert (r.plan.idx_pruned < 0).sum() > 0, "the skewed router must overflow expert 0"
    assert np.array_equal(mod.last_plan[4].cpu().numpy(), r.plan.pos)
    assert (out - r.out).abs().max().item() < 3e-5
    assert torch.all(out[torch.from_numpy(r.plan.idx_pruned < 0)] == 0)
    assert abs(float(mod.gate.get_loss()) - float(r.aux_loss)) < 1e-4


def test_zero_token_rows_from_skip_gate_route_by_bias():
    """Skipped tokens enter the MoE as all-zero rows (resMoE.py:140-143): they all go to argmax(bias) and
    still receive W2 gelu(b1) + b2."""
    d, h, E, T = 192, 768, 4, 500
    x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=5)
    bg = torch.tensor([0.0, 0.3, 0.1, 0.3])
    x[::3] = 0
    mod = _load_module(sm.CustomizedMoEMLP(d, h, E, 1, 0.0, compute_dtype=torch.float32), wg, bg, w1, b1, w2, b2)
    with torch.no_grad():
        out = mod(x.to(DEV)).cpu()
    assert torch.all(mod.last_plan[0].cpu()[::3, 0] == 1)
    const = torch.nn.functional.gelu(b1[1]) @ w2[1].t() + b2[1]
    assert torch.allclose(out[::3], const.expand(len(out[::3]), -1), atol=3e-5)


@pytest.mark.parametrize("T", [0, 1, 3, 64])
def test_moe_module_tiny_and_empty_batches(T):
    d, h, E = 192, 768, 4
    _, wg, bg, w1, b1, w2, b2 = _mk(8, d, h, E, seed=1)
    x = torch.randn(T, d, generator=_gen(T))
    for k in (1, 2):
        mod = _load_module(sm.CustomizedMoEMLP(d, h, E, k, 0.0, compute_dtype=torch.float32), wg, bg, w1, b1, w2, b2)
        ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
        with torch.no_grad():
            out = mod(x.to(DEV))
            out2 = mod.forward_norm_add(x.to(DEV), ln)
        assert out.shape == (T, d) and out2.shape == (T, d)
        if T:
            r = mo.moe_forward(x, wg, bg, w1, b1, w2, b2, k)
            assert (out.cpu() - r.out).abs().max().item() < 3e-5


@pytest.mark.parametrize("d,h,E,k,T", [(768, 3072, 16, 1, 3000), (1024, 4096, 32, 1, 2500), (1024, 4096, 32, 2, 1500)])
def test_moe_module_cfg3_cfg4_dims(d, h, E, k, T):
    """BASELINE cfg 3 / cfg 4 operator shapes (ViT-B E=16; ViT-L d 1024 / h 4096, E=32): general router path
    (E > 8) + the default GEMM variant, f16 operands."""
    x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=E + k)
    wg = wg * 4
    mod = _load_module(sm.CustomizedMoEMLP(d, h, E, k, 0.0), wg, bg, w1, b1, w2, b2)
    with torch.no_grad():
        out = mod(x.to(DEV)).cpu()
    r = mo.moe_forward(x, wg, bg, w1, b1, w2, b2, k)
    assert torch.equal(mod.last_plan[0].cpu(), r.idx)
    assert np.array_equal(mod.last_plan[4].cpu().numpy(), r.plan.pos)
    _float_bar(out, r.out, 1e-3)


# ------------------------------------------------------------------------------------------ full size (cfg 2)
def test_cfg2_full_size_properties():
    """ViT-B/16 E=8 top-1, batch 256 x 197 tokens (BASELINE cfg 2): size-independent properties + a sampled
    oracle comparison (the full CPU oracle would take minutes)."""
    d, h, E, B, N = 768, 3072, 8, 256, 197
    T = B * N
    x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=0)
    mod = _load_module(sm.CustomizedMoEMLP(d, h, E, 1, 0.0), wg, bg, w1, b1, w2, b2)
    xg = x.to(DEV)
    with torch.no_grad():
        out = mod(xg.reshape(B, N, d))
        idx, score, counts, offsets, pos, inv_pos = mod.last_plan
        # permutation properties
        assert int(counts.sum()) == T and int(offsets[-1]) == T
        assert torch.equal(torch.sort(pos).values, torch.arange(T, device=DEV))
        assert torch.equal(inv_pos[pos], torch.arange(T, device=DEV))
        assert torch.equal(idx.reshape(-1)[pos], torch.repeat_interleave(torch.arange(E, device=DEV), counts.long()))
        seg_start = torch.zeros(T, dtype=torch.bool, device=DEV); seg_start[offsets[:-1].long().clamp(max=T - 1)] = True
        assert torch.all((pos[1:] > pos[:-1]) | seg_start[1:]), "ascending token index inside every expert"
        # routing bit-exact against the oracle on all tokens (router is cheap on the CPU)
        o_idx, _, _ = mo.naive_gate(x, wg, bg, 1)
        assert torch.equal(idx.cpu(), o_idx)
        # determinism + row-wise property: permuting the batch permutes the output
        out2 = mod(xg.reshape(B, N, d))
        assert torch.equal(out, out2)
        perm = torch.randperm(T, generator=_gen(1)).to(DEV)
        outp = mod(xg[perm].reshape(B, N, d)).reshape(T, d)
        assert (outp - out.reshape(T, d)[perm]).abs().max().item() == 0.0
    # sampled oracle comparison on 2048 random tokens, f16 MFMA operands (the benchmarked mode), at the float bar:
    # max |diff| <= 1e-3 * max(1, max |ref|) and relative L2 <= 1e-3 (error budget in DESIGN.md section 2)
    sel = torch.randperm(T, generator=_gen(2))[:2048]
    r = mo.moe_forward(x[sel], wg, bg, w1, b1, w2, b2, 1)
    _float_bar(out.reshape(T, d).cpu()[sel], r.out, 1e-3)
    # the f32-exact MFMA mode meets the strict bound on every element
    mod32 = _load_module(sm.CustomizedMoEMLP(d, h, E, 1, 0.0, compute_dtype=torch.float32), wg, bg, w1, b1, w2, b2)
    with torch.no_grad():
        out32 = mod32(xg[sel.to(DEV)].reshape(8, 256, d)).reshape(-1, d).cpu()
    assert (out32 - r.out).abs().max().item() <= 1e-4


# ------------------------------------------------------------------------------------------ expert-parallel code path
def test_expert_parallel_path_on_one_gpu():
    """The expert-parallel forward (ep.py: chunked plans, count exchange, all-to-all-v over RCCL, grouped GEMM with
    a group->expert map, gather_combine into output slices) driven on the real GPU with a world of ONE rank
    (the multi-rank exchange logic itself is covered with gloo in test_ep_gloo.py)."""
    import socket
    import torch.distributed as dist

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(DEV))
    try:
        d, h, E, T = 192, 768, 8, 2500
        for k, chunks, cd, tol in ((1, 1, torch.float32, 3e-5), (1, 3, torch.float32, 3e-5), (2, 2, torch.float32, 3e-5),
                                   (1, 2, torch.float16, 2e-3)):
            x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=50 + k + chunks)
            mod = _load_module(sm.CustomizedMoEMLP(d, h, E, k, 0.0, compute_dtype=cd), wg, bg, w1, b1, w2, b2)
            r = torch.randn(T, d, generator=_gen(9)).to(DEV)
            with torch.no_grad():
                ref = mod(x.to(DEV))
                ref_add = mod.forward_add(x.to(DEV), r)
                mod.force_ep, mod.ep_chunks = True, chunks
                got = mod(x.to(DEV))
                got_add = mod.forward_add(x.to(DEV), r)
            o = mo.moe_forward(x, wg, bg, w1, b1, w2, b2, k).out
            if cd == torch.float16:
                _float_bar(got.cpu(), o, 1e-3)   # expert outputs vs the oracle: the one float bar
            else:
                assert (got.cpu() - o).abs().max().item() <= tol
            assert (got - ref).abs().max().item() <= tol
            assert (got_add - ref_add).abs().max().item() <= tol
            # block half with the fused LayerNorm + router in front of the expert-parallel exchange
            ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
            with torch.no_grad():
                ep_ln = mod.forward_norm_add(x.to(DEV), ln)
                mod.force_ep = False
                ref_ln = mod.forward_norm_add(x.to(DEV), ln)
            assert (ep_ln - ref_ln).abs().max().item() <= max(tol, 2e-3 if cd == torch.float16 else tol)
        # switch gate with drops runs un-chunked and keeps dropped rows at zero / at the residual
        x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=99, skew=True)
        mod = sm.FMoETransformerMLP(E, d, h, torch.nn.GELU(), top_k=1, gate="switch", capacity_factor=1.0,
                                    compute_dtype=torch.float32)
        mod = _load_module(mod, wg, bg, w1, b1, w2, b2)
        mod.force_ep = True
        with torch.no_grad():
            got = mod(x.to(DEV)).cpu()
        o = mo.moe_forward(x, wg, bg, w1, b1, w2, b2, 1, mo.GATE_SWITCH, mo.switch_capacity(1.0, T, 1, E))
        assert (got - o.out).abs().max().item() <= 3e-5
        assert torch.all(got[torch.from_numpy(o.plan.idx_pruned < 0)] == 0)
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------- expert-parallel layouts on one GPU
@pytest.mark.parametrize("variant,cd,tol", [(0, torch.float32, 2e-5), (4, torch.float16, 1e-3), (5, torch.float16, 1e-3),
                                            (6, torch.bfloat16, 8e-3)])
def test_grouped_gemm_group_expert_map_many_groups_per_expert(variant, cd, tol):
    """The expert-parallel receive layout: W * E_local row groups ordered [source rank][local expert], several
    groups per weight, some empty -- the group -> expert map must pick the right weight for every group."""
    W_ranks, E_local, K, N = 4, 2, 128, 192
    counts = [300, 5, 0, 130, 77, 0, 256, 321]           # [w][e]
    gexp = torch.arange(E_local, dtype=torch.int32).repeat(W_ranks)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    M = int(offsets[-1])
    g = _gen(71)
    A = torch.randn(M, K, generator=g).to(cd)
    Wt = (torch.randn(E_local, N, K, generator=g) * 0.05).to(cd)
    bias = torch.randn(E_local, N, generator=g) * 0.1
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ops.grouped_gemm(A.to(DEV), Wt.to(DEV), bias.to(DEV), torch.from_numpy(offsets).to(DEV), ops.EPI_GELU, out=out,
                     variant=variant, group_expert=gexp.to(DEV))
    ref = torch.zeros(M, N, dtype=torch.float64)
    for gi in range(len(counts)):
        lo, hi, e = int(offsets[gi]), int(offsets[gi + 1]), int(gexp[gi])
        if hi > lo:
            ref[lo:hi] = torch.nn.functional.gelu(A[lo:hi].double() @ Wt[e].double().t() + bias[e].double())
    assert (out.cpu().double() - ref).abs().max() <= tol * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("W_ranks,E_local,k,d,h", [(2, 4, 1, 192, 768), (4, 2, 1, 192, 768), (8, 1, 1, 192, 768),
                                                   (4, 2, 2, 192, 768),
                                                   (4, 4, 1, 768, 3072),      # BASELINE cfg 3's own layout (E = 16)
                                                   (8, 4, 1, 1024, 4096)])    # BASELINE cfg 4's own layout (E = 32)
def test_expert_parallel_data_path_simulated_ranks(W_ranks, E_local, k, d, h):
    """Every rank's side of ep.ep_forward_steps with W > 1, replayed on one GPU: the ranks' token shards are routed
    with the HIP router / plan, the all-to-all is done by hand (slices of the send buffers, [source rank][local
    expert] receive order), each simulated rank runs the HIP expert FFN on its receive buffer through the
    group -> expert map and device-side group offsets exactly as ep.py builds them, rows travel back and are combined
    with the HIP gather -- the result must equal the oracle's single-rank forward of every shard."""
    from slim_switch_moe_vit_amd import ep
    E = W_ranks * E_local
    cd = torch.float16
    T_r = [700, 333, 1, 512, 64, 900, 257, 128][:W_ranks]
    xs, wg, bg, w1, b1, w2, b2 = [], None, None, None, None, None, None
    _, wg, bg, w1, b1, w2, b2 = _mk(1, d, h, E, seed=500 + W_ranks + k)
    xs = [torch.randn(t, d, generator=_gen(600 + r)) for r, t in enumerate(T_r)]
    mods = []
    for r in range(W_ranks):   # rank r holds the gate for all E experts and the weights of its E_local experts
        m = sm.FMoETransformerMLP(E_local, d, h, torch.nn.GELU(), top_k=k, world_size=W_ranks, compute_dtype=cd)
        sl = slice(r * E_local, (r + 1) * E_local)
        mods.append(_load_module(m, wg, bg, w1[sl], b1[sl], w2[sl], b2[sl]))
    # sender side
    plans, sends, scores, lec = [], [], [], []
    for r in range(W_ranks):
        x = xs[r].to(DEV)
        idx, score, _, _ = ops.router_topk(x, wg.to(DEV), bg.to(DEV), k, ops.GATE_NAIVE)
        counts, offsets, pos, inv_pos, _ = ops.dispatch_plan(idx, E, -1)
        plans.append((counts, offsets, pos, inv_pos))
        scores.append(score)
        sends.append(ops.scatter_rows(x, pos, k, cd))
        lec.append(counts.cpu().long().reshape(W_ranks, E_local))
    # the exchange, by hand
    outs = []
    backs = [[None] * W_ranks for _ in range(W_ranks)]   # backs[src][dst]
    for dst in range(W_ranks):
        pieces, gec = [], torch.zeros(W_ranks, E_local, dtype=torch.int32)
        for src in range(W_ranks):
            off = plans[src][1].cpu().long()
            lo, hi = int(off[dst * E_local]), int(off[(dst + 1) * E_local])
            pieces.append(sends[src][lo:hi])
            gec[src] = lec[src][dst].int()
        recv = torch.cat(pieces, 0)
        both = torch.zeros(2, W_ranks, 1, E_local, dtype=torch.int32, device=DEV)
        both[1, :, 0, :] = gec.to(DEV)
        offs_dev = ep.PendingCounts(None, None, False, both).group_offsets(0)
        assert int(offs_dev[-1]) == recv.shape[0]
        assert offs_dev.cpu().tolist() == ep.segment_table(gec.long())[0]
        gexp = ep._group_expert_ids(W_ranks, E_local, torch.device(DEV))
        assert gexp.cpu().tolist() == ep.segment_table(gec.long())[1]
        y = mods[dst]._experts_fwd(recv, offs_dev, cd, out_dtype=cd, group_expert=gexp) if recv.shape[0] else recv
        at = 0
        for src in range(W_ranks):
            n = int(gec[src].sum())
            backs[src][dst] = y[at:at + n]
            at += n
    for r in range(W_ranks):
        back = torch.cat(backs[r], 0)
        T = xs[r].shape[0]
        got = ops.gather_combine(back, plans[r][3], scores[r], T, k, torch.float32).cpu()
        ref = mo.moe_forward(xs[r], wg, bg, w1, b1, w2, b2, k).out
        _float_bar(got, ref, 1e-3)


@pytest.mark.parametrize("variant", [9, 10, 11, 12, 13, 14])
def test_persistent_gemm_equals_one_workgroup_per_tile_kernel_bitwise(variant):
    """grouped_gemm_ps (one workgroup per CU walking tiles, the next tile's operands streaming under the epilogue) must
    reproduce grouped_gemm_pp256 bit for bit in every fused form it is used in: gathered A rows + bias + GELU (GEMM-1),
    row-mapped scaled store + in-place residual (GEMM-2), many more tiles than CUs, ragged / empty groups, N tails."""
    counts = [5000, 0, 333, 7001, 64, 2900, 1, 4100]
    E, d, h = len(counts), 256, 1096                       # h: n-tile tail (1096 = 4 * 256 + 72)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), device=DEV)
    M = int(offsets[-1])
    g = _gen(variant)
    x16 = torch.randn(M, d, generator=g).half().to(DEV)
    pos = torch.randperm(M, generator=g).to(DEV)           # a_gather: any permutation of the rows
    w1 = (torch.randn(E, h, d, generator=g) * 0.05).half().to(DEV)
    b1 = (torch.randn(E, h, generator=g) * 0.1).to(DEV)
    w2 = (torch.randn(E, d, h + 56, generator=g) * 0.05).half().to(DEV)[:, :, :h].contiguous()
    b2 = (torch.randn(E, d, generator=g) * 0.1).to(DEV)
    score = torch.rand(M, generator=g).to(DEV)
    res = torch.randn(M, d, generator=g).to(DEV)
    base = {9: 4, 10: 5, 11: 6, 12: 7, 13: 8, 14: 4}[variant]     # the same tile height / schedule, one workgroup per tile
    for _ in range(3):
        h_ref = ops.grouped_gemm(x16, w1, b1, offsets, ops.EPI_GELU, torch.float16, variant=base, a_gather=pos)
        h_ps = ops.grouped_gemm(x16, w1, b1, offsets, ops.EPI_GELU, torch.float16, variant=variant, a_gather=pos)
        assert torch.equal(h_ps, h_ref)
    hk = h_ref[:, :1088].contiguous()                      # K = 1088 = 17 * 64
    w2k = w2[:, :, :1088].contiguous()
    for _ in range(3):
        o_ref = res.clone()
        ops.grouped_gemm(hk, w2k, b2, offsets, ops.EPI_NONE, torch.float32, row_map=pos, row_scale=score, out=o_ref,
                         variant=base, residual=o_ref)
        o_ps = res.clone()
        ops.grouped_gemm(hk, w2k, b2, offsets, ops.EPI_NONE, torch.float32, row_map=pos, row_scale=score, out=o_ps,
                         variant=variant, residual=o_ps)
        assert torch.equal(o_ps, o_ref)


def _plan_rule(rows, G, K, N, cus):
    """include/slimmoe.h's statement of the tile rule (smoe_grouped_gemm_plan), in integers: the explicit persistent variant."""
    ceil = lambda a, b: -(-a // b)
    t256, t320 = ((ceil(rows, h) + G // 2) * ceil(N, 256) for h in (256, 320))
    tall = ceil(t320, cus) * 1.25 <= ceil(t256, cus)
    if K >= 2048:
        return 13 if tall else 12
    return 10 if tall else 11


# (rows, G, K, N); the comment = the outcome on 256 CUs (tiles of 256 / 320 rows -> rounds of workgroups)
_PLAN_CASES = [(50432, 8, 768, 3072),       # 10: 2412 / 1944 tiles, 10 / 8 rounds, 8 * 1.25 == 10: the tie goes to the tall tile
               (50432, 8, 3072, 768),       # 13: 603 / 486 tiles, 3 / 2 rounds; K >= 2048
               (50432, 1, 768, 2304),       # 11: 1773 / 1422 tiles, 7 / 6 rounds, 7.5 > 7
               (50432, 1, 2048, 2304),      # 12: the same tiles at K = 2048
               (50432, 1, 1984, 2304),      # 11: K = 2047 rounded down to a multiple of 64
               (50432, 1, 2112, 2304),      # 12: K = 2049 rounded up
               (50432, 8, 1984, 768),       # 10: the K threshold on the tall tile, below ...
               (50432, 8, 2048, 768),       # 13: ... and at it
               (20224, 1, 768, 1024),       # 10: one group adds no expected tile (G // 2 == 0): 316 / 256 tiles, 2 / 1 rounds
               (30000, 63, 768, 3072),      # 11: 31 expected extra m-tiles: 1788 / 1500 tiles, 7 / 6 rounds
               (400, 3, 128, 264),          # 11: one round either way
               (1, 1, 64, 8),               # 11: a single tile
               (0, 1, 64, 8),               # 10: no tile at all: 0 * 1.25 <= 0
               (2 ** 31 - 1, 63, 4096, 8192)]   # 12: 64-bit tile counts (268436448 / 214749376 tiles)


def test_grouped_gemm_plan_is_the_library_rule():
    """smoe_grouped_gemm_plan -- what ops.grouped_gemm asks for the static expert exchange's tile height -- is the rule the header
    states: t = (ceil(rows / h) + G // 2) * ceil(N / 256) expected tiles of h rows, tall iff ceil(t320 / cus) * 1.25 <=
    ceil(t256 / cus), deep iff K >= 2048.  The cases cover the four outcomes, a tie and the K threshold."""
    assert {_plan_rule(*c, 256) for c in _PLAN_CASES} == {10, 11, 12, 13}
    lib = sm._lib.load()
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    with torch.cuda.device(DEV):
        got = [lib.smoe_grouped_gemm_plan(*c) for c in _PLAN_CASES]
        print(f"cus = {cus}; plans = {got}")
        assert got == [_plan_rule(*c, cus) for c in _PLAN_CASES]
        if cus == 256:   # the benchmark model's GEMM-1, GEMM-2 and qkv: the instantiations bench.py names
            assert lib.smoe_grouped_gemm_plan(50432, 8, 768, 3072) == 10
            assert lib.smoe_grouped_gemm_plan(50432, 8, 3072, 768) == 13
            assert lib.smoe_grouped_gemm_plan(50432, 1, 768, 2304) == 11


def test_auto_variant_equals_its_planned_variant_bitwise():
    """The variant table from the outside: the auto variant of each family (9 persistent, 4 one workgroup per tile) gives the bits
    of the explicit variant smoe_grouped_gemm_plan names -- the same column of the other family's row for 4."""
    counts = [70, 0, 330]
    E, K, N = len(counts), 128, 264
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), device=DEV)
    M = int(offsets[-1])
    g = _gen(9)
    a = torch.randn(M, K, generator=g).half().to(DEV)
    w = (torch.randn(E, N, K, generator=g) * 0.05).half().to(DEV)
    bias = (torch.randn(E, N, generator=g) * 0.1).to(DEV)
    with torch.cuda.device(DEV):
        plan = sm._lib.load().smoe_grouped_gemm_plan(M, E, K, N)
    assert plan in (10, 11, 12, 13)
    run = lambda v: ops.grouped_gemm(a, w, bias, offsets, ops.EPI_GELU, torch.float16, variant=v)
    assert torch.equal(run(9), run(plan))
    assert torch.equal(run(4), run(plan - 9 + 4))


@pytest.mark.parametrize("N", [256, 512, 768, 1024, 1280])
@pytest.mark.parametrize("K", [256, 2048])
def test_persistent_gemm_f32_epilogue_and_tile_orders_bitwise(N, K):
    """The f32-output forms of the persistent kernel (round 3): the buffer-addressed staged epilogue (every load / store issued,
    invalid ones out of the descriptors' range) and the XCD-contiguous tile order it runs under for N <= 1024 (1-4 n-tiles; 5
    n-tiles keep the strided order), on the plain (K 256) and the deep (K 2048) schedule: bit for bit the one-workgroup-per-tile
    kernel -- row-mapped + scaled + in-place residual, plain with a separate residual, plain without one, ragged / empty groups,
    an output with more rows than dispatched rows."""
    counts = [1900, 0, 333, 2101, 64, 700, 1, 960]
    E = len(counts)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), device=DEV)
    M = int(offsets[-1])
    T = M + 500                                            # token rows: some tokens were not dispatched
    g = _gen(N + K)
    a = torch.randn(M, K, generator=g).half().to(DEV)
    w = (torch.randn(E, N, K, generator=g) * 0.05).half().to(DEV)
    bias = (torch.randn(E, N, generator=g) * 0.1).to(DEV)
    pos = torch.randperm(T, generator=g)[:M].to(DEV)       # row_map: dispatch row -> token row (values up to T - 1 >= M)
    score = torch.rand(T, generator=g).to(DEV)
    res = torch.randn(T, N, generator=g).to(DEV)
    outs = {}
    for v in (4, 9, 14):
        o = res.clone()
        ops.grouped_gemm(a, w, bias, offsets, ops.EPI_NONE, torch.float32, row_map=pos, row_scale=score, out=o, variant=v, residual=o)
        p_res = ops.grouped_gemm(a, w, bias, offsets, ops.EPI_NONE, torch.float32, variant=v, residual=res[:M].contiguous())
        p_gelu = ops.grouped_gemm(a, w, bias, offsets, ops.EPI_GELU, torch.float32, variant=v)
        outs[v] = (o, p_res, p_gelu)
    for v in (9, 14):
        for got, ref in zip(outs[v], outs[4]):
            assert torch.equal(got, ref), f"variant {v}"
    untouched = torch.ones(T, dtype=torch.bool, device=DEV)
    untouched[pos] = False
    assert torch.equal(outs[9][0][untouched], res[untouched]), "token rows that were not dispatched keep the residual"


def test_cabi_exchange_context_world_of_one_and_ep_transport():
    """include/slimmoe.h smoe_ctx_* / smoe_a2a_*: RCCL communicator from a unique-id blob, dedicated communication
    stream, event fences.  One GPU = a world of one rank (what hardware this box has): counts and rows come back
    unchanged, blocking, split (wait=False + wait_stream) and in-line (on the caller's stream) forms; then the expert-parallel
    forward on this transport (SLIMMOE_EP_TRANSPORT=cabi, and with SLIMMOE_EP_INLINE=1) reproduces the torch.distributed
    transport bit for bit."""
    import socket
    import torch.distributed as dist
    from slim_switch_moe_vit_amd.comm import ExchangeContext
    from slim_switch_moe_vit_amd import ep

    ctx = ExchangeContext(ExchangeContext.new_unique_id(), 1, 0, torch.device(DEV))
    try:
        cnt = torch.tensor([5, 0, 7, 1], dtype=torch.int32, device=DEV)
        assert torch.equal(ctx.exchange_counts(cnt, 4), cnt)
        rows = torch.randn(1000, 192, generator=_gen(1)).half().to(DEV)
        got = ctx.all_to_all_rows(rows, [777], [777])
        assert torch.equal(got, rows[:777])
        big = torch.randn(50000, 768, generator=_gen(2)).half().to(DEV)
        got2 = ctx.all_to_all_rows(big, [50000], [50000], wait=False)   # rows travel on the context's stream ...
        busy = (big.float() @ torch.randn(768, 64, device=DEV)).sum()   # ... while this stream computes
        ctx.wait_stream(got2)
        assert torch.equal(got2, big) and torch.isfinite(busy)
        empty = ctx.all_to_all_rows(rows[:0], [0], [0])
        assert empty.shape == (0, 192)
        # two exchanges in flight, waited for OUT OF ORDER through their tickets (a micro-batch pipeline does exactly this)
        a = ctx.all_to_all_rows(big, [50000], [50000], wait=False)
        ta = ctx.last_ticket()
        b = ctx.all_to_all_rows(rows, [777], [777], wait=False)
        tb = ctx.last_ticket()
        assert tb == ta + 1
        ctx.wait_stream(b, tb)
        assert torch.equal(b, rows[:777])
        ctx.wait_stream(a, ta)
        assert torch.equal(a, big)
        # more exchanges in flight than the completion ring holds: the oldest ticket still waits correctly (for a later one)
        outs = [(ctx.all_to_all_rows(rows, [100 + i], [100 + i], wait=False), ctx.last_ticket()) for i in range(40)]
        for i in (0, 39, 17):
            o, t = outs[i]
            ctx.wait_stream(o, t)
            assert torch.equal(o, rows[:100 + i])
        with pytest.raises(Exception):
            ctx.wait_stream(rows, ctx.last_ticket() + 5)    # no such exchange
        # SMOE_A2A_INLINE: on the caller's stream itself -- in order with the kernels either side, no ticket taken
        t_before = ctx.last_ticket()
        src = big.clone()
        src.mul_(2)
        inl = ctx.all_to_all_rows(src, [50000], [50000], wait="inline")
        src.zero_()                                          # later on the same stream: must not reach the exchange
        assert torch.equal(inl, big * 2) and ctx.last_ticket() == t_before
    finally:
        ctx.close()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        d, h, E, T = 192, 768, 8, 2500
        x, wg, bg, w1, b1, w2, b2 = _mk(T, d, h, E, seed=61)
        mod = _load_module(sm.CustomizedMoEMLP(d, h, E, 2, 0.0), wg, bg, w1, b1, w2, b2)
        mod.force_ep, mod.ep_chunks = True, 2
        with torch.no_grad():
            ref = mod(x.to(DEV))
            os.environ["SLIMMOE_EP_TRANSPORT"] = "cabi"
            try:
                got = mod(x.to(DEV))
                os.environ["SLIMMOE_EP_INLINE"] = "1"
                got_inline = mod(x.to(DEV))
            finally:
                os.environ.pop("SLIMMOE_EP_TRANSPORT", None)
                os.environ.pop("SLIMMOE_EP_INLINE", None)
        assert len(ep._ctx_cache) == 1, "the C-ABI transport must have been the one that ran"
        assert torch.equal(got, ref) and torch.equal(got_inline, ref)
    finally:
        for c in ep._ctx_cache.values():
            c.close()
        ep._ctx_cache.clear()
        dist.destroy_process_group()


# ------------------------------------------------------------------------- static (capacity-padded) exchange layout
@pytest.mark.parametrize("n,E,cap", [(50432, 8, 6304), (3000, 8, 100), (777, 4, 1000), (36928, 32, 1154), (5000, 16, 1)])
def test_dispatch_plan_padded_layout_bit_exact(n, E, cap):
    """smoe_dispatch_plan_padded: expert e owns slots [e slot, (e + 1) slot), slot >= cap (the size every rank agreed on); same
    kept set, same order inside an expert as the compact plan (= the oracle's), unused slots -1, group_end = e slot + counts."""
    slot = cap + (n % 3) * 5
    rng = np.random.default_rng(n + E)
    idx = rng.integers(-1 if n % 2 else 0, E, size=n).astype(np.int64)
    idx[rng.random(n) < 0.3] = 0   # overloaded expert: drops
    counts, offsets, gend, pos_pad, inv_pos, pruned = ops.dispatch_plan_padded(torch.from_numpy(idx).to(DEV), E, cap, slot)
    p = mo.dispatch_plan(idx, E, cap)
    cap_keep, cap = cap, slot       # below: the layout's stride
    assert np.array_equal(counts.cpu().numpy(), p.counts) and np.array_equal(offsets.cpu().numpy(), p.offsets)
    assert np.array_equal(pruned.cpu().numpy(), p.idx_pruned)
    assert np.array_equal(gend.cpu().numpy(), np.arange(E) * cap + p.counts)
    want_pos = np.full(E * cap, -1, dtype=np.int64)
    want_inv = np.full(n, -1, dtype=np.int64)
    for e in range(E):
        seg = p.pos[p.offsets[e]:p.offsets[e + 1]]
        want_pos[e * cap:e * cap + len(seg)] = seg
        want_inv[seg] = e * cap + np.arange(len(seg))
    assert np.array_equal(pos_pad.cpu().numpy(), want_pos)
    assert np.array_equal(inv_pos.cpu().numpy(), want_inv)


@pytest.mark.parametrize("variant", [9, 10, 14])
@pytest.mark.parametrize("out_dt", [torch.float16, torch.float32])
def test_grouped_gemm_separate_row_ranges_touch_only_their_rows(variant, out_dt):
    """group_end: G padded slots of `cap` rows, only [start, end) of each filled (some empty, one full, one past a tile
    boundary); rows outside the ranges hold NaN in A and a sentinel in out -- neither may matter / change."""
    cap, K, N = 700, 256, 328
    fill = [700, 0, 1, 321, 64, 699, 320, 5]
    gexp = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1], dtype=torch.int32)
    G, E = len(fill), 3
    g = _gen(variant)
    A = torch.randn(G * cap, K, generator=g).half()
    W = (torch.randn(E, N, K, generator=g) * 0.05).half()
    bias = torch.randn(E, N, generator=g) * 0.1
    starts = (torch.arange(G) * cap).int()
    ends = starts + torch.tensor(fill, dtype=torch.int32)
    valid = torch.zeros(G * cap, dtype=torch.bool)
    for l in range(G):
        valid[l * cap:l * cap + fill[l]] = True
    A_dev = A.clone()
    A_dev[~valid] = float("nan")
    out = torch.full((G * cap, N), 7.0, dtype=out_dt, device=DEV)
    ops.grouped_gemm(A_dev.to(DEV), W.to(DEV), bias.to(DEV), starts.to(DEV), ops.EPI_GELU, out_dt, out=out, variant=variant,
                     group_expert=gexp.to(DEV), group_end=ends.to(DEV))
    got = out.float().cpu()
    assert torch.all(got[~valid] == 7.0), "rows outside the ranges must stay untouched"
    ref = torch.zeros(G * cap, N, dtype=torch.float64)
    for l in range(G):
        r = slice(l * cap, l * cap + fill[l])
        ref[r] = torch.nn.functional.gelu(A[r].double() @ W[gexp[l]].double().t() + bias[gexp[l]].double())
    assert (got.double()[valid] - ref[valid]).abs().max() <= 1e-3 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("T,d,E,k,cap", [(50432, 768, 8, 1, -1), (1576, 192, 4, 1, -1), (3001, 768, 8, 2, -1), (9000, 384, 8, 1, 700),
                                         (777, 1024, 5, 4, -1), (64, 192, 8, 1, -1), (65, 192, 8, 2, 10)])
def test_router_chunk_histogram_gives_the_same_plan_without_the_counting_launch(T, d, E, k, cap):
    """count_by_gate folded into the fused LayerNorm + router pass (chunk_hist): the table equals a bincount of idx per 64-token
    chunk -- INCLUDING the tokens the f64 redo pass decides (exact ties planted below) -- and smoe_dispatch_plan_hist builds from it,
    bit for bit, the plan smoe_dispatch_plan builds by counting idx itself (oracle-pinned in test_dispatch_plan_bit_exact)."""
    from slim_switch_moe_vit_amd import ops
    ops.ROUTER_HIST = True                           # (opt-in: measured no faster, ops.py)
    g = torch.Generator().manual_seed(T + E)
    x = torch.randn(T, d, generator=g)
    wg = torch.randn(E, d, generator=g) * 0.1
    bg = torch.randn(E, generator=g) * 0.05
    if E >= 2:
        wg[1] = wg[0]; bg[1] = bg[0]                 # experts 0 and 1 tie on EVERY token: wherever they are in the top k + 1
    lw, lb = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    hist = ops.chunk_hist(T, d, E, k, DEV)
    if k == 3 or hist is None:
        pytest.skip("this shape's router writes no histogram")
    hist.fill_(-7)                                   # every row must be written
    xn16, _, idx, score, _, _ = ops.ln_router_topk(x.to(DEV), lw.to(DEV), lb.to(DEV), 1e-6, wg.to(DEV), bg.to(DEV), k, hist=hist)
    ref_idx = ops.ln_router_topk(x.to(DEV), lw.to(DEV), lb.to(DEV), 1e-6, wg.to(DEV), bg.to(DEV), k)[2]
    assert torch.equal(idx, ref_idx), "the chunked token order must not change a decision"
    tok = hist.tok
    want = torch.zeros_like(hist)
    chunk = (torch.arange(T, device=DEV) // tok)[:, None].expand(T, k).reshape(-1)
    want.view(-1).index_add_(0, chunk * E + idx.reshape(-1), torch.ones(T * k, dtype=torch.int32, device=DEV))
    assert torch.equal(hist, want)
    a = ops.dispatch_plan(idx, E, cap, hist=hist)
    b = ops.dispatch_plan(idx, E, cap)
    ops.ROUTER_HIST = False
    for u, v, nm in zip(a, b, ("counts", "offsets", "pos", "inv_pos", "pruned")):
        assert (u is None and v is None) or torch.equal(u, v), nm


def test_gated_router_chunk_histogram_counts_only_dispatched_tokens():
    """The token-skip gate's fused pass (smoe_gate_ln_router): skipped tokens (idx_plan = -1) are not in the histogram, tokens on the
    gate's threshold are counted by the pass that decides them, and the plan over idx_plan equals the counting plan."""
    from slim_switch_moe_vit_amd import ops
    ops.ROUTER_HIST = True
    T, d, E, k = 5000, 192, 8, 2
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, d, generator=g)
    gw, gb = torch.randn(1, d, generator=g) * 0.1, torch.zeros(1)
    wg, bgr = torch.randn(E, d, generator=g) * 0.1, torch.randn(E, generator=g) * 0.05
    lw, lb = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    thr = torch.tensor(0.5, device=DEV)
    hist = ops.chunk_hist(T, d, E, k, DEV)
    hist.fill_(-7)
    r = ops.gate_ln_router(x.to(DEV), gw.to(DEV), gb.to(DEV), thr, ln=(lw.to(DEV), lb.to(DEV), 1e-6), wg=wg.to(DEV), bg=bgr.to(DEV),
                           k=k, xn16_dtype=torch.float16, want_xn32=True, want_mask=True, hist=hist)
    ip = r["idx_plan"]
    n_skip = int((ip[:, 0] < 0).sum())
    assert 0 < n_skip < T
    keep = (ip >= 0).reshape(-1)
    chunk = (torch.arange(T, device=DEV) // hist.tok)[:, None].expand(T, k).reshape(-1)
    want = torch.zeros_like(hist)
    want.view(-1).index_add_(0, (chunk * E + ip.reshape(-1).clamp(min=0))[keep], torch.ones(int(keep.sum()), dtype=torch.int32, device=DEV))
    assert torch.equal(hist, want)
    a = ops.dispatch_plan(ip, E, -1, hist=hist)
    b = ops.dispatch_plan(ip, E, -1)
    ops.ROUTER_HIST = False
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)
