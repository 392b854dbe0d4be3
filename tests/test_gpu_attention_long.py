"""Attention training for 256 < N <= 640 (ViT-L/16 @384: N = 577) on the library's own kernels: the long forward's log-sum-exp and
the two backward kernels behind smoe_attention_bwd (attn_bwd_dq_kernel, attn_bwd_dkv_kernel; csrc/attention_bwd.hip).

Bars.  lse: the project's bar for the short kernel (tests/test_gpu_dense.py: 2e-3 f16 / 2e-2 bf16, absolute).  dq / dk / dv: the
short kernel's bar is relative L2 <= tol and max |diff| <= 5 tol max |ref| with tol = 4e-3 f16 / 2e-2 bf16 -- the long kernels round
at the same points (16-bit P and dS operands, f32 accumulation).  Measured on an MI355X over the shapes below (worst of dq / dk / dv):
relative L2 3.12e-4 f16 / 2.52e-3 bf16, max |diff| / max |ref| 7.91e-4 f16 / 5.52e-3 bf16 -- so both bars are tightened to 3 x the
measured error (the project's rule), which is inside the short kernel's bar in every case.  The tests print what they measure;
profiles/r07_attn_bwd_long.md holds the table."""
import functools
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import dense, ops, vit  # noqa: E402
import test_nonfinite_cones as nc  # noqa: E402
import test_gpu_nonfinite as gnf  # noqa: E402  (the module, for check_case: none of its tests is collected here)

DEV = "cuda:0"
SCALE = 64 ** -0.5
# the forward's own long-sequence list (tests/test_gpu_parity.py::test_attention_kernel_long_sequences_online_softmax)
SHAPES = [(2, 577, 16), (1, 257, 2), (2, 300, 3), (1, 592, 2), (1, 640, 1), (3, 321, 4), (1, 480, 2)]
DTYPES = [torch.float16, torch.bfloat16]
LSE_TOL = {torch.float16: 2e-3, torch.bfloat16: 2e-2}
BWD_REL = {torch.float16: 9.4e-4, torch.bfloat16: 7.6e-3}       # relative L2: 3 x measured (short kernel's bar: 4e-3 / 2e-2)
BWD_MAX = {torch.float16: 2.4e-3, torch.bfloat16: 1.7e-2}       # max |diff| / max |ref|: 3 x measured (short kernel's: 2e-2 / 1e-1)


def _inputs(B, N, H, dt):
    """as tests/test_gpu_dense.py::test_attention_backward_matches_float64_autograd generates them"""
    g = torch.Generator().manual_seed(B * 1000 + N + H)
    qkv = (torch.randn(B, N, 3, H, 64, generator=g) * 1.2).to(dt)
    do = (torch.randn(B, N, H * 64, generator=g) * 0.5).to(dt)
    return qkv, do


def _f64(qkv, do):
    B, N, _, H, _ = qkv.shape
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.permute(2, 0, 3, 1, 4).unbind(0)
    s = q @ k.transpose(-2, -1) * SCALE
    (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, H * 64).backward(do.double())
    lse = torch.logsumexp(s.detach(), -1) / torch.log(torch.tensor(2.0, dtype=torch.float64))
    return lse, qr.grad


@functools.lru_cache(maxsize=None)
def _run(B, N, H, dt):
    """inputs, float64 reference and the kernels' results of one (shape, dtype), computed once and shared by the tests below"""
    qkv, do = _inputs(B, N, H, dt)
    lse_ref, grad_ref = _f64(qkv, do)
    qd, dd = qkv.to(DEV), do.to(DEV)
    out, lse = ops.attention(qd, B, N, H, 64, SCALE, want_lse=True)
    dqkv = ops.attention_bwd(qd, out, dd, lse, B, N, H, 64, SCALE)
    return dict(qkv=qd, do=dd, out=out, lse=lse, dqkv=dqkv, lse_ref=lse_ref, grad_ref=grad_ref)


def _bwd_errors(dqkv, grad_ref):
    """per q / k / v: (relative L2, max |diff| / max |ref|)"""
    res = []
    for i in range(3):
        got, ref = dqkv[:, :, i].double().cpu(), grad_ref[:, :, i]
        res.append((float((got - ref).norm() / ref.norm().clamp(min=1e-30)), float((got - ref).abs().max() / ref.abs().max())))
    return res


def _assert_bwd(dqkv, grad_ref, dt, what):
    errs = _bwd_errors(dqkv, grad_ref)
    print(f"{what} {str(dt)[6:]}: " + "  ".join(f"d{nm} rel L2 {e[0]:.2e} max/max|ref| {e[1]:.2e}" for nm, e in zip("qkv", errs)))
    for nm, (rel, mx) in zip("qkv", errs):
        assert rel <= BWD_REL[dt], (what, nm, rel)
        assert mx <= BWD_MAX[dt], (what, nm, mx)


@pytest.mark.parametrize("B,N,H", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_long_forward_hands_out_the_log_sum_exp(B, N, H, dt):
    """lse of attn_fwd_long_kernel against float64 logsumexp / ln 2, and `out` is the same bits with and without it."""
    r = _run(B, N, H, dt)
    err = float((r["lse"].cpu().double() - r["lse_ref"]).abs().max())
    print(f"lse B {B} N {N} H {H} {str(dt)[6:]}: max |lse - f64| {err:.2e}")
    assert err <= LSE_TOL[dt]
    assert torch.equal(r["out"], ops.attention(r["qkv"], B, N, H, 64, SCALE))


@pytest.mark.parametrize("B,N,H", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_long_backward_matches_float64_autograd(B, N, H, dt):
    """dq, dk, dv of softmax(q k^T scale) v (models/vision_transformer.py:263-275) on the fused [B, N, 3, H, 64] layout, N > 256."""
    r = _run(B, N, H, dt)
    _assert_bwd(r["dqkv"], r["grad_ref"], dt, f"B {B} N {N} H {H}")
    qg = r["qkv"].clone().requires_grad_(True)
    dense.AttentionFn.apply(qg, B, N, H, 64, SCALE).backward(r["do"])
    assert torch.equal(qg.grad, r["dqkv"])


@pytest.mark.parametrize("B,N,H", [(2, 577, 16), (1, 640, 1)])
@pytest.mark.parametrize("dt", DTYPES)
def test_long_backward_is_deterministic(B, N, H, dt):
    r = _run(B, N, H, dt)
    again = ops.attention_bwd(r["qkv"], r["out"], r["do"], r["lse"], B, N, H, 64, SCALE)
    assert torch.equal(again, r["dqkv"])
    out2, lse2 = ops.attention(r["qkv"], B, N, H, 64, SCALE, want_lse=True)
    assert torch.equal(out2, r["out"]) and torch.equal(lse2, r["lse"])


@pytest.mark.parametrize("dt", DTYPES)
def test_the_256_257_switch_of_kernels(dt):
    """The same random head at N = 256 (whole-in-LDS kernel) and N = 257 (its extra token appended; the two long kernels): both
    inside the bars above -- an off-by-one in tile counts would sit here."""
    g = torch.Generator().manual_seed(256257)
    qkv = (torch.randn(1, 257, 3, 1, 64, generator=g) * 1.2).to(dt)
    do = (torch.randn(1, 257, 64, generator=g) * 0.5).to(dt)
    for N in (256, 257):
        q_n, d_n = qkv[:, :N].contiguous(), do[:, :N].contiguous()
        lse_ref, grad_ref = _f64(q_n, d_n)
        out, lse = ops.attention(q_n.to(DEV), 1, N, 1, 64, SCALE, want_lse=True)
        assert float((lse.cpu().double() - lse_ref).abs().max()) <= LSE_TOL[dt]
        _assert_bwd(ops.attention_bwd(q_n.to(DEV), out, d_n.to(DEV), lse, 1, N, 1, 64, SCALE), grad_ref, dt, f"boundary N {N}")


def _long_nonfinite_cases():
    """The six sites the short kernel is tested at (tests/test_nonfinite_cones.py::_attn_cases), at B 1 / H 2."""
    out = []
    for dt in ("f16", "bf16"):
        for N in (257, 577, 640):
            p = dict(B=1, N=N, H=2, dt=dt)
            t = f"{dt}-N{N}-long"
            out.append(nc.case("attn_bwd", p, "qkv", (0, N - 1, 0, 1, 63), f"{t}-q[last row]"))
            out.append(nc.case("attn_bwd", p, "qkv", (0, 0, 1, 0, 0), f"{t}-k[key 0]"))
            out.append(nc.case("attn_bwd", p, "qkv", (0, N - 1, 1, 0, 7), f"{t}-k[key N-1]"))
            out.append(nc.case("attn_bwd", p, "qkv", (0, N - 1, 2, 1, 5), f"{t}-v[key N-1]"))
            out.append(nc.case("attn_bwd", p, "dout", (0, N - 1, 64 + 3), f"{t}-dout[last row]"))
            out.append(nc.case("attn_bwd", p, "dout", (0, 0, 0), f"{t}-dout[0,0]"))
    return out


LONG_CASES = _long_nonfinite_cases()


@pytest.mark.parametrize("c", LONG_CASES, ids=nc.case_id)
def test_long_backward_containment_and_propagation(c):
    """INTEGRATION.md's non-finite contract for the long kernels, with NO exception: a single poisoned element never empties a whole
    160-key chunk, so the forward's pinned all--inf-chunk behaviour is not in play."""
    assert len(LONG_CASES) == 36
    used = set(gnf._exceptions_used)
    bad = gnf.check_case(c)
    assert gnf._exceptions_used == used, "a long attn_bwd case must not lean on an EXCEPTIONS entry"
    assert not bad, nc.case_id(c) + "\n  " + "\n  ".join(bad)


def _step(model, images, target, backend):
    dense.TRAIN_BACKEND = backend
    try:
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            loss = torch.nn.functional.cross_entropy(model(images).float(), target)
        loss.backward()
        return float(loss), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    finally:
        dense.TRAIN_BACKEND = "own"


def test_vit_large_384_trains_on_the_own_attention_kernels():
    """One training step of moe_large_patch16_384_expert32_top1 (depth 1; N = 577) under fp16 autocast: no fallback warning, loss
    and gradients as on torch's autocast path (the bars of test_training_step_on_own_dense_kernels_matches_torch_autocast_path),
    and no aotriton / vendor attention kernel in the own path's step."""
    torch.manual_seed(0)
    model = sm.create_model("moe_large_patch16_384_expert32_top1", num_classes=64, depth=1).to(DEV).train()
    g = torch.Generator().manual_seed(7)
    images = torch.randn(2, 3, 384, 384, generator=g).to(DEV)
    target = torch.randint(0, 64, (2,), generator=g).to(DEV)
    vit._fallbacks_seen.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error", vit.SlimMoEFallbackWarning)
        l_own, g_own = _step(model, images, target, "own")
    l_ref, g_ref = _step(model, images, target, "torch")
    assert abs(l_own - l_ref) <= 2e-3 * max(1.0, abs(l_ref)), (l_own, l_ref)
    assert set(g_own) == set(g_ref)

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))
    worst = max((rel(g_own[n], g_ref[n]), n) for n in g_ref if float(g_ref[n].abs().max()) > 0)
    print(f"ViT-L/16 @384 depth 1: loss {l_own:.5f} vs {l_ref:.5f}; worst relative L2 gradient difference {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 3e-2, worst
    from torch.profiler import profile, ProfilerActivity
    names = set()
    for _attempt in range(3):      # (the tracer now and then delivers a cycle's runtime-API rows without its kernel rows: ask again)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _step(model, images, target, "own")
            torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}
        if any(not n.startswith("hip") for n in names):
            break
    aotriton = {"bwd_kernel_dk_dv", "bwd_kernel_dq", "bwd_preprocess", "attn_fwd"}           # exact symbol names
    bad = [n for n in names if n in aotriton or ("at::native" in n and "attention" in n.lower()) or "flash" in n.lower()]
    assert not bad, bad
    for own in ("attn_fwd_long_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"):
        assert any(own in n for n in names), (own, names)
