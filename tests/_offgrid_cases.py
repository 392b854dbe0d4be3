"""Shapes off the four ViT widths (d = 192 / 384 / 768 / 1024): case lists, inputs and float64 references shared by
tests/test_gpu_offgrid_shapes.py (which runs the kernels) and tests/test_offgrid_host.py (which checks, without a GPU, every reference
here against an independent formulation and every case list against the form of the kernel it claims to reach).

The constants below restate launch code of csrc/ (named where they stand); test_offgrid_host.py compares them with the sources, so
that an edit of either side has to look at the other."""
import numpy as np
import torch

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
U = 2.0 ** -24              # half an f32 ulp: the relative error of one f32 rounding
EPS = 1e-6                  # nn.LayerNorm(d, eps = 1e-6) of the reference's blocks


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ================================================================================================ 1. generic router (csrc/router.hip)
ROUTER_T = 37                                   # one wave per token, 4 waves per workgroup: nine full workgroups and one wave
ROUTER_WAVES = 4                                # router.hip ROUTER_WAVES
ROUTER_LDS_LIMIT = 64 * 1024                    # router.hip launch_router: weights in LDS iff logit block + weights fit
ROUTER_MAX_D, ROUTER_MAX_E, ROUTER_MAX_K = 2048, 4096, 4
# (d, E, k) of the naive gate
ROUTER_CASES = [(520, 3, 3), (776, 9, 4), (1032, 8, 1), (1280, 33, 2), (1536, 4, 2), (1792, 5, 4), (2048, 7, 2), (2040, 8, 2),
                (64, 257, 4), (192, 16, 2)]
SWITCH_CASES = [(1280, 9), (2048, 7)]           # (d, E) of the switch gate: k = 1, noise, probabilities
NEAR_TIE_CASES = [(520, 3, 3), (776, 9, 4), (1280, 33, 2), (1536, 4, 2), (1792, 5, 4), (2048, 7, 2)]    # one per NCH >= 3


def router_nch(d: int) -> int:
    """router.hip dispatch_nch: the NCH template argument"""
    return (d + 255) // 256


def router_is_generic(d: int, E: int, k: int) -> bool:
    """not a shape of router16.hip shape_ok16 (those never reach router.hip's kernel)"""
    if k > 4:
        return True
    if E <= 8:
        return d not in (192, 384, 768, 1024)
    return not (E <= 32 and d in (768, 1024))


def router_weights_in_lds(d: int, E: int) -> bool:
    """router.hip launch_router's w_lds"""
    epad = (E + 7) & ~7
    logit_bytes = ((ROUTER_WAVES + 1) * epad * 4 + 15) & ~15
    return logit_bytes + epad * d * 4 <= ROUTER_LDS_LIMIT


def router_inputs(d: int, E: int, k: int, dtype=F32):
    g = gen(7 * d + 3 * E + k)
    x = torch.randn(ROUTER_T, d, generator=g).to(dtype)
    wg = torch.randn(E, d, generator=g) * 0.05
    bg = torch.randn(E, generator=g) * 0.1
    return x, wg, bg


def switch_noise(d: int, E: int):
    return torch.rand(ROUTER_T, E, generator=gen(d + E)) * 0.2 + 0.9


def near_tie_inputs(d: int, E: int):
    """Expert E - 1 = expert 0 changed by one ulp in one column of the LAST 256-column chunk; with three experts or more expert
    E - 2 = expert 1 exactly.  The gaps are far below the f32 summation error: only the f64 redo orders them as the oracle does."""
    x, wg, bg = router_inputs(d, E, 1)
    col = d - 3
    wg[E - 1] = wg[0]
    wg[E - 1, col] = torch.nextafter(wg[0, col], torch.tensor(float("inf")))
    if E >= 4:
        wg[E - 2] = wg[1]
    bg = torch.zeros(E)
    return x, wg, bg


def router_logits64(x, wg, bg):
    return x.double() @ wg.double().t() + bg.double()


def f32_ulp(v: torch.Tensor) -> torch.Tensor:
    """the spacing of f32 numbers at |v| (float64 in, float64 out; normal range)"""
    _, e = torch.frexp(v.abs().double().clamp(min=2.0 ** -126))        # |v| = m 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 24)


def router_logit_bound(x, wg, ref64):
    """router.hip's header: |logit_f32 - exact| <= (n1 + 7) u |x| max_e |w_e| with n1 = 4 ceil(d / 256) fused multiply-adds per
    lane, six butterfly levels and the bias; plus one f32 ulp of the logit for the store.  [T, E], float64."""
    d = x.shape[1]
    row = x.double().norm(dim=1) * wg.double().norm(dim=1).max()
    return (4 * router_nch(d) + 7) * U * row[:, None] + f32_ulp(ref64)


# ================================================================================================ 2. row kernels and reductions
DGRAD_CASES = [(d, E) for d in (1028, 1280, 2048) for E in (8, 16, 33)]
WGRAD_CASES = [(C, E) for C in (100, 1028, 2048) for E in (1, 16)]
ROW_DIMS = (520, 1032, 2048)                    # scatter / combine / rowdot
COMBINE_KS = (1, 3, 8)
LN_DIMS = (8, 100, 260, 516, 772, 1020)         # the two LayerNorm backwards: NJ = ceil(d / 256) = 1, 1, 2, 3, 4, 4
LN_TS = (1, 37)
COMBINE_LN_CASES = [(d, k) for d in (264, 520, 776, 1016) for k in (1, 3, 4)]
COLSUM_CS = (100, 1284)
COLSUM_COUNTS = (37, 0, 100, 1)                 # an empty group and a one-row group
SWITCH_BWD_ES = (257, 1000)
PLAN_NS = (1000, 1025)
PLAN_ES = (1, 63, 64, 65, 257, 1025, 8192)
PLAN_CAPS = (-1, 3)
PLAN_FUSED_E, PLAN_THREADS, PLAN_CH = 64, 256, 1024      # csrc/dispatch.hip


def ln_nj(d: int) -> int:
    """dense_bwd.hip lnb_launch / glnb_launch (wave_row4.h wr4_dispatch_nj): 64 lanes x 4 columns per register chunk"""
    return (d // 4 + 63) // 64


def combine_ln_nj(d: int) -> int:
    """dispatch.hip combine_ln_launch: 64 lanes x 8 columns per register chunk (k = 3 runs the KMAX = 4 instantiation)"""
    return (d + 511) // 512


def gate_dgrad_kernel(E: int) -> str:
    return "regs8" if E <= 8 else ("regs16" if E <= 16 else "any")


def gate_dgrad_trips(d: int) -> int:
    """column trips of gate_dgrad_kernel / per-row trips of gate_dgrad_any_kernel: d / 4 chunks over at most 256 threads"""
    return (d // 4 + 255) // 256


def plan_is_fused(n: int, E: int) -> bool:
    nblk = (n + PLAN_CH - 1) // PLAN_CH
    return n > 0 and E <= PLAN_FUSED_E and nblk * E <= 8192


def plan_ids(n: int, E: int, kind: str) -> np.ndarray:
    rng = np.random.default_rng(n * 31 + E)
    if kind == "last":
        return np.full(n, E - 1, dtype=np.int64)
    idx = rng.integers(0, E, size=n).astype(np.int64)
    idx[rng.random(n) < 0.2] = 0            # an overloaded expert (a capacity of 3 then drops)
    idx[5::97] = -1                         # entries an earlier stage dropped
    return idx


def ln_inputs(T: int, d: int, dyt=F32):
    g = gen(11 * d + T)
    x = torch.randn(T, d, generator=g) * 2 + 0.5
    w, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    dy = (torch.randn(T, d, generator=g) * 0.1).to(dyt)
    dres = torch.randn(T, d, generator=g) * 0.3
    return x, w, b, dy, dres


def _ln_stats(x, dt=torch.float64):
    xd = x.to(dt)
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    return (xd - mean) * rstd, rstd


def _ln_dx(xhat, rstd, dxn, gamma):
    g = dxn * gamma.to(dxn.dtype)
    return rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def ln_bwd_ref(x, w, dy, dres=None):
    """the closed form of dense_bwd.hip's header in float64: dict(dx, dw, db)"""
    xhat, rstd = _ln_stats(x)
    dyd = dy.double()
    dx = _ln_dx(xhat, rstd, dyd, w)
    if dres is not None:
        dx = dx + dres.double()
    return dict(dx=dx, dw=(dyd * xhat).sum(0), db=dyd.sum(0))


GATE_MODES = ("off", "hard", "soft")
GATE_THR = 0.55
# One case cannot meet GLNB_BAR_D4 (relative L2 8e-7) for an arithmetic reason: at d = 772, T = 1 the single row's <g_f, xn> cancels
# (sum |g_f xn| / |<g_f, xn>| = 214; at most 13 in every other T = 1 case; test_offgrid_host.py asserts both), dz is that one number
# times p (1 - p), and dgate_w = dz xn inherits its relative error.  Bar by the measurement rule, 4 x the error of the same
# expressions evaluated by torch in f32 (gate_ln_bwd_ref(dt=torch.float32)) on the same inputs against float64:
#     g_f f32:  kernel (MI355X) dz 1.02e-6, dgate_w 1.06e-6;  f32 torch dz 2.33e-6, dgate_w 2.39e-6;  bars 9.3e-6 / 9.5e-6
# (with g_f rounded to f16 the kernel measures dz 2.13e-7, dgate_w 2.54e-7 and keeps the 8e-7).  hard and soft share |dz|.
GLNB_MEASURED_BARS = {(772, 1, F32): {"dz": 9.3e-6, "dgate_w": 9.5e-6}}


def gate_ln_inputs(T: int, d: int, gdt=F32):
    g = gen(3 * d + T)
    x = torch.randn(T, d, generator=g) * 1.7 + 0.3
    gam, bet = 1.0 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    w, b = torch.randn(d, generator=g) * (0.1 * (192.0 / d) ** 0.5), torch.randn(1, generator=g) * 0.1     # logits of order one at every d
    g_f = (torch.randn(T, d, generator=g) * 0.3).to(gdt)
    g_out = torch.randn(T, d, generator=g) * 0.2
    return x, gam, bet, w, b, g_f, g_out


def gate_ln_bwd_ref(x, gam, bet, w, b, g_f, g_out, mode: str, dt=torch.float64, mask=None):
    """dense_bwd.hip gate_ln_bwd_kernel's stated formulas in float64.  dict(dx, dgamma, dbeta, dgate_w, dgate_b, dz, mask) with
    mask [T, 2] f32 = what the forward hands the kernel: (skip, keep) decisions (hard), (1 - p, p) (soft), None (off).
    ``dt`` = torch.float32 with the float64 run's ``mask``: the same expressions evaluated by torch in f32 (keep = mask[:, 1], as
    the kernel takes it) -- the emulation that the measurement rule of a bar refers to."""
    xhat, rstd = _ln_stats(x, dt)
    xn = xhat * gam.to(dt) + bet.to(dt)
    T = x.shape[0]
    z = xn @ w.to(dt) + b.to(dt)
    p = torch.sigmoid(z)
    dot = (g_f.to(dt) * xn).sum(-1)
    if mode == "off":
        keep, dz = torch.ones(T, dtype=dt), torch.zeros(T, dtype=dt)
    elif mode == "hard":
        keep = (p <= GATE_THR).to(dt) if mask is None else mask[:, 1].to(dt)
        dz = -dot * p * (1 - p)
        mask = torch.stack((1 - keep, keep), dim=1).float() if mask is None else mask
    else:
        keep = p if mask is None else mask[:, 1].to(dt)
        dz = dot * p * (1 - p)
        mask = torch.stack((torch.sigmoid(-z), p), dim=1).float() if mask is None else mask
    dxn = g_f.to(dt) * keep[:, None] + g_out.to(dt) + dz[:, None] * w.to(dt)[None]
    return dict(dx=_ln_dx(xhat, rstd, dxn, gam), dgamma=(dxn * xhat).sum(0), dbeta=dxn.sum(0), dgate_w=(dz[:, None] * xn).sum(0),
                dgate_b=dz.sum().reshape(1), dz=dz, mask=mask)


def combine_inputs(T: int, k: int, d: int, ydt, rdt, seed: int = 0):
    g = gen(T * 10 + k + d + seed)
    n_y = T * k + 5
    y = torch.randn(n_y, d, generator=g).to(ydt)
    inv = torch.randperm(n_y, generator=g)[:T * k].contiguous()
    inv[2::5] = -1                     # entries a capacity dropped
    score = torch.rand(T * k, generator=g)
    res = torch.randn(T, d, generator=g).to(rdt)
    return y, inv, score, res


def combine_ref(y, inv, score, res, T, k):
    """(out64, S): out[t] = sum_j score[t, j] y[inv[t k + j]] (+ res[t]) and S = the sum of the terms' magnitudes"""
    d = y.shape[1]
    yy = torch.where((inv >= 0)[:, None], y.double()[inv.clamp(min=0)], torch.zeros((), dtype=torch.float64))
    terms = (score.double()[:, None] * yy).reshape(T, k, d)
    out, mag = terms.sum(1), terms.abs().sum(1)
    if res is not None:
        out, mag = out + res.double(), mag + res.double().abs()
    return out, mag


def rowdot_inputs(n: int, k: int, d: int, ddt, ydt):
    T = (n + k - 1) // k
    g = gen(n + d)
    dout = torch.randn(T, d, generator=g).to(ddt)
    y = torch.randn(n + 9, d, generator=g).to(ydt)
    inv = torch.randperm(n + 9, generator=g)[:n].contiguous()
    inv[1::6] = -1
    return dout, y, inv


def rowdot_ref(dout, y, inv, k):
    """(ref64 [n], S [n] = sum |a b|): dscore[i] = <dout[i // k], y[inv[i]]>, 0 for dropped entries"""
    n = inv.numel()
    prod = dout.double()[torch.arange(n) // k] * y.double()[inv.clamp(min=0)]
    live = inv >= 0
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(live, prod.sum(-1), zero), torch.where(live, prod.abs().sum(-1), zero)


def rowdot_fmas(d: int) -> float:
    """a lane's chain: d / 64 fused multiply-adds, then six butterfly levels"""
    return d / 64 + 6


def switch_bwd_inputs(T: int, E: int):
    g = gen(T * 31 + E)
    logits = torch.randn(T, E, generator=g) * 2
    idx = torch.randint(0, E, (T,), generator=g)
    idx[::9] = -1
    return logits, idx, torch.randn(T, generator=g), torch.randn(E, generator=g) * 0.1


def switch_bwd_ref(logits, idx, dscore, coef):
    """softmax backward of g[t, e] = coef[e] + (e == idx[t]) dscore[t], closed form: p (g - <g, p>)"""
    p = torch.softmax(logits.double(), -1)
    g = coef.double()[None].expand_as(p).clone()
    sel = idx >= 0
    g[sel, idx[sel]] += dscore.double()[sel]
    return p * (g - (g * p).sum(-1, keepdim=True))


# ================================================================================================ 3. grouped GEMM, f32 operands
GEMM_COUNTS = (5, 0, 130, 1)
GEMM_KS = (32, 96, 160)
GEMM_NS = (8, 72, 136)
GEMM_PAD = 7                                    # rows past offsets[E] that must keep their sentinel
GEMM_TOL = 2e-5                                 # test_grouped_gemm_matches_fp64_reference, f32 operands


def gemm_inputs(K: int, N: int):
    E, M = len(GEMM_COUNTS), sum(GEMM_COUNTS)
    g = gen(M + K + N)
    A = torch.randn(M + GEMM_PAD, K, generator=g)
    W = torch.randn(E, N, K, generator=g) * 0.05
    bias = torch.randn(E, N, generator=g) * 0.1
    offsets = np.concatenate([[0], np.cumsum(GEMM_COUNTS)]).astype(np.int32)
    return A, W, bias, offsets


def gemm_ref(A, W, bias, offsets, gelu: bool):
    """written row by row with einsum on purpose: test_offgrid_host.py checks it against the per-expert matmul form"""
    M = int(offsets[-1])
    expert = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    v = torch.einsum("mk,mnk->mn", A[:M].double(), W.double()[expert])
    if bias is not None:
        v = v + bias.double()[expert]
    return torch.nn.functional.gelu(v) if gelu else v


# ================================================================================================ 4. the layer
LAYER_T = 150
LAYER_CASES = [(256, 512, 3, 3), (320, 1280, 9, 4), (576, 1152, 17, 1), (1280, 128, 33, 2), (2048, 64, 9, 2)]      # (d, h, E, k), naive gate
LAYER_SWITCH = (1280, 128, 8, 1)                # switch gate, capacity factor 1.0, switch_eps = 0
LAYER_F32 = (96, 160, 4, 2)                     # f32 compute: GEMMs at K = 96 and K = 160 (section 3)
GATE_WGRAD_MAX_E = 16                           # autograd._GateLogits.backward: own gate_wgrad kernel up to here, torch above


def layer_params(T, d, h, E, seed, skew=False):
    """tests/test_gpu_backward._params, draw for draw (that module needs a GPU to import)"""
    g = gen(seed)
    x = torch.randn(T, d, generator=g)
    wg = torch.randn(E, d, generator=g) * 0.05
    bg = torch.zeros(E)
    if skew:
        bg[0] = 1.0
    w1 = torch.randn(E, h, d, generator=g) * 0.05
    b1 = torch.randn(E, h, generator=g) * 0.05
    w2 = torch.randn(E, d, h, generator=g) * 0.05
    b2 = torch.randn(E, d, generator=g) * 0.05
    gout = torch.randn(T, d, generator=g)
    return x, wg, bg, w1, b1, w2, b2, gout


# ================================================================================================ 5. one block through the Python seams
# VisionTransformer(img_size=64, depth=1, num_classes=10, **kwargs) patched with patch_blocks_with_moe(E = 4, k = 2), and the pieces
# that announce a torch / vendor kernel (the `what` of vit._warn_fallback) over an eval pass and a training step under fp16 autocast.
#   a  d = 256: off ops.LN_DIMS -- the patch embedding's fused tail says so; the LayerNorms take nn.LayerNorm without a warning of
#      their own (dense.layer_norm_supported has no loud side); head dim 64 and every K % 64 == 0: own attention and linears
#   b  d = 192 with 6 heads: head dim 32 is not the attention kernels' (eval and training each say so); everything else is own
#   c  d = 320, 8 x 8 patches (65 tokens, K = 192 for the patch GEMM): as a
BLOCK_IMG = 64
BLOCK_CONFIGS = {
    "a": (dict(embed_dim=256, num_heads=4, patch_size=16), ("patch embedding",)),
    "b": (dict(embed_dim=192, num_heads=6, patch_size=16), ("attention", "attention (training)")),
    "c": (dict(embed_dim=320, num_heads=5, patch_size=8), ("patch embedding",)),
}


# ================================================================================================ 6. refusals (no launch)
ROWS_REFUSAL = 64    # token rows of the layer calls that must be refused, and of the good call behind them
FAKE = 4096          # a non-null pointer that is never dereferenced: every call below must be refused by its argument checks


def refusal_calls(lib):
    """[(label, thunk -> return code, words the error message must carry)] through the C ABI as ops.py calls it"""
    f = FAKE

    def router(d, E, k):
        return lambda: lib.smoe_router_topk(f, 0, f, f, None, 1, d, E, k, 0, f, f, None, None, f, 1 << 20, None)

    def gemm(dtype_code, K):
        return lambda: lib.smoe_grouped_gemm(f, f, None, f, None, 1, 1, 16, K, 64, dtype_code, 0, None, None, None, None, 1, f, 16,
                                             0, 0, None, None)

    def combine(k):
        return lambda: lib.smoe_gather_combine(f, 1, f, f, 4, k, 64, None, f, 0, None)

    def combine_ln(d, k):
        return lambda: lib.smoe_gather_combine_ln(f, 1, f, f, 4, k, d, None, f, f, f, 1e-6, f, 1, None)

    return [
        ("router d=2056", router(2056, 4, 1), (b"smoe_router_topk", b"d=2056", b"<= 2048")),
        ("router d=20", router(20, 4, 1), (b"smoe_router_topk", b"d=20", b"multiple of 8")),
        ("router k=5", router(64, 8, 5), (b"smoe_router_topk", b"k=5", b"max 4")),
        ("router E=4097", router(64, 4097, 1), (b"smoe_router_topk", b"E=4097")),
        ("gemm f16 K=200", gemm(1, 200), (b"smoe_grouped_gemm", b"K=200", b"multiple of 64")),
        ("gemm f32 K=48", gemm(0, 48), (b"smoe_grouped_gemm", b"K=48", b"multiple of 32")),
        ("combine k=9", combine(9), (b"smoe_gather_combine", b"k=9")),
        ("combine_ln d=1032", combine_ln(1032, 1), (b"smoe_gather_combine_ln", b"d=1032")),
        ("combine_ln k=5", combine_ln(64, 5), (b"smoe_gather_combine_ln", b"k=5")),
        ("layernorm_bwd d=1028", lambda: lib.smoe_layernorm_bwd(f, f, 0, f, None, 1e-6, 4, 1028, f, f, f, 1 << 30, None),
         (b"smoe_layernorm_bwd", b"d=1028", b"<= 1024")),
        ("switch_aux E=257", lambda: lib.smoe_switch_aux(f, f, 4, 257, f, f, f, 1 << 30, None), (b"smoe_switch_aux", b"E=257", b"256")),
        ("dispatch_plan E=8193", lambda: lib.smoe_dispatch_plan(f, 16, 8193, -1, f, f, f, f, None, f, 1 << 30, None),
         (b"smoe_dispatch_plan", b"E=8193", b"8192")),
    ]
