"""inf / NaN containment and propagation across the training kernels (the loss scaler's safety chain).

THE NON-FINITE CONTRACT OF THE LIBRARY, as pinned here:
  * Containment.  A non-finite input element changes only the output elements that depend on it in exact arithmetic (its
    dependency cone: a GEMM row, an expert's rows x one column for a weight element, one (image, head) for a key, one expert's
    row / column of a weight gradient).  Everything else is bit-identical to a run with a finite value in its place: masked
    lanes (tile rows past a group, duplicated attention keys >= N, rows past offsets[E], gaps of separate row ranges) are
    selected away, never multiplied away.
  * Propagation.  Wherever the float64 result of the operation is non-finite, the kernel's output is non-finite (inf and NaN may
    swap).  Where float64 is finite inside the cone (a -inf score whose probability is 0) the kernel meets its ordinary bar, or
    the case is listed in EXCEPTIONS, which holds only the conservative direction (kernel non-finite, float64 finite).
  * 16-bit stores.  An f32 value beyond the largest finite f16 / bf16 value is stored as inf of its sign, never as the largest
    finite value; every NaN (quiet or signalling, either sign, any payload) is stored as a NaN.
  * GELU.  gelu(+inf) = +inf, gelu(-inf) = NaN (as erf-GELU in float64: -inf * 0), gelu(NaN) = NaN, and the saturated sides are
    exact for every finite input up to +-3e38; gelu'(+-inf) = NaN.
  * The scaler.  smoe_grad_sumsq[_multi] raises found_inf for ONE non-finite element anywhere (vector path, scalar tail, any
    tensor of the table, f32 / f16 / bf16, or finite until multiplied by inv_scale); with found_inf set the AdamW kernels, the
    step counter and the 16-bit weight images are untouched bit for bit and smoe_amp_update backs the scale off.

Covered: grouped GEMM (variants 0, 4, 9, 10, 13, 14; every epilogue; row map / scale / residual / gathered rows / separate row
ranges), gelu_keep, the weight-gradient kernels (every row-piece count, K-major form), group_colsum, rowdot, attention forward
(short and long kernel) and backward (eight and four waves), LayerNorm forward (both layouts) and backward, the elementwise 16-bit
stores, the GELU forms, grad_sumsq / AdamW / amp_update.  NOT covered yet: the routers, the dispatch plan and the rest of the
operator on NaN rows (no statement is made here about what a NaN row routes to), the skip-gate and gate kernels, gather-combine(+LN),
the embedding stage, switch_aux / zero_group_fold, the dense.LinearFn face, and the end-to-end loss-scale walk through train_one_epoch.

The cases, float64 references and cones live in tests/test_nonfinite_cones.py, which checks them against each other on the CPU.
Each case runs the kernel on the poisoned input (+inf, -inf, NaN) and on two finite stand-ins."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import slim_switch_moe_vit_amd as sm  # noqa: E402,F401
from slim_switch_moe_vit_amd import _lib, ops, optim  # noqa: E402
import test_nonfinite_cones as nc  # noqa: E402

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32

# (family, substring of the case tag, poison) -> why the kernel is non-finite where float64 is finite.  Conservative direction only.
EXCEPTIONS = [
    # observed on an MI355X at N = 257 / 577 / 640, f16 and bf16: -inf in column 11 of keys 0..159 for the queries with q[11] > 0 ...
    ("attn_fwd", "k[first chunk,col 11]", "-inf",
     "slim-switch-moe-vit_amd/csrc/attention.hip:104-105: when every score of the first 160-key chunk is -inf the running maximum "
     "stays -inf and the rescale factor exp2((-inf) - (-inf)) is NaN; float64 softmax gives those keys probability 0"),
    # ... and +inf there for the queries with q[11] < 0 (their scores are -inf as well)
    ("attn_fwd", "k[first chunk,col 11]", "+inf",
     "slim-switch-moe-vit_amd/csrc/attention.hip:104-105: the same all -inf first chunk, reached through (+inf) x (a negative q[11])"),
]
_exceptions_used = set()
_cases_run = [0]


def _exception_for(c, poison):
    for i, (fam, sub, pz, _) in enumerate(EXCEPTIONS):
        if fam == c.fam and sub in c.tag and pz == poison:
            _exceptions_used.add(i)
            return True
    return False


# ---------------------------------------------------------------------------------------------------------------- runners
def _dev(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


def run_gemm(inp, p):
    d = _dev(inp)
    out = nc.Gemm.out_init(inp, p).to(DEV)
    mode = p.get("mode", "plain")
    epi = {"none": ops.EPI_NONE, "gelu": ops.EPI_GELU, "gelu_grad": ops.EPI_GELU_GRAD}[p.get("epi", "none")]
    residual = None
    if epi == ops.EPI_GELU_GRAD:
        residual = d["H"]
    elif "residual" in d:
        residual = out if mode.endswith("inplace") else d["residual"]
    offsets, group_end = d["offsets"], None
    if "group_end" in d:
        offsets, group_end = d["offsets"][:-1].contiguous(), d["group_end"]
    ops.grouped_gemm(d["A"], d["W"], d["bias"], offsets, epi, out=out, variant=p["variant"], row_map=d.get("row_map"),
                     row_scale=d.get("row_scale"), residual=residual, a_gather=d.get("a_gather"), a_div=2 if "a_gather" in d else 1,
                     group_end=group_end)
    return {"out": out.cpu()}


def run_gelu_keep(inp, p):
    d = _dev(inp)
    M = int(inp["offsets"][-1])
    pre, out = ops.grouped_gemm_gelu_keep(d["A"], d["W"], d["bias"], d["offsets"])
    pre[M:] = 7.0       # the wrapper allocates both outputs: rows past offsets[E] are nobody's
    out[M:] = 7.0
    return {"pre": pre.cpu(), "out": out.cpu()}


def run_wgrad(inp, p):
    d = _dev(inp)
    if p.get("kmajor"):
        E = d["offsets"].numel() - 1
        offs_pad = ops.pad_offsets(d["offsets"])
        Lp = ops.padded_len(d["P"].shape[0], E)
        return {"out": ops.grouped_wgrad(ops.transpose_pad(d["P"], d["offsets"], offs_pad, Lp),
                                         ops.transpose_pad(d["Q"], d["offsets"], offs_pad, Lp), offs_pad).cpu()}
    return {"out": ops.grouped_wgrad_rows_split(d["P"], d["Q"], d["offsets"], p["S"]).cpu()}


def run_colsum(inp, p):
    d = _dev(inp)
    return {"out": ops.group_colsum(d["src"], d["offsets"]).cpu()}


def run_attn_fwd(inp, p):
    got = ops.attention(inp["qkv"].to(DEV), p["B"], p["N"], p["H"], 64, nc.AttnFwd.scale, want_lse=bool(p.get("lse")))
    return {"out": got[0].cpu(), "lse": got[1].cpu()} if p.get("lse") else {"out": got.cpu()}


def run_attn_bwd(inp, p):
    qkv = inp["qkv"].to(DEV)
    out, lse = ops.attention(qkv, p["B"], p["N"], p["H"], 64, nc.AttnFwd.scale, want_lse=True)
    return {"dqkv": ops.attention_bwd(qkv, out, inp["dout"].to(DEV), lse, p["B"], p["N"], p["H"], 64, nc.AttnFwd.scale).cpu()}


def run_ln_fwd(inp, p):
    return {"y": ops.layernorm(inp["x"].to(DEV), inp["w"].to(DEV), inp["b"].to(DEV), 1e-6, nc.DT[p["od"]]).cpu()}


def run_ln_bwd(inp, p):
    dx, dw, db = ops.layernorm_bwd(inp["x"].to(DEV), inp["dy"].to(DEV), inp["w"].to(DEV), 1e-6)
    return {"dx": dx.cpu(), "dw": dw.cpu(), "db": db.cpu()}


def run_rowdot(inp, p):
    return {"dscore": ops.rowdot(inp["dout"].to(DEV), inp["y"].to(DEV), inp["inv_pos"].to(DEV), nc.Rowdot.K_TOP).cpu()}


RUNNERS = {"rowdot": run_rowdot, "ln_fwd": run_ln_fwd, "ln_bwd": run_ln_bwd, "gemm": run_gemm, "gelu_keep": run_gelu_keep, "wgrad": run_wgrad, "colsum": run_colsum, "attn_fwd": run_attn_fwd,
           "attn_bwd": run_attn_bwd}


# ---------------------------------------------------------------------------------------------------------------- bars
# the bars of the kernels' own finite tests, applied to the elements whose float64 reference is finite
def _max_abs_bar(got, ref, fin, tol, what):
    if not fin.any():
        return []
    g, r = got.double()[fin], ref.double()[fin]
    scale = max(1.0, float(r.abs().max()))
    err = float((g - r).abs().max())
    return [] if err <= tol * scale else [f"{what}: max |got - f64| = {err:.3e} > {tol:g} x {scale:.3g} on the finite elements"]


def bar_gemm(c, k, got, ref, fin):
    """tests/test_gpu_parity.py::test_grouped_gemm_matches_fp64_reference: (operand dtype, tol) = f32 2e-5, f16 1e-3, bf16 8e-3"""
    return _max_abs_bar(got, ref, fin, {"f32": 2e-5, "f16": 1e-3, "bf16": 8e-3}[c.p["cd"]], k)


def bar_wgrad(c, k, got, ref, fin):
    """tests/test_gpu_backward.py::test_grouped_wgrad_rows_tail_rows_never_meet_foreign_bytes: 2e-3 (f16); bf16 at 8 x (_mp.dtype_factor)"""
    return _max_abs_bar(got, ref, fin, 2e-3 if c.p["cd"] == "f16" else 1.6e-2, k)


def bar_colsum(c, k, got, ref, fin):
    """tests/test_gpu_backward.py::test_group_colsum_many_chunks_and_empty_groups: f16 2e-3, bf16 2e-2"""
    return _max_abs_bar(got, ref, fin, 2e-3 if c.p["cd"] == "f16" else 2e-2, k)


def bar_attn_fwd(c, k, got, ref, fin):
    """tests/test_gpu_parity.py::test_attention_kernel_matches_reference_attention: f16 2e-3, bf16 1.5e-2 (x max(1, max |ref|));
    lse as tests/test_gpu_dense.py::test_attention_backward_matches_float64_autograd: 2e-3 / 2e-2 absolute"""
    f16 = c.p["dt"] == "f16"
    if k == "lse":
        err = float((got.double()[fin] - ref.double()[fin]).abs().max()) if fin.any() else 0.0
        return [] if err <= (2e-3 if f16 else 2e-2) else [f"lse: max |got - f64| = {err:.3e}"]
    return _max_abs_bar(got, ref, fin, 2e-3 if f16 else 1.5e-2, k)


def bar_attn_bwd(c, k, got, ref, fin):
    """tests/test_gpu_dense.py::test_attention_backward_matches_float64_autograd, per q / k / v: relative L2 <= tol and
    max |diff| <= 5 tol max |ref|, tol = 4e-3 (f16) / 2e-2 (bf16)"""
    tol = 4e-3 if c.p["dt"] == "f16" else 2e-2
    bad = []
    for i, nm in enumerate("qkv"):
        f = fin[:, :, i]
        if not f.any():
            continue
        g, r = got[:, :, i].double()[f], ref[:, :, i].double()[f]
        rel = float((g - r).norm() / r.norm().clamp(min=1e-30))
        mx = float((g - r).abs().max())
        if rel > tol or mx > 5 * tol * float(r.abs().max()):
            bad.append(f"d{nm}: rel L2 {rel:.3e}, max |diff| {mx:.3e} (tol {tol:g}, max |ref| {float(r.abs().max()):.3g}) on the finite elements")
    return bad


def bar_ln_fwd(c, k, got, ref, fin):
    """tests/test_gpu_parity.py::test_layernorm_kernel_matches_reference_layernorm: 2e-6 (f32 out) / 2e-3 (f16 out) x max(1, max |ref|);
    bf16 out at 8 x the f16 bar (_mp.dtype_factor)"""
    return _max_abs_bar(got, ref, fin, {"f32": 2e-6, "f16": 2e-3, "bf16": 1.6e-2}[c.p["od"]], k)


def bar_ln_bwd(c, k, got, ref, fin):
    """tests/test_gpu_dense.py::test_layernorm_backward_matches_float64_autograd: relative L2 <= 2e-6 for dx, dw and db"""
    if not fin.any():
        return []
    g, r = got.double()[fin], ref.double()[fin]
    rel = float((g - r).norm() / r.norm().clamp(min=1e-30))
    return [] if rel <= 2e-6 else [f"{k}: relative L2 {rel:.3e} > 2e-6 on the finite elements"]


def bar_rowdot(c, k, got, ref, fin):
    """No test of its own in the suite; from the arithmetic: exact 16-bit products summed in f32 by at most 16 FMAs per lane (d <= 1024)
    and 6 cross-lane adds, so |error| <= 22 x 2^-24 x sum |dout| |y| per entry (the standard bound of a 22-term f32 sum)."""
    if not fin.any():
        return []
    inp = nc.inputs_of(c)
    inv = inp["inv_pos"]
    mag = (inp["dout"].double()[torch.arange(inv.numel()) // nc.Rowdot.K_TOP].abs() * inp["y"].double()[inv.clamp(min=0)].abs()).sum(-1)
    mag = torch.nan_to_num(mag, nan=0.0, posinf=0.0)       # entries of the poisoned row are not finite in the reference anyway
    over = ((got.double() - ref.double()).abs() > 22 * 2.0 ** -24 * 1.01 * mag + 1e-30) & fin
    return [f"{k}: {int(over.sum())} entries beyond 22 x 2^-24 x sum |dout| |y|"] if over.any() else []


BARS = {"rowdot": bar_rowdot, "ln_fwd": bar_ln_fwd, "ln_bwd": bar_ln_bwd, "gemm": bar_gemm, "gelu_keep": bar_gemm, "wgrad": bar_wgrad, "colsum": bar_colsum, "attn_fwd": bar_attn_fwd, "attn_bwd": bar_attn_bwd}


# ---------------------------------------------------------------------------------------------------------------- one case
def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_case(c, runner=None):
    """Both properties for one table row; returns the list of violations (empty = pass)."""
    runner = runner or RUNNERS[c.fam]
    F = nc.FAMILIES[c.fam]
    inp = nc.inputs_of(c)
    cone, dts = F.cone(inp, c.p, c.target, c.where), F.out_dtypes(c.p)
    dt_in = inp[c.target].dtype
    subs = [runner(nc.put(inp, c.target, c.where, s), c.p) for s in nc.SUBS]
    bad = []
    for k, m in cone.items():       # the two finite runs agree outside the cone, and are finite
        if not torch.equal(_bits(subs[0][k])[~m], _bits(subs[1][k])[~m]):
            bad.append(f"{k}: the two FINITE stand-ins differ outside the cone in {int((_bits(subs[0][k]) != _bits(subs[1][k]))[~m].sum())} elements")
        if not torch.isfinite(subs[0][k].float()).all():
            bad.append(f"{k}: non-finite output for an all-finite input")
    for name in nc.POISONS:
        pin = nc.put(inp, c.target, c.where, nc.poison_value(name, dt_in))
        got = runner(pin, c.p)
        ref = F.ref(pin, c.p)
        for k, m in cone.items():
            g = got[k]
            assert g.dtype == dts[k] and g.shape == m.shape, (k, g.dtype, g.shape)
            leak = (_bits(g) != _bits(subs[0][k])) & ~m
            if leak.any():
                at = leak.nonzero()[0].tolist()
                bad.append(f"{name} {k}: {int(leak.sum())} elements OUTSIDE the cone changed, first at {at}: "
                           f"{subs[0][k][tuple(at)].item()} -> {g[tuple(at)].item()}")
            r = nc.cast_like(ref[k], dts[k])
            ref_bad, got_bad = ~torch.isfinite(r.float()), ~torch.isfinite(g.float())
            swallowed = ref_bad & ~got_bad
            if swallowed.any():
                at = swallowed.nonzero()[0].tolist()
                bad.append(f"{name} {k}: {int(swallowed.sum())} of {int(ref_bad.sum())} non-finite reference elements are FINITE on the "
                           f"device, first at {at}: f64 {ref[k][tuple(at)].item()} -> {g[tuple(at)].item()}")
            spurious = got_bad & ~ref_bad
            if spurious.any() and not _exception_for(c, name):
                at = spurious.nonzero()[0].tolist()
                bad.append(f"{name} {k}: {int(spurious.sum())} elements are non-finite on the device where float64 is finite (no entry "
                           f"in EXCEPTIONS), first at {at}: f64 {ref[k][tuple(at)].item()} -> {g[tuple(at)].item()}")
            bad += [f"{name} " + s for s in BARS[c.fam](c, k, g, r, ~ref_bad & ~got_bad)]
    return bad


IN_PROCESS = [c for c in nc.CASES if c.p.get("waves", 8) == 8]
FOUR_WAVES = [c for c in nc.CASES if c.p.get("waves") == 4]


@pytest.mark.parametrize("c", IN_PROCESS, ids=nc.case_id)
def test_containment_and_propagation(c):
    bad = check_case(c)
    _cases_run[0] += 1
    assert not bad, nc.case_id(c) + "\n  " + "\n  ".join(bad)


def _four_wave_worker(q):
    os.environ["SMOE_ATTN_BWD_WAVES"] = "4"     # read once per process (csrc/attention_bwd.hip)
    out = {}
    for c in FOUR_WAVES:
        bad = check_case(c)
        if bad:
            out[nc.case_id(c)] = bad
    q.put((out, sorted(_exceptions_used)))


def test_attention_backward_four_wave_form_in_a_child_process():
    """The attn_bwd cases marked waves=4 under SMOE_ATTN_BWD_WAVES=4 (an existing switch, read once per process)."""
    import torch.multiprocessing as mp
    from _mp import join_or_kill
    assert len(FOUR_WAVES) >= 12
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_four_wave_worker, args=(q,))
    p.start()
    got = None
    try:
        got, used = q.get(timeout=600)
    finally:
        join_or_kill([p], 60)
    _exceptions_used.update(used)
    assert not got, "\n".join(f"{k}\n  " + "\n  ".join(v) for k, v in got.items())


# ---------------------------------------------------------------------------------------------------------------- 16-bit stores
def _tile(vec, shape):
    n = 1
    for s in shape:
        n *= s
    return vec.repeat(-(-n // vec.numel()))[:n].reshape(shape).contiguous()


@pytest.mark.parametrize("dt", [F16, BF16])
def test_elementwise_16_bit_stores_keep_inf_and_nan(dt):
    """smoe_cast, smoe_transpose_cast, smoe_scatter_rows (plain and with the combine's scale), smoe_gate_dgrad: f32 -> 16 bit."""
    v = nc.store_vector(dt)
    x = _tile(v, (200, 72))
    nc.check_store(ops.cast(x.to(DEV), dt).cpu(), x.double(), dt, "smoe_cast")
    x1 = _tile(v, (v.numel() * 3 + 5,))                 # a length that is neither a multiple of 8 nor of 4
    nc.check_store(ops.cast(x1.to(DEV), dt).cpu(), x1.double(), dt, "smoe_cast (odd length)")
    x3 = _tile(v, (2, 64, 128))
    nc.check_store(ops.transpose_cast(x3.to(DEV), dt).cpu(), x3.transpose(1, 2).double(), dt, "smoe_transpose_cast")
    pos = torch.randperm(200, generator=nc.gen(1)).to(DEV)
    nc.check_store(ops.scatter_rows(x.to(DEV), pos, 1, dt).cpu(), x[pos.cpu()].double(), dt, "smoe_scatter_rows")
    # with a scale the product is formed in f32: a finite 0.25 * max times 16 overflows the format
    m = nc.FMAX[dt]
    y = _tile(torch.tensor([0.25 * m, -0.25 * m, 1.0, -2.0, 0.0]), (200, 72))
    sc = torch.full((200,), 16.0)
    if dt == F16:
        nc.check_store(ops.scatter_rows(y.to(DEV), pos, 1, dt, scale=sc.to(DEV)).cpu(), (y[pos.cpu()] * 16.0).double(), dt,
                       "smoe_scatter_rows with scale")
    # gate_dgrad with ONE expert: dx[t] = dl[t, 0] * w[0] exactly, no 0 x inf from another expert's row
    d = 192
    w = _tile(v, (1, d))
    dl = torch.ones(300, 1)
    nc.check_store(ops.gate_dgrad(dl.to(DEV), w.to(DEV), dt).cpu(), dl.double() @ w.double(), dt, "smoe_gate_dgrad")


GEMM_STORE_VARIANTS = (0, 4, 9, 10, 13, 14)


@pytest.mark.parametrize("variant", GEMM_STORE_VARIANTS)
@pytest.mark.parametrize("dt", [F16, BF16])
def test_gemm_16_bit_epilogue_stores_keep_inf_and_nan(variant, dt):
    """Every 16-bit epilogue of the grouped GEMM (0 register-staged, 4 / 14 LDS-staged, 9 / 10 / 13 direct store) on EXACT f32
    pre-activations: A = 0, so the value stored is the f32 bias, which carries both sides of the format's range and every NaN class;
    and on exact products (one non-zero product per output) beyond twice the format's range."""
    v = nc.store_vector(dt)
    counts = (330, 1, 0, 70)
    M, K, N, E = sum(counts), 128, 72, len(counts)
    offsets = torch.tensor([0, 330, 331, 331, 401], dtype=torch.int32, device=DEV)
    bias = _tile(v, (E, N))
    A = torch.zeros(M, K, dtype=dt, device=DEV)
    W = torch.ones(E, N, K, dtype=dt, device=DEV)
    ref = torch.cat([bias[e].double().expand(n, N) for e, n in enumerate(counts)])
    got = ops.grouped_gemm(A, W, bias.to(DEV), offsets, ops.EPI_NONE, dt, variant=variant)
    n_inf, n_nan = nc.check_store(got.cpu(), ref, dt, f"variant {variant} EPI_NONE")
    assert n_inf > 0 and n_nan > 0
    if variant:
        pre, act = ops.grouped_gemm_gelu_keep(A, W, bias.to(DEV), offsets)
        nc.check_store(pre.cpu(), ref, dt, "gelu_keep, kept pre-activations")
        nc.check_store(act.cpu(), nc.gelu64(ref), dt, "gelu_keep, activations")
    # residual + row map: the fused add / scale re-round through the same conversions
    # (max + max = twice the range exactly; every term is exact in the format, so the value is rounded once)
    res = _tile(torch.tensor([nc.FMAX[dt], -nc.FMAX[dt], 1.0]), (M, N)).to(dt)
    b2 = _tile(torch.tensor([nc.FMAX[dt], -nc.FMAX[dt], 1.0, float("nan")]), (E, N))
    got = ops.grouped_gemm(A, W, b2.to(DEV), offsets, ops.EPI_NONE, dt, variant=variant, residual=res.to(DEV))
    ref2 = res.double() + torch.cat([b2[e].double().expand(n, N) for e, n in enumerate(counts)])
    nc.check_store(got.cpu(), ref2, dt, f"variant {variant} fused residual")
    # exact products: A[m, m % K] = a, W[e, n, k] = w -> out[m, n] = a w
    a, w = (60000.0, 4.0) if dt == F16 else (3e38, 4.0)
    A2 = torch.zeros(M, K, dtype=dt)
    A2[torch.arange(M), torch.arange(M) % K] = torch.where(torch.arange(M) % 2 == 0, a, -a).to(dt)
    W2 = torch.full((E, N, K), w, dtype=dt)
    ref3 = (A2.double().sum(1, keepdim=True) * w).expand(M, N).float().double()     # as the f32 accumulator holds it (bf16: +-inf)
    for epi, r in ((ops.EPI_NONE, ref3), (ops.EPI_GELU, nc.gelu64(ref3))):
        got = ops.grouped_gemm(A2.to(DEV), W2.to(DEV), None, offsets, epi, dt, variant=variant)
        n_inf, _ = nc.check_store(got.cpu(), r, dt, f"variant {variant} exact products, epilogue {epi}")
        assert n_inf > 0
    # the dgrad epilogue: value * gelu'(H) with H = 4 (gelu' = 1.0005): the product is re-rounded to 16 bit
    H = torch.full((M, N), 4.0, dtype=dt)
    got = ops.grouped_gemm(A2.to(DEV), W2.to(DEV), None, offsets, ops.EPI_GELU_GRAD, dt, variant=variant, residual=H.to(DEV))
    nc.check_store(got.cpu(), ref3 * nc.gelu_grad64(H), dt, f"variant {variant} GELU_GRAD")


@pytest.mark.parametrize("dt", [F16, BF16])
def test_attention_backward_store_overflows_to_inf(dt):
    """dV[key 0] = sum over the N queries of P[q, 0] dO[q] with P[q, 0] ~ 1 and dO = 0.75 max: N x 0.75 max is far beyond the format.
    (The forward's output is a convex combination of V rows and cannot leave the format's range.)"""
    B, N, H = 1, 100, 2
    qkv = torch.zeros(B, N, 3, H, 64)
    u = torch.ones(64) * 0.5
    qkv[:, :, 0] = u
    qkv[:, 0, 1] = 8.0 * u             # score of key 0: 0.125 * 8 * 16 = 16 above every other key
    qkv[:, :, 2] = torch.randn(N, 1, 64, generator=nc.gen(5)) * 0.1
    do = torch.full((B, N, H * 64), 0.75 * nc.FMAX[dt])
    do[:, :, ::2] *= -1.0
    inp = {"qkv": qkv.to(dt), "dout": do.to(dt)}
    p = dict(B=B, N=N, H=H, dt="f16" if dt == F16 else "bf16")
    got = run_attn_bwd(inp, p)["dqkv"]
    ref = nc.AttnBwd.ref(inp, p)["dqkv"]
    n_inf, _ = nc.check_store(got[:, :, 2], ref[:, :, 2], dt, "dv")
    assert n_inf >= 64 * H


@pytest.mark.parametrize("d", [192, 768])
@pytest.mark.parametrize("dt", [F16, BF16])
def test_layernorm_16_bit_store_keeps_inf_and_nan(d, dt):
    """Both LayerNorm layouts (16 lanes per token below d = 768, a wave per row from there): the affine output (x - mean) rstd g + b with
    b beyond twice the format's range in some columns stores +-inf there; a NaN row stores NaN."""
    T = 37
    x = torch.randn(T, d, generator=nc.gen(d))
    big = 4.0 * nc.FMAX[dt] if dt == F16 else float("inf")     # bf16 shares f32's exponent range: no finite f32 lies beyond twice its range
    g = torch.ones(d)
    b = torch.zeros(d)
    b[0::7] = big
    b[3::7] = -big
    x[5, d - 1] = nc.poison_value("nan", F32)
    got = ops.layernorm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-6, dt).cpu()
    ref = torch.nn.functional.layer_norm(x.double(), (d,), g.double(), b.double(), 1e-6)
    n_inf, n_nan = nc.check_store(got, ref, dt, f"smoe_layernorm d={d}")
    assert n_inf > 0 and n_nan >= d
    same = torch.ones(T, dtype=torch.bool)
    same[5] = False
    x2 = x.clone()
    x2[5, d - 1] = 0.5
    got2 = ops.layernorm(x2.to(DEV), g.to(DEV), b.to(DEV), 1e-6, dt).cpu()
    assert torch.equal(_bits(got)[same], _bits(got2)[same]), "a NaN row must not touch another row"


# ---------------------------------------------------------------------------------------------------------------- GELU forms
def _gelu_bar(got, ref64, od, what):
    """f32 outputs: the bar of tests/test_gpu_parity.py::test_grouped_gemm_gelu_epilogue_over_the_whole_input_range (1e-5 + 1e-5 |ref|);
    16-bit outputs: that bar plus one unit in the last place of the format (2^-10 / 2^-7 relative)."""
    r = ref64.to(od)
    ref_bad, got_bad = ~torch.isfinite(r.float()), ~torch.isfinite(got.float())
    assert torch.equal(ref_bad, got_bad), (f"{what}: finite / non-finite pattern differs from float64 at reference values "
                                           f"{ref64[ref_bad != got_bad][:6].tolist()} -> {got[ref_bad != got_bad][:6].tolist()}")
    fin = ~ref_bad
    ulp = {F32: 0.0, F16: 2.0 ** -10, BF16: 2.0 ** -7}[od]
    err = (got.double() - ref64)[fin].abs()
    lim = 1e-5 + (1e-5 + ulp) * ref64[fin].abs()
    assert (err <= lim).all(), f"{what}: {float((err - lim).max()):.3e} over the bar at f64 value {float(ref64[fin][(err - lim).argmax()])}"


_GELU_FORMS = [(0, F32), (0, F16), (4, F16), (4, BF16), (9, F16), (9, BF16), (10, F16), (13, BF16), (14, F16), (14, BF16)]


# a 16-bit output has the operands' dtype
@pytest.mark.parametrize("variant,cd,od", [(v, cd, od) for v, cd in _GELU_FORMS for od in (F32, F16, BF16) if od in (F32, cd)])
def test_gelu_epilogues_from_minus_inf_to_plus_inf(variant, cd, od):
    """GELU and GELU_GRAD epilogues on exact pre-activations 0 .. +-6e4, +-1e6, +-3e38, +-inf, NaN (A = 0: the pre-activation is the f32
    bias): erf form (variant 0), fitted sigmoid form alone and packed (f32 and 16-bit epilogues), against float64 erf-GELU."""
    v = nc.gelu_sweep_values()
    M, K, N = 330, 64 if cd != F32 else 32, 48
    bias = _tile(v, (1, N))
    A = torch.zeros(M, K, dtype=cd, device=DEV)
    W = torch.ones(1, N, K, dtype=cd, device=DEV)
    offsets = torch.tensor([0, M], dtype=torch.int32, device=DEV)
    got = ops.grouped_gemm(A, W, bias.to(DEV), offsets, ops.EPI_GELU, od, variant=variant).cpu()
    _gelu_bar(got, nc.gelu64(bias.double().expand(M, N)), od, f"GELU epilogue variant {variant}")
    if variant and od == cd:
        _, act = ops.grouped_gemm_gelu_keep(A, W, bias.to(DEV), offsets)
        _gelu_bar(act.cpu(), nc.gelu64(bias.double().expand(M, N)), od, "gelu_keep")
    # GELU_GRAD: value = 1 (bias), H = the sweep as the output dtype holds it
    H = _tile(v, (M, N)).to(od)
    one = torch.ones(1, N)
    got = ops.grouped_gemm(A, W, one.to(DEV), offsets, ops.EPI_GELU_GRAD, od, variant=variant, residual=H.to(DEV)).cpu()
    _gelu_bar(got, nc.gelu_grad64(H), od, f"GELU_GRAD epilogue variant {variant}")


@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_gelu_pass_from_minus_inf_to_plus_inf(dt):
    x = _tile(nc.gelu_sweep_values(), (1000,)).to(dt)
    _gelu_bar(ops.gelu(x.to(DEV)).cpu(), nc.gelu64(x), dt, "smoe_gelu")


# ---------------------------------------------------------------------------------------------------------------- the scaler's chain
def _sumsq(g, inv_scale):
    lib = _lib.load()
    n = g.numel()
    nb = lib.smoe_grad_sumsq_blocks(n)
    partial = torch.zeros(nb, device=DEV)
    found = torch.zeros(1, device=DEV)
    inv = torch.tensor([inv_scale], dtype=F32, device=DEV)
    _lib.check(lib.smoe_grad_sumsq(g.data_ptr(), ops.dtype_code(g.dtype), n, inv.data_ptr(), partial.data_ptr(), found.data_ptr(),
                                   ops._stream(g)), "smoe_grad_sumsq")
    return float(found), partial.cpu().double().sum()


def _sumsq_multi(gs, inv_scale):
    lib = _lib.load()
    numels = [g.numel() for g in gs]
    blk, nb = optim._block_table(numels, torch.device(DEV))
    ptrs = [g.data_ptr() for g in gs]
    tab = torch.tensor([ptrs, ptrs, ptrs, ptrs, numels], dtype=torch.int64, device=DEV)
    partial = torch.zeros(sum(nb), device=DEV)
    found = torch.zeros(1, device=DEV)
    inv = torch.tensor([inv_scale], dtype=F32, device=DEV)
    _lib.check(lib.smoe_grad_sumsq_multi(tab.data_ptr(), len(gs), blk.data_ptr(), sum(nb), ops.dtype_code(gs[0].dtype), inv.data_ptr(),
                                         partial.data_ptr(), found.data_ptr(), ops._stream(gs[0])), "smoe_grad_sumsq_multi")
    return float(found), partial.cpu().double().sum()


@pytest.mark.parametrize("gdt", [F32, F16, BF16])
def test_grad_sumsq_raises_found_inf_for_one_element_anywhere(gdt):
    """One inf and, separately, one NaN at element 0, the end of a full 8-vector, a block boundary and EACH slot of the scalar tail;
    the multi-tensor table with the poison in the last element of its last tensor; a value that is finite until multiplied by
    inv_scale.  The clean tensor gives 0 and the float64 sum (the norm bar of test_native_scaler_step_...: 1e-4 relative)."""
    n = nc.SUMSQ_N
    g = (torch.randn(n, generator=nc.gen(11)) * 0.1).to(gdt)
    found, ss = _sumsq(g.to(DEV), 0.5)
    ref = float((g.double() * 0.5).pow(2).sum())
    assert found == 0.0 == nc.found_inf_ref(g, 0.5) and abs(ss - ref) <= 2e-4 * ref
    missed = []
    for pos in nc.sumsq_positions(n):
        for name in ("+inf", "-inf", "nan"):
            g2 = g.clone()
            g2[pos] = nc.poison_value(name, gdt)
            assert nc.found_inf_ref(g2, 0.5) == 1.0
            if _sumsq(g2.to(DEV), 0.5)[0] != 1.0:
                missed.append((pos, name))
    assert not missed, f"found_inf stayed 0 for a poison at (position, value) {missed} of {n} elements"
    # finite until unscaled
    big, inv = (60000.0, 1e35) if gdt == F16 else (1e30, 1e10)
    for pos in (0, n - 1):
        g2 = g.clone()
        g2[pos] = big
        assert _sumsq(g2.to(DEV), 1e-6)[0] == 0.0 == nc.found_inf_ref(g2, 1e-6)
        assert _sumsq(g2.to(DEV), inv)[0] == 1.0 == nc.found_inf_ref(g2, inv), pos
    # the table form: tensors of 5, n, 1 and 40001 elements
    sizes = [5, n, 1, 40001]
    base = [(torch.randn(s, generator=nc.gen(s)) * 0.1).to(gdt) for s in sizes]
    found, ss = _sumsq_multi([t.to(DEV) for t in base], 0.5)
    ref = sum(float((t.double() * 0.5).pow(2).sum()) for t in base)
    assert found == 0.0 and abs(ss - ref) <= 2e-4 * ref
    for ti, pos in ((3, 40000), (3, 39999), (0, 4), (2, 0), (1, n - 1), (1, n - 5), (0, 0)):
        for name in ("+inf", "nan"):
            gs = [t.clone() for t in base]
            gs[ti][pos] = nc.poison_value(name, gdt)
            if _sumsq_multi([t.to(DEV) for t in gs], 0.5)[0] != 1.0:
                missed.append((ti, pos, name))
    assert not missed, f"smoe_grad_sumsq_multi: found_inf stayed 0 for a poison at (tensor, position, value) {missed}"


def _adamw_state(sizes, seed):
    g = nc.gen(seed)
    mk = lambda s: torch.randn(s, generator=g)
    return [dict(p=mk(s), g=mk(s), m=mk(s) * 0.1, v=mk(s).abs() * 0.01) for s in sizes]


def _launch_adamw(st, found, multi, shadows=None, gdt=F32):
    lib = _lib.load()
    step = torch.tensor([3.0], device=DEV)
    _lib.check(lib.smoe_step_advance(step.data_ptr(), found.data_ptr(), None), "smoe_step_advance")
    if not multi:
        for s in st:
            _lib.check(lib.smoe_adamw_step(s["p"].data_ptr(), s["g"].data_ptr(), ops.dtype_code(gdt), s["m"].data_ptr(), s["v"].data_ptr(),
                                           s["p"].numel(), 1e-2, 0.9, 0.999, 1e-8, 0.05, step.data_ptr(), None, found.data_ptr(), None),
                       "smoe_adamw_step")
        return step
    numels = [s["p"].numel() for s in st]
    blk, nb = optim._block_table(numels, torch.device(DEV))
    tab = torch.tensor([[s[k].data_ptr() for s in st] for k in "pgmv"] + [numels], dtype=torch.int64, device=DEV)
    hyp = torch.tensor([[1e-2] * len(st), [0.05] * len(st)], dtype=F32, device=DEV)
    sh = None
    if shadows is not None:
        sh = torch.tensor([[t.data_ptr() for t in shadows], [ops.dtype_code(t.dtype) for t in shadows]], dtype=torch.int64, device=DEV)
    _lib.check(lib.smoe_adamw_step_multi(tab.data_ptr(), hyp.data_ptr(), len(st), blk.data_ptr(), sum(nb), ops.dtype_code(gdt), 0.9, 0.999,
                                         1e-8, step.data_ptr(), None, found.data_ptr(), sh.data_ptr() if sh is not None else None, None),
               "smoe_adamw_step_multi")
    torch.cuda.synchronize()
    return step


@pytest.mark.parametrize("multi", [False, True])
def test_found_inf_leaves_weights_moments_step_and_images_untouched_and_backs_the_scale_off(multi):
    sizes = [nc.SUMSQ_N, 5, 1, 40001, 4096]
    host = _adamw_state(sizes, 21)
    host[0]["g"][nc.SUMSQ_N - 1] = float("inf")
    host[3]["g"][0] = float("nan")
    st = [{k: t.to(DEV) for k, t in s.items()} for s in host]
    shadows = [torch.full((s,), 3.0, dtype=F16 if i % 2 == 0 else BF16, device=DEV) for i, s in enumerate(sizes)] if multi else None
    found = torch.ones(1, device=DEV)
    step = _launch_adamw(st, found, multi, shadows)
    assert float(step) == 3.0, "the step counter must not advance"
    for s, h in zip(st, host):
        for k in "pmv":
            assert torch.equal(_bits(s[k].cpu()), _bits(h[k])), k
    if multi:
        for t in shadows:
            assert bool((t == 3.0).all()), "a 16-bit weight image was written by a skipped step"
    lib = _lib.load()
    scale, tracker = torch.tensor([65536.0], device=DEV), torch.tensor([7.0], device=DEV)
    _lib.check(lib.smoe_amp_update(scale.data_ptr(), tracker.data_ptr(), found.data_ptr(), 2.0, 0.5, 2000, None), "smoe_amp_update")
    assert float(scale) == 32768.0 and float(tracker) == 0.0
    # and the same launch with found_inf = 0 does step (the test above is not vacuous)
    found.zero_()
    step = _launch_adamw(st, found, multi, shadows)
    assert float(step) == 4.0 and not torch.equal(st[1]["p"].cpu(), host[1]["p"])
    assert not torch.isfinite(st[0]["p"][nc.SUMSQ_N - 1]), "an applied non-finite gradient reaches the weight"


def test_adamw_16_bit_weight_images_keep_inf_and_nan():
    """The images the fused step writes (vector path and scalar tail): a weight beyond the f16 range stores inf, a NaN weight of
    any payload stores NaN in both formats."""
    n = 16384 + 8 + 3
    for dt in (F16, BF16):
        host = _adamw_state([n, n], 33)
        v = nc.store_vector(dt)
        for s in host:
            s["p"][:v.numel()] = v
            s["p"][n - v.numel():] = v          # ... and through the scalar tail
            s["g"].zero_()
            s["m"].zero_()
        st = [{k: t.to(DEV) for k, t in s.items()} for s in host]
        shadows = [torch.zeros(n, dtype=dt, device=DEV) for _ in st]
        _launch_adamw(st, torch.zeros(1, device=DEV), True, shadows)
        for s, img in zip(st, shadows):
            p_after = s["p"].cpu()
            assert torch.isnan(p_after[:v.numel()][torch.isnan(v)]).all()
            nc.check_store(img.cpu(), p_after.double(), dt, f"AdamW {dt} image")


# ---------------------------------------------------------------------------------------------------------------- the table, printed
def test_zz_the_exceptions_table_is_short_one_directional_and_printed(capsys):
    with capsys.disabled():
        sys.stdout.write(f"\nEXCEPTIONS ({len(EXCEPTIONS)} entries; kernel non-finite where float64 is finite):\n")
        for i, (fam, sub, pz, why) in enumerate(EXCEPTIONS):
            sys.stdout.write(f"  [{'used' if i in _exceptions_used else 'NOT USED'}] {fam} / {sub} / {pz}: {why}\n")
    assert len(EXCEPTIONS) <= 4
    if _cases_run[0] == len(IN_PROCESS):      # a whole run: an entry that no case needed is stale
        assert _exceptions_used == set(range(len(EXCEPTIONS))), "an EXCEPTIONS entry was not needed by any case"
    for fam, sub, pz, why in EXCEPTIONS:
        assert fam in nc.FAMILIES and pz in nc.POISONS and (".hip:" in why or ".h:" in why)
        assert any(c.fam == fam and sub in c.tag for c in nc.CASES), (fam, sub)
