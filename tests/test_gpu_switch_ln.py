"""GPU tests of SwitchableLayerNorm on its own kernels (smoe_switch_ln_fwd / smoe_switch_ln_bwd) and of SwitchableVisionTransformer:
the kernels over the case table of tests/_switch_ln_cases.py against the float64 restatement, the reference's fixture, guard bands
around caller-owned buffers, the non-finite contract, the module's autograd and launch count, the model against a plain twin, and
evaluate() / train_one_epoch() replayed from HIP graphs."""
import warnings

import pytest
import torch

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib, ops

import _switch_ln_cases as sc
from _switch_ln_cases import FIXTURE_CASES, fixture_case, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELLS = sc.cells()


def _dev(t):
    return t.to(DEV) if isinstance(t, torch.Tensor) else t


def _compose32(c, buckets):
    """The accepted f32 evaluation of a cell: the module's torch composition on the CPU, gradients by autograd."""
    x = c["x"].clone().requires_grad_(True)
    w = c["weights"].clone().requires_grad_(True)
    b = c["biases"].clone().requires_grad_(True)
    y, _ = sm.switch_ln_compose(x, sc.EPS, w, b, c["cent"], buckets, w.shape[0])
    y.backward(c["dy"])
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad}


def _run_kernels(c, buckets, dy=None):
    x = c["x"].to(DEV)
    w, b, cent = c["weights"].to(DEV), c["biases"].to(DEV), c["cent"].to(DEV)
    y, bk = ops.switch_ln(x, w, b, cent, sc.EPS, _dev(buckets))
    dx, dw, db = ops.switch_ln_bwd(x, (c["dy"] if dy is None else dy).to(DEV), w, bk, sc.EPS)
    return x, {"y": y, "b": bk, "dx": dx, "dw": dw, "db": db}


# ------------------------------------------------------------------------------------------------------- kernels over the table
@pytest.mark.parametrize("cell", CELLS, ids=[sc.cell_id(c) for c in CELLS])
def test_kernels_over_the_case_table(cell):
    regime, T, d, K = cell
    c = sc.make_cell(*cell)
    r64 = sc.restate64(c["x"], c["dy"], c["weights"], c["biases"], c["cent"], c["buckets"])
    acc = _compose32(c, c["buckets"])
    x_dev, got = _run_kernels(c, c["buckets"])
    _, again = _run_kernels(c, c["buckets"])
    torch.cuda.synchronize()
    assert torch.equal(x_dev.cpu(), c["x"]), "x was modified"
    assert got["b"].dtype == torch.int64 and torch.equal(got["b"].cpu(), r64["b"]), "buckets differ from the float64 restatement"
    for key in ("y", "dx", "dw", "db"):
        assert torch.equal(got[key], again[key]), f"{key}: two runs differ"
        bound = sc.bar(r64[key], acc[key])
        err = float((got[key].cpu().double() - r64[key]).abs().max())
        print(f"{sc.cell_id(cell)} {key}: err {err:.3e} bar {bound:.3e}")
        assert err <= bound, (cell, key, err, bound)
    empty = torch.bincount(r64["b"], minlength=K) == 0
    if bool(empty.any()):
        assert float(got["dw"].cpu()[empty].abs().max()) == 0.0 and float(got["db"].cpu()[empty].abs().max()) == 0.0
        assert not bool(torch.signbit(got["dw"].cpu()[empty]).any())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_backward_takes_16_bit_dy(dt):
    cell = ("separated", 65, 384, 5)
    c = sc.make_cell(*cell)
    dy16 = c["dy"].to(dt)
    c["dy"] = dy16.float()                    # the same values in f32 for both references
    r64 = sc.restate64(c["x"], c["dy"], c["weights"], c["biases"], c["cent"], None)
    acc = _compose32(c, None)
    _, got = _run_kernels(c, None, dy=dy16)
    for key in ("dx", "dw", "db"):
        assert float((got[key].cpu().double() - r64[key]).abs().max()) <= sc.bar(r64[key], acc[key]), key


def test_no_affine_and_empty_input():
    c = sc.make_cell("separated", 17, 192, 5)
    x = c["x"].to(DEV)
    y, b = ops.switch_ln(x, None, None, c["cent"].to(DEV), sc.EPS)
    r = sc.restate64(c["x"], c["dy"], None, None, c["cent"], None)
    assert torch.equal(b.cpu(), r["b"]) and float((y.cpu().double() - r["y"]).abs().max()) <= 3 * sc.ulp32(r["y"]) + 1e-6
    dx, dw, db = ops.switch_ln_bwd(x, c["dy"].to(DEV), None, b, sc.EPS, num_buckets=5, want_param_grads=False)
    assert dw is None and float((dx.cpu().double() - r["dx"]).abs().max()) <= 1e-5
    e = torch.empty(0, 192, device=DEV)
    w = c["weights"].to(DEV)
    y0, b0 = ops.switch_ln(e, w, c["biases"].to(DEV), c["cent"].to(DEV), sc.EPS)
    assert y0.shape == (0, 192) and b0.shape == (0,)
    dx0, dw0, db0 = ops.switch_ln_bwd(e, e.clone(), w, b0, sc.EPS)
    assert dx0.shape == (0, 192) and float(dw0.abs().max()) == 0.0 and float(db0.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------- fixture
@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


@pytest.mark.parametrize("name,src,mode", FIXTURE_CASES, ids=[c[0] for c in FIXTURE_CASES])
def test_module_on_the_gpu_against_the_fixture(fixture, name, src, mode):
    t, buckets, ref = fixture_case(fixture, name, src, mode)
    K, d = t["weights"].shape
    mod = sm.SwitchableLayerNorm(d, switchable_buckets=K).to(DEV)
    with torch.no_grad():
        mod.weights.copy_(t["weights"])
        mod.biases.copy_(t["biases"])
    mod.set_centroids(t["centroids"])
    x = t["x"].to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", sm.vit.SlimMoEFallbackWarning)
        y, b = mod(x, _dev(buckets))
        y.backward(t["dy"].to(DEV))
    assert torch.equal(b.cpu(), ref["buckets"]) and mod.centroids.grad is None
    r64 = sc.restate64(t["x"].flatten(0, 1), t["dy"].flatten(0, 1), t["weights"], t["biases"], t["centroids"],
                       buckets.flatten() if isinstance(buckets, torch.Tensor) else buckets)
    for got, key, rk in ((y.detach(), "y", "y"), (x.grad, "dx", "dx"), (mod.weights.grad, "dw", "dweights"), (mod.biases.grad, "db", "dbiases")):
        want = r64[key].reshape(got.shape)
        bound = sc.bar(want, ref[rk])
        err = float((got.cpu().double() - want).abs().max())
        print(f"{name} {key}: err {err:.3e} bar {bound:.3e}")
        assert err <= bound, (name, key, err, bound)


# ---------------------------------------------------------------------------------------------------------------- guard bands
GUARD = 64                       # elements on each side
PAYLOAD32 = 0x7FC0BEEF           # a NaN with a payload no kernel produces


def _banded(n, dtype):
    """(whole buffer, the n-element window between two guard bands), every element a payload pattern."""
    if dtype == torch.float32:
        whole = torch.full((n + 2 * GUARD,), PAYLOAD32, dtype=torch.int32, device=DEV).view(torch.float32)
    else:
        whole = torch.full((n + 2 * GUARD,), 0x7EADBEEF12345678, dtype=torch.int64, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _check_band(whole, n, name, inside=True):
    bits = whole.view(torch.int32 if whole.dtype == torch.float32 else torch.int64).cpu()
    pat = PAYLOAD32 if whole.dtype == torch.float32 else 0x7EADBEEF12345678
    assert bool((bits[:GUARD] == pat).all()) and bool((bits[GUARD + n:] == pat).all()), f"{name}: written outside its buffer"
    if inside:
        assert not bool((bits[GUARD:GUARD + n] == pat).any()), f"{name}: elements left unwritten"


@pytest.mark.parametrize("T", [1, 65])
@pytest.mark.parametrize("d,K", [(192, 5), (1024, 32)])
def test_entry_points_write_exactly_their_buffers(T, d, K):
    c = sc.make_cell("separated", T, d, K)
    lib = _lib.load()
    x, w, b, cent, dy = (c[k].to(DEV) for k in ("x", "weights", "biases", "cent", "dy"))
    stream = ops._stream(x)
    y_all, y = _banded(T * d, torch.float32)
    bk_all, bk = _banded(T, torch.int64)
    rc = lib.smoe_switch_ln_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), cent.data_ptr(), None, -1, sc.EPS, T, d, K, y.data_ptr(),
                                bk.data_ptr(), stream)
    _lib.check(rc, "smoe_switch_ln_fwd")
    torch.cuda.synchronize()
    _check_band(y_all, T * d, "y")
    _check_band(bk_all, T, "buckets_out")
    r64 = sc.restate64(c["x"], c["dy"], c["weights"], c["biases"], c["cent"], None)
    assert torch.equal(bk.cpu(), r64["b"])
    dx_all, dx = _banded(T * d, torch.float32)
    dw_all, dw = _banded(K * d, torch.float32)
    db_all, db = _banded(K * d, torch.float32)
    ws_bytes = lib.smoe_switch_ln_bwd_workspace_bytes(T, d, K)
    assert ws_bytes % 4 == 0
    ws_all, ws = _banded(ws_bytes // 4, torch.float32)
    rc = lib.smoe_switch_ln_bwd(x.data_ptr(), dy.data_ptr(), 0, w.data_ptr(), bk.data_ptr(), sc.EPS, T, d, K, dx.data_ptr(), dw.data_ptr(),
                                db.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    _lib.check(rc, "smoe_switch_ln_bwd")
    torch.cuda.synchronize()
    _check_band(dx_all, T * d, "dx")
    _check_band(dw_all, K * d, "dweights")
    _check_band(db_all, K * d, "dbiases")
    _check_band(ws_all, ws_bytes // 4, "workspace", inside=False)
    acc = _compose32(c, None)
    for got, key in ((dx, "dx"), (dw, "dw"), (db, "db")):
        assert float((got.cpu().double().reshape(r64[key].shape) - r64[key]).abs().max()) <= sc.bar(r64[key], acc[key]), key


# ------------------------------------------------------------------------------------------------------- the non-finite contract
def test_non_finite_contract():
    T, d, K = 65, 192, 5
    c = sc.make_cell("separated", T, d, K)
    x, w, b, cent, dy = (c[k].to(DEV) for k in ("x", "weights", "biases", "cent", "dy"))
    y0, b0 = ops.switch_ln(x, w, b, cent, sc.EPS)
    keep = torch.arange(T, device=DEV) != 7
    # a NaN in one row of x: that row is NaN and selects bucket 0 (every distance is NaN: the first NaN wins); no other row moves a bit
    xn = x.clone()
    xn[7, 100] = float("nan")
    y1, b1 = ops.switch_ln(xn, w, b, cent, sc.EPS)
    assert torch.equal(y1[keep], y0[keep]) and torch.equal(b1[keep], b0[keep]) and int(b1[7]) == 0 and bool(y1[7].isnan().all())
    # a NaN centroid k draws every finite row to k (the first such k)
    cn = cent.clone()
    cn[3, 5] = float("nan")
    cn[4, 0] = float("nan")
    assert bool((ops.switch_ln(x, w, b, cn, sc.EPS)[1] == 3).all())
    # K = 1 never reads the centroids
    nan1 = torch.full((1, d), float("nan"), device=DEV)
    y2, b2 = ops.switch_ln(x, w[:1].contiguous(), b[:1].contiguous(), nan1, sc.EPS)
    assert int(b2.abs().sum()) == 0 and bool(torch.isfinite(y2).all())
    assert torch.equal(y2, ops.switch_ln(x, w[:1].contiguous(), b[:1].contiguous(), None, sc.EPS, 0)[0])
    # an out-of-range given bucket (the C entry point: the Python layers refuse it): a NaN row, nothing read out of bounds, the
    # other rows as if nothing had happened
    given = b0.clone()
    given[7] = K + 1000000
    given[9] = -1
    y3 = torch.empty_like(x)
    b3 = torch.empty_like(given)
    rc = _lib.load().smoe_switch_ln_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, given.data_ptr(), -1, sc.EPS, T, d, K,
                                        y3.data_ptr(), b3.data_ptr(), ops._stream(x))
    _lib.check(rc, "smoe_switch_ln_fwd")
    ok = keep & (torch.arange(T, device=DEV) != 9)
    assert torch.equal(y3[ok], y0[ok]) and bool(y3[7].isnan().all()) and bool(y3[9].isnan().all()) and torch.equal(b3, given)
    # a NaN row of dy poisons its own dx row and its own bucket's two gradient rows, nothing else
    dx0, dw0, db0 = ops.switch_ln_bwd(x, dy, w, b0, sc.EPS)
    dyn = dy.clone()
    dyn[7] = float("nan")
    dx1, dw1, db1 = ops.switch_ln_bwd(x, dyn, w, b0, sc.EPS)
    k7 = int(b0[7])
    others = torch.arange(K, device=DEV) != k7
    assert torch.equal(dx1[keep], dx0[keep]) and bool(dx1[7].isnan().all())
    assert torch.equal(dw1[others], dw0[others]) and torch.equal(db1[others], db0[others])
    assert bool(dw1[k7].isnan().all()) and bool(db1[k7].isnan().all())


# --------------------------------------------------------------------------------------------------------------------- module
def test_module_autograd_against_float64_autograd_and_one_launch():
    d, K = 384, 5
    c = sc.make_cell("separated", 3 * 37, d, K)
    mod = sm.SwitchableLayerNorm(d, switchable_buckets=K).to(DEV).train()
    with torch.no_grad():
        mod.weights.copy_(c["weights"])
        mod.biases.copy_(c["biases"])
    mod.set_centroids(c["cent"])
    x = c["x"].reshape(3, 37, d).to(DEV).requires_grad_(True)
    y, b = mod(x)
    y.backward(c["dy"].reshape(3, 37, d).to(DEV))
    x64 = c["x"].double().reshape(3, 37, d).requires_grad_(True)
    w64, b64 = c["weights"].double().requires_grad_(True), c["biases"].double().requires_grad_(True)
    y64, bk64 = sm.switch_ln_compose(x64, sc.EPS, w64, b64, c["cent"].double(), None, K)
    y64.backward(c["dy"].double().reshape(3, 37, d))
    acc = _compose32(c, None)
    assert torch.equal(b.cpu(), bk64) and mod.centroids.grad is None and not b.requires_grad
    for got, want, key in ((y.detach(), y64.detach(), "y"), (x.grad, x64.grad, "dx"), (mod.weights.grad, w64.grad, "dw"),
                           (mod.biases.grad, b64.grad, "db")):
        bound = sc.bar(want.reshape(acc[key].shape), acc[key])
        assert float((got.cpu().double() - want).abs().max()) <= bound, key
    from torch.profiler import profile, ProfilerActivity
    kernels = []
    xin = x.detach()
    for _attempt in range(3):      # (roctracer now and then delivers the runtime-API rows of a cycle without its kernel rows: ask again)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            with torch.no_grad():
                mod(xin)
            torch.cuda.synchronize()
        kernels = [(e.key, e.count) for e in prof.key_averages() if not e.key.startswith("hip")]
        if kernels:
            break
    assert len(kernels) == 1 and kernels[0][1] == 1 and "switch_ln_fwd_kernel" in kernels[0][0], kernels


def test_fallbacks_say_so_and_compute_the_same_rule():
    c = sc.make_cell("separated", 17, 192, 5)
    mod = sm.SwitchableLayerNorm(192, switchable_buckets=5).to(DEV)
    mod.set_centroids(c["cent"])
    x = c["x"].to(DEV)
    with torch.no_grad():
        y, b = mod(x)
        with pytest.warns(sm.vit.SlimMoEFallbackWarning):
            y64, b64 = mod(x.to(torch.float64))
    assert torch.equal(b64, b) and float((y64 - y.double()).abs().max()) <= 1e-5
    view = torch.zeros(17 * 192 + 1, device=DEV)[1:].view(17, 192)              # contiguous f32, 4 bytes off a 16-byte boundary
    view.copy_(x)
    with torch.no_grad(), pytest.warns(sm.vit.SlimMoEFallbackWarning, match="aligned"):
        yv, bv = mod(view)
    assert torch.equal(bv, b) and float((yv - y).abs().max()) <= 1e-5
    with pytest.raises(ValueError):
        mod(x, torch.full((17,), 5, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------- model
def _models(buckets=3, **kw):
    torch.manual_seed(11)
    m = sm.create_model("deit_sw_tiny_patch16_224", buckets=buckets, depth=2, img_size=32, num_classes=10, **kw)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        m.router.weights.copy_(1.0 + 0.25 * torch.randn(buckets, 192, generator=g))
        m.router.biases.copy_(0.25 * torch.randn(buckets, 192, generator=g))
    m.router.set_centroids(0.05 * torch.randn(buckets, 192, generator=g))
    return m.to(DEV)


def _images(B=4, seed=13):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_model_eval_equals_a_plain_twin_fed_the_router_output():
    from slim_switch_moe_vit_amd import vit
    from slim_switch_moe_vit_amd.ep import drain
    m = _models(collect_embeddings=True).eval()
    twin = sm.create_model("deit_tiny_patch16_224", depth=2, img_size=32, num_classes=10).to(DEV).eval()
    sd = {k.replace("mid_blocks.0.", "blocks.0.").replace("post_blocks.0.", "blocks.1."): v for k, v in m.state_dict().items()
          if not k.startswith("router.")}
    twin.load_state_dict(sd)
    img = _images()
    seen = set(vit._fallbacks_seen)
    caught = {}
    hook = m.router.register_forward_hook(lambda mod, args, out: caught.update(inp=args[0], out=out))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        logits, emb = m(img)
        hook.remove()
        stream = m._embed(img)
        y, b = ops.switch_ln(stream, m.router.weights.detach(), m.router.biases.detach(), m.router.centroids.detach(), m.router.eps)
        assert torch.equal(caught["inp"], stream) and torch.equal(emb, stream)           # the pre-router stream, unmodified
        assert torch.equal(caught["out"][0], y) and torch.equal(caught["out"][1], b) and b.shape == (4, 5)
        assert len(set(b.flatten().tolist())) > 1, "the test's centroids should split the rows"
        # the twin enters at its blocks with no norm1 handed along: block 0's norm1 runs through the same kernel on both sides
        x = drain(twin._blocks_steps(y, None, head_rows_only=True))
        want = twin._head(twin.head, twin.pre_logits(twin._final_norm_cls(x)), "head_gemm")
        assert logits.shape == (4, 10) and torch.equal(logits, want)
        ones = torch.ones(4, 5, dtype=torch.int64, device=DEV)
        assert torch.equal(m(img, bucket=1)[0], m(img, bucket=ones)[0]) and not torch.equal(m(img, bucket=1)[0], logits)
    assert set(vit._fallbacks_seen) == seen, set(vit._fallbacks_seen) - seen


def test_distilled_and_moe_patched_models_run():
    img = _images()
    d = _models(distilled=True)
    with torch.autocast("cuda", dtype=torch.float16):
        out = d.train()(img)
        assert isinstance(out, tuple) and out[0].shape == (4, 10) and out[1].shape == (4, 10)
        (out[0].float().sum() + out[1].float().sum()).backward()
        assert d.router.weights.grad is not None and d.router.centroids.grad is None
        with torch.no_grad():
            ev = d.eval()(img)
    assert ev.shape == (4, 10) and bool(torch.isfinite(ev).all())
    p = sm.patch_blocks_with_moe(_models().cpu(), 4, 1, True).to(DEV).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        o = p(img)
    assert o.shape == (4, 10) and bool(torch.isfinite(o).all())


# --------------------------------------------------------------------------------------------------------------------- graphs
def test_evaluate_from_a_hip_graph_equals_eager_without_a_fallback_warning():
    from slim_switch_moe_vit_amd import vit
    m = _models()
    g = torch.Generator().manual_seed(21)
    batches = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(2)]
    seen = set(vit._fallbacks_seen)
    sa = sm.evaluate(batches, m, DEV, hip_graph=True)
    sb = sm.evaluate(batches, m, DEV, hip_graph=False)
    assert sa["hip_graph"] and not sb["hip_graph"] and all(sa[k] == sb[k] for k in ("loss", "acc1", "acc5")), (sa, sb)
    assert set(vit._fallbacks_seen) == seen, set(vit._fallbacks_seen) - seen


def _epoch(graph):
    g = torch.Generator().manual_seed(22)
    n = sm.GraphedTrainStep.WARM + 3
    batches = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(n)]
    model = _models(drop_path_rate=0.0)
    opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    scaler = sm.NativeScaler()
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), batches, opt, DEV, 0, scaler, 1.0, hip_graph=graph)
    torch.cuda.synchronize()
    return st, {k: p.detach().clone() for k, p in model.named_parameters()}, scaler.state_dict()


def test_training_steps_on_a_hip_graph_replay_bit_equal_to_eager_without_a_fallback_warning():
    from slim_switch_moe_vit_amd import vit
    seen = set(vit._fallbacks_seen)
    s_e, p_e, sc_e = _epoch(False)
    s_g, p_g, sc_g = _epoch(True)
    assert s_g["hip_graph_steps"] == 3 and s_e["hip_graph_steps"] == 0, (s_g, s_e)
    assert s_g["loss"] == s_e["loss"], (s_g, s_e)
    assert all(torch.equal(p_e[k], p_g[k]) for k in p_e), [k for k in p_e if not torch.equal(p_e[k], p_g[k])]
    assert sc_e == sc_g
    fresh = _models(drop_path_rate=0.0).router
    assert not torch.equal(p_e["router.weights"], fresh.weights) and not torch.equal(p_e["router.biases"], fresh.biases)   # trained
    assert torch.equal(p_e["router.centroids"], fresh.centroids)
    assert set(vit._fallbacks_seen) == seen, set(vit._fallbacks_seen) - seen
