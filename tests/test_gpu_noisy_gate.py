"""GPU tests of the noisy top-k gate (fmoe.gates.NoisyGate; rule in INTEGRATION.md) against the float64 restatement of
tests/_noisy_gate_cases.py: the kernels over the whole case table (idx bit for bit; score, importance, load, loss, coefficients and
dlogits2 within 3 x the host emulation's error, floor one f32 ulp at the row's scale), the non-finite contract, the module in
training against float64 autograd, eval bit for bit against a bias-free NaiveGate, the harness, HIP-graph capture, and a one-rank
expert-parallel group.

Measured error / bar ratios on an MI355X, worst over the 35 cells of each T (profiles/r20_noisy_gate.md holds the table):
    score <= 0.33, keep 0.00 (stored in f64), imp, load, aux, coef_imp, coef_load <= 0.33, dlogits2 <= 0.30, its score term alone
    <= 0.26, its loss term alone <= 0.55 (T = 1).  0.33 = the emulation's own error set the bar and the kernel sits at the output's
    rounding.  The file takes 15 s: 3 s for the kernel table, the rest for the model-level cases.
"""
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

import _noisy_gate_cases as nc  # noqa: E402
from _mp import float_bar, join_or_kill  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402

DEV = "cuda:0"
_TABLE = {}


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(11)


def _cases(T):
    if T not in _TABLE:
        _TABLE[T] = nc.table((T,))
    return _TABLE[T]


def _dev(t):
    return None if t is None else t.to(DEV)


def _same(a, b):
    """bit-equal, NaNs included"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                    b.reshape(-1).contiguous().view(torch.uint8))


def _fwd(c, eps="case", training=True):
    return ops.noisy_gate_fwd(_dev(c.logits2), _dev(c.eps if isinstance(eps, str) else eps), c.k, training)


def _bwd(c, r, dscore, scale, eps="case", training=True):
    e = c.eps if isinstance(eps, str) else eps
    cs = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
    return ops.noisy_gate_bwd(_dev(c.logits2), _dev(e), r["idx"], r["keep"], r["next"], _dev(dscore), r["coef_imp"], r["coef_load"],
                              cs, training)


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("T", nc.TS)
def test_kernels_against_float64_over_the_case_table(T):
    """idx (and the (k+1)-th expert) bit-equal to the restatement; every float output within nc.within_bar: 3 x the error of the host
    emulation on the same case, floor one f32 ulp at the row's scale ([E] sums and the loss: the tensor's scale).  Two runs are
    bit-equal.  The worst error / bar ratio per output is printed."""
    worst, fails = {}, []
    for c in _cases(T):
        ref = nc.forward64(c.logits2, c.eps, c.k)
        ref["coef_imp"], ref["coef_load"] = nc.coefs64(ref["imp"], ref["load"])
        ref["keep"] = torch.stack((ref["vk"], ref["vk1"]), 1)
        emu = nc.fwd_emulated(c.logits2, c.eps, c.k)
        r, again = _fwd(c), _fwd(c)
        assert r["idx"].dtype == torch.int64 and r["next"].dtype == torch.int32
        assert torch.equal(r["idx"].cpu(), ref["idx"]), c.id
        assert torch.equal(r["next"].cpu().long(), ref["next"]), c.id
        for name in ("idx", "score", "keep", "next", "imp", "load", "aux", "coef_imp", "coef_load"):
            assert _same(r[name], again[name]), (c.id, name)
        for name in ("score", "keep", "imp", "load", "aux", "coef_imp", "coef_load"):
            ok, ratio = nc.within_bar(r[name].cpu(), ref[name], emu[name], per_row=name in ("score", "keep"))
            worst[name] = max(worst.get(name, 0.0), ratio)
            if not ok:
                fails.append((c.id, name, round(ratio, 2)))
        for tag, ds, sc in (("dlogits2", c.dscore, c.scale), ("dlogits2/score", c.dscore, None), ("dlogits2/loss", None, c.scale)):
            want = nc.backward64(c.logits2, c.eps, c.k, ds, sc)
            got = _bwd(c, r, ds, sc)
            assert _same(got, _bwd(c, r, ds, sc)), (c.id, tag)
            ok, ratio = nc.within_bar(got.cpu(), want, nc.bwd_emulated(c.logits2, c.eps, c.k, emu, ds, sc))
            worst[tag] = max(worst.get(tag, 0.0), ratio)
            if not ok:
                fails.append((c.id, tag, round(ratio, 2)))
    print(f"noisy gate T={T}: worst error / bar " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not fails, fails


@pytest.mark.parametrize("T", (65, 257))
def test_null_arguments_leave_out_their_term_and_eval_has_no_noise(T):
    for c in _cases(T):
        if c.regime not in ("plain", "offset"):
            continue
        zero = torch.zeros_like(c.eps)
        r0, rn = _fwd(c, eps=zero), _fwd(c, eps=None)
        for name in r0:
            assert _same(r0[name], rn[name]), (c.id, name)                                  # a NULL eps is a zero eps
        assert _same(_bwd(c, r0, c.dscore, c.scale, eps=zero), _bwd(c, rn, c.dscore, c.scale, eps=None)), c.id
        r = _fwd(c)
        full, score_only, loss_only = _bwd(c, r, c.dscore, c.scale), _bwd(c, r, c.dscore, None), _bwd(c, r, None, c.scale)
        # a NULL scale leaves out the loss terms, a NULL dscore the score term: each equals float64 of that term alone (the table
        # test) and neither is the whole
        assert not _same(full, score_only) and (c.k == 1 or not _same(full, loss_only))      # (k = 1: the score is the constant 1)
        assert _same(score_only, _bwd(c, r, c.dscore, None)) and float(_bwd(c, r, None, None).abs().max()) == 0.0
        assert c.k == 1 or float(score_only[:, c.E:].abs().max()) > 0                     # the noise carries the score's gradient to raw
        # eval: sigma = 0 -- the top-k of the clean logits whatever eps holds, no load, no gradient for raw
        e = _fwd(c, training=False)
        val, idx = torch.topk(c.logits2[:, :c.E], c.k, dim=1)
        assert torch.equal(e["idx"].cpu(), idx) and float(e["load"].abs().max()) == 0.0 and float(e["coef_load"].abs().max()) == 0.0
        ref = nc.forward64(c.logits2, None, c.k, training=False)
        ok, _ = nc.within_bar(e["aux"].cpu(), ref["aux"], nc.fwd_emulated(c.logits2, None, c.k, training=False)["aux"])
        assert ok, c.id
        de = _bwd(c, e, c.dscore, c.scale, training=False)
        assert float(de[:, c.E:].abs().max()) == 0.0
        want = nc.backward64(c.logits2, None, c.k, c.dscore, c.scale, training=False)
        fe = nc.fwd_emulated(c.logits2, None, c.k, training=False)
        ok, ratio = nc.within_bar(de.cpu(), want, nc.bwd_emulated(c.logits2, None, c.k, fe, c.dscore, c.scale, training=False))
        assert ok, (c.id, ratio)


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), float("-inf")))
def test_a_non_finite_row_stays_in_its_row_and_reaches_the_loss(bad):
    c = nc.Case(257, 8, 2, "plain")
    clean = _fwd(c)
    dclean = _bwd(c, clean, c.dscore, None)
    l2 = c.logits2.clone()
    rows = torch.tensor([5, 70, 256])
    l2[5, 3] = bad                      # a clean logit
    l2[70, :8] = bad                    # a whole clean row
    l2[256, 8 + 2] = bad                # a raw logit (-inf there: sigma = 0.01, everything stays finite)
    r = ops.noisy_gate_fwd(_dev(l2), _dev(c.eps), c.k, True)
    d = ops.noisy_gate_bwd(_dev(l2), _dev(c.eps), r["idx"], r["keep"], r["next"], _dev(c.dscore), None, None, None, True)
    others = torch.ones(c.T, dtype=torch.bool)
    others[rows] = False
    others = others.to(DEV)
    assert _same(r["idx"][others], clean["idx"][others]) and _same(r["score"][others], clean["score"][others])
    assert _same(d[others], dclean[others])
    assert int(r["idx"].min()) >= 0 and int(r["idx"].max()) < c.E and int(r["next"].min()) >= 0 and int(r["next"].max()) < c.E
    assert bool(torch.isnan(r["aux"]))                                                     # the loss propagates it
    assert bool(torch.isfinite(d[others]).all())


# ---------------------------------------------------------------------------------------------------------------- the module
def _weights(d, h, E, seed):
    g = torch.Generator().manual_seed(seed)
    wg = torch.randn(d, E, generator=g) * 0.3
    wn = torch.randn(d, E, generator=g) * 0.1
    w1 = torch.randn(E, h, d, generator=g) * 0.05
    b1 = torch.randn(E, h, generator=g) * 0.05
    w2 = torch.randn(E, d, h, generator=g) * 0.05
    b2 = torch.randn(E, d, generator=g) * 0.05
    return wg, wn, w1, b1, w2, b2


def _module(d, h, E, weights, k=2, **kw):
    wg, wn, w1, b1, w2, b2 = weights
    mod = sm.FMoETransformerMLP(E, d, h, torch.nn.GELU(), top_k=k, gate="noisy", **kw)
    with torch.no_grad():
        mod.gate.w_gate.copy_(wg); mod.gate.w_noise.copy_(wn)
        mod.experts.htoh4.weight.copy_(w1); mod.experts.htoh4.bias.copy_(b1)
        mod.experts.h4toh.weight.copy_(w2); mod.experts.h4toh.bias.copy_(b2)
    return mod.to(DEV)


def _naive_twin(d, h, E, weights, k=2):
    """a NaiveGate module whose gate.weight = w_gate.T and whose bias is absent"""
    wg, _, w1, b1, w2, b2 = weights
    mod = sm.FMoETransformerMLP(E, d, h, torch.nn.GELU(), top_k=k)
    mod.gate.gate = torch.nn.Linear(d, E, bias=False)
    with torch.no_grad():
        mod.gate.gate.weight.copy_(wg.t())
        mod.experts.htoh4.weight.copy_(w1); mod.experts.htoh4.bias.copy_(b1)
        mod.experts.h4toh.weight.copy_(w2); mod.experts.h4toh.bias.copy_(b2)
    return mod.to(DEV)


def _inject(mod, eps):
    mod.gate.make_noise = lambda T, device: eps.to(device)


def _reference(x, weights, eps, k, w, aux_w, residual=False):
    leaves = [t.double().clone().requires_grad_(True) for t in (x,) + tuple(weights)]
    xl, wg, wn, w1, b1, w2, b2 = leaves
    r = nc.forward64(torch.cat((xl @ wg, xl @ wn), 1), eps, k)
    out = nc.moe64(xl, r["idx"], r["score"], w1, b1, w2, b2, residual=xl if residual else None)
    ((out * w.double()).sum() + aux_w * r["aux"]).backward()
    return out.detach(), r, [t.grad for t in leaves]


@pytest.mark.parametrize("aux_w", (0.1, 0.0))
@pytest.mark.parametrize("T", (129, 300))
def test_training_forward_and_gradients_match_float64_autograd_of_the_restatement(T, aux_w):
    d, h, E, k = 192, 768, 8, 2
    weights = _weights(d, h, E, 31)
    mod = _module(d, h, E, weights).train()
    g = torch.Generator().manual_seed(40 + T)
    x, w, eps = torch.randn(T, d, generator=g), torch.randn(T, d, generator=g), torch.randn(T, E, generator=g)
    _inject(mod, eps)
    xg = x.to(DEV).requires_grad_(True)
    out = mod.forward_add(xg, xg)
    aux = mod.gate.get_loss()
    assert aux is not None and aux.requires_grad
    loss = (out * w.to(DEV)).sum()
    if aux_w:
        loss = loss + aux_w * aux
    loss.backward()
    ref_out, r, ref = _reference(x, weights, eps, k, w, aux_w, residual=True)
    assert float(nc.min_margin(r["noisy"]).min()) > 1e-5                                   # the routing is decidable in f32
    assert torch.equal(mod.last_plan[0].cpu(), r["idx"])                                   # bit-equal routing
    float_bar(out.detach().cpu(), ref_out)
    assert abs(float(aux.detach()) - float(r["aux"])) <= 1e-5 * max(1.0, abs(float(r["aux"])))
    got = [xg.grad, mod.gate.w_gate.grad, mod.gate.w_noise.grad, mod.experts.htoh4.weight.grad, mod.experts.htoh4.bias.grad,
           mod.experts.h4toh.weight.grad, mod.experts.h4toh.bias.grad]
    for name, a, b in zip(("x", "w_gate", "w_noise", "w1", "b1", "w2", "b2"), got, ref):
        print(name, float_bar(a.cpu(), b))
    assert float(mod.gate.w_noise.grad.abs().max()) > 0


def test_eval_is_bit_equal_to_a_bias_free_naive_gate_on_every_naive_path():
    d, h, E, T = 192, 768, 8, 394
    weights = _weights(d, h, E, 32)
    mod, naive = _module(d, h, E, weights).eval(), _naive_twin(d, h, E, weights).eval()
    ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        assert torch.equal(mod(x), naive(x))
        assert all(torch.equal(a, b) for a, b in zip(mod.last_plan, naive.last_plan))
        assert mod.gate.get_loss() is None
        assert torch.equal(mod.forward_norm_add(x, ln), naive.forward_norm_add(x, ln))
        assert all(torch.equal(a, b) for a, b in zip(mod.last_plan, naive.last_plan))
        assert torch.equal(mod.forward_add(x, x), naive.forward_add(x, x))
        # tail_rows_only's subset of the rows
        a = drain(mod.forward_norm_add_steps(x.clone(), ln, tail=(197, 1)))
        b = drain(naive.forward_norm_add_steps(x.clone(), ln, tail=(197, 1)))
        assert torch.equal(a, b)
    # the image follows the parameter
    with torch.no_grad():
        mod.gate.w_gate.mul_(-1.0); naive.gate.gate.weight.mul_(-1.0)
        assert torch.equal(mod(x), naive(x))


def drain(gen):
    from slim_switch_moe_vit_amd.ep import drain as _drain
    return _drain(gen)


def _twin_models(**kw):
    torch.manual_seed(5)
    noisy = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2, gate="noisy", **kw)
    naive = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2, **kw)
    sd = noisy.state_dict()
    for name, m in naive.named_modules():
        if isinstance(m, sm.FMoETransformerMLP):
            m.gate.gate = torch.nn.Linear(m.d_model, m.gate.tot_expert, bias=False)
            with torch.no_grad():
                m.gate.gate.weight.copy_(sd[name + ".gate.w_gate"].t())
    naive.load_state_dict({k: v for k, v in sd.items() if ".gate.w_" not in k}, strict=False)
    return noisy.to(DEV), naive.to(DEV)


def test_model_eval_forward_and_evaluate_equal_the_naive_twin_without_a_fallback_warning():
    from slim_switch_moe_vit_amd import vit
    noisy, naive = _twin_models()
    noisy.eval(); naive.eval()
    seen = set(vit._fallbacks_seen)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(4, 3, 224, 224, generator=g).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(noisy(x), naive(x))
    for m in noisy.modules():
        if isinstance(m, sm.FMoETransformerMLP):
            assert m.gate.get_loss() is None
    batches = [(torch.randn(4, 3, 224, 224, generator=g), torch.randint(0, 10, (4,), generator=g)) for _ in range(2)]
    sa, sb = sm.evaluate(batches, noisy, DEV), sm.evaluate(batches, naive, DEV)      # replays the forward from one HIP graph
    assert sa["hip_graph"] and all(sa[m] == sb[m] for m in ("loss", "acc1", "acc5")), (sa, sb)
    assert set(vit._fallbacks_seen) == seen, set(vit._fallbacks_seen) - seen


def test_a_no_grad_forward_in_training_mode_routes_with_noise_and_computes_no_loss():
    d, h, E, T, k = 192, 768, 8, 257, 2
    weights = _weights(d, h, E, 33)
    mod = _module(d, h, E, weights).train()
    ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(4))
    xd = x.to(DEV)
    mod.gate.set_loss("stale")
    with torch.no_grad():
        out = mod(xd)
    assert mod.gate.get_loss() is None
    eps, idx, score = mod.gate.last_noise[0].cpu(), mod.last_plan[0].cpu(), mod.last_plan[1].cpu()
    r = nc.forward64(torch.cat((x.double() @ weights[0].double(), x.double() @ weights[1].double()), 1), eps, k)
    sure = nc.min_margin(r["noisy"]) > 1e-5          # (a real draw: a row may sit within f32 rounding of a tie)
    assert float(sure.double().mean()) > 0.98 and torch.equal(idx[sure], r["idx"][sure])
    float_bar(out.cpu(), nc.moe64(x, idx, score, *weights[2:]))
    assert not torch.equal(idx, torch.topk(x @ weights[0], k, dim=1).indices)              # the noise moved some rows
    # the LayerNorm-fused entry point hands a noisy gate to the unfused sequence
    mod.gate.set_loss("stale")
    with torch.no_grad():
        out2 = mod.forward_norm_add(xd, ln)
    assert mod.gate.get_loss() is None
    idx2, score2 = mod.last_plan[0].cpu(), mod.last_plan[1].cpu()
    xn = torch.nn.functional.layer_norm(x.double(), (d,), ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu(), 1e-6)
    float_bar(out2.cpu(), nc.moe64(xn, idx2, score2, *weights[2:], residual=x))
    assert not torch.equal(mod.gate.last_noise[0].cpu(), eps)                              # a fresh draw per forward


def test_train_one_epoch_with_the_aux_loss_changes_w_noise_without_a_fallback_warning():
    from slim_switch_moe_vit_amd import vit
    g = torch.Generator().manual_seed(73)
    batches = [(torch.randn(4, 3, 224, 224, generator=g), torch.randint(0, 10, (4,), generator=g)) for _ in range(2)]
    torch.manual_seed(0)
    model = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2, drop_path_rate=0.0, gate="noisy").to(DEV)
    moes = [m for m in model.modules() if isinstance(m, sm.FMoETransformerMLP)]
    before = [m.gate.w_noise.detach().clone() for m in moes]
    seen = set(vit._fallbacks_seen)
    opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), batches, opt, DEV, 0, sm.NativeScaler(), 1.0, aux_loss_weight=0.01)
    torch.cuda.synchronize()
    assert moes and all(not torch.equal(a, m.gate.w_noise.detach()) for a, m in zip(before, moes))
    assert all(bool(torch.isfinite(m.gate.w_noise).all()) for m in moes) and st["loss"] == st["loss"]
    assert set(vit._fallbacks_seen) == seen, set(vit._fallbacks_seen) - seen


def _epoch(graph, static_noise):
    g = torch.Generator().manual_seed(72)
    batches = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(5)]
    torch.manual_seed(0)
    model = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2, drop_path_rate=0.0, gate="noisy").to(DEV)
    moes = [m for m in model.modules() if isinstance(m, sm.FMoETransformerMLP)]
    if static_noise:
        for i, m in enumerate(moes):
            _inject(m, torch.randn(8 * 197, 8, generator=torch.Generator().manual_seed(100 + i)).to(DEV))
    opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    scaler = sm.NativeScaler()
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), batches, opt, DEV, 0, scaler, 1.0, aux_loss_weight=0.01, hip_graph=graph)
    torch.cuda.synchronize()
    return st, [p.detach().clone() for p in model.parameters()], scaler.state_dict()


def test_training_step_with_static_noise_on_one_hip_graph_replays_bit_equal_to_eager():
    s_e, p_e, sc_e = _epoch(False, True)
    s_g, p_g, sc_g = _epoch(True, True)
    assert s_g["hip_graph_steps"] == 2 and s_e["hip_graph_steps"] == 0, (s_g, s_e)
    assert s_g["loss"] == s_e["loss"], (s_g, s_e)
    assert all(torch.equal(a, b) for a, b in zip(p_e, p_g)), "parameters after 5 steps"
    assert sc_e == sc_g


def test_training_step_with_the_real_draw_captures_and_replays_with_a_finite_loss():
    st, params, _ = _epoch(True, False)
    assert st["hip_graph_steps"] == 2, st
    assert st["loss"] == st["loss"] and abs(st["loss"]) < 1e4, st
    assert all(bool(torch.isfinite(p).all()) for p in params)


# ---------------------------------------------------------------------------------------------------------------- expert parallel
def _port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _one_rank_worker(q):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_port()}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        d, h, E, T = 192, 768, 8, 300
        weights = _weights(d, h, E, 36)
        mod = _module(d, h, E, weights)
        ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
        g = torch.Generator().manual_seed(9)
        x, eps = torch.randn(T, d, generator=g).to(DEV), torch.randn(T, E, generator=g)
        _inject(mod, eps)
        res = {"same": [], "routing": []}
        mod.eval()
        outs = {}
        for ep_on in (False, True):
            mod.force_ep = ep_on
            with torch.no_grad():
                outs[ep_on] = (mod(x), mod.forward_norm_add(x, ln), mod.last_plan[0].clone())
        res["same"] = [bool(torch.equal(a, b)) for a, b in zip(outs[False], outs[True])]
        mod.train()
        grads, routes, fwd = [], [], []
        for ep_on in (False, True):
            mod.force_ep = ep_on
            mod.zero_grad()
            xg = x.clone().requires_grad_(True)
            out = mod(xg)
            ((out * out).sum() + 0.1 * mod.gate.get_loss()).backward()
            grads.append([xg.grad.clone()] + [p.grad.clone() for p in mod.parameters()])
            routes.append(mod.last_plan[0].clone())
            fwd.append(out.detach().clone())
            with torch.no_grad():                                 # training mode without grad: the noisy route under ep
                fwd.append(mod(x).clone())
                routes.append(mod.last_plan[0].clone())
        res["routing"] = all(bool(torch.equal(routes[0], r)) for r in routes[1:])       # the same injected eps everywhere
        res["out_bar"] = [float_bar(fwd[2].cpu(), fwd[0].double().cpu()), float_bar(fwd[3].cpu(), fwd[1].double().cpu())]
        res["grad_bar"] = [float_bar(b.cpu(), a.double().cpu()) for a, b in zip(*grads)]
        q.put(res)
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_force_ep_on_a_one_rank_group_equals_the_single_rank_path():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(q,))
    p.start()
    join_or_kill([p], 300)
    res = q.get(timeout=10)
    print("NoisyGate, force_ep, one-rank group:", res)
    assert all(res["same"]) and res["routing"], res
