"""GPU tests of the GShard gate (fmoe.gates.GShardGate; rule in INTEGRATION.md) against the float64 restatement of
tests/_gshard_cases.py: the prune kernels bit for bit over the whole case table, the balance loss and the backward against float64
with bars taken from the host emulation of the same arithmetic, the module without and with autograd, the expert-parallel paths
(one-rank group: static exchange by capacity, no host read-back; two ranks on one GPU) and the training step on one HIP graph."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

import _gshard_cases as gc  # noqa: E402
from _mp import dtype_factor, float_bar, join_or_kill  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402

DEV = "cuda:0"
_TABLE = {}


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(7)          # the gate's uniform draw comes from the device generator: the same draw in every run


def _cases(T):
    if T not in _TABLE:
        _TABLE[T] = gc.table((T,))
    return _TABLE[T]


def _dev(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------------------------------------------- prune
@pytest.mark.parametrize("T", gc.TS)
def test_prune_is_bit_equal_to_the_restatement(T):
    for c in _cases(T):
        want, want_top1, _, _ = gc.prune(c.idx, c.score, c.u, c.E, c.cap)
        got, top1 = ops.gshard_prune(_dev(c.idx), _dev(c.score), _dev(c.u), c.E, c.cap)
        again, top1_again = ops.gshard_prune(_dev(c.idx), _dev(c.score), _dev(c.u), c.E, c.cap)
        assert got.dtype == torch.int64 and top1.dtype == torch.int32
        assert torch.equal(got.cpu(), want), c.id
        assert torch.equal(top1.cpu().long(), want_top1), c.id
        assert torch.equal(got, again) and torch.equal(top1, top1_again), c.id


@pytest.mark.parametrize("T", (129, 513, 1500))
def test_prune_reads_ids_outside_the_expert_range_as_dropped_and_negative_capacity_as_no_clamp(T):
    c = gc.Case(T, 8, 0.5, 2.0, True)
    idx = c.idx.clone()
    idx[::3, 1] = 8
    idx[1::5, 0] = -1
    idx[2::7, 0] = (1 << 32) + 1          # the low word lies inside [0, E)
    for cap in (c.cap, -1, 0):
        want, want_top1, _, _ = gc.prune(idx, c.score, c.u, c.E, cap)
        got, top1 = ops.gshard_prune(_dev(idx), _dev(c.score), _dev(c.u), c.E, cap)
        assert torch.equal(got.cpu(), want) and torch.equal(top1.cpu().long(), want_top1), (T, cap)
    got, _ = ops.gshard_prune(_dev(c.idx), _dev(c.score), None, c.E, -1)
    assert torch.equal(got.cpu(), c.idx)                                          # no capacity, no random routing: the identity


# ---------------------------------------------------------------------------------------------------------------- aux, coef, dlogits
@pytest.mark.parametrize("T", gc.TS)
def test_aux_coef_and_dlogits_against_float64_within_three_times_the_emulations_error(T):
    """Per case: bar = max(3 x the error of the host emulation of the same f32 arithmetic, one f32 ulp of the largest reference
    value) (gc.bar).  The measured errors are printed (profiles/r19_gshard_gate.md holds them)."""
    aux_seen = {}
    for c in _cases(T):
        ne = c.E if c.E == 2 else c.E // 2            # (the local expert count of a two-rank group: not E)
        idx_out, top1, _, _ = gc.prune(c.idx, c.score, c.u, c.E, c.cap)
        key = (c.E, c.offset)
        if key not in aux_seen:                        # (aux sees neither the rate nor u)
            aux64, coef64 = gc.aux64(c.logits, top1, ne)
            aux_e, coef_e = gc.aux_emulated(c.logits, top1, ne)
            aux, coef = ops.gshard_aux(_dev(c.logits), _dev(top1.int()), ne)
            aux2, coef2 = ops.gshard_aux(_dev(c.logits), _dev(top1.int()), ne)
            assert torch.equal(aux, aux2) and torch.equal(coef, coef2), c.id                      # bit-reproducible
            e_aux, b_aux = abs(float(aux.double().cpu() - aux64)), gc.bar(abs(float(aux_e.double() - aux64)), float(aux64))
            e_coef = float((coef.double().cpu() - coef64).abs().max())
            b_coef = gc.bar(float((coef_e.double() - coef64).abs().max()), float(coef64.abs().max()))
            print(f"gshard_aux {c.id}: aux err {e_aux:.3e} bar {b_aux:.3e}; coef err {e_coef:.3e} bar {b_coef:.3e}")
            assert e_aux <= b_aux and e_coef <= b_coef, c.id
            aux_seen[key] = coef.cpu()
        coef = aux_seen[key]
        scale = torch.tensor([0.01])
        for ds, cf, sc in ((c.dscore, coef, scale), (c.dscore, None, None), (None, coef, None)):
            ref = gc.gate_bwd64(c.logits, c.idx, idx_out, c.score, ds, cf, 1.0 if sc is None else float(sc.double()))
            emu = gc.gate_bwd_emulated(c.logits, c.idx, idx_out, c.score, ds, cf, sc)
            got = ops.gshard_gate_bwd(_dev(c.logits), _dev(c.idx), _dev(idx_out), _dev(c.score), _dev(ds), _dev(cf), _dev(sc))
            err = float((got.double().cpu() - ref).abs().max())
            b = gc.bar(float((emu.double() - ref).abs().max()), float(ref.abs().max()))
            if ds is not None and cf is not None:
                print(f"gshard_gate_bwd {c.id}: err {err:.3e} bar {b:.3e}")
            assert err <= b, (c.id, ds is None, cf is None, err, b)


def test_backward_ignores_the_score_gradient_of_dropped_entries_whatever_the_buffer_holds():
    c = gc.Case(513, 8, 0.5, 2.0, True)
    idx_out, top1, _, _ = gc.prune(c.idx, c.score, c.u, c.E, c.cap)
    assert (idx_out < 0).any()
    args = (_dev(c.logits), _dev(c.idx), _dev(idx_out), _dev(c.score))
    clean = ops.gshard_gate_bwd(*args, _dev(c.dscore * (idx_out >= 0)), None)
    poisoned = torch.where(idx_out >= 0, c.dscore, torch.full_like(c.dscore, float("nan")))
    assert torch.equal(ops.gshard_gate_bwd(*args, _dev(poisoned), None), clean)
    with pytest.raises(RuntimeError, match="top-2"):
        ops.gshard_gate_bwd(_dev(c.logits), _dev(c.idx[:, :1].contiguous()), _dev(idx_out), _dev(c.score), None, None)
    with pytest.raises(RuntimeError, match="top-2"):
        ops.gshard_prune(_dev(c.idx.reshape(-1, 1)), _dev(c.score), None, 8, 1)


# ---------------------------------------------------------------------------------------------------------------- the module
def _weights(d, h, E, seed):
    g = torch.Generator().manual_seed(seed)
    wg = torch.randn(E, d, generator=g) * 0.3
    bg = torch.randn(E, generator=g) * 0.1
    bg[0] += 1.0                                       # a favoured expert: the capacity binds
    w1 = torch.randn(E, h, d, generator=g) * 0.05
    b1 = torch.randn(E, h, generator=g) * 0.05
    w2 = torch.randn(E, d, h, generator=g) * 0.05
    b2 = torch.randn(E, d, generator=g) * 0.05
    return wg, bg, w1, b1, w2, b2


def _module(d, h, E, weights, sl=None, **kw):
    wg, bg, w1, b1, w2, b2 = weights
    sl = slice(0, E) if sl is None else sl
    mod = sm.FMoETransformerMLP(sl.stop - sl.start, d, h, torch.nn.GELU(), top_k=2, **kw)
    with torch.no_grad():
        mod.gate.gate.weight.copy_(wg); mod.gate.gate.bias.copy_(bg)
        mod.experts.htoh4.weight.copy_(w1[sl]); mod.experts.htoh4.bias.copy_(b1[sl])
        mod.experts.h4toh.weight.copy_(w2[sl]); mod.experts.h4toh.bias.copy_(b2[sl])
    return mod.to(DEV)


def _plan(idx_out, E):
    """(counts [E], inv_pos [2 T]) of the stable counting sort over the kept entries, in flat order."""
    flat = idx_out.reshape(-1)
    kept = (flat >= 0).nonzero().squeeze(1)
    counts = torch.bincount(flat[kept], minlength=E)
    order = torch.sort(flat[kept], stable=True).indices
    inv_pos = torch.full_like(flat, -1)
    inv_pos[kept[order]] = torch.arange(kept.numel())
    return counts, inv_pos


def _check_routing(mod, E, cap):
    """The module's latest forward against the restatement evaluated on ITS OWN idx / f32 score / u: no token excluded."""
    idx, score = mod.last_plan[0].cpu(), mod.last_plan[1].cpu()
    u, idx_out, top1 = mod.gate.last_routing
    want, want_top1, by_cap, by_rand = gc.prune(idx, score, None if u is None else u.cpu(), E, cap)
    assert torch.equal(idx_out.cpu(), want) and torch.equal(top1.cpu().long(), want_top1)
    counts, inv_pos = _plan(want, E)
    assert torch.equal(mod.last_plan[2].cpu().long(), counts)
    assert torch.equal(mod.last_plan[5].cpu(), inv_pos)
    return idx, score, want, by_cap, by_rand


@pytest.mark.parametrize("T", (129, 513))
@pytest.mark.parametrize("d,h,E", [(192, 768, 8), (64, 128, 2)])
def test_module_without_grad_routes_by_the_rule_and_meets_the_float_bar(d, h, E, T):
    weights = _weights(d, h, E, 11)
    mod = _module(d, h, E, weights, gate="gshard", capacity_factor=0.5).eval()
    ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
    with torch.no_grad():
        ln.weight.uniform_(0.8, 1.2, generator=torch.Generator(device=DEV).manual_seed(1)); ln.bias.fill_(0.05)
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(T))
    cap = gc.capacity(0.5, T, E)
    assert mod.gate.capacity(T) == cap
    with torch.no_grad():
        out = mod(x.to(DEV))
    idx, score, idx_out, by_cap, by_rand = _check_routing(mod, E, cap)
    assert by_cap.any() and by_rand.any() and (idx_out >= 0).any()
    assert mod.gate.get_loss() is None                      # no balance loss in a no-grad forward
    float_bar(out.cpu(), gc.moe64(x, idx_out, score, *weights[2:]))
    with torch.no_grad():
        out2 = mod.forward_norm_add(x.to(DEV), ln)
    idx, score, idx_out, by_cap, by_rand = _check_routing(mod, E, cap)
    assert by_cap.any() and by_rand.any()
    xn = torch.nn.functional.layer_norm(x.double(), (d,), ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu(), 1e-6)
    float_bar(out2.cpu(), gc.moe64(xn, idx_out, score, *weights[2:], residual=x))


def test_without_random_routing_and_capacity_the_gate_is_the_naive_top2_gate_bit_for_bit():
    d, h, E, T = 192, 768, 8, 513
    weights = _weights(d, h, E, 12)
    naive = _module(d, h, E, weights).eval()
    mod = _module(d, h, E, weights, gate="gshard", capacity_factor=1e6).eval()
    mod.gate.random_routing = False
    ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        assert torch.equal(mod(x), naive(x))
        assert torch.equal(mod.last_plan[5], naive.last_plan[5]) and mod.gate.last_routing[0] is None
        assert torch.equal(mod.forward_norm_add(x, ln), naive.forward_norm_add(x, ln))
        assert torch.equal(mod.forward_add(x, x), naive.forward_add(x, x))


@pytest.mark.parametrize("T", (1, 2))
def test_zero_capacity_returns_the_residual_or_zeros(T):
    d, h, E = 192, 768, 8
    mod = _module(d, h, E, _weights(d, h, E, 13), gate="gshard", capacity_factor=1.2).eval()      # (ceil(1.2 T) * 2) // 8 = 0 for T <= 2
    assert mod.gate.capacity(T) == 0
    ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        assert float(mod(x).abs().max()) == 0.0
        assert bool((mod.gate.last_routing[1] < 0).all()) and int(mod.last_plan[2].sum()) == 0
        assert torch.equal(mod.forward_norm_add(x, ln), x)
        assert torch.equal(mod.forward_add(x, x), x)


# ---------------------------------------------------------------------------------------------------------------- training
def _reference_grads(x, weights, idx, idx_out, top1, ne, w, aux_w, residual=False):
    leaves = [t.double().clone().requires_grad_(True) for t in (x,) + tuple(weights)]
    xl, wg, bg, w1, b1, w2, b2 = leaves
    logits = xl @ wg.t() + bg
    score = torch.softmax(logits.gather(1, idx), dim=-1)
    out = gc.moe64(xl, idx_out, score, w1, b1, w2, b2, residual=xl if residual else None)
    T, E = logits.shape
    aux = ((top1.double() / T) * torch.softmax(logits, 1).mean(0)).mean() * ne ** 2
    ((out * w.double()).sum() + aux_w * aux).backward()
    return out.detach(), aux.detach(), [t.grad for t in leaves]


def _bias_sigma(x, w, idx, idx_out, score, weights, E):
    """[E] float64: the standard deviation that the 16-bit roundings in front of the score gradient give the gate's bias gradient.
    ds[t, b] = <dout[t], y[t, b]> with y the 16-bit store of GEMM-2, whose operands A = gelu(H), W2 and, through H, x and W1 are
    16-bit images too: five roundings of relative rms 2^-11 / sqrt(3), modelled as independent relative errors of y's elements, so
    ds[t, b] carries delta q[t, b] with delta = sqrt(5) 2^-11 / sqrt(3) and q = sqrt(sum_c (dout[t, c] y[t, b, c])^2) (the dot
    product cancels: q is not |ds|).  dlogits[t, idx[t, a]] takes ds[t, b] with the coefficient score_a ([a == b] - score_b), and
    the bias gradient of expert e is the column sum over the tokens: independent terms, the variances add.  dout = w here."""
    _, _, w1, b1, w2, b2 = weights
    delta = (5.0 ** 0.5) * 2.0 ** -11 / 3.0 ** 0.5
    q = torch.zeros(x.shape[0], 2, dtype=torch.float64)
    for e in range(E):
        for j in range(2):
            rows = (idx_out[:, j] == e).nonzero().squeeze(1)
            if rows.numel():
                q[rows, j] = (w[rows].double() * gc.ffn64(x[rows], w1, b1, w2, b2, e)).pow(2).sum(1).sqrt()
    s = score.double()
    var = torch.zeros(E, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            c = s[:, a] * ((1.0 if a == b else 0.0) - s[:, b])
            var.index_add_(0, idx[:, a], (c * delta * q[:, b]) ** 2)
    return var.sqrt()


@pytest.mark.parametrize("aux_w", (0.01, 0.0))
@pytest.mark.parametrize("T", (129, 513))
def test_training_gradients_match_float64_autograd_of_the_restatement(T, aux_w):
    """loss = sum(out * w) + 0.01 aux; with weight 0 the aux output is not part of the objective at all (daux = None: the score
    gradient alone).  Output and gradients within THE float bar (_mp.float_bar at its 1e-3), with one exception, the gate's bias
    gradient: its max-|diff| half is max(1e-3 max(1, max |ref|), 3 sigma) with sigma from _bias_sigma (the 16-bit roundings in front
    of the score gradient, propagated to this column sum, which cancels: 3 sigma = 1.1e-2 at T = 513 against a scale of 6.1, where
    6.6e-3 was measured and 1e-3 allows 6.1e-3); its relative L2 stays at 1e-3 (measured 8.8e-4)."""
    d, h, E = 128, 256, 8
    weights = _weights(d, h, E, 14)
    mod = _module(d, h, E, weights, gate="gshard", capacity_factor=0.5).train()
    g = torch.Generator().manual_seed(20 + T)
    x, w = torch.randn(T, d, generator=g), torch.randn(T, d, generator=g)
    xg = x.to(DEV).requires_grad_(True)
    out = mod(xg)
    aux = mod.gate.get_loss()
    assert aux is not None and aux.requires_grad
    loss = (out * w.to(DEV)).sum()
    if aux_w:
        loss = loss + aux_w * aux
    loss.backward()
    cap = gc.capacity(0.5, T, E)
    idx, score, idx_out, by_cap, by_rand = _check_routing(mod, E, cap)
    assert by_cap.any() and by_rand.any()
    top1 = mod.gate.last_routing[2].cpu().long()
    ref_out, ref_aux, ref = _reference_grads(x, weights, idx, idx_out, top1, E, w, aux_w)
    float_bar(out.detach().cpu(), ref_out)
    assert abs(float(aux.detach()) - float(ref_aux)) <= 1e-5 * max(1.0, abs(float(ref_aux)))
    got = [xg.grad, mod.gate.gate.weight.grad, mod.gate.gate.bias.grad, mod.experts.htoh4.weight.grad, mod.experts.htoh4.bias.grad,
           mod.experts.h4toh.weight.grad, mod.experts.h4toh.bias.grad]
    for name, a, b in zip(("x", "wg", "bg", "w1", "b1", "w2", "b2"), got, ref):
        if name != "bg":
            print(name, float_bar(a.cpu(), b))
            continue
        diff = a.cpu().double() - b
        scale = max(1.0, float(b.abs().max()))
        sigma = float(_bias_sigma(x, w, idx, idx_out, score, weights, E).max())
        max_abs, rel_l2 = float(diff.abs().max()), float(diff.norm() / b.norm())
        print(name, (max_abs, scale, rel_l2), "3 sigma", 3 * sigma)
        assert max_abs <= max(1e-3 * dtype_factor() * scale, 3 * dtype_factor() * sigma) and rel_l2 <= 1e-3 * dtype_factor(), \
            dict(max_abs=max_abs, ref_abs_max=scale, rel_l2=rel_l2, three_sigma=3 * sigma)


def test_training_with_the_residual_add_and_the_aux_loss_alone():
    d, h, E, T = 128, 256, 8, 129
    weights = _weights(d, h, E, 15)
    mod = _module(d, h, E, weights, gate="gshard", capacity_factor=0.5).train()
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(5))
    xg = x.to(DEV).requires_grad_(True)
    out = mod.forward_add(xg, xg)
    aux = mod.gate.get_loss()
    aux.backward()                                     # dscore = None: the balance-loss term alone reaches the router
    idx, score, idx_out, _, _ = _check_routing(mod, E, gc.capacity(0.5, T, E))
    top1 = mod.gate.last_routing[2].cpu().long()
    ref_out, ref_aux, ref = _reference_grads(x, weights, idx, idx_out, top1, E, torch.zeros(T, d), 1.0, residual=True)
    float_bar(out.detach().cpu(), ref_out)
    for name, a, b in (("x", xg.grad, ref[0]), ("wg", mod.gate.gate.weight.grad, ref[1]), ("bg", mod.gate.gate.bias.grad, ref[2])):
        float_bar(a.cpu(), b)
    assert mod.experts.htoh4.weight.grad is None or float(mod.experts.htoh4.weight.grad.abs().max()) == 0.0


def test_without_a_capacity_random_routing_still_prunes_the_plan_under_the_zero_row_hint():
    """GShardGate(capacity=None): capacity() is -1, and a training forward that names its all-zero rows (the residual-MoE block's
    hint) must still plan over the pruned ids: what random routing dropped is neither dispatched nor combined."""
    d, h, E, T = 128, 256, 8, 257
    weights = _weights(d, h, E, 18)
    mod = _module(d, h, E, weights, gate="gshard").train()
    mod.gate.capacity_factor = None
    assert mod.gate.capacity(T) == -1
    g = torch.Generator().manual_seed(8)
    x, w = torch.randn(T, d, generator=g), torch.randn(T, d, generator=g)
    x[::3] = 0.0
    zero = (x.abs().sum(1) == 0)
    xg = x.to(DEV).requires_grad_(True)
    out = mod.forward_add(xg, xg, zero_rows=zero.to(DEV))
    (out * w.to(DEV)).sum().backward()
    idx, score, idx_out, by_cap, by_rand = _check_routing(mod, E, -1)
    assert not by_cap.any() and by_rand.any() and by_rand[zero].any()
    top1 = mod.gate.last_routing[2].cpu().long()
    ref_out, _, ref = _reference_grads(x, weights, idx, idx_out, top1, E, w, 0.0, residual=True)
    float_bar(out.detach().cpu(), ref_out)
    float_bar(xg.grad.cpu(), ref[0])


# ---------------------------------------------------------------------------------------------------------------- expert parallel
def _port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _one_rank_worker(q):
    import torch.distributed as dist
    from slim_switch_moe_vit_amd import ep
    from test_gpu_ep_static import _count_readbacks
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_port()}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        d, h, E, T = 192, 768, 8, 513
        weights = _weights(d, h, E, 16)
        mod = _module(d, h, E, weights, gate="gshard", capacity_factor=0.5).eval()
        ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
        x = torch.randn(T, d, generator=torch.Generator().manual_seed(6)).to(DEV)
        res = {}

        def run(fn):
            torch.manual_seed(99)                      # the same uniform draw in both modes
            with torch.no_grad():
                out = fn()
            return out, mod.gate.last_routing[0].clone(), mod.gate.last_routing[1].clone()

        single = run(lambda: mod(x))
        single_ln = run(lambda: mod.forward_norm_add(x, ln))
        mod.force_ep = True
        calls, restore = _count_readbacks(ep)
        res["kind"] = ep.static_kind(mod, torch.float16)
        forced = run(lambda: mod(x))
        forced_ln = run(lambda: mod.forward_norm_add(x, ln))
        res["readbacks"] = calls["n"]
        restore()
        res["same"] = [bool(torch.equal(a, b)) for a, b in zip(single + single_ln, forced + forced_ln)]
        res["dropped"] = int((forced[2] < 0).sum())
        # training through the static exchange: the single-rank path's gradients
        mod.train()
        grads = []
        for ep_on in (False, True):
            mod.force_ep = ep_on
            mod.zero_grad()
            torch.manual_seed(98)
            xg = x.clone().requires_grad_(True)
            out = mod(xg)
            ((out * out).sum() + 0.01 * mod.gate.get_loss()).backward()
            grads.append([xg.grad.clone()] + [p.grad.clone() for p in mod.parameters()])
        res["train_rel"] = max(float((a - b).norm() / b.norm().clamp(min=1e-30)) for a, b in zip(*grads))
        q.put(res)
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_force_ep_on_a_one_rank_group_takes_the_static_exchange_by_capacity_without_a_read_back():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(q,))
    p.start()
    join_or_kill([p], 300)
    res = q.get(timeout=10)
    print("GShardGate, force_ep, one-rank group:", res)
    assert res["kind"] == "capacity" and res["readbacks"] == 0, res
    assert all(res["same"]) and res["dropped"] > 0, res
    # the same kernels on the same rows; the slot layout regroups the weight gradients' f32 sums over ~500 rows (re-association:
    # ~sqrt(500) 2^-24 = 1.3e-6 typical, 500 x 2^-24 = 3e-5 at worst); one lost or mis-scaled row of 1026 would be ~3e-2
    assert res["train_rel"] <= 1e-4, res


def _two_ranks_worker(rank, world, port, q):
    """One rank of two sharing cuda:0 over gloo: E = 8 experts split over the ranks, ragged batches, per-source-rank capacity."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        d, h, E = 192, 768, 8
        E_local = E // world
        weights = _weights(d, h, E, 17)
        part = _module(d, h, E, weights, sl=slice(rank * E_local, (rank + 1) * E_local), gate="gshard", capacity_factor=0.5,
                       world_size=world).eval()
        assert part.gate.tot_expert == E and part.gate.num_expert == E_local
        ln = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
        T = 300 + 13 * rank
        x = torch.randn(T, d, generator=torch.Generator().manual_seed(500 + rank))
        res = {}
        with torch.no_grad():
            out = part.forward_norm_add(x.to(DEV), ln)
        cap = gc.capacity(0.5, T, E)                  # per source rank, on ITS rows
        idx, score = part.last_plan[0].cpu(), part.last_plan[1].cpu()
        u, idx_out, top1 = part.gate.last_routing
        want, want_top1, by_cap, by_rand = gc.prune(idx, score, u.cpu(), E, cap)
        res["routing"] = (bool(torch.equal(idx_out.cpu(), want)), bool(torch.equal(top1.cpu().long(), want_top1)),
                          bool(by_cap.any()), bool(by_rand.any()))
        xn = torch.nn.functional.layer_norm(x.double(), (d,), ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu(), 1e-6)
        ref = gc.moe64(xn, want, score, *weights[2:], residual=x)
        res["bar"] = float_bar(out.cpu(), ref)
        q.put((rank, res))
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_apply_the_capacity_per_source_rank():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_two_ranks_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    join_or_kill(procs, 300)
    got = dict(q.get(timeout=10) for _ in range(2))
    for rank in range(2):
        print(f"GShardGate rank {rank}/2:", got[rank])
        assert got[rank]["routing"] == (True, True, True, True), (rank, got[rank])


# ---------------------------------------------------------------------------------------------------------------- graph capture
def test_training_step_with_the_gshard_gate_on_one_hip_graph_reproduces_the_eager_harness():
    """train_one_epoch(hip_graph=True): three eager steps, then the captured step replayed twice.  The second choice's random draw is
    off, as the SwitchGate's noise is in the other graph tests (a draw comes from another point of the generator's stream under a
    graph); capacity, balance loss and the gate's backward are all inside the graph."""
    g = torch.Generator().manual_seed(72)
    batches = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(5)]

    def run(graph):
        torch.manual_seed(0)
        model = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2, drop_path_rate=0.0, gate="gshard",
                                capacity_factor=0.5).to(DEV)
        moes = [m for m in model.modules() if isinstance(m, sm.FMoETransformerMLP)]
        for m in moes:
            m.gate.random_routing = False
        opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
        scaler = sm.NativeScaler()
        st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), batches, opt, DEV, 0, scaler, 1.0, aux_loss_weight=0.01,
                                hip_graph=graph)
        torch.cuda.synchronize()
        dropped = int(sum((m.last_plan[5] < 0).sum() for m in moes))
        return st, [p.detach().clone() for p in model.parameters()], scaler.state_dict(), dropped, len(moes)

    s_e, p_e, sc_e, d_e, n_e = run(False)
    s_g, p_g, sc_g, d_g, _ = run(True)
    assert n_e > 0 and d_e > 0 and d_e == d_g, (n_e, d_e, d_g)
    assert s_g["hip_graph_steps"] == 2 and s_e["hip_graph_steps"] == 0, (s_g, s_e)
    assert s_g["loss"] == s_e["loss"], (s_g, s_e)
    assert all(torch.equal(a, b) for a, b in zip(p_e, p_g)), "parameters after 5 steps"
    assert sc_e == sc_g
