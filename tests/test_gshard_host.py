"""CPU tests of the GShard gate (fmoe.gates.GShardGate; the rule is restated in INTEGRATION.md): the vectorised restatement of
tests/_gshard_cases.py against a per-entry walk of the rule, the backward formulas against float64 autograd, an f32 emulation of
smoe_gshard_aux / smoe_gshard_gate_bwd in the kernels' summation order against float64 (its measured error is where the GPU bars come
from), ``capacity()``, the constructor, the module surface, and the three entry points without a GPU."""
import ctypes
import os
import re

import pytest
import torch

import _gshard_cases as gc
import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slimmoe.h")
NEW = {"smoe_gshard_prune_workspace_bytes": 2, "smoe_gshard_prune": 11, "smoe_gshard_aux_workspace_bytes": 2, "smoe_gshard_aux": 10,
       "smoe_gshard_gate_bwd": 11}

TABLE = gc.table()


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("T", gc.TS)
def test_vectorised_restatement_equals_the_per_entry_walk(T):
    for c in (c for c in TABLE if c.T == T):
        out, top1, _, _ = gc.prune(c.idx, c.score, c.u, c.E, c.cap)
        w_out, w_top1 = gc.prune_walk(c.idx, c.score, c.u, c.E, c.cap)
        assert torch.equal(out, w_out) and torch.equal(top1, w_top1), c.id
    # no clamp, and ids outside [0, E)
    c = gc.Case(T, 8, 0.5, 2.0, True)
    idx = c.idx.clone()
    idx[::3, 1] = 8
    idx[1::5, 0] = -1
    for cap in (-1, c.cap):
        out, top1, _, _ = gc.prune(idx, c.score, c.u, c.E, cap)
        w_out, w_top1 = gc.prune_walk(idx, c.score, c.u, c.E, cap)
        assert torch.equal(out, w_out) and torch.equal(top1, w_top1), (T, cap)


def _binding(c):
    return c.rate == 0.5 or (c.offset == 2.0 and ((c.rate == 1.2 and c.E >= 8) or (c.rate == 4.0 and c.E == 32)))


def test_the_table_holds_both_regimes():
    """The regimes the module docstring of _gshard_cases states: drops of both kinds with plenty kept, and cap = 0."""
    seen_zero = 0
    for c in TABLE:
        out, _, by_cap, by_rand = gc.prune(c.idx, c.score, c.u, c.E, c.cap)
        if c.T >= 127 and _binding(c):
            assert by_cap.any(), c.id
            assert int((out >= 0).sum()) > 75, (c.id, int((out >= 0).sum()))
            if c.with_u:
                assert by_rand.any(), c.id
        if c.T <= 2 and c.E >= 8 and c.rate <= 1.2:
            assert c.cap == 0 and bool((out < 0).all()), c.id
            seen_zero += 1
    assert seen_zero == 2 * 2 * 2 * 2 * 2
    assert gc.prune(TABLE[0].idx, TABLE[0].score, TABLE[0].u, TABLE[0].E, -1)[2].sum() == 0       # capacity < 0: no clamp


def test_second_scores_are_at_most_a_half_and_the_random_compare_is_exact_in_f32():
    for c in TABLE:
        assert float(c.score[:, 1].max()) <= 0.5
        two_s = 2.0 * c.score[:, 1]
        assert torch.equal(two_s.double(), 2.0 * c.score[:, 1].double())      # a power-of-two scaling: no rounding


# ---------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("E", gc.ES)
@pytest.mark.parametrize("T", (2, 129, 513))
def test_backward_formulas_equal_float64_autograd(T, E):
    c = gc.Case(T, E, 0.5, 2.0, True)
    idx_out, top1, _, _ = gc.prune(c.idx, c.score, c.u, E, c.cap)
    ne = E // 2 if E > 2 else E                      # a local expert count that is not E (world size 2)
    for w_aux, use_ds in ((0.01, True), (0.0, True), (0.37, False)):
        l = c.logits.double().requires_grad_(True)
        w = c.dscore if use_ds else torch.zeros_like(c.dscore)
        gc.objective64(l, c.idx, idx_out, top1, ne, w, w_aux).backward()
        _, coef = gc.aux64(c.logits, top1, ne)
        s64 = torch.softmax(c.logits.double().gather(1, c.idx), dim=-1)
        got = gc.gate_bwd64(c.logits, c.idx, idx_out, s64, c.dscore if use_ds else None, coef if w_aux else None, w_aux)
        assert float((got - l.grad).abs().max()) <= 1e-14 * max(1.0, float(l.grad.abs().max())), (T, E, w_aux, use_ds)
    # the balance loss itself, against its definition written out
    aux, coef = gc.aux64(c.logits, top1, ne)
    p = torch.softmax(c.logits.double(), 1)
    want = sum((float(top1[e]) / T) * float(p[:, e].mean()) for e in range(E)) / E * ne ** 2
    assert abs(float(aux) - want) <= 1e-14
    assert torch.allclose(coef, ne ** 2 * top1.double() / (E * T * T), rtol=1e-15, atol=0)


def emulation_errors(c, ne):
    """(|aux error|, max |coef error|, max |dlogits error|, the float64 references) of the f32 emulation for one case."""
    idx_out, top1, _, _ = gc.prune(c.idx, c.score, c.u, c.E, c.cap)
    aux64, coef64 = gc.aux64(c.logits, top1, ne)
    aux32, coef32 = gc.aux_emulated(c.logits, top1, ne)
    scale = torch.tensor([0.01])
    dl64 = gc.gate_bwd64(c.logits, c.idx, idx_out, c.score, c.dscore, coef32, float(scale.double()))
    dl32 = gc.gate_bwd_emulated(c.logits, c.idx, idx_out, c.score, c.dscore, coef32, scale)
    return (abs(float(aux32.double() - aux64)), float((coef32.double() - coef64).abs().max()),
            float((dl32.double() - dl64).abs().max()), (aux64, coef64, dl64))


def test_f32_emulation_in_kernel_order_against_float64(capsys):
    """The measured maxima are printed; per case they are the source of the GPU bars (gc.bar: 3 x, and at least one f32 ulp)."""
    worst = {}
    for c in TABLE:
        if c.rate != 0.5 or not c.with_u:       # aux does not see rate / u; the backward sees them through idx_out only
            continue
        e_aux, e_coef, e_dl, (aux64, coef64, dl64) = emulation_errors(c, c.E)
        # f32 arithmetic: an error far above rounding of these O(1) sums would be a mistake in the emulation or the formulas
        assert e_aux <= 1e-5 * max(1.0, abs(float(aux64))), c.id
        assert e_coef <= 4 * gc.ulp32(float(coef64.abs().max())) if c.T else True, c.id
        assert e_dl <= 1e-5 * max(1.0, float(dl64.abs().max())), c.id
        key = (c.E, c.T)
        worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0, 0, 0)), (e_aux, e_coef, e_dl)))
    with capsys.disabled():
        print("\nGShard f32 emulation vs float64, max over offsets: (E, T) -> |aux|, max |coef|, max |dlogits|")
        for key in sorted(worst):
            print("  E=%-3d T=%-5d %.3e %.3e %.3e" % (key + worst[key]))


# ---------------------------------------------------------------------------------------------------------------- the gate
def test_capacity_values():
    g = sm.GShardGate(64, 8, 1)
    assert g.top_k == 2 and g.kind == sm.ops.GATE_NAIVE and g.tot_expert == 8
    g.train()
    assert g.capacity(197) == (237 * 2) // 8 == 59          # ceil(1.2 * 197) = 237
    assert g.capacity(1) == (2 * 2) // 8 == 0 and g.capacity(2) == (3 * 2) // 8 == 0 and g.capacity(4) == 1
    g.eval()
    assert g.capacity(197) == (473 * 2) // 8 == 118         # ceil(2.4 * 197) = 473
    g2 = sm.GShardGate(64, 4, 2, capacity=0.5)              # a scalar serves both modes; E is the global count
    assert g2.tot_expert == 8
    for mode in (True, False):
        g2.train(mode)
        assert g2.capacity(513) == (257 * 2) // 8 == 64
    for c in TABLE:
        g3 = sm.GShardGate(16, c.E, 1, capacity=c.rate)
        assert g3.capacity(c.T) == c.cap == gc.capacity(c.rate, c.T, c.E)
    assert sm.GShardGate(16, 8, 1, capacity=None).capacity(100) == -1


def test_constructor_refusals_and_uniform():
    with pytest.raises(AssertionError, match="top-2"):
        sm.GShardGate(64, 8, 1, topk=1)
    with pytest.raises(AssertionError, match="top-2"):
        sm.GShardGate(64, 8, 1, 3)
    with pytest.raises(AssertionError, match="top-2"):
        sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=1, gate="gshard")
    with pytest.raises(ValueError, match="unknown gate"):
        sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), gate="gshard2")
    g = sm.GShardGate(64, 8, 1)
    u = g.make_uniform(33, "cpu")
    assert u.shape == (33,) and u.dtype == torch.float32 and float(u.min()) >= 0 and float(u.max()) < 1
    assert sm.GShardGate(64, 8, 1, random_routing=False).make_uniform(33, "cpu") is None
    assert sm.GShardGate(64, 8, 1, gate_bias=False).gate.bias is None
    assert g.get_loss() is None and g.last_routing is None


def test_gate_string_reaches_the_module_and_a_factory_with_naive_state_dict_keys():
    naive = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2)
    mod = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2, gate="gshard")
    assert isinstance(mod.gate, sm.GShardGate) and mod.gate.capacity_factor == (1.2, 2.4) and mod.gate.random_routing
    assert list(mod.state_dict()) == list(naive.state_dict())
    assert [k for k in mod.state_dict() if k.startswith("gate.")] == ["gate.gate.weight", "gate.gate.bias"]
    mod.load_state_dict(naive.state_dict())
    pair = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2, gate="gshard", capacity_factor=(0.5, 1.0))
    assert pair.gate.capacity_factor == (0.5, 1.0)
    scalar = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2, gate="gshard", capacity_factor=0.5)
    assert scalar.gate.capacity(512) == 64
    byclass = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2, gate=sm.GShardGate)      # a passed class, positionally
    assert isinstance(byclass.gate, sm.GShardGate) and byclass.gate.top_k == 2
    model = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2, gate="gshard", capacity_factor=1.0)
    moes = [m for m in model.modules() if isinstance(m, sm.FMoETransformerMLP)]
    assert moes and all(isinstance(m.gate, sm.GShardGate) and m.gate.capacity_factor == 1.0 for m in moes)
    ref = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2)
    assert list(model.state_dict()) == list(ref.state_dict())
    # every "is this a capacity gate" decision asks capacity(): the static expert exchange's kind
    from slim_switch_moe_vit_amd import ep
    mod.force_ep = True
    assert ep.static_kind(mod, torch.float16) == "capacity"
    with pytest.raises(RuntimeError, match="GPU"):
        mod(torch.zeros(4, 64))


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_gshard_entry_points_are_declared_prototyped_and_exported_and_the_abi_stays_29():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s, n in NEW.items():
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
        assert hasattr(lib, s), f"libslimmoe_hip.so does not export {s}"
        n_args = len([a for a in re.search(r"%s\s*\((.*?)\)" % s, text, re.S).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[s][1]) == n, s
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    assert "gshard.hip" in _lib._HASHED and _lib.source_build_id() == _lib.binary_build_id()


def test_gshard_argument_checks_come_before_any_launch():
    lib = _lib.load()
    fake = 4096          # never dereferenced
    big = 1 << 24
    prune = lambda idx=fake, score=fake, u=fake, T=100, E=8, cap=10, out=fake, top1=fake, ws=fake, nb=big: \
        lib.smoe_gshard_prune(idx, score, u, T, E, cap, out, top1, ws, nb, None)                            # noqa: E731
    aux = lambda logits=fake, top1=fake, T=100, E=8, ne=8, a=fake, coef=fake, ws=fake, nb=big: \
        lib.smoe_gshard_aux(logits, top1, T, E, ne, a, coef, ws, nb, None)                                  # noqa: E731
    bwd = lambda logits=fake, idx=fake, out=fake, score=fake, ds=fake, coef=fake, cs=fake, T=100, E=8, dl=fake: \
        lib.smoe_gshard_gate_bwd(logits, idx, out, score, ds, coef, cs, T, E, dl, None)                     # noqa: E731
    err = lib.smoe_last_error
    for kw in (dict(idx=None), dict(out=None), dict(top1=None), dict(ws=None)):
        assert prune(**kw) != 0 and b"smoe_gshard_prune" in err() and b"null" in err(), kw
    assert prune(score=None) != 0 and b"scores" in err()
    assert prune(E=1) != 0 and b"top-2" in err()
    assert prune(E=257) != 0 and b"E=257" in err()
    assert prune(T=-1) != 0 and b"T=-1" in err()
    assert prune(T=1 << 30) != 0 and b"out of range" in err()
    assert prune(T=(1 << 21) + 1, E=256) != 0 and b"exceeds" in err()        # 4097 chunks x 256 experts > 2^20 table entries
    assert prune(nb=16) != 0 and b"workspace too small" in err()
    assert lib.smoe_gshard_prune_workspace_bytes(100, 8) == 2 * 1 * 8 * 4
    assert lib.smoe_gshard_prune_workspace_bytes(513, 32) == 2 * 2 * 32 * 4      # 1026 entries: two 1024-entry chunks
    for kw in (dict(logits=None), dict(top1=None), dict(a=None), dict(coef=None), dict(ws=None)):
        assert aux(**kw) != 0 and b"smoe_gshard_aux" in err() and (b"null" in err() or b"workspace" in err()), kw
    assert aux(E=1) != 0 and b"E=1" in err()
    assert aux(E=257) != 0 and b"E <= 256" in err()
    assert aux(ne=3) != 0 and b"num_expert=3" in err()
    assert aux(ne=0) != 0 and b"num_expert=0" in err()
    assert aux(nb=8) != 0 and b"workspace too small" in err()
    assert lib.smoe_gshard_aux_workspace_bytes(513, 8) == (3 + 1) * 8 * 4
    assert bwd(T=0) == 0                                                            # T == 0 returns at once
    for kw in (dict(logits=None), dict(idx=None), dict(out=None), dict(score=None), dict(dl=None)):
        assert bwd(**kw) != 0 and b"smoe_gshard_gate_bwd" in err() and b"null" in err(), kw
    assert bwd(coef=None) != 0 and b"coef_scale without coef" in err()
    assert bwd(E=1) != 0 and b"E=1" in err()
    assert bwd(E=300) != 0 and b"E=300" in err()
    with pytest.raises(_lib.SlimMoEError, match="top-2"):
        _lib.check(prune(E=1), "smoe_gshard_prune")


def test_python_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from slim_switch_moe_vit_amd import ops
    idx = torch.zeros(4, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gshard_prune(idx, torch.zeros(4, 2), None, 8, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gshard_aux(torch.zeros(4, 8), torch.zeros(8, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gshard_gate_bwd(torch.zeros(4, 8), idx, idx, torch.zeros(4, 2), None, None)
    # the k-shape refusal is the wrapper's: the GShard gate is top-2
    with pytest.raises(RuntimeError, match="top-2"):
        ops._gshard_pairs(_fake_cuda(torch.zeros(4, 1, dtype=torch.int64)), "idx", torch.int64)
    with pytest.raises(RuntimeError, match="expected 5 rows"):
        ops._gshard_pairs(_fake_cuda(torch.zeros(4, 2)), "score", torch.float32, 5)


def _fake_cuda(t):
    """A CPU tensor that says it lives on the GPU: enough for the wrappers' shape checks, which run before any launch."""
    class T(torch.Tensor):
        is_cuda = True
    return t.as_subclass(T)
