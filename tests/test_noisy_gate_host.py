"""CPU tests of the noisy top-k gate (fmoe.gates.NoisyGate; the rule is restated in INTEGRATION.md): the vectorised float64
restatement of tests/_noisy_gate_cases.py against a literal row-by-row walk of the rule, the tie-free margin of every row of the case
table, the f32 emulation of smoe_noisy_gate_fwd / _bwd against float64 (its measured error is where the GPU bars come from), the
module's CPU composition against the restatement, the constructor, the state dict, ``gate="noisy"`` and the entry points without a
GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

import _noisy_gate_cases as nc
import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slimmoe.h")
NEW = {"smoe_noisy_gate_workspace_bytes": 2, "smoe_noisy_gate_fwd": 18, "smoe_noisy_gate_bwd": 15}

_TABLE = {}


def _cases(T):
    if T not in _TABLE:
        _TABLE[T] = nc.table((T,))
    return _TABLE[T]


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("T", nc.TS)
def test_every_row_of_every_case_is_tie_free_and_the_regimes_are_what_they_say(T):
    cases = _cases(T)
    assert len(cases) == len(nc.EKS) * len(nc.REGIMES)
    for c in cases:
        clean, raw, sigma, noisy = nc.noisy64(c.logits2, c.eps)
        assert float(nc.min_margin(noisy).min()) > nc.MARGIN, c.id          # no row excluded
        assert c.logits2.shape == (T, 2 * c.E) and c.eps.shape == (T, c.E) and c.k < c.E
        if c.regime == "sat":
            assert float(sigma.median()) < 0.012           # softplus(-8) = 3.4e-4 on top of the 0.01
        elif c.regime == "lin":
            lin = raw > 20.0                               # (a 5-sigma draw may fall below the threshold: both branches in one case)
            assert float(lin.double().mean()) > 0.99 and torch.equal(sigma[lin], raw[lin] + nc.NOISE_EPS)
        elif c.regime == "zero":
            assert float(raw.abs().max()) == 0.0 and abs(float(sigma[0, 0]) - (math.log(2.0) + nc.NOISE_EPS)) < 1e-15


@pytest.mark.parametrize("T", (1, 2, 65))
def test_vectorised_restatement_equals_the_literal_walk_of_the_rule(T):
    for c in _cases(T):
        for training, eps in ((True, c.eps), (True, None), (False, c.eps)):
            r = nc.forward64(c.logits2, eps, c.k, training)
            idx, score, imp, load, aux = nc.forward_literal(c.logits2, eps, c.k, training)
            assert torch.equal(r["idx"], idx), c.id
            for a, b in ((r["score"], score), (r["imp"], imp), (r["load"], load), (r["aux"], torch.tensor(aux, dtype=torch.float64))):
                assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), c.id
    # ties go to the lowest expert id
    l2 = torch.zeros(1, 8)
    assert nc.forward64(l2, None, 2)["idx"].tolist() == [[0, 1]] and int(nc.forward64(l2, None, 2)["next"]) == 2


@pytest.mark.parametrize("T", (2, 65, 257))
def test_f32_emulation_against_float64_and_its_backward_against_autograd(T):
    """The emulation restates the kernels' formulas (rule 7 written out by hand); float64 autograd over the restatement is the oracle.
    An error far above f32 rounding would be a wrong formula, not rounding."""
    for c in _cases(T):
        r = nc.forward64(c.logits2, c.eps, c.k)
        ci, cl = nc.coefs64(r["imp"], r["load"])
        f = nc.fwd_emulated(c.logits2, c.eps, c.k)
        assert torch.equal(f["idx"], r["idx"]) and torch.equal(f["next"], r["next"]), c.id
        tol = lambda ref: 2e-5 * max(1.0, float(ref.abs().max()))          # noqa: E731
        for name, ref in (("score", r["score"]), ("imp", r["imp"]), ("load", r["load"]), ("aux", r["aux"]), ("coef_imp", ci),
                          ("coef_load", cl)):
            assert float((f[name].double() - ref).abs().max()) <= max(tol(ref), 1e-4 * float(ref.abs().max())), (c.id, name)
        for ds, sc in ((c.dscore, c.scale), (c.dscore, None), (None, c.scale)):
            ref = nc.backward64(c.logits2, c.eps, c.k, ds, sc)
            emu = nc.bwd_emulated(c.logits2, c.eps, c.k, f, ds, sc)
            assert float((emu.double() - ref).abs().max()) <= max(tol(ref), 1e-3 * float(ref.abs().max())), (c.id, ds is None, sc is None)
        # eval: sigma = 0, no load term, raw gets no gradient
        ref = nc.backward64(c.logits2, None, c.k, c.dscore, c.scale, training=False)
        fe = nc.fwd_emulated(c.logits2, None, c.k, training=False)
        emu = nc.bwd_emulated(c.logits2, None, c.k, fe, c.dscore, c.scale, training=False)
        assert float(ref[:, c.E:].abs().max()) == 0.0 and float(emu[:, c.E:].abs().max()) == 0.0
        assert float((emu.double() - ref).abs().max()) <= max(tol(ref), 1e-3 * float(ref.abs().max())), c.id


# ---------------------------------------------------------------------------------------------------------------- the module
def test_constructor_state_dict_and_refusals():
    g = sm.NoisyGate(64, 4, 2, top_k=2)
    assert g.tot_expert == 8 and g.num_expert == 4 and g.world_size == 2 and g.top_k == 2 and g.noise_epsilon == 1e-2
    assert list(g.state_dict()) == ["w_gate", "w_noise"]
    assert g.w_gate.shape == (64, 8) and g.w_noise.shape == (64, 8) and g.w_gate.dtype == torch.float32
    bound = 1.0 / math.sqrt(8)                        # kaiming_uniform_(a=sqrt(5)) on [64, 8]: fan_in = 8
    assert float(g.w_gate.detach().abs().max()) <= bound and 0 < float(g.w_noise.detach().abs().max()) <= bound
    assert g.capacity(1000) == -1 and g.get_loss() is None
    assert g.make_noise(33, "cpu").shape == (33, 8)
    assert sm.NoisyGate(64, 8, 1).top_k == 2
    for E, k in ((2, 2), (4, 4), (4, 5), (4, 0)):
        with pytest.raises(ValueError, match="top_k"):
            sm.NoisyGate(64, E, 1, top_k=k)
    # what the naive paths read: the [E, d] image of w_gate, no bias, cached per parameter version, not a sub-module
    img = g.gate
    assert img.bias is None and torch.equal(img.weight, g.w_gate.detach().t()) and img.weight.is_contiguous()
    assert g.gate.weight is img.weight and not img.weight.requires_grad
    with torch.no_grad():
        g.w_gate.add_(1.0)
    assert torch.equal(g.gate.weight, g.w_gate.detach().t())
    assert [n for n, _ in g.named_modules()] == [""] and g.image2().shape == (16, 64)
    assert torch.equal(g.image2(), torch.cat((g.w_gate.t(), g.w_noise.t()), 0))


def test_gate_string_reaches_the_module_and_a_factory_and_fastmoe_keys_load():
    mod = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2, gate="noisy")
    assert isinstance(mod.gate, sm.NoisyGate) and mod.gate.top_k == 2
    assert [k for k in mod.state_dict() if k.startswith("gate.")] == ["gate.w_gate", "gate.w_noise"]
    ckpt = {k: torch.randn_like(v) for k, v in mod.state_dict().items()}
    mod.load_state_dict(ckpt)
    assert torch.equal(mod.gate.gate.weight, ckpt["gate.w_gate"].t())           # the image follows a loaded checkpoint
    byclass = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2, gate=sm.NoisyGate)
    assert isinstance(byclass.gate, sm.NoisyGate)
    assert all(p.dp_comm == "none" for p in mod.gate.parameters())
    with pytest.raises(ValueError, match="top_k"):
        sm.FMoETransformerMLP(2, 64, 128, torch.nn.GELU(), top_k=2, gate="noisy")
    model = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2, gate="noisy")
    moes = [m for m in model.modules() if isinstance(m, sm.FMoETransformerMLP)]
    assert moes and all(isinstance(m.gate, sm.NoisyGate) for m in moes)
    keys = [k for k in model.state_dict() if ".gate." in k]
    assert keys and all(k.endswith(("gate.w_gate", "gate.w_noise")) for k in keys)
    # no capacity: every "is this a capacity gate" decision comes out as for the NaiveGate
    from slim_switch_moe_vit_amd import ep
    naive = sm.FMoETransformerMLP(8, 64, 128, torch.nn.GELU(), top_k=2)
    mod.force_ep = naive.force_ep = True
    assert ep.static_kind(mod, torch.float16) == ep.static_kind(naive, torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        mod(torch.zeros(4, 64))


@pytest.mark.parametrize("E,k", [(8, 2), (4, 1), (40, 5)])
def test_cpu_composition_forward_and_backward_against_the_restatement(E, k):
    d, T = 32, 67
    torch.manual_seed(3)
    g = sm.NoisyGate(d, E, 1, top_k=k).double()
    x = torch.randn(T, d, dtype=torch.float64, requires_grad=True)
    eps = torch.randn(T, E, dtype=torch.float64)
    w = torch.randn(T, k, dtype=torch.float64)
    idx, score = g(x, eps)
    aux = g.get_loss()
    assert aux is not None and aux.requires_grad
    ((score * w).sum() + 0.3 * aux).backward()
    xl = x.detach().clone().requires_grad_(True)
    wg, wn = (p.detach().clone().requires_grad_(True) for p in (g.w_gate, g.w_noise))
    r = nc.forward64(torch.cat((xl @ wg, xl @ wn), 1), eps, k)
    ((r["score"] * w).sum() + 0.3 * r["aux"]).backward()
    assert torch.equal(idx, r["idx"])
    for a, b in ((score, r["score"]), (aux, r["aux"]), (x.grad, xl.grad), (g.w_gate.grad, wg.grad), (g.w_noise.grad, wn.grad)):
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))
    assert float(g.w_noise.grad.abs().max()) > 0
    # eval: sigma = 0 -- the top-k of x @ w_gate, the importance term alone, no gradient for w_noise; no grad: no loss
    g.eval().zero_grad()
    idx_e, score_e = g(x.detach().requires_grad_(True))
    val, want = torch.topk(x.detach() @ g.w_gate.detach(), k, dim=1)
    assert torch.equal(idx_e, want) and torch.allclose(score_e, torch.softmax(val, -1))
    r = nc.forward64(torch.cat((x.detach() @ g.w_gate.detach(), x.detach() @ g.w_noise.detach()), 1), None, k, training=False)
    assert abs(float(g.get_loss()) - float(r["aux"])) <= 1e-12
    with torch.no_grad():
        g(x)
    assert g.get_loss() is None


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_noisy_gate_entry_points_are_declared_prototyped_and_exported_and_the_abi_stays_29():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s, n in NEW.items():
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
        assert hasattr(lib, s), f"libslimmoe_hip.so does not export {s}"
        n_args = len([a for a in re.search(r"%s\s*\((.*?)\)" % s, text, re.S).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[s][1]) == n, s
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    assert "noisy_gate.hip" in _lib._HASHED and _lib.source_build_id() == _lib.binary_build_id()


def test_noisy_gate_argument_checks_come_before_any_launch():
    lib = _lib.load()
    fake = 4096          # never dereferenced
    big = 1 << 24

    def fwd(l2=fake, eps=fake, T=100, E=8, k=2, idx=fake, score=fake, keep=fake, nxt=fake, imp=fake, load=fake, aux=fake, ci=fake,
            cl=fake, ws=fake, nb=big):
        return lib.smoe_noisy_gate_fwd(l2, eps, T, E, k, 1, idx, score, keep, nxt, imp, load, aux, ci, cl, ws, nb, None)

    def bwd(l2=fake, eps=fake, idx=fake, keep=fake, nxt=fake, ds=fake, ci=fake, cl=fake, cs=fake, T=100, E=8, k=2, out=fake):
        return lib.smoe_noisy_gate_bwd(l2, eps, idx, keep, nxt, ds, ci, cl, cs, T, E, k, 1, out, None)

    err = lib.smoe_last_error
    for fn, who in ((fwd, b"smoe_noisy_gate_fwd"), (bwd, b"smoe_noisy_gate_bwd")):
        assert fn(E=1) != 0 and who in err() and b"E=1 " in err()
        assert fn(E=33) != 0 and who in err() and b"E=33" in err()
        assert fn(k=0) != 0 and who in err() and b"k=0" in err()
        assert fn(k=5) != 0 and who in err() and b"k=5" in err()
        assert fn(E=4, k=4) != 0 and who in err() and b"k < E=4" in err()            # k = E
        assert fn(E=2, k=2) != 0 and who in err() and b"k=2" in err()
        assert fn(T=-1) != 0 and who in err() and b"T=-1" in err()
        assert fn(T=(1 << 32) + 1) != 0 and who in err() and b"out of range" in err()
    for kw in (dict(l2=None), dict(idx=None), dict(score=None), dict(keep=None), dict(nxt=None), dict(imp=None), dict(load=None),
               dict(aux=None), dict(ci=None), dict(cl=None)):
        assert fwd(**kw) != 0 and b"smoe_noisy_gate_fwd" in err() and b"null" in err(), kw
    assert fwd(ws=None) != 0 and b"workspace" in err()
    assert fwd(nb=16) != 0 and b"workspace too small" in err()
    assert fwd(T=257, nb=lib.smoe_noisy_gate_workspace_bytes(257, 8) - 1) != 0 and b"workspace too small" in err()
    assert lib.smoe_noisy_gate_workspace_bytes(100, 8) == (1 + 1) * 16 * 8
    assert lib.smoe_noisy_gate_workspace_bytes(257, 32) == (2 + 1) * 64 * 8          # two 256-row chunks
    assert bwd(T=0) == 0                                                              # T == 0 returns at once
    for kw in (dict(l2=None), dict(idx=None), dict(keep=None), dict(nxt=None), dict(out=None)):
        assert bwd(**kw) != 0 and b"smoe_noisy_gate_bwd" in err() and b"null" in err(), kw
    assert bwd(ci=None) != 0 and b"coef_scale without" in err()
    assert bwd(cl=None) != 0 and b"coef_scale without" in err()
    with pytest.raises(_lib.SlimMoEError, match="E=33"):
        _lib.check(fwd(E=33), "smoe_noisy_gate_fwd")


def test_python_wrappers_refuse_cpu_tensors():
    from slim_switch_moe_vit_amd import ops
    assert ops.noisy_gate_supported(8, 2) and ops.noisy_gate_supported(32, 4) and ops.noisy_gate_supported(2, 1)
    assert not any(ops.noisy_gate_supported(E, k) for E, k in ((1, 1), (33, 2), (8, 0), (8, 5), (4, 4)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.noisy_gate_fwd(torch.zeros(4, 16), None, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.noisy_gate_bwd(torch.zeros(4, 16), None, torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, 2, dtype=torch.float64),
                           torch.zeros(4, dtype=torch.int32), None, None, None)
