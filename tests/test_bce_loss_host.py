"""CPU tests of the ``--bce-loss`` criterion (main.py:663-664 ``torch.nn.BCEWithLogitsLoss``; engine.py:49-50 the target rewrite): the two
entry points without a GPU, ``BCEWithLogitsLoss`` on its torch lines, the ``binarize`` rule, a float64 emulation of the kernels'
arithmetic against torch's float64 result on the rows the GPU tests use, and ``train_one_epoch`` with ``args.bce_loss``."""
import ctypes
import inspect
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bce_cases as cases
import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slimmoe.h")
NEW = ["smoe_bce_fwd", "smoe_bce_bwd"]


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_bce_entry_points_are_declared_prototyped_and_exported_and_the_abi_is_29():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
        assert hasattr(lib, s), f"libslimmoe_hip.so does not export {s}"
        n_args = len([a for a in re.search(r"%s\s*\((.*?)\)" % s, text, re.S).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[s][1]) == 9, s
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30


def test_bce_argument_checks_come_before_any_launch():
    lib = _lib.load()
    fake = 4096          # never dereferenced
    fwd = lambda logits=fake, dtype=0, target=fake, B=4, C=10, rows=fake, loss=fake: \
        lib.smoe_bce_fwd(logits, dtype, target, 1, B, C, rows, loss, None)                                  # noqa: E731
    bwd = lambda logits=fake, dtype=0, target=fake, B=4, C=10, g=fake, out=fake: \
        lib.smoe_bce_bwd(logits, dtype, target, 1, B, C, g, out, None)                                      # noqa: E731
    for f, name in ((fwd, b"smoe_bce_fwd"), (bwd, b"smoe_bce_bwd")):
        assert f(B=0) == 0                                                                                  # B == 0 returns at once
        assert f(logits=None) != 0 and b"null" in lib.smoe_last_error() and name in lib.smoe_last_error()
        assert f(target=None) != 0 and b"null" in lib.smoe_last_error()
        assert f(dtype=7) != 0 and b"dtype" in lib.smoe_last_error()
        assert f(dtype=-1) != 0 and b"dtype" in lib.smoe_last_error()
        assert f(C=0) != 0 and b"C <= 2^30" in lib.smoe_last_error()
        assert f(C=(1 << 30) + 1) != 0 and b"C <= 2^30" in lib.smoe_last_error()
        assert f(B=65536) != 0 and b"65535" in lib.smoe_last_error()
        assert f(B=-1) != 0
        assert f(target=fake + 2) != 0 and b"misaligned" in lib.smoe_last_error()
        assert f(logits=fake + 2) != 0 and b"misaligned" in lib.smoe_last_error()                           # f32 logits on 2 bytes
        assert f(logits=fake + 1, dtype=1) != 0 and b"misaligned" in lib.smoe_last_error()
    assert fwd(rows=None) != 0 and b"null" in lib.smoe_last_error()
    assert fwd(loss=None) != 0 and b"null" in lib.smoe_last_error()
    assert fwd(loss=fake + 1) != 0 and b"misaligned" in lib.smoe_last_error()
    assert bwd(g=None) != 0 and b"null" in lib.smoe_last_error()
    assert bwd(out=None) != 0 and b"null" in lib.smoe_last_error()
    assert bwd(g=fake + 2) != 0 and b"misaligned" in lib.smoe_last_error()
    with pytest.raises(_lib.SlimMoEError, match="65535"):
        _lib.check(fwd(B=65536), "smoe_bce_fwd")


# ------------------------------------------------------------------------------------------------------------ the module on CPU tensors
def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def test_surface_is_upstreams_plus_a_keyword_only_binarize():
    params = list(inspect.signature(sm.BCEWithLogitsLoss.__init__).parameters.values())[1:]
    up = list(inspect.signature(torch.nn.BCEWithLogitsLoss.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params[:-1]] == [(p.name, p.default) for p in up]
    assert params[-1].name == "binarize" and params[-1].kind is params[-1].KEYWORD_ONLY and params[-1].default is False
    crit = sm.BCEWithLogitsLoss()
    assert isinstance(crit, torch.nn.BCEWithLogitsLoss) and sm.BCEWithLogitsLoss is sm.loss.BCEWithLogitsLoss
    assert crit.binarize is False and crit.reduction == "mean" and crit.weight is None and crit.pos_weight is None
    assert sm.BCEWithLogitsLoss(binarize=True).binarize is True
    with pytest.raises(TypeError):
        sm.BCEWithLogitsLoss(None, None, None, "mean", None, True)


@pytest.mark.parametrize("binarize", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(reduction="sum"), dict(reduction="none"), dict(weight=True), dict(pos_weight=True),
                                dict(weight=True, pos_weight=True, reduction="sum")], ids=lambda k: "-".join(sorted(k)) or "mean")
def test_on_cpu_tensors_it_is_torchs_line_bit_for_bit(kw, binarize):
    B, C = 7, 10
    g = torch.Generator().manual_seed(3)
    kw = dict(kw)
    if kw.get("weight"):
        kw["weight"] = torch.rand(C, generator=g) + 0.5
    if kw.get("pos_weight"):
        kw["pos_weight"] = torch.rand(C, generator=g) + 0.5
    t = cases.targets("mixup_smoothed" if binarize else "uniform", B, C)
    t[0, :len(cases.SPECIAL)] = torch.tensor(cases.SPECIAL) if binarize else t[0, :len(cases.SPECIAL)]
    x = cases.logits(B, C, 4.0).requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    got = sm.BCEWithLogitsLoss(binarize=binarize, **kw)(x, t)
    want = torch.nn.BCEWithLogitsLoss(**kw)(x2, t.gt(0.0).type(t.dtype) if binarize else t)
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    got.sum().backward()
    want.sum().backward()
    assert torch.equal(_bits(x.grad), _bits(x2.grad))


def test_a_target_that_needs_a_gradient_takes_torchs_line_and_gets_it():
    x, t = cases.logits(2, 3, 2.0), cases.targets("uniform", 2, 3).requires_grad_(True)
    sm.BCEWithLogitsLoss()(x, t).backward()
    t2 = t.detach().clone().requires_grad_(True)
    F.binary_cross_entropy_with_logits(x, t2).backward()
    assert torch.equal(t.grad, t2.grad) and float(t.grad.abs().max()) > 0


def test_the_binarize_rule_on_special_values():
    """engine.py:50's strict ``> 0``: -0.0, 0.0, a negative value and NaN give 0; the smallest subnormal and 0.1 / 1000 give 1."""
    t = torch.tensor([cases.SPECIAL], dtype=torch.float32)
    assert t[0, 3].item() > 0 and t[0, 3].item() < 1e-44, "1e-45 is the smallest f32 subnormal, not 0"
    want = torch.tensor([cases.SPECIAL_BITS])
    assert torch.equal(t.gt(0.0).type(t.dtype), want)
    x = torch.linspace(-3, 3, len(cases.SPECIAL)).reshape(1, -1)
    assert torch.equal(sm.BCEWithLogitsLoss(binarize=True)(x, t), F.binary_cross_entropy_with_logits(x, want))
    assert torch.equal(cases.emulate64(x, t, True)[1], cases.emulate64(x, want, False)[1])
    assert math.isnan(sm.BCEWithLogitsLoss()(x, t).item()), "without binarize the NaN target reaches the loss"
    # a label-smoothed Mixup row has no zero: every target binarizes to 1 (the reference's behaviour at --smoothing 0.1)
    ts = cases.targets("mixup_smoothed", 8, 10)
    assert bool((ts > 0).all()) and torch.equal(ts.gt(0.0).type(ts.dtype), torch.ones(8, 10))
    t0 = cases.targets("mixup", 8, 10)
    assert 8 <= int((t0 > 0).sum()) <= 16 and bool(((t0 > 0) & (t0 < 1)).any()), "one or two classes per row, mixed rows among them"


# ------------------------------------------------------------------------------------ the kernels' arithmetic, in float64, against torch
@pytest.mark.parametrize("scale", cases.SCALES)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_float64_emulation_of_the_kernel_arithmetic_matches_torchs_float64_result(kind, scale):
    """What the GPU bars are anchored to: on the GPU tests' rows the two float64 computations agree to a few float64 roundings.  Measured maxima
    over all cases: loss 2.16e-16 and row sums 1.91e-16 in units of cases.term_scale, (B C) x the gradient (a difference of two values
    in [0, 1]) 3.28e-16; the bars are at most 3 x those."""
    worst = [0.0, 0.0, 0.0]
    for B in cases.BATCHES:
        for C in cases.CLASSES:
            x, t = cases.logits(B, C, scale), cases.targets(kind, B, C)
            for binarize in ((False,) if kind == "uniform" else (False, True)):
                tb = t.gt(0.0).type(t.dtype) if binarize else t         # the rule applied by hand for torch
                loss, rows, grad = cases.ref64(x, tb)
                e_loss, e_rows, e_grad = cases.emulate64(x, t, binarize)
                unit = cases.term_scale(x, tb)
                worst[0] = max(worst[0], abs(e_loss.item() - loss.item()) / unit.mean().item() * C)
                worst[1] = max(worst[1], ((e_rows - rows).abs() / unit).max().item())
                worst[2] = max(worst[2], (e_grad - grad).abs().max().item() * B * C)
    print(f"float64 emulation vs torch float64 ({kind}, scale {scale}): loss {worst[0]:.2e} rows {worst[1]:.2e} grad x BC {worst[2]:.2e}")
    assert worst[0] <= 6e-16 and worst[1] <= 5.5e-16 and worst[2] <= 9e-16, worst


# ------------------------------------------------------------------------------------------------------------------- the harness
def _tiny():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 4 * 4, 10))


class _RefBCE(torch.nn.Module):
    """What the reference runs under --bce-loss: its criterion, after engine.py:49-50's line (applied by the harness)."""

    def __init__(self):
        super().__init__()
        self.crit = torch.nn.BCEWithLogitsLoss()

    def forward(self, outputs, targets):
        assert bool(((targets == 0) | (targets == 1)).all()), "the harness applied engine.py:50 before the criterion"
        return self.crit(outputs, targets)


@pytest.mark.parametrize("wrapped", [False, True], ids=["bare", "distillation-none"])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_train_one_epoch_with_bce_loss_own_criterion_equals_the_references_lines(smoothing, wrapped):
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(4, 3, 4, 4, generator=g), torch.randint(0, 10, (4,), generator=g)) for _ in range(3)]
    args = SimpleNamespace(bce_loss=True)
    seen = []

    class _Spy(sm.BCEWithLogitsLoss):
        def forward(self, input, target):
            seen.append(target.detach().clone())
            return super().forward(input, target)

    def run(crit):
        model = _tiny()
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        np.random.seed(1)
        if wrapped:
            crit = sm.DistillationLoss(crit, None, "none", 0.5, 1.0)
        batches = [(x.clone(), y.clone()) for x, y in data]       # (Mixup works in place, and a CPU batch is not copied on its way in)
        stats = sm.train_one_epoch(model, crit, batches, opt, "cpu", 0, sm.NativeScaler(), None, None,
                                   sm.Mixup(0.8, 1.0, label_smoothing=smoothing, num_classes=10), args=args, autocast=False)
        return stats, [p.detach().clone() for p in model.parameters()]

    s_own, p_own = run(_Spy(binarize=True))
    s_ref, p_ref = run(_RefBCE())
    assert s_own["steps"] == s_ref["steps"] == 3 and s_own["loss"] == s_ref["loss"] and np.isfinite(s_own["loss"])
    assert all(torch.equal(a, b) for a, b in zip(p_own, p_ref))
    assert len(seen) == 3 and not all(bool(((t == 0) | (t == 1)).all()) for t in seen), "the own criterion got the raw Mixup rows"
    # the own criterion WITHOUT binarize keeps today's line: the harness binarizes for it
    seen.clear()
    s_plain, p_plain = run(_Spy())
    assert all(bool(((t == 0) | (t == 1)).all()) for t in seen) and s_plain["loss"] == s_ref["loss"]
    assert all(torch.equal(a, b) for a, b in zip(p_plain, p_ref))
