"""GPU tests of the ``--bce-loss`` criterion on the library's kernels (smoe_bce_fwd / smoe_bce_bwd): values against torch's float64
result on the host (the reference tests/test_bce_loss_host.py checks), binarisation, determinism and row independence, the size
limits on the module, the non-finite contract, launch counts, and the graphed training step.

Error units (tests/_bce_cases.py): the loss and the row sums in units of sum (|x| + 1) over what they sum (its mean per element for
the loss); the gradient as |dlogits - reference| x (B C) / g -- the error of ``sigmoid(x) - t``, a value in [-1, 1].  The bars are
at most 3 x the maxima measured on an MI355X over every case below (profiles/r14_bce_loss.md), and at most 3 x the error of torch's
own f32 device result against the same float64 values."""
import math
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bce_cases as cases
import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# dtype -> (loss, row sums, gradient): the bars; measured maxima (own / torch's f32 device result) in profiles/r14_bce_loss.md
BARS = {
    torch.float32: (1.2e-7, 1.5e-7, 3.4e-7),
    torch.float16: (1.2e-7, 1.6e-7, 3.0e-4),
    torch.bfloat16: (1.2e-7, 1.5e-7, 2.4e-3),
}
INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _bits(t):
    return t.contiguous().view(INT[t.dtype])


def _scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def _own(x, t, binarize=False, g=1.0):
    loss, rows = ops.bce_fwd(x, t, binarize)
    return loss, rows, ops.bce_bwd(x, t, _scalar(g), binarize)


def _offset_view(x):
    """The same [B, C] values one element into a larger buffer: rows of C % 8 == 0 elements that are not 16-byte aligned."""
    store = torch.zeros(x.numel() + 8, dtype=x.dtype, device=x.device)
    v = store[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------------- values against float64
@pytest.mark.parametrize("scale", cases.SCALES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_bce_values_against_float64_within_the_measured_bars(dtype, scale):
    """B in {1, 2, 7, 128} x C in {1, 3, 10, 100, 1000, 1001, 1008} (both load paths, a row shorter than a wave, C % 8 != 0) x Mixup
    rows at smoothing 0 / 0.1, {0, 1} rows and uniform rows, and for the C % 8 == 0 sizes the logits one element off their
    alignment.  g = 1 for f32 logits; g = B C for 16-bit ones (dlogits is then ``sigmoid - t`` itself, inside the type's range)."""
    own, ref32 = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for B in cases.BATCHES:
        for C in cases.CLASSES:
            g = 1.0 if dtype == torch.float32 else float(B * C)
            x_cpu = cases.logits(B, C, scale, dtype)
            x = x_cpu.to(DEV)
            unit_rows = cases.term_scale(x_cpu, None)
            unit_loss = unit_rows.sum().item() / (B * C)
            for kind in cases.KINDS:
                t_cpu = cases.targets(kind, B, C)
                t = t_cpu.to(DEV)
                l64, r64, g64 = cases.ref64(x_cpu, t_cpu, g)

                def errors(loss, rows, dx):
                    return (abs(loss.double().item() - l64.item()) / unit_loss,
                            ((rows.double().cpu() - r64).abs() / unit_rows).max().item(),
                            (dx.double().cpu() - g64).abs().max().item() * (B * C) / g)
                for xv in ((x, _offset_view(x)) if C % 8 == 0 else (x,)):
                    loss, rows, dx = _own(xv, t, False, g)
                    assert loss.dtype == torch.float32 and loss.dim() == 0 and rows.shape == (B,) and dx.dtype == dtype
                    own = [max(a, b) for a, b in zip(own, errors(loss, rows, dx))]
                # torch's own f32 result on the device (what autocast runs for 16-bit logits: f32 arithmetic, the gradient cast back)
                x32 = x.detach().clone().float().requires_grad_(True)       # (a copy: .float() of f32 logits is the tensor itself)
                l32 = F.binary_cross_entropy_with_logits(x32, t)
                (l32 * g).backward()
                with torch.no_grad():
                    rows32 = F.binary_cross_entropy_with_logits(x32, t, reduction="none").sum(1)
                ref32 = [max(a, b) for a, b in zip(ref32, errors(l32.detach(), rows32, x32.grad.to(dtype)))]
    bars = BARS[dtype]
    print(f"BCE {dtype} scale {scale}: max error own loss {own[0]:.3e} rows {own[1]:.3e} grad {own[2]:.3e} | "
          f"torch f32 loss {ref32[0]:.3e} rows {ref32[1]:.3e} grad {ref32[2]:.3e} | bars {bars}")
    assert own[0] <= bars[0] and own[1] <= bars[1] and own[2] <= bars[2], (own, bars)
    # (torch's error at THIS scale is a lower bound of its maximum over the scales, which is what the bars may be 3 x of)
    _TORCH_ERR.setdefault(dtype, {})[scale] = ref32


_TORCH_ERR = {}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_the_bars_are_within_three_times_torchs_own_error(dtype):
    """Runs after the value tests of its dtype (file order) and takes torch's errors from them; run alone, it runs them first."""
    if len(_TORCH_ERR.get(dtype, {})) < len(cases.SCALES):
        for scale in cases.SCALES:
            test_bce_values_against_float64_within_the_measured_bars(dtype, scale)
    worst = [max(e[i] for e in _TORCH_ERR[dtype].values()) for i in range(3)]
    bars = BARS[dtype]
    print(f"BCE {dtype}: torch's f32 device result, max error loss {worst[0]:.3e} rows {worst[1]:.3e} grad {worst[2]:.3e}; bars {bars}")
    assert all(bar <= 3 * w for bar, w in zip(bars, worst)), (bars, worst)


# ---------------------------------------------------------------------------------------------------------------- binarisation
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", ["mixup", "mixup_smoothed"])
def test_binarize_in_the_kernel_is_bit_equal_to_binarized_targets(kind, dtype):
    for B, C in ((2, 10), (7, 1001), (128, 1000)):
        x = cases.logits(B, C, 4.0, dtype).to(DEV)
        t = cases.targets(kind, B, C).to(DEV)
        tb = t.gt(0.0).float()
        a, b = _own(x, t, True, 512.0), _own(x, tb, False, 512.0)
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b)), (kind, B, C)
        if kind == "mixup_smoothed":          # the reference's behaviour at --smoothing 0.1: every class becomes a positive
            assert bool((tb == 1).all())
            c = _own(x, torch.ones_like(t), False, 512.0)
            assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, c))
        else:
            assert B <= int(tb.sum()) <= 2 * B and (B < 7 or not torch.equal(t, tb))


def test_binarize_rule_on_special_target_values():
    t = torch.tensor([cases.SPECIAL], dtype=torch.float32, device=DEV)
    want = torch.tensor([cases.SPECIAL_BITS], dtype=torch.float32, device=DEV)
    assert torch.equal(t.gt(0.0).type(t.dtype), want)
    x = torch.linspace(-3, 3, len(cases.SPECIAL), device=DEV).reshape(1, -1)
    a, b = _own(x, t, True), _own(x, want, False)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
    l64, r64, g64 = cases.ref64(x.cpu(), want.cpu())
    assert abs(a[0].item() - l64.item()) <= BARS[torch.float32][0] * cases.term_scale(x.cpu(), None).sum().item() / x.numel()
    assert (a[2].double().cpu() - g64).abs().max().item() * x.numel() <= BARS[torch.float32][2]
    assert math.isnan(_own(x, t, False)[0].item()), "without binarize the NaN target reaches the loss"
    crit = sm.BCEWithLogitsLoss(binarize=True)
    assert torch.equal(crit(x, t), a[0]) and torch.equal(crit(x, t.double()), a[0]), "f64 targets are binarized before the cast"
    tiny = torch.full((1, 7), 1e-60, dtype=torch.float64, device=DEV)              # positive, and 0 once rounded to f32
    assert torch.equal(crit(x, tiny), _own(x, torch.ones_like(x), False)[0])


# ------------------------------------------------------------------------------------------------ the two paths of the backward
@pytest.mark.parametrize("binarize", [False, True], ids=["raw", "binarize"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_bce_bwd_base_that_is_not_16_byte_aligned_takes_the_element_path_and_writes_the_same_bits(dtype, binarize):
    """C = 2056 = one step of 256 x 8 logits + one vector; the same logits, targets and g once on 16-byte aligned bases (8 logits per
    lane) and once with logits and dlogits 4 bytes into larger buffers (element by element)."""
    B, C = 3, 2056
    n = B * C
    words = 4 // torch.empty(0, dtype=dtype).element_size()          # elements in 4 bytes
    x = cases.logits(B, C, 4.0, dtype).to(DEV)
    t = cases.targets("mixup", B, C).to(DEV)
    g = _scalar(512.0)
    assert x.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0 and C % 8 == 0
    dx = ops.bce_bwd(x, t, g, binarize)
    assert dx.data_ptr() % 16 == 0
    store = torch.zeros(n + 16, dtype=dtype, device=DEV)
    xo = store[words:words + n].view(B, C)
    xo.copy_(x)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    out = torch.zeros(n + 16, dtype=dtype, device=DEV)
    rc = sm._lib.load().smoe_bce_bwd(xo.data_ptr(), ops.dtype_code(dtype), t.data_ptr(), int(binarize), B, C, g.data_ptr(),
                                     out.data_ptr() + 4, ops._stream(x))
    assert rc == 0
    assert torch.equal(_bits(out[words:words + n].view(B, C)), _bits(dx))
    assert bool(dx.float().abs().sum() > 0)
    assert float(out[:words].float().abs().sum()) == 0 and float(out[words + n:].float().abs().sum()) == 0, "nothing written outside dlogits"


# ------------------------------------------------------------------------------------------------- determinism and independence
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [10, 1000, 1001])
def test_two_runs_give_the_same_bits_and_a_row_does_not_depend_on_its_batch(C, dtype):
    B = 7
    x = cases.logits(B, C, 30.0, dtype).to(DEV)
    t = cases.targets("mixup", B, C).to(DEV)
    first = _own(x, t, True, float(B))
    again = _own(x, t, True, float(B))
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(first, again))
    for b in (0, 3, 6):
        # g = B for the batch and 1 for the row alone: g / (B C) is the same correctly rounded quotient 1 / C in both
        _, row, dx = _own(x[b:b + 1].clone(), t[b:b + 1].clone(), True, 1.0)
        assert torch.equal(_bits(row), _bits(first[1][b:b + 1])), (b, C)
        assert torch.equal(_bits(dx[0]), _bits(first[2][b])), (b, C)


# ------------------------------------------------------------------------------------------------------- limits, on the module
def test_module_just_below_at_and_past_the_batch_limit():
    """65534 and 65535 rows of C = 8 against the same rows in two halves (row sums and gradients bit for bit); 65536 rows take torch's
    line and give the right value."""
    C, top = 8, 65536
    g = torch.Generator(device=DEV).manual_seed(3)
    x_all = torch.randn(top, C, generator=g, device=DEV) * 3
    t_all = (torch.rand(top, C, generator=g, device=DEV) < 0.3).float() * torch.rand(top, C, generator=g, device=DEV)
    crit = sm.BCEWithLogitsLoss(binarize=True)
    for B in (65534, 65535):
        x, t = x_all[:B], t_all[:B]
        loss, rows, dx = _own(x, t, True, float(B))
        h = B // 2
        _, r1, d1 = _own(x[:h], t[:h], True, float(h))
        _, r2, d2 = _own(x[h:], t[h:], True, float(B - h))
        assert torch.equal(rows, torch.cat([r1, r2])) and torch.equal(dx, torch.cat([d1, d2])), B
        want = F.binary_cross_entropy_with_logits(x.double(), t.gt(0).double()).item()
        assert abs(loss.item() - want) <= BARS[torch.float32][0] * (x.abs().double().mean().item() + 1)
        xm = x.clone().requires_grad_(True)
        lm = crit(xm, t)
        (lm * B).backward()
        assert torch.equal(lm, loss) and torch.equal(xm.grad, dx), "the module runs the kernels up to the limit"
    xm = x_all.clone().requires_grad_(True)
    lm = crit(xm, t_all)
    lm.backward()
    x32 = x_all.clone().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(x32, t_all.gt(0.0).float())
    want.backward()
    assert torch.equal(lm, want) and torch.equal(xm.grad, x32.grad), "past the limit: torch's line, after the gt line"
    with pytest.raises(sm._lib.SlimMoEError, match="65535"):
        ops.bce_fwd(x_all, t_all, True)


def test_module_falls_back_for_weights_and_other_reductions_and_takes_any_leading_shape():
    x = cases.logits(7, 10, 3.0).to(DEV)
    t = cases.targets("uniform", 7, 10).to(DEV)
    w = torch.rand(10, device=DEV) + 0.5
    for kw in (dict(weight=w), dict(pos_weight=w), dict(reduction="sum"), dict(reduction="none")):
        assert torch.equal(sm.BCEWithLogitsLoss(**kw)(x, t), torch.nn.BCEWithLogitsLoss(**kw)(x, t)), kw
    loss3 = sm.BCEWithLogitsLoss()(x.view(7, 2, 5), t.view(7, 2, 5))           # [7, 2, 5]: rows of 5, the same mean
    l64 = cases.ref64(x.cpu(), t.cpu())[0].item()
    assert abs(loss3.item() - l64) <= BARS[torch.float32][0] * (x.abs().mean().item() + 1)
    with torch.autocast("cuda", dtype=torch.float16):
        xh = x.half().requires_grad_(True)
        lh = sm.BCEWithLogitsLoss()(xh, t)
        assert lh.dtype == torch.float32
    lh.backward()
    assert xh.grad.dtype == torch.float16 and torch.equal(lh, ops.bce_fwd(x.half(), t)[0])


# ------------------------------------------------------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("poison", ["+inf", "-inf", "nan"])
def test_non_finite_logits_poison_their_row_loss_and_their_own_gradient_element_only(poison, target, dtype):
    B, C, row, col = 6, 1000, 2, 37
    x = cases.logits(B, C, 3.0, dtype).to(DEV)
    t = cases.targets("binary", B, C).to(DEV)
    t[row, col] = target
    _, clean_rows, clean_dx = _own(x, t)
    xp = x.clone()
    xp[row, col] = float(poison)
    loss, rows, dx = _own(xp, t)
    l64, r64, _ = cases.ref64(xp.cpu(), t.cpu())
    assert torch.equal(torch.isfinite(rows).cpu(), torch.isfinite(r64)), "finite exactly where float64 is"
    assert math.isfinite(loss.item()) == math.isfinite(l64.item()) and not math.isfinite(loss.item())
    others = [r for r in range(B) if r != row]
    assert torch.equal(rows[others], clean_rows[others])
    assert not math.isfinite(float(dx[row, col]))
    keep = torch.ones(B, C, dtype=torch.bool, device=DEV)
    keep[row, col] = False
    assert torch.equal(_bits(dx)[keep], _bits(clean_dx)[keep]), "every other gradient element keeps the clean run's bits"


# ---------------------------------------------------------------------------------------------------------------- launch counts
def _kernels(fn):
    """name -> count of the device kernels ``fn`` launches (``fn`` has already run once outside the profiler)."""
    from torch.profiler import profile, ProfilerActivity
    calls = {}
    for _attempt in range(3):      # (only an EMPTY trace is asked for again, never a failing step)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        calls = {e.key: e.count for e in prof.key_averages()}
        if any(not n.startswith("hip") for n in calls):
            break
    return {n: c for n, c in calls.items() if not n.startswith("hip") and not n.startswith("Memcpy") and not n.startswith("Memset")}


def test_criterion_is_two_launches_forward_and_one_backward():
    x = cases.logits(128, 1000, 3.0, torch.float16).to(DEV).requires_grad_(True)
    t = cases.targets("mixup", 128, 1000).to(DEV)
    crit = sm.BCEWithLogitsLoss(binarize=True)
    g = _scalar(1024.0)
    state = {}

    def fwd():
        state["loss"] = crit(x, t)

    def bwd():
        torch.autograd.grad(state["loss"], x, g, retain_graph=True)
    fwd(), bwd()
    kf, kb = _kernels(fwd), _kernels(bwd)
    assert sum(kf.values()) == 2 and any("bce_fwd_kernel" in n for n in kf) and any("bce_mean_kernel" in n for n in kf), kf
    assert sum(kb.values()) == 1 and any("bce_bwd_kernel" in n for n in kb), kb


def _linear_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 8 * 8, 16)).to(DEV)


def test_train_one_epoch_with_the_own_criterion_launches_no_gt_or_cast_on_the_targets():
    """The kernels of engine.py:50's line are found by running it: with the own criterion (binarize=True) ``args.bce_loss`` adds none
    of them to the epoch; with ``torch.nn.BCEWithLogitsLoss`` it still adds one of each per step -- the unchanged path."""
    tt = cases.targets("mixup", 8, 16).to(DEV)
    tt.gt(0.0).type(tt.dtype)
    line = set(_kernels(lambda: tt.gt(0.0).type(tt.dtype)))
    assert len(line) == 2, line
    gen = torch.Generator().manual_seed(1)
    data = [(torch.randn(8, 3, 8, 8, generator=gen), torch.randint(0, 16, (8,), generator=gen)) for _ in range(3)]

    def epoch(crit, flag):
        model = _linear_model()
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        np.random.seed(2)
        mix = sm.Mixup(0.8, 1.0, label_smoothing=0.0, num_classes=16)
        return lambda: sm.train_one_epoch(model, crit, data, opt, DEV, 0, sm.NativeScaler(), None, None, mix,
                                          args=SimpleNamespace(bce_loss=flag))

    def count(crit, flag):
        run = epoch(crit, flag)
        run()
        k = _kernels(run)
        return {n: k.get(n, 0) for n in line}, k
    own, k_own = count(sm.BCEWithLogitsLoss(binarize=True), True)
    base, _ = count(sm.BCEWithLogitsLoss(binarize=True), False)
    ref, _ = count(torch.nn.BCEWithLogitsLoss(), True)
    assert own == base, (own, base)
    assert all(ref[n] == base[n] + 3 for n in line), (ref, base)
    assert sum(c for n, c in k_own.items() if "bce_fwd_kernel" in n) == 3 and sum(c for n, c in k_own.items() if "bce_bwd_kernel" in n) == 3


# ---------------------------------------------------------------------------------------------------------------------- capture
KW = dict(depth=2, num_classes=10, img_size=64)


def _moe_model(name):
    torch.manual_seed(0)
    model = sm.resmoe.patch_blocks_with_moe(sm.create_model(name, **KW), 8, 2, True, starting_threshold=0.55, target_threshold=0.5)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if "_gate.head.1.weight" in n_:
                p.normal_(0, 0.3, generator=torch.Generator().manual_seed(5))
    return model.to(DEV)


def _teacher():
    torch.manual_seed(1)
    t = sm.create_model("deit_tiny_patch16_224", depth=1, num_classes=10, img_size=64).to(DEV).eval()
    for p in t.parameters():
        p.requires_grad_(False)
    return t


@pytest.mark.parametrize("wrapped", [False, True], ids=["bare", "distillation-hard"])
def test_graphed_training_step_with_the_bce_criterion_reproduces_the_eager_harness(wrapped):
    g = torch.Generator().manual_seed(70)
    batches = [(torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(6)]

    def run(graph):
        model = _moe_model("deit_tiny_distilled_patch16_224" if wrapped else "deit_tiny_patch16_224")
        opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
        crit = sm.BCEWithLogitsLoss(binarize=True)
        if wrapped:
            crit = sm.DistillationLoss(crit, _teacher(), "hard", 0.5, 1.0)
        np.random.seed(123)
        mix = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.0, num_classes=10)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            stats = sm.train_one_epoch(model, crit, [(x.clone(), y) for x, y in batches], opt, DEV, 0, sm.NativeScaler(), 1.0, None, mix,
                                       args=SimpleNamespace(bce_loss=True), hip_graph=graph)
        ours = [str(w.message) for w in caught if "HIP graph" in str(w.message) or "captured" in str(w.message)
                or "eagerly" in str(w.message) or "fallback" in str(w.message) or "libslimmoe_hip" in str(w.message)]
        assert not ours, ours
        return stats, {k: v.detach().clone() for k, v in model.state_dict().items()}

    s_e, p_e = run(False)
    s_g, p_g = run(True)
    assert s_g["hip_graph_steps"] == 3 and s_e["hip_graph_steps"] == 0, (s_g, s_e)
    assert s_g["loss"] == s_e["loss"] and math.isfinite(s_g["loss"]), (s_g, s_e)
    assert all(torch.equal(p_e[k], p_g[k]) for k in p_e), "parameters after 3 eager + 3 replayed steps against 6 eager steps"
    fresh = _moe_model("deit_tiny_distilled_patch16_224" if wrapped else "deit_tiny_patch16_224").state_dict()
    assert not torch.equal(p_e["head.weight"], fresh["head.weight"]), "the head trains"
