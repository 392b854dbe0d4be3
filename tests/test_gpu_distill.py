"""GPU tests of DeiT distillation on the library's kernels: smoe_embed_ln2 bit-equal to its torch lines and to smoe_embed_ln,
smoe_distill_fwd / smoe_distill_bwd against float64 with bars taken from torch's own f32 composition of the reference's lines on the same
inputs (the rule of test_gpu_mixup_loss.py), ties, misaligned bases, the non-finite contract, and the distilled model in a training
step, the graphed harness and the eval forward."""
import math
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distill", "ref_distill_loss.npz")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------- smoe_embed_ln2
@pytest.mark.parametrize("tok_dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,P", [(1, 1), (3, 4), (130, 196)])
@pytest.mark.parametrize("d", [192, 384, 768, 1024])
def test_embed_ln2_is_bit_equal_to_its_torch_lines_and_to_embed_ln(d, B, P, tok_dtype):
    g = _gen(d + B + P)
    tok = torch.randn(B * P, d, generator=g, device=DEV).to(tok_dtype)
    cls, dist = torch.randn(1, 1, d, generator=g, device=DEV) * 0.5, torch.randn(1, 1, d, generator=g, device=DEV) * 0.5
    pos = torch.randn(1, P + 2, d, generator=g, device=DEV) * 0.5
    w, b = 1 + 0.3 * torch.randn(d, generator=g, device=DEV), 0.2 * torch.randn(d, generator=g, device=DEV)
    want = torch.cat((cls.expand(B, -1, -1), dist.expand(B, -1, -1), tok.float().reshape(B, P, d)), 1) + pos     # one f32 add per element
    x32, xn = ops.embed_ln(tok, cls, pos, B, P, ln=(w, b, 1e-6), dist_token=dist)
    assert x32.shape == (B, P + 2, d) and xn.shape == (B, P + 2, d) and xn.dtype == torch.float16
    assert torch.equal(_bits(x32), _bits(want))
    assert torch.equal(_bits(xn), _bits(ops.layernorm(want, w, b, 1e-6, torch.float16))), "the promise smoe_embed_ln makes"
    x32b, none = ops.embed_ln(tok, cls, pos, B, P, dist_token=dist)
    assert none is None and torch.equal(_bits(x32b), _bits(want))
    # no LayerNorm asked for: the ABI selects the LayerNorm by xn != NULL, so 'without LN' has no xn buffer that could be touched;
    # the stream alone; dist_token == NULL: smoe_embed_ln's bits (straight at the entry points)
    lib = sm._lib.load()
    st = ops._stream(tok)
    code = ops.dtype_code(tok_dtype)
    out = torch.empty((B, P + 2, d), dtype=torch.float32, device=DEV)
    flat = lambda t: t.reshape(-1).contiguous()
    rc = lib.smoe_embed_ln2(tok.data_ptr(), code, flat(cls).data_ptr(), flat(dist).data_ptr(), pos.data_ptr(), None, None, 1e-6, B, P, d,
                            out.data_ptr(), None, 1, st)
    assert rc == 0 and torch.equal(_bits(out), _bits(want))
    pos1 = pos[:, :P + 1].contiguous()
    ref32, refn = ops.embed_ln(tok, cls, pos1, B, P, ln=(w, b, 1e-6), xn_dtype=torch.bfloat16)
    o32 = torch.empty_like(ref32)
    on = torch.empty_like(refn)
    rc = lib.smoe_embed_ln2(tok.data_ptr(), code, flat(cls).data_ptr(), None, pos1.data_ptr(), w.data_ptr(), b.data_ptr(), 1e-6, B, P, d,
                            o32.data_ptr(), on.data_ptr(), 2, st)
    assert rc == 0 and torch.equal(_bits(o32), _bits(ref32)) and torch.equal(_bits(on), _bits(refn))


# ------------------------------------------------------------------------------------------------------------ loss kernels
def _ulp32(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def _lines(kd, te, mode, tau, dtype):
    """losses.py:53-72 without the reductions, in ``dtype`` with autograd: (row values, gradient of the distillation loss)."""
    x = kd.detach().to(dtype).requires_grad_(True)
    t = te.detach().to(dtype)
    if mode == "soft":
        rows = F.kl_div(F.log_softmax(x / tau, dim=1), F.log_softmax(t / tau, dim=1), reduction='none', log_target=True).sum(1)
        loss = rows.sum() * (tau * tau) / x.numel()
    else:
        rows = F.cross_entropy(x, t.argmax(dim=1), reduction='none')
        loss = rows.mean()
    loss.backward()
    return rows.detach(), loss.detach(), x.grad


def _own(kd, te, mode, tau, alpha=1.0, base=0.0, g=1.0):
    b = torch.tensor(base, dtype=torch.float32, device=DEV)
    loss, distill, rows, stats, labels = ops.distill_fwd(kd, te, b, mode, tau, alpha)
    dx = ops.distill_bwd(kd, te, stats, labels, torch.tensor(g, dtype=torch.float32, device=DEV), mode, tau, alpha)
    return loss, distill, rows, dx, labels


def _bars(kd, te, mode, tau):
    """(float64 rows, loss, gradient; row bar, loss bar, gradient bar; torch's own errors): 3 x the max error of torch's f32 composition
    against float64 on these inputs, and at least one f32 ulp of the largest reference value."""
    r64, l64, g64 = _lines(kd, te, mode, tau, torch.float64)
    r32, l32, g32 = _lines(kd.float(), te.float(), mode, tau, torch.float32)
    e_row, e_grad = (r32.double() - r64).abs().max().item(), (g32.double() - g64).abs().max().item()
    e_loss = abs(l32.double().item() - l64.item())
    bar_row = max(3 * e_row, _ulp32(r64.abs().max().item()))
    bar_loss = max(3 * e_loss, _ulp32(abs(l64.item())))
    bar_grad = max(3 * e_grad, _ulp32(g64.abs().max().item()))
    return r64, l64, g64, bar_row, bar_loss, bar_grad, (e_row, e_loss, e_grad)


def _inputs(B, C, scale, seed, close=False):
    te = torch.randn(B, C, generator=_gen(seed), device=DEV) * scale
    if close:
        kd = te + 0.05 * torch.randn(B, C, generator=_gen(seed + 1), device=DEV)
    else:
        kd = torch.randn(B, C, generator=_gen(seed + 1), device=DEV) * scale
    return kd, te


def _check_f32(kd, te, mode, tau, what):
    r64, l64, g64, bar_row, bar_loss, bar_grad, (e_row, e_loss, e_grad) = _bars(kd, te, mode, tau)
    loss, distill, rows, dx, _ = _own(kd, te, mode, tau)
    o_row, o_grad = (rows.double() - r64).abs().max().item(), (dx.double() - g64).abs().max().item()
    o_loss = abs(distill.double().item() - l64.item())
    print(f"distill {what}: rows own {o_row:.3e} / torch {e_row:.3e} (bar {bar_row:.3e}); loss own {o_loss:.3e} / torch {e_loss:.3e} "
          f"(bar {bar_loss:.3e}); dlogits own {o_grad:.3e} / torch {e_grad:.3e} (bar {bar_grad:.3e})")
    assert o_row <= bar_row, (what, o_row, e_row)
    assert o_loss <= bar_loss, (what, o_loss, e_loss)
    assert o_grad <= bar_grad, (what, o_grad, e_grad)
    assert torch.equal(loss, distill), "alpha 1, base 0: the blend is the distillation loss"


@pytest.mark.parametrize("mode,tau", [("soft", 1.0), ("soft", 3.0), ("hard", 1.0)])
@pytest.mark.parametrize("scale", [1.0, 12.0])
@pytest.mark.parametrize("C", [10, 1000, 1003, 2056])
def test_distill_f32_within_three_times_torchs_own_error_against_float64(C, scale, mode, tau):
    for B in (1, 2, 64, 130):
        kd, te = _inputs(B, C, scale, 7 * B + C)
        _check_f32(kd, te, mode, tau, f"{mode} tau {tau} [{B}, {C}] scale {scale}")


@pytest.mark.parametrize("tau", [1.0, 3.0])
@pytest.mark.parametrize("C", [1000, 1003])
def test_distill_soft_student_close_to_the_teacher(C, tau):
    kd, te = _inputs(64, C, 4.0, 90 + C, close=True)
    _check_f32(kd, te, "soft", tau, f"soft tau {tau} [64, {C}] student = teacher + 0.05 noise")


def test_distill_blend_base_gradient_and_run_to_run_identity():
    kd, te = _inputs(130, 1000, 4.0, 5)
    for mode, tau, alpha in (("soft", 3.0, 0.1), ("hard", 1.0, 0.5)):
        _, l64, g64, _, bar_loss, bar_grad, _ = _bars(kd, te, mode, tau)
        loss, distill, rows, dx, labels = _own(kd, te, mode, tau, alpha=alpha, base=2.5, g=3.0)
        want = 2.5 * (1 - alpha) + l64.item() * alpha
        assert abs(loss.double().item() - want) <= alpha * bar_loss + _ulp32(want)
        assert (dx.double() - 3.0 * alpha * g64).abs().max().item() <= 3.0 * alpha * bar_grad
        for _ in range(3):
            l2, d2, r2, dx2, lab2 = _own(kd, te, mode, tau, alpha=alpha, base=2.5, g=3.0)
            assert torch.equal(l2, loss) and torch.equal(d2, distill) and torch.equal(r2, rows) and torch.equal(dx2, dx) and torch.equal(lab2, labels)


def _ulp16(ref64, dtype):
    a = ref64.abs().clamp_min(2.0 ** -140)
    e = torch.floor(torch.log2(a))
    if dtype == torch.float16:
        return torch.exp2(e.clamp_min(-14.0) - 10)
    return torch.exp2(e.clamp_min(-126.0) - 7)


@pytest.mark.parametrize("mode,tau", [("soft", 3.0), ("hard", 1.0)])
@pytest.mark.parametrize("t_dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("s_dtype", [torch.float16, torch.bfloat16])
def test_distill_16_bit_students_and_teachers_under_the_loss_scale(s_dtype, t_dtype, mode, tau):
    B, C, g = 64, 1000, 65536.0
    kd, te = _inputs(B, C, 4.0, 31)
    kd, te = kd.to(s_dtype), te.to(t_dtype)
    r64, l64, g64, bar_row, bar_loss, bar_grad, _ = _bars(kd, te, mode, tau)
    loss, distill, rows, dx, _ = _own(kd, te, mode, tau, g=g)
    assert dx.dtype == s_dtype and loss.dtype == torch.float32
    err = (dx.double() - g * g64).abs()
    bound = _ulp16(g * g64, s_dtype) + g * bar_grad
    worst = (err / bound).max().item()
    print(f"distill {mode} student {s_dtype} teacher {t_dtype} g=65536: worst |dlogits - ref64| / (ulp16 + g bar32) = {worst:.3f}")
    assert bool((err <= bound).all()), worst
    assert (rows.double() - r64).abs().max().item() <= bar_row and abs(distill.double().item() - l64.item()) <= bar_loss


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_distill_student_base_that_is_not_16_byte_aligned_takes_the_element_path(mode, dtype):
    B, C = 6, 1000
    n = B * C
    words = 4 // torch.empty(0, dtype=dtype).element_size()          # elements in 4 bytes
    kd, te = _inputs(B, C, 3.0, 17)
    kd, te = kd.to(dtype), te.to(dtype)
    assert kd.data_ptr() % 16 == 0 and C % 8 == 0
    loss, distill, rows, dx, labels = _own(kd, te, mode, 2.0)
    store = torch.zeros(n + 16, dtype=dtype, device=DEV)
    x = store[words:words + n].view(B, C)
    x.copy_(kd)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    b = torch.tensor(0.0, device=DEV)
    l2, d2, r2, stats, lab2 = ops.distill_fwd(x, te, b, mode, 2.0, 1.0)
    assert torch.equal(r2, rows) and torch.equal(l2, loss) and torch.equal(lab2, labels)
    lib = sm._lib.load()
    out = torch.zeros(n + 16, dtype=dtype, device=DEV)
    one = torch.tensor(1.0, device=DEV)
    m = ops._DISTILL_MODES[mode]
    rc = lib.smoe_distill_bwd(x.data_ptr(), ops.dtype_code(dtype), te.data_ptr(), ops.dtype_code(dtype), m, 2.0, 1.0, B, C, stats.data_ptr(),
                              lab2.data_ptr(), one.data_ptr(), out.data_ptr() + 4, ops._stream(x))
    assert rc == 0
    assert torch.equal(_bits(out[words:words + n].view(B, C)), _bits(dx))
    assert float(out[:words].float().abs().sum()) == 0 and float(out[words + n:].float().abs().sum()) == 0, "nothing written outside dlogits"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_distill_hard_mode_takes_torchs_argmax_on_tied_teacher_rows(dtype):
    B, C = 64, 1000
    kd, te = _inputs(B, C, 2.0, 23)
    te = te.to(dtype)
    for row in range(0, B, 2):                  # every second row: its maximum twice or three times, the later copies at higher AND lower indices
        top = te[row].max()
        idx = torch.randint(0, C, (2,), generator=_gen(row), device=DEV)
        te[row, idx] = top
    tied = (te == te.max(dim=1, keepdim=True).values).sum(1) >= 2
    assert int(tied.sum()) >= B // 4, "at least a quarter of the rows are tied"
    _, _, rows, dx, labels = _own(kd, te, "hard", 1.0)
    want = te.argmax(dim=1)
    assert torch.equal(labels.long(), want)
    r64, _, g64, bar_row, _, bar_grad, _ = _bars(kd, te, "hard", 1.0)
    assert (rows.double() - r64).abs().max().item() <= bar_row and (dx.double() - g64).abs().max().item() <= bar_grad
    for vals, first in (([1., 3., 3., 2.], 1), ([float("nan"), 5., float("nan"), 1.], 0), ([float("-inf")] * 4, 0)):
        t = torch.tensor([vals], device=DEV)
        assert int(t.argmax(dim=1)) == first
        assert int(_own(torch.zeros(1, 4, device=DEV), t, "hard", 1.0)[4]) == first, vals


@pytest.mark.parametrize("who", ["student", "teacher"])
@pytest.mark.parametrize("poison", ["nan", "+inf", "-inf"])
@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_distill_non_finite_inputs_stay_in_their_row(mode, poison, who):
    """loss and the poisoned row's gradient are non-finite wherever float64's are; every other row's gradient
    keeps its bits."""
    B, C, row, tau = 16, 1000, 5, 2.0
    kd, te = _inputs(B, C, 3.0, 41)
    _, _, _, clean, clean_labels = _own(kd, te, mode, tau)
    kp, tp = kd.clone(), te.clone()
    (kp if who == "student" else tp)[row, 7] = float(poison)
    if who == "teacher" and poison == "nan":
        tp[row, 400] = float("nan")               # a second NaN: the first one is the label
    r64, l64, g64 = _lines(kp, tp, mode, tau, torch.float64)
    loss, distill, rows, dx, labels = _own(kp, tp, mode, tau)
    others = [r for r in range(B) if r != row]
    assert torch.equal(_bits(dx[others]), _bits(clean[others])), "the other rows' gradients meet their bar: they are bit-identical"
    _, _, g64c, _, _, bar_grad, _ = _bars(kd, te, mode, tau)
    assert (clean.double() - g64c).abs().max().item() <= bar_grad
    if not math.isfinite(l64.item()):
        assert not math.isfinite(loss.item()) and not math.isfinite(distill.item()), (mode, poison, who)
    else:
        assert mode == "hard" and who == "teacher" or (mode == "hard" and poison == "-inf"), "only these leave float64's loss finite"
        assert abs(distill.double().item() - l64.item()) <= _bars(kp, tp, mode, tau)[4]
    bad64 = ~torch.isfinite(g64[row])
    assert bool((~torch.isfinite(dx[row]))[bad64].all()), (mode, poison, who, int(bad64.sum()))
    assert bool(torch.isfinite(dx[others]).all())
    if mode == "hard":
        assert torch.equal(labels.long(), tp.argmax(dim=1))
        if who == "teacher" and poison == "nan":
            assert int(labels[row]) == 7, "the first NaN index, as torch.argmax"
    if mode == "soft" and who == "teacher" and poison == "-inf":
        assert math.isnan(r64[row].item()) and math.isnan(rows[row].item()), "0 * -inf: NaN in the reference and here"


# ---------------------------------------------------------------------------------------------------------- class, fixture
def test_distillation_loss_class_against_the_references_fixture():
    fx = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in fx.files})
    assert len(names) == 12
    for n in names:
        kind = n.split("_")[0]
        tau, alpha = float(n.split("_tau")[1].split("_")[0]), float(n.split("_alpha")[1].split("_")[0])
        cls = torch.from_numpy(fx[n + "/cls"]).to(DEV).requires_grad_(True)
        kd = torch.from_numpy(fx[n + "/kd"]).to(DEV).requires_grad_(True)
        te = torch.from_numpy(fx[n + "/teacher"]).to(DEV)
        labels = torch.from_numpy(fx[n + "/labels"]).to(DEV)
        crit = sm.DistillationLoss(sm.LabelSmoothingCrossEntropy(0.0), lambda inp: te, kind, alpha, tau)
        loss = crit(None, (cls, kd), labels)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        loss.backward()
        _, _, _, bar_row, bar_loss, bar_grad, _ = _bars(kd.detach(), te, kind, tau)
        ce64 = F.cross_entropy(cls.detach().double(), labels).item()
        ce_bar = max(3 * abs(F.cross_entropy(cls.detach(), labels).double().item() - ce64), _ulp32(ce64))
        want = float(fx[n + "/loss_f64"])
        got = loss.double().item()
        print(f"fixture {n}: loss own {got:.8f} reference f64 {want:.8f} f32 {float(fx[n + '/loss_f32']):.8f}")
        assert abs(got - want) <= (1 - alpha) * ce_bar + alpha * bar_loss + _ulp32(want)
        assert (kd.grad.double().cpu() - torch.from_numpy(fx[n + "/dkd_f64"])).abs().max().item() <= alpha * bar_grad
        dcls64 = torch.from_numpy(fx[n + "/dcls_f64"])
        dcls_bar = max(3 * (torch.from_numpy(fx[n + "/dcls_f32"]).double() - dcls64).abs().max().item(), _ulp32(dcls64.abs().max().item()))
        assert (cls.grad.double().cpu() - dcls64).abs().max().item() <= dcls_bar
        if kind == "hard":
            assert torch.equal(ops.distill_fwd(kd.detach(), te, loss.detach(), "hard", 1.0, alpha)[4].long(), te.argmax(1))


# ------------------------------------------------------------------------------------------------------------- model step
KW = dict(depth=2, num_classes=10, img_size=64)


def _student(moe=False):
    torch.manual_seed(0)
    model = sm.create_model("deit_tiny_distilled_patch16_224", **KW)
    if moe:
        model = sm.resmoe.patch_blocks_with_moe(model, 8, 2, True, starting_threshold=0.55, target_threshold=0.5)
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


class _TorchDistill(torch.nn.Module):
    """losses.py's lines, restated: the composition the own criterion replaces."""

    def __init__(self, base, teacher, kind, alpha, tau):
        super().__init__()
        self.base, self.teacher, self.kind, self.alpha, self.tau = base, teacher, kind, alpha, tau

    def forward(self, inputs, outputs, labels):
        out, kd = outputs
        base = self.base(out, labels)
        with torch.no_grad():
            te = self.teacher(inputs)
        if self.kind == "soft":
            T = self.tau
            d = F.kl_div(F.log_softmax(kd / T, dim=1), F.log_softmax(te / T, dim=1), reduction='sum', log_target=True) * (T * T) / kd.numel()
        else:
            # (.float(): under autocast F.cross_entropy hands log_softmax the logits' own dtype, and f16 log-probabilities are off by
            # ~1e-4 -- measured here: 5e-5 in the loss; the own kernels take the f16 logits as they are and compute past f32)
            d = F.cross_entropy(kd.float(), te.argmax(dim=1))
        return base * (1 - self.alpha) + d * self.alpha


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("moe", [False, True], ids=["dense", "resmoe"])
@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_model_step_with_the_own_distillation_loss_matches_the_torch_composition(kind, moe):
    model, teacher = _student(moe).train(), _teacher()
    x = torch.randn(8, 3, 64, 64, generator=_gen(3), device=DEV)
    y = torch.randint(0, 10, (8,), generator=_gen(4), device=DEV)
    alpha, tau = 0.5, 3.0
    base = sm.LabelSmoothingCrossEntropy(0.1)

    def step(crit):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = model(x)
            loss = crit(x, out, y)
        (loss * 1024.0).backward()
        return (loss.detach().float().item(), tuple(o.detach() for o in out),
                {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})

    own_crit = sm.DistillationLoss(base, teacher, kind, alpha, tau)
    ref_crit = _TorchDistill(base, teacher, kind, alpha, tau)
    l_own, out, g_own = step(own_crit)
    l_ref, out_ref, g_ref = step(ref_crit)
    assert isinstance(out, tuple) and out[0].shape == (8, 10) and out[0].dtype == torch.float16
    assert torch.equal(out[0], out_ref[0]) and torch.equal(out[1], out_ref[1]), "the forward is deterministic"
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        te = teacher(x)
        base_val = base(out[0], y).double().item()
    _, d64, _, bar_row, _, _, _ = _bars(out[1], te, kind, tau)
    l64 = base_val * (1 - alpha) + d64.item() * alpha
    print(f"distilled model step ({kind}, {'resmoe' if moe else 'dense'}): loss own {l_own:.7f} torch {l_ref:.7f} float64 lines {l64:.7f} "
          f"(row bar {bar_row:.3e})")
    assert abs(l_own - l64) <= bar_row, "the own loss against the float64 lines on the same logits"
    assert abs(l_own - l_ref) <= 2 * bar_row, (l_own, l_ref, l64)
    assert set(g_own) == set(g_ref)
    for name in ("dist_token", "head_dist.weight", "head_dist.bias", "pos_embed", "cls_token"):
        assert name in g_own and float(g_own[name].abs().max()) > 0, name
    worst = max((_rel(g_own[n], g_ref[n]), n) for n in g_ref if float(g_ref[n].abs().max()) > 0)
    print(f"worst relative L2 gradient difference own loss vs torch composition {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 3e-2, worst
    if moe:
        return
    from torch.profiler import profile, ProfilerActivity

    def kernels(crit):
        calls = {}
        for _attempt in range(3):      # (the step has already completed outside the profiler; only an EMPTY trace is asked for again)
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step(crit)
                torch.cuda.synchronize()
            calls = {e.key: e.count for e in prof.key_averages()}
            if any(not n.startswith("hip") for n in calls):
                break
        return calls

    def torch_softmax(calls):
        return sum(c for n, c in calls.items() if ("softmax" in n.lower() or "kl_div" in n.lower()) and "soft_ce" not in n and "distill" not in n)

    class _NoLoss(torch.nn.Module):           # the model's and the teacher's own launches, and nothing of a criterion's
        def forward(self, inputs, outputs, labels):
            with torch.no_grad():
                teacher(inputs)
            return (outputs[0].float().sum() + outputs[1].float().sum()) * 1e-3
    base_count = torch_softmax(kernels(_NoLoss()))
    assert torch_softmax(kernels(ref_crit)) >= base_count + 2
    own = kernels(own_crit)
    assert torch_softmax(own) == base_count, [n for n in own if "softmax" in n.lower()]
    assert any("distill_fwd_kernel" in n for n in own) and any("distill_bwd_kernel" in n for n in own) and \
        any("distill_blend_kernel" in n for n in own), sorted(own)


def test_graphed_training_with_the_distillation_loss_reproduces_the_eager_harness():
    g = torch.Generator().manual_seed(70)
    batches = [(torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(6)]

    def run(graph):
        model, teacher = _student(), _teacher()
        opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
        scaler = sm.NativeScaler()
        crit = sm.DistillationLoss(sm.LabelSmoothingCrossEntropy(0.1), teacher, "soft", 0.5, 3.0)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            stats = sm.train_one_epoch(model, crit, batches, opt, DEV, 0, scaler, 1.0, None, None, hip_graph=graph)
        ours = [str(w.message) for w in caught if "HIP graph" in str(w.message) or "captured" in str(w.message)
                or "eagerly" in str(w.message) or "fallback" in str(w.message) or "libslimmoe_hip" in str(w.message)]
        assert not ours, ours
        return stats, {k: v.detach().clone() for k, v in model.state_dict().items()}

    s_e, p_e = run(False)
    s_g, p_g = run(True)
    assert s_g["hip_graph_steps"] == 3 and s_e["hip_graph_steps"] == 0, (s_g, s_e)
    assert s_g["loss"] == s_e["loss"], (s_g, s_e)
    assert all(torch.equal(p_e[k], p_g[k]) for k in p_e), "parameters after 6 steps"
    assert not torch.equal(p_e["dist_token"], _student().state_dict()["dist_token"]), "the distillation token trains"


# -------------------------------------------------------------------------------------------------------------------- eval
def test_distilled_eval_forward_mean_of_the_pair_graph_replay_and_error_against_float64():
    model = _student().eval()
    torch.manual_seed(0)
    plain = sm.create_model("deit_tiny_patch16_224", **KW).to(DEV).eval()
    x = torch.randn(8, 3, 64, 64, generator=_gen(9), device=DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            out = model(x)
            out_plain = plain(x)
        model.train()
        with torch.autocast("cuda", dtype=torch.float16):
            a, b = model(x)
        model.eval()
    assert not [str(w.message) for w in caught if "libslimmoe_hip" in str(w.message)], "no piece left the own kernels"
    assert out.shape == (8, 10) and out.dtype == torch.float16
    mean = (a.detach().double() + b.detach().double()) / 2
    ulp = _ulp16(mean, torch.float16) + _ulp16(a.detach().double().abs().max(b.detach().double().abs()), torch.float16)
    # (the pair itself is rounded to f16 by each path's head GEMM: one ulp of the pair's rounding, one of the mean's)
    assert bool(((out.double() - mean).abs() <= ulp).all()), ((out.double() - mean).abs() / ulp).max().item()
    gf = sm.GraphedForward(model)
    first, rep = gf(x), gf(x)
    assert gf.failed is None and gf.captures == 1
    assert torch.equal(first, out) and torch.equal(rep, out), "eager == graph replay"
    # (fresh float64 CPU modules with the same weights: the GPU modules carry stream caches that do not copy)
    m64 = sm.create_model("deit_tiny_distilled_patch16_224", **KW).double()
    p64 = sm.create_model("deit_tiny_patch16_224", **KW).double()
    m64.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()}, strict=True)
    p64.load_state_dict({k: v.detach().cpu().double() for k, v in plain.state_dict().items()}, strict=True)
    m64.eval(), p64.eval()
    with torch.no_grad():
        ref, ref_plain = m64(x.cpu().double()), p64(x.cpu().double())
    e_dist = (out.double().cpu() - ref).abs().max().item()
    e_plain = (out_plain.double().cpu() - ref_plain).abs().max().item()
    print(f"eval forward max logit error against float64: distilled {e_dist:.3e}, deit_tiny_patch16_224 {e_plain:.3e}")
    assert e_dist <= 3 * e_plain, (e_dist, e_plain)
