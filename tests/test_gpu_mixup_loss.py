"""GPU tests of the recipe around the model on the library's kernels: smoe_mixup_images / smoe_mixup_target bit-equal to timm's torch
lines (restated here, on the device), the soft-target / label-smoothing cross-entropy against float64 with a bar taken from torch's
own f32 composition on the same inputs, the non-finite contract, and the training harness with
``Mixup`` + ``SoftTargetCrossEntropy`` eager against graphed."""
import math
import warnings

import numpy as np
import pytest
import torch

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------- Mixup
def _one_hot(labels, C, on, off):
    return torch.full((labels.numel(), C), off, device=labels.device).scatter_(1, labels.view(-1, 1), on)


def _timm_lines(x0, labels, m):
    """timm's lines on the device for the draw ``m`` recorded, written out independently of the class."""
    B, C = len(x0), m.num_classes
    off = m.label_smoothing / C
    on = 1. - m.label_smoothing + off
    y1, y2 = _one_hot(labels, C, on, off), _one_hot(labels.flip(0), C, on, off)
    flipped = x0.flip(0)
    out = x0.clone()
    if m.mode == "batch":
        lam = m.lam
        if m.use_cutmix:
            yl, yh, xl, xh = (int(v) for v in m.boxes[0])
            out[:, :, yl:yh, xl:xh] = flipped[:, :, yl:yh, xl:xh]
        elif lam != 1.:
            out = out.mul_(lam).add_(flipped.mul_(1. - lam))
        return out, y1 * lam + y2 * (1. - lam)
    lam = m.lam
    for i in range(B):
        if m.use_cutmix[i]:
            yl, yh, xl, xh = (int(v) for v in m.boxes[i])
            out[i, :, yl:yh, xl:xh] = flipped[i, :, yl:yh, xl:xh]
        elif lam[i] != 1.:
            out[i] = x0[i] * float(lam[i]) + flipped[i] * float(np.float32(1) - lam[i])
    lt = torch.from_numpy(lam.copy()).to(x0.device).unsqueeze(1)
    return out, y1 * lt + y2 * (1. - lt)


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("B,shape", [(2, (3, 224, 224)), (64, (3, 224, 224)), (128, (3, 224, 224)), (8, (3, 30, 34)), (6, (3, 5, 7))])
def test_mixup_kernels_are_bit_equal_to_timms_torch_lines(mode, B, shape):
    """Same IEEE operations in the same order, so no tolerance.  3x30x34: rows that are no multiple of 16 bytes (a vector crosses row
    ends); 3x5x7 = 105 elements per image: the element-wise path."""
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.9, mode=mode, label_smoothing=0.1, num_classes=1000)
    np.random.seed(B + shape[1])
    kinds = set()
    for call in range(4 if B <= 8 or mode == "batch" else 1):
        x0 = torch.randn((B,) + shape, generator=_gen(call), device=DEV)
        labels = torch.randint(0, 1000, (B,), generator=_gen(100 + call), device=DEV)
        x = x0.clone()
        got_x, got_t = m(x, labels)
        assert got_x is x and got_t.dtype == torch.float32 and got_t.shape == (B, 1000)
        want_x, want_t = _timm_lines(x0, labels, m)
        assert torch.equal(got_x, want_x), (mode, B, shape, call, m.lam, m.use_cutmix)
        assert torch.equal(got_t, want_t), (mode, B, shape, call)
        lam = np.atleast_1d(m.lam)
        kinds |= {("cut" if c else "mix") for c, l in zip(np.broadcast_to(m.use_cutmix, lam.shape), lam) if l != 1.}
    if B >= 64 and mode != "batch":
        assert kinds == {"cut", "mix"}, kinds       # (pairs of both kinds in one launch)


def _table(lam, om, boxes):
    return (torch.tensor(lam, dtype=torch.float32, device=DEV), torch.tensor(om, dtype=torch.float32, device=DEV),
            torch.tensor(boxes, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("shape", [(3, 224, 224), (3, 30, 34), (3, 5, 7)])
def test_mixup_images_pairs_of_unlike_samples_and_edge_boxes(shape):
    """Hand-made tables: a pair of a CutMix and a Mixup sample (both ways round), a box covering the image, a box of zero area next
    to a factor (= Mixup by the header's rule), lam == 1 beside a partner holding inf, and a pair of two different boxes."""
    C, H, W = shape
    B = 12
    x0 = torch.randn((B,) + shape, generator=_gen(1), device=DEV)
    x0[10, 1, 2, 3] = float("inf")                       # the partner (1) has lam == 1: nothing of sample 10 may reach it
    x0[1, 0, 0, 0] = float("-inf")
    lam = [0.3, 1.0, 0.0, 0.6, 0.0, 0.25, 0.75, 0.0, 0.4, 0.0, 0.7, 0.0]
    om = [0.7, 0.0, 0.0, 0.4, 0.0, 0.75, 0.25, 0.0, 0.6, 0.0, 0.3, 0.0]
    boxes = [[0, 0, 0, 0], [0, 0, 0, 0], [0, H, 0, W], [2, 2, 1, W], [1, H - 1, 2, W - 1], [0, 0, 0, 0],
             [0, 0, 0, 0], [0, 3, 0, 2], [H, H, 0, 0], [H - 2, H, W - 3, W], [0, 0, 0, 0], [1, 2, 0, W]]
    x = x0.clone()
    ops.mixup_images_(x, *_table(lam, om, boxes))
    want = x0.clone()
    for b in range(B):
        j = B - 1 - b
        yl, yh, xl, xh = boxes[b]
        if lam[b] == 1.0:
            continue
        if yh > yl and xh > xl:
            want[b, :, yl:yh, xl:xh] = x0[j, :, yl:yh, xl:xh]
        else:
            want[b] = x0[b] * lam[b] + x0[j] * om[b]
    assert torch.equal(x.view(torch.int32), want.view(torch.int32))           # (bit patterns: the batch holds inf and NaN)
    assert torch.equal(x[1], x0[1]) and torch.equal(x[2], x0[9])
    with pytest.raises(sm._lib.SlimMoEError, match="even"):
        ops.mixup_images_(x0[:3].clone(), *_table(lam[:3], om[:3], boxes[:3]))


def test_mixup_target_out_of_range_label_is_off_everywhere():
    labels = torch.tensor([3, -1, 10, 7], device=DEV)
    lam, om, _ = _table([0.25, 0.5, 1.0, 0.75], [0.75, 0.5, 0.0, 0.25], [[0, 0, 0, 0]] * 4)
    t = ops.mixup_target(labels, lam, om, 0.91, 0.01, 10)
    f = np.float32
    assert t[1].tolist() == [float(f(f(0.01) * f(0.5)) + f(f(0.01) * f(0.5)))] * 10
    assert t[2].tolist() == [float(f(0.01) * f(1.0) + f(0.01) * f(0.0))] * 10
    assert t[0, 3].item() == float(f(f(0.91) * f(0.25)) + f(f(0.01) * f(0.75))) and t[0, 7].item() == float(f(f(0.01) * f(0.25)) + f(f(0.91) * f(0.75)))


# -------------------------------------------------------------------------------------------------------------------- loss
def _ulp32(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def _dense_targets(B, C, seed):
    g = _gen(seed)
    labels = torch.randint(0, C, (B,), generator=g, device=DEV)
    lam = torch.rand(B, 1, generator=g, device=DEV)
    off = 0.1 / C
    return _one_hot(labels, C, 1. - 0.1 + off, off) * lam + _one_hot(labels.flip(0), C, 1. - 0.1 + off, off) * (1 - lam), labels


def _ref64(x, t=None, labels=None, smoothing=0.0, g=1.0):
    """The defining formula in float64 with autograd: (row losses, d mean / d logits * g)."""
    x64 = x.detach().double().requires_grad_(True)
    lp = torch.log_softmax(x64, -1)
    if t is not None:
        rows = (-(t.double()) * lp).sum(-1)
    else:
        rows = (1. - smoothing) * -lp.gather(-1, labels.view(-1, 1)).squeeze(1) + smoothing * -lp.mean(-1)
    (rows.mean() * g).backward()
    return rows.detach(), x64.grad


def _torch32(x, t=None, labels=None, smoothing=0.0):
    """torch's f32 composition (timm's lines) on the device: (row losses, gradient of the mean)."""
    x32 = x.detach().float().requires_grad_(True)
    lp = torch.log_softmax(x32, -1)
    if t is not None:
        rows = torch.sum(-t * lp, dim=-1)
    else:
        rows = (1. - smoothing) * -lp.gather(-1, labels.view(-1, 1)).squeeze(1) + smoothing * -lp.mean(-1)
    rows.mean().backward()
    return rows.detach(), x32.grad


def _own(x, t=None, labels=None, smoothing=0.0, g=1.0):
    loss, rows = ops.soft_ce_fwd(x, t, labels, smoothing)
    dx = ops.soft_ce_bwd(x, rows, torch.tensor(g, dtype=torch.float32, device=x.device), t, labels, smoothing)
    return loss, rows[0], dx


def _bars(x, t=None, labels=None, smoothing=0.0):
    """(float64 rows, float64 gradient, row bar, gradient bar, torch's own errors): 3 x the max error of torch's f32 composition against
    float64 on these inputs, and at least one f32 ulp of the largest reference value."""
    r64, g64 = _ref64(x, t, labels, smoothing)
    r32, g32 = _torch32(x, t, labels, smoothing)
    e_row, e_grad = (r32.double() - r64).abs().max().item(), (g32.double() - g64).abs().max().item()
    bar_row = max(3 * e_row, _ulp32(r64.abs().max().item()))
    bar_grad = max(3 * e_grad, _ulp32(g64.abs().max().item()))
    return r64, g64, bar_row, bar_grad, (e_row, e_grad)


@pytest.mark.parametrize("scale", [1.0, 4.0, 12.0])
@pytest.mark.parametrize("B", [128, 256])
def test_soft_ce_f32_within_three_times_torchs_own_error_against_float64(B, scale):
    C = 1000
    t, _ = _dense_targets(B, C, 11)
    x = torch.randn(B, C, generator=_gen(12 + B), device=DEV) * scale
    r64, g64, bar_row, bar_grad, (e_row, e_grad) = _bars(x, t)
    loss, rows, dx = _own(x, t)
    o_row, o_grad = (rows.double() - r64).abs().max().item(), (dx.double() - g64).abs().max().item()
    o_mean = abs(loss.double().item() - r64.mean().item())
    print(f"soft CE f32 [{B}, {C}] scale {scale}: row loss max error own {o_row:.3e} / torch {e_row:.3e} (bar {bar_row:.3e}); "
          f"dlogits own {o_grad:.3e} / torch {e_grad:.3e} (bar {bar_grad:.3e}); mean own {o_mean:.3e}")
    assert o_row <= bar_row, (o_row, e_row)
    assert o_grad <= bar_grad, (o_grad, e_grad)
    assert o_mean <= bar_row, (o_mean, bar_row)


def _ulp16(ref64, dtype):
    """Spacing of the 16-bit type at the reference value."""
    a = ref64.abs().clamp_min(2.0 ** -140)
    e = torch.floor(torch.log2(a))
    if dtype == torch.float16:
        return torch.exp2(e.clamp_min(-14.0) - 10)
    return torch.exp2(e.clamp_min(-126.0) - 7)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_soft_ce_16_bit_logits_under_the_loss_scale(dtype, seed):
    B, C, g = 128, 1000, 65536.0
    t, _ = _dense_targets(B, C, 20 + seed)
    x = (torch.randn(B, C, generator=_gen(30 + seed), device=DEV) * 4).to(dtype)
    r64, _, bar_row, bar_grad, _ = _bars(x.float(), t)
    _, g64 = _ref64(x, t, g=g)
    loss, rows, dx = _own(x, t, g=g)
    assert dx.dtype == dtype and loss.dtype == torch.float32
    err = (dx.double() - g64).abs()
    bound = _ulp16(g64, dtype) + g * bar_grad
    worst = (err / bound).max().item()
    print(f"soft CE {dtype} g=65536: worst |dlogits - ref64| / (ulp16 + g bar32) = {worst:.3f}; row loss max error "
          f"{(rows.double() - r64).abs().max().item():.3e} (bar {bar_row:.3e})")
    assert bool((err <= bound).all()), worst
    assert (rows.double() - r64).abs().max().item() <= bar_row


@pytest.mark.parametrize("C", [10, 1000, 1001, 21843])
@pytest.mark.parametrize("B", [1, 2, 128, 255])
def test_soft_ce_shapes_both_target_forms_and_run_to_run_identity(B, C):
    t, labels = _dense_targets(B, C, B + C)
    x = torch.randn(B, C, generator=_gen(B * 3 + C), device=DEV) * 3
    for kw in (dict(t=t), dict(labels=labels, smoothing=0.0), dict(labels=labels, smoothing=0.1)):
        r64, g64, bar_row, bar_grad, _ = _bars(x, **kw)
        loss, rows, dx = _own(x, **kw)
        assert (rows.double() - r64).abs().max().item() <= bar_row, (kw.keys(), B, C)
        assert (dx.double() - g64).abs().max().item() <= bar_grad, (kw.keys(), B, C)
        assert abs(loss.double().item() - r64.mean().item()) <= bar_row
        for _ in range(4):
            l2, r2, d2 = _own(x, **kw)
            assert torch.equal(l2, loss) and torch.equal(r2, rows) and torch.equal(d2, dx)
    crit = sm.LabelSmoothingCrossEntropy(0.0)
    assert abs(crit(x, labels).item() - torch.nn.functional.cross_entropy(x.double(), labels).item()) <= \
        max(3e-6, 3 * abs(torch.nn.functional.cross_entropy(x, labels).item() - torch.nn.functional.cross_entropy(x.double(), labels).item()))


@pytest.mark.parametrize("poison", ["logit+inf", "logit-inf", "logitnan", "targetinf", "targetnan"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_soft_ce_non_finite_inputs_stay_in_their_row(poison, dtype):
    """a poisoned row leaves the other rows' gradients bit-identical; the mean loss and that row's
    gradient are non-finite wherever float64's are."""
    B, C, row = 16, 1000, 5
    t, _ = _dense_targets(B, C, 41)
    x = (torch.randn(B, C, generator=_gen(42), device=DEV) * 3).to(dtype)
    _, _, clean = _own(x, t)
    xp, tp = x.clone(), t.clone()
    col = 7 if poison.startswith("logit") else int(t[row].argmax())
    val = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "inf": float("inf")}[poison.replace("logit", "").replace("target", "")]
    (xp if poison.startswith("logit") else tp)[row, col] = val
    r64, g64 = _ref64(xp, tp)
    loss, rows, dx = _own(xp, tp)
    others = [r for r in range(B) if r != row]
    assert torch.equal(dx[others].view(torch.int16 if dtype == torch.float16 else torch.int32),
                       clean[others].view(torch.int16 if dtype == torch.float16 else torch.int32))
    assert torch.equal(rows[others], _own(x, t)[1][others])
    assert not math.isfinite(r64.mean().item()), "the poison reaches float64's mean loss in every case listed"
    assert not math.isfinite(loss.item())
    bad64 = ~torch.isfinite(g64[row])
    assert bool((~torch.isfinite(dx[row].float()))[bad64].all()), (poison, int(bad64.sum()))
    assert bool(torch.isfinite(dx[others].float()).all())


# ----------------------------------------------------------------------------------------------------------------- harness
RES, RES_KW = "resmoe_tiny_patch16_224_expert8", dict(num_classes=10, depth=2, starting_threshold=0.55, target_threshold=0.5)


def _resmoe():
    torch.manual_seed(0)
    model = sm.create_model(RES, **RES_KW)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if "_gate.head.1.weight" in n_:
                p.normal_(0, 0.3, generator=torch.Generator().manual_seed(5))
    return model.to(DEV)


def test_graphed_training_step_with_mixup_and_soft_target_loss_reproduces_the_eager_harness():
    g = torch.Generator().manual_seed(70)
    batches = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(9)]

    def run(graph):
        model = _resmoe()
        opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
        scaler = sm.NativeScaler()
        ema = sm.ModelEma(model, 0.99996)
        np.random.seed(123)
        mix = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=10)
        draws = []

        def mixup_fn(x, y):
            out = mix(x, y)
            draws.append((mix.lam, mix.use_cutmix))
            return out
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            stats = sm.train_one_epoch(model, sm.SoftTargetCrossEntropy(), batches, opt, DEV, 0, scaler, 1.0, ema, mixup_fn,
                                       hip_graph=graph)
        ours = [str(w.message) for w in caught if "HIP graph" in str(w.message) or "captured" in str(w.message)
                or "eagerly" in str(w.message) or "fallback" in str(w.message) or "libslimmoe_hip" in str(w.message)]
        assert not ours, ours
        moments = [opt.state[p]["exp_avg"].clone() for p in model.parameters() if p in opt.state]
        moments += [opt.state[p]["exp_avg_sq"].clone() for p in model.parameters() if p in opt.state]
        final = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return stats, final, moments, scaler.state_dict(), {k: v.clone() for k, v in ema.state_dict().items()}, draws

    s_e, p_e, m_e, sc_e, ema_e, d_e = run(False)
    s_g, p_g, m_g, sc_g, ema_g, d_g = run(True)
    assert d_e == d_g and len(d_e) == 9 and len({c for _, c in d_e}) == 2, "the same draws, of both kinds"
    assert s_g["hip_graph_steps"] == 6 and s_e["hip_graph_steps"] == 0
    assert s_g["loss"] == s_e["loss"], (s_g, s_e)
    assert all(torch.equal(p_e[k], p_g[k]) for k in p_e), "parameters after 9 steps"
    assert all(torch.equal(a, b) for a, b in zip(m_e, m_g)), "AdamW moments after 9 steps"
    assert sc_e == sc_g
    assert all(torch.equal(ema_e[k], ema_g[k]) for k in ema_e), "EMA after 9 steps"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_model_step_with_the_own_loss_matches_the_torch_composition_and_runs_no_torch_softmax():
    model = _resmoe().train()
    np.random.seed(5)
    x = torch.randn(8, 3, 224, 224, generator=_gen(3), device=DEV)
    y = torch.randint(0, 10, (8,), generator=_gen(4), device=DEV)
    x, t = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", num_classes=10)(x, y)

    def torch_crit(out, tt):
        return torch.sum(-tt * torch.nn.functional.log_softmax(out, dim=-1), dim=-1).mean()

    def step(crit):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = model(x)
            loss = crit(out, t)
        (loss * 1024.0).backward()
        return loss.detach().float().item(), out.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    l_own, out, g_own = step(sm.SoftTargetCrossEntropy())
    l_ref, out_ref, g_ref = step(torch_crit)
    _, _, bar_row, _, _ = _bars(out.float(), t)
    print(f"model step: loss own {l_own:.7f} torch {l_ref:.7f} (bar {bar_row:.3e})")
    assert abs(l_own - _ref64(out.float(), t)[0].mean().item()) <= bar_row
    assert torch.equal(out, out_ref), "the forward is deterministic"
    assert abs(l_own - l_ref) <= 2 * bar_row
    assert set(g_own) == set(g_ref)
    worst = max((_rel(g_own[n], g_ref[n]), n) for n in g_ref if float(g_ref[n].abs().max()) > 0)
    print(f"worst relative L2 gradient difference own loss vs torch composition {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 3e-2, worst
    from torch.profiler import profile, ProfilerActivity

    def kernels(crit):
        calls = {}
        for _attempt in range(3):      # (the step has already completed once outside the profiler; roctracer now and then delivers a
            # cycle's runtime-API rows without its kernel rows: only such an EMPTY trace is asked for again, never a failing step)
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step(crit)
                torch.cuda.synchronize()
            calls = {e.key: e.count for e in prof.key_averages()}
            if any(not n.startswith("hip") for n in calls):
                break
        return calls

    def torch_softmax(calls):
        return sum(c for n, c in calls.items() if "softmax" in n.lower() and "soft_ce" not in n)
    # what the MODEL itself launches of torch's softmax family (a criterion without one), the torch composition on top of it (the
    # detector sees its log-softmax forward and backward), and the own loss: nothing on top
    base = torch_softmax(kernels(lambda o, tt: (o.float() * tt).sum()))
    assert torch_softmax(kernels(torch_crit)) >= base + 2
    own = kernels(sm.SoftTargetCrossEntropy())
    assert torch_softmax(own) == base, [n for n in own if "softmax" in n.lower()]
    assert any("soft_ce_fwd_kernel" in n for n in own) and any("soft_ce_bwd_kernel" in n for n in own) and \
        any("row_mean_kernel" in n for n in own), sorted(own)


def test_mixup_images_on_a_base_that_is_not_16_byte_aligned_takes_the_element_path():
    """n % 4 == 0 but the data pointer sits 4 bytes into a larger buffer: 16-byte accesses are impossible, the results the same."""
    B, shape = 12, (3, 8, 12)
    n = B * 3 * 8 * 12
    buf = torch.randn(n + 8, generator=_gen(9), device=DEV)
    lam = [0.3, 1.0, 0.0, 0.6, 0.0, 0.25, 0.75, 0.0, 0.4, 0.0, 0.7, 0.0]
    om = [0.7, 0.0, 0.0, 0.4, 0.0, 0.75, 0.25, 0.0, 0.6, 0.0, 0.3, 0.0]
    boxes = [[0, 0, 0, 0], [0, 0, 0, 0], [0, 8, 0, 12], [0, 0, 0, 0], [1, 7, 2, 11], [0, 0, 0, 0],
             [0, 0, 0, 0], [0, 3, 0, 2], [0, 0, 0, 0], [6, 8, 9, 12], [0, 0, 0, 0], [1, 2, 0, 12]]
    tab = _table(lam, om, boxes)
    aligned = buf[:n].clone().view((B,) + shape)
    assert aligned.data_ptr() % 16 == 0
    ops.mixup_images_(aligned, *tab)
    for off in (1, 2, 3):
        store = torch.zeros(n + 8, device=DEV)
        x = store[off:off + n].view((B,) + shape)
        x.copy_(buf[:n].view((B,) + shape))
        assert x.data_ptr() % 16 == 4 * off and x.is_contiguous()
        ops.mixup_images_(x, *tab)
        assert torch.equal(x, aligned), off
        assert float(store[:off].abs().sum()) == 0 and float(store[off + n:].abs().sum()) == 0, "nothing written outside the batch"
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=0., num_classes=10)        # ... and through the class
    np.random.seed(1)
    store = buf.clone()
    x = store[1:1 + n].view((B,) + shape)
    labels = torch.randint(0, 10, (B,), generator=_gen(2), device=DEV)
    got, t = m(x, labels)
    want, want_t = _timm_lines(buf[1:1 + n].view((B,) + shape), labels, m)
    assert torch.equal(got, want) and torch.equal(t, want_t) and m.lam != 1.


@pytest.mark.parametrize("form", ["dense", "labels"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_soft_ce_bwd_base_that_is_not_16_byte_aligned_takes_the_element_path_and_writes_the_same_bits(dtype, form):
    """C = 2056 = one step of 256 x 8 logits + one vector; the same logits, row statistics and g once on 16-byte aligned bases (8
    logits per lane) and once with logits and dlogits 4 bytes into larger buffers (element by element)."""
    B, C, smoothing = 3, 2056, 0.1
    n = B * C
    words = 4 // torch.empty(0, dtype=dtype).element_size()          # elements in 4 bytes
    x = (torch.randn(B, C, generator=_gen(71), device=DEV) * 3).to(dtype)
    t, labels = _dense_targets(B, C, 72)
    t, labels = (t.contiguous(), None) if form == "dense" else (None, labels)
    g = torch.tensor(3.0, dtype=torch.float32, device=DEV)
    _, rows = ops.soft_ce_fwd(x, t, labels, smoothing)
    assert x.data_ptr() % 16 == 0 and (t is None or t.data_ptr() % 16 == 0) and C % 8 == 0
    dx = ops.soft_ce_bwd(x, rows, g, t, labels, smoothing)
    assert dx.data_ptr() % 16 == 0
    store = torch.zeros(n + 16, dtype=dtype, device=DEV)
    xo = store[words:words + n].view(B, C)
    xo.copy_(x)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    out = torch.zeros(n + 16, dtype=dtype, device=DEV)
    rc = sm._lib.load().smoe_soft_ce_bwd(xo.data_ptr(), ops.dtype_code(dtype), ops._ptr(t), ops._ptr(labels), smoothing, B, C,
                                         rows.data_ptr() + 4 * B, rows.data_ptr() + 8 * B, rows.data_ptr() + 12 * B, g.data_ptr(),
                                         out.data_ptr() + 4, ops._stream(x))
    assert rc == 0
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(out[words:words + n].view(B, C).view(bits), dx.view(bits))
    assert bool(dx.float().abs().sum() > 0)
    assert float(out[:words].float().abs().sum()) == 0 and float(out[words + n:].float().abs().sum()) == 0, "nothing written outside dlogits"


def test_batch_mode_calls_cover_mixup_cutmix_and_untouched():
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.7, mode="batch", label_smoothing=0.1, num_classes=1000)
    np.random.seed(0)
    kinds = set()
    for call in range(12):
        x0 = torch.randn(4, 3, 30, 34, generator=_gen(call), device=DEV)
        labels = torch.randint(0, 1000, (4,), generator=_gen(50 + call), device=DEV)
        got_x, got_t = m(x0.clone(), labels)
        want_x, want_t = _timm_lines(x0, labels, m)
        assert torch.equal(got_x, want_x) and torch.equal(got_t, want_t), call
        kinds.add("none" if m.lam == 1. else "cut" if m.use_cutmix else "mix")
    assert kinds == {"none", "cut", "mix"}, kinds


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_label_smoothing_module_forward_and_autograd_backward_on_the_kernels(smoothing, dtype):
    B, C, scale = 128, 1000, 1024.0
    _, labels = _dense_targets(B, C, 61)
    x = (torch.randn(B, C, generator=_gen(62), device=DEV) * 3).to(dtype).requires_grad_(True)
    crit = sm.LabelSmoothingCrossEntropy(smoothing)
    loss = crit(x, labels)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * scale).backward()
    r64, g64 = _ref64(x.detach(), labels=labels, smoothing=smoothing, g=scale)
    _, _, bar_row, bar_grad, _ = _bars(x.detach().float(), labels=labels, smoothing=smoothing)
    assert abs(loss.double().item() - r64.mean().item()) <= bar_row
    err = (x.grad.double() - g64).abs()
    assert x.grad.dtype == dtype
    if dtype == torch.float32:
        assert err.max().item() <= scale * bar_grad
    else:
        assert bool((err <= _ulp16(g64, dtype) + scale * bar_grad).all())
    from torch.profiler import profile, ProfilerActivity
    names = set()
    for _attempt in range(3):      # (a pass that already completed outside the profiler; repeated only when the trace came back empty)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            (crit(x, labels) * scale).backward()
            torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}
        if any(not n.startswith("hip") for n in names):
            break
    assert any("soft_ce_fwd_kernel" in n for n in names) and any("soft_ce_bwd_kernel" in n for n in names), names
    assert not [n for n in names if "softmax" in n.lower() and "soft_ce" not in n], names
