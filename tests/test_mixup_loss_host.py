"""CPU tests of the recipe objects around the model: ``Mixup`` (timm.data.Mixup's surface, main.py:505-517), ``SoftTargetCrossEntropy``
and ``LabelSmoothingCrossEntropy`` (main.py:653-661) on their torch lines, and what the library answers for the four new entry
points without a GPU.  The restatement of timm's lines below is this file's own: it replays the draw a call recorded on the object."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slimmoe.h")
NEW = ["smoe_mixup_images", "smoe_mixup_target", "smoe_soft_ce_fwd", "smoe_soft_ce_bwd"]


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_are_declared_prototyped_and_exported_and_the_abi_is_29():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
        assert hasattr(lib, s), f"libslimmoe_hip.so does not export {s}"
        n_args = len([a for a in re.search(r"%s\s*\((.*?)\)" % s, text, re.S).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[s][1]), s
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    assert "loss.hip" in _lib._HASHED and _lib.binary_build_id() == _lib.source_build_id()


def test_argument_checks_come_before_any_launch():
    lib = _lib.load()
    fake = 4096          # never dereferenced
    assert lib.smoe_mixup_images(fake, 0, 3, 8, 8, fake, fake, fake, None) == 0           # B == 0 returns at once
    assert lib.smoe_mixup_images(fake, 3, 3, 8, 8, fake, fake, fake, None) != 0
    assert b"even" in lib.smoe_last_error()
    assert lib.smoe_mixup_images(None, 2, 3, 8, 8, fake, fake, fake, None) != 0
    assert b"null" in lib.smoe_last_error()
    assert lib.smoe_mixup_images(fake, 2, 3, 8, 8, fake, fake, None, None) != 0
    assert b"null" in lib.smoe_last_error()
    assert lib.smoe_mixup_target(fake, fake, fake, 0.9, 0.1, 0, 10, fake, None) == 0
    assert lib.smoe_mixup_target(fake, fake, fake, 0.9, 0.1, 4, 0, fake, None) != 0
    assert b"num_classes" in lib.smoe_last_error()
    assert lib.smoe_mixup_target(fake, fake, fake, 0.9, 0.1, 4, -3, fake, None) != 0
    assert lib.smoe_mixup_target(None, fake, fake, 0.9, 0.1, 4, 10, fake, None) != 0
    assert b"null" in lib.smoe_last_error()
    assert lib.smoe_soft_ce_fwd(fake, 0, fake, None, 0.0, 0, 10, fake, fake, fake, fake, fake, None) == 0
    assert lib.smoe_soft_ce_fwd(None, 0, fake, None, 0.0, 4, 10, fake, fake, fake, fake, fake, None) != 0
    assert b"null" in lib.smoe_last_error()
    assert lib.smoe_soft_ce_fwd(fake, 0, None, None, 0.0, 4, 10, fake, fake, fake, fake, fake, None) != 0      # neither target form
    assert lib.smoe_soft_ce_fwd(fake, 0, fake, fake, 0.0, 4, 10, fake, fake, fake, fake, fake, None) != 0      # both
    assert lib.smoe_soft_ce_fwd(fake, 7, fake, None, 0.0, 4, 10, fake, fake, fake, fake, fake, None) != 0      # no such dtype
    assert lib.smoe_soft_ce_fwd(fake, 0, fake, None, 0.0, 4, 0, fake, fake, fake, fake, fake, None) != 0 # C == 0
    assert lib.smoe_soft_ce_bwd(fake, 1, fake, None, 0.0, 0, 10, fake, fake, fake, fake, fake, None) == 0
    assert lib.smoe_soft_ce_bwd(fake, 1, fake, None, 0.0, 4, 10, fake, fake, fake, None, fake, None) != 0
    assert b"null" in lib.smoe_last_error()
    assert lib.smoe_soft_ce_bwd(fake, 1, fake, None, 0.0, 4, 10, fake, fake, fake, fake, None, None) != 0


# ------------------------------------------------------------------------------------------------------------------- Mixup
def _one_hot(labels, C, on, off):
    out = torch.full((labels.numel(), C), off)
    out[torch.arange(labels.numel()), labels] = on
    return out


def replay(x0, labels, m):
    """timm's lines for the draw ``m`` recorded (``m.lam``, ``m.use_cutmix``, ``m.boxes``), written out independently of the class."""
    B, C = len(x0), m.num_classes
    off = m.label_smoothing / C
    on = 1. - m.label_smoothing + off
    y1, y2 = _one_hot(labels, C, on, off), _one_hot(labels.flip(0), C, on, off)
    flipped = x0.flip(0)
    out = x0.clone()
    if m.mode == "batch":
        lam = m.lam
        assert isinstance(lam, float)
        if m.use_cutmix:
            yl, yh, xl, xh = (int(v) for v in m.boxes[0])
            out[:, :, yl:yh, xl:xh] = flipped[:, :, yl:yh, xl:xh]
        elif lam != 1.:
            out = x0 * lam + flipped * (1. - lam)                       # factors f32(lam) and f32(1 - lam), the difference in double
        return out, y1 * lam + y2 * (1. - lam)
    lam = m.lam
    assert lam.dtype == np.float32 and lam.shape == (B,)
    for i in range(B):
        if m.use_cutmix[i]:
            yl, yh, xl, xh = (int(v) for v in m.boxes[i])
            out[i, :, yl:yh, xl:xh] = flipped[i, :, yl:yh, xl:xh]
        elif lam[i] != 1.:
            om = np.float32(1) - lam[i]                                 # in f32
            out[i] = x0[i] * float(lam[i]) + flipped[i] * float(om)
    lt = torch.from_numpy(lam.copy()).unsqueeze(1)
    return out, y1 * lt + y2 * (torch.ones_like(lt) - lt)


CONFIGS = {
    "mixup": dict(mixup_alpha=0.8, cutmix_alpha=0.),
    "cutmix": dict(mixup_alpha=0., cutmix_alpha=1.0),
    "both": dict(mixup_alpha=0.8, cutmix_alpha=1.0),
    "both_uncorrected": dict(mixup_alpha=0.8, cutmix_alpha=1.0, correct_lam=False),
    "minmax": dict(mixup_alpha=0.8, cutmix_alpha=0., cutmix_minmax=(0.2, 0.7)),
    "half": dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5),
}


def _data(B, C=10, H=12, W=14, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, H, W, generator=g), torch.randint(0, C, (B,), generator=g)


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_mixup_on_cpu_is_timms_lines_for_the_recorded_draw(mode, config):
    m = sm.Mixup(mode=mode, label_smoothing=0.1, num_classes=10, **CONFIGS[config])
    np.random.seed(3)            # (chosen so that every mode takes both branches and clips a box: checked below)
    seen = {"mixup": False, "cutmix": False, "clipped": False, "untouched": False}
    for call in range(24):
        x0, labels = _data(8, seed=call)
        x = x0.clone()
        got_x, got_t = m(x, labels)
        assert got_x is x, "the images are mixed in place"
        want_x, want_t = replay(x0, labels, m)
        assert torch.equal(got_x, want_x), (mode, config, call)
        assert got_t.dtype == torch.float32 and torch.equal(got_t, want_t), (mode, config, call)
        assert (got_t.sum(1) - 1).abs().max().item() <= 10 * 2.0 ** -24
        lam = np.full(8, m.lam, dtype=np.float64) if mode == "batch" else m.lam.astype(np.float64)
        cut = np.full(8, m.use_cutmix) if mode == "batch" else m.use_cutmix
        assert m.boxes.shape == (8, 4) and m.boxes.dtype == np.int32
        for i in range(8):
            yl, yh, xl, xh = m.boxes[i]
            if lam[i] == 1.:
                assert torch.equal(got_x[i], x0[i]), "lam == 1: the sample is untouched"
                seen["untouched"] = True
            elif cut[i]:
                seen["cutmix"] = True
                seen["clipped"] |= bool(yh > yl and xh > xl and (yl == 0 or xl == 0 or yh == 12 or xh == 14))
            else:
                seen["mixup"] = True
                assert not torch.equal(got_x[i], x0[i])
        if mode == "pair":
            assert np.array_equal(m.lam, m.lam[::-1]) and np.array_equal(m.boxes, m.boxes[::-1])
    if config == "mixup":
        assert seen["mixup"] and not seen["cutmix"]
    elif config == "cutmix":
        assert seen["cutmix"] and not seen["mixup"] and seen["clipped"]
    else:
        assert seen["mixup"] and seen["cutmix"], seen                                 # both branches of the mode were taken
        if config != "minmax":                                                        # (a min-max box lies inside by construction)
            assert seen["clipped"], seen
    if config == "half":
        assert seen["untouched"]


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_prob_zero_leaves_the_images_and_gives_smoothed_one_hot_rows(mode):
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0, mode=mode, label_smoothing=0.1, num_classes=10)
    np.random.seed(3)
    x0, labels = _data(6)
    x0[2, 0, 0, 0] = float("inf")          # nothing of a partner may leak into an untouched sample (0 * inf)
    x, t = m(x0.clone(), labels)
    assert torch.equal(x, x0)
    assert torch.equal(t, _one_hot(labels, 10, 1. - 0.1 + 0.01, 0.01) * 1.0 + _one_hot(labels.flip(0), 10, 1. - 0.1 + 0.01, 0.01) * 0.0)
    m.mixup_enabled = False
    m.mix_prob = 1.0
    x, _ = m(x0.clone(), labels)
    assert torch.equal(x, x0) and m.mixup_enabled is False


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_the_same_numpy_seed_gives_the_same_draw(mode):
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, num_classes=10)
    x0, labels = _data(8)
    outs = []
    for _ in range(2):
        np.random.seed(77)
        x, t = m(x0.clone(), labels)
        outs.append((x, t, np.array(m.lam), np.array(m.use_cutmix), m.boxes.copy()))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(np.array_equal(p, q) for p, q in zip(a[2:], b[2:]))
    np.random.seed(78)
    m(x0.clone(), labels)
    assert not (np.array_equal(np.array(m.lam), a[2]) and np.array_equal(m.boxes, a[4]))


def test_surface_matches_timm_and_an_odd_batch_asserts():
    params = list(inspect.signature(sm.Mixup.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [
        ("mixup_alpha", 1.), ("cutmix_alpha", 0.), ("cutmix_minmax", None), ("prob", 1.0), ("switch_prob", 0.5), ("mode", "batch"),
        ("correct_lam", True), ("label_smoothing", 0.1), ("num_classes", 1000)]
    m = sm.Mixup(0.8, 1.0, None, 1.0, 0.5, "batch", True, 0.1, 1000)       # main.py:508-517's positional meaning
    assert m.mixup_enabled is True and sm.Mixup is sm.mixup.Mixup
    x0, labels = _data(5)
    with pytest.raises(AssertionError):
        m(x0, labels)
    x, t = m(*_data(4, C=1000))
    assert t.shape == (4, 1000) and (t.sum(1) - 1).abs().max().item() <= 1000 * 2.0 ** -24
    with pytest.raises(AssertionError):
        sm.Mixup(mode="half")


# ------------------------------------------------------------------------------------------------------------------ losses
def _soft_targets(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, 1, generator=g)
    return _one_hot(labels, C, 0.9 + 0.1 / C, 0.1 / C) * lam + _one_hot(labels.flip(0), C, 0.9 + 0.1 / C, 0.1 / C) * (1 - lam), labels


@pytest.mark.parametrize("B,C", [(1, 10), (16, 1000), (7, 1001)])
def test_soft_target_cross_entropy_on_cpu_against_float64(B, C):
    t, _ = _soft_targets(B, C, 5)
    x = torch.randn(B, C, generator=torch.Generator().manual_seed(6)) * 4
    x.requires_grad_(True)
    loss = sm.SoftTargetCrossEntropy()(x, t)
    loss.backward()
    x64 = x.detach().double().requires_grad_(True)
    ref = (-(t.double()) * torch.log_softmax(x64, -1)).sum(-1).mean()
    ref.backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert (x.grad.double() - x64.grad).abs().max().item() <= 1e-6 / B
    assert isinstance(sm.SoftTargetCrossEntropy(), torch.nn.Module) and sm.SoftTargetCrossEntropy is sm.loss.SoftTargetCrossEntropy


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_label_smoothing_cross_entropy_on_cpu_against_float64(smoothing):
    B, C = 16, 1000
    _, labels = _soft_targets(B, C, 8)
    x = (torch.randn(B, C, generator=torch.Generator().manual_seed(9)) * 4).requires_grad_(True)
    crit = sm.LabelSmoothingCrossEntropy(smoothing)
    assert crit.smoothing == smoothing and crit.confidence == 1. - smoothing
    loss = crit(x, labels)
    loss.backward()
    x64 = x.detach().double().requires_grad_(True)
    lp = torch.log_softmax(x64, -1)
    ref = ((1. - smoothing) * -lp[torch.arange(B), labels] + smoothing * -lp.mean(-1)).mean()
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert (x.grad.double() - x64.grad).abs().max().item() <= 1e-6 / B
    if smoothing == 0.0:
        assert abs(crit(x64, labels).item() - F.cross_entropy(x64, labels).item()) <= 1e-12
        assert torch.allclose(loss, F.cross_entropy(x, labels), rtol=1e-6, atol=0)
    assert list(inspect.signature(sm.LabelSmoothingCrossEntropy.__init__).parameters)[1:] == ["smoothing"]
    assert sm.LabelSmoothingCrossEntropy().smoothing == 0.1
    with pytest.raises(AssertionError):
        sm.LabelSmoothingCrossEntropy(1.0)


def test_train_one_epoch_takes_the_new_objects_on_cpu_tensors():
    """The harness' positions (engine.py:46-47, 54): ``mixup_fn(samples, targets)`` before the forward, ``criterion(outputs, targets)``."""
    torch.manual_seed(0)
    np.random.seed(0)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 4 * 4, 10))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    data = [(torch.randn(4, 3, 4, 4), torch.randint(0, 10, (4,))) for _ in range(3)]
    scaler = sm.NativeScaler()
    stats = sm.train_one_epoch(model, sm.SoftTargetCrossEntropy(), data, opt, "cpu", 0, scaler, None, None,
                               sm.Mixup(0.8, 1.0, num_classes=10), autocast=False)
    assert stats["steps"] == 3 and np.isfinite(stats["loss"])


# ------------------------------------------------------------------------------------------- the draw itself, against the contract
def _expected_box(H, W, lam):
    """rand_bbox in the documented order: ratio, cut sizes, cy then cx from randint, the four clips."""
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    cy = np.random.randint(0, H)
    cx = np.random.randint(0, W)
    return (int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H)),
            int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W)))


@pytest.mark.parametrize("correct_lam", [True, False])
def test_batch_mode_draw_follows_the_documented_order_of_numpy_calls(correct_lam):
    H, W, prob, switch = 12, 14, 0.8, 0.5
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=prob, switch_prob=switch, mode="batch", correct_lam=correct_lam, num_classes=10)
    kinds = set()
    for seed in range(40):
        np.random.seed(seed)
        m(*_data(4, H=H, W=W))
        got = (m.lam, m.use_cutmix, m.boxes.copy())
        np.random.seed(seed)                              # the same stream, drawn by hand
        lam, cut, box = 1., False, (0, 0, 0, 0)
        if np.random.rand() < prob:
            cut = bool(np.random.rand() < switch)
            lam = float(np.random.beta(1.0, 1.0) if cut else np.random.beta(0.8, 0.8))
            if cut:
                box = _expected_box(H, W, lam)
                if correct_lam:
                    lam = 1. - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
        if box[1] <= box[0] or box[3] <= box[2]:
            box = (0, 0, 0, 0)                            # (a box without area is recorded as zeros)
        assert got[0] == lam and got[1] == cut and (got[2] == np.array(box, dtype=np.int32)).all(), (seed, got, lam, cut, box)
        kinds.add("cut" if cut else "mix" if lam != 1. else "none")
    assert kinds == {"cut", "mix", "none"}


@pytest.mark.parametrize("mode", ["elem", "pair"])
@pytest.mark.parametrize("correct_lam", [True, False])
def test_elem_and_pair_mode_draw_follows_the_documented_order_of_numpy_calls(mode, correct_lam):
    H, W, B, prob = 12, 14, 8, 0.7
    n = B if mode == "elem" else B // 2
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=prob, mode=mode, correct_lam=correct_lam, num_classes=10)
    for seed in range(10):
        np.random.seed(seed)
        m(*_data(B, H=H, W=W))
        got = (m.lam.copy(), m.use_cutmix.copy(), m.boxes.copy())
        np.random.seed(seed)
        cut = np.random.rand(n) < 0.5
        lam_cut, lam_mix = np.random.beta(1.0, 1.0, size=n), np.random.beta(0.8, 0.8, size=n)
        lam = np.where(np.random.rand(n) < prob, np.where(cut, lam_cut, lam_mix).astype(np.float32), np.float32(1)).astype(np.float32)
        boxes = np.zeros((n, 4), dtype=np.int32)
        for i in range(n):
            if lam[i] != 1. and cut[i]:
                b = _expected_box(H, W, lam[i])
                if correct_lam:
                    lam[i] = 1. - (b[1] - b[0]) * (b[3] - b[2]) / float(H * W)
                if b[1] > b[0] and b[3] > b[2]:
                    boxes[i] = b
        if mode == "pair":
            lam, cut, boxes = np.concatenate((lam, lam[::-1])), np.concatenate((cut, cut[::-1])), np.concatenate((boxes, boxes[::-1]))
        assert np.array_equal(got[0], lam) and got[0].dtype == np.float32, (seed, got[0], lam)
        assert np.array_equal(got[1], cut) and np.array_equal(got[2], boxes), (seed, got[2], boxes)


def test_min_max_boxes_lie_inside_and_always_correct_lam():
    H, W = 12, 14
    m = sm.Mixup(mixup_alpha=0., cutmix_alpha=0., cutmix_minmax=(0.25, 0.75), mode="elem", correct_lam=False, num_classes=10)
    np.random.seed(0)
    for _ in range(10):
        m(*_data(8, H=H, W=W))
        for lam, cut, (yl, yh, xl, xh) in zip(m.lam, m.use_cutmix, m.boxes):
            assert cut and 0 <= yl < yh <= H and 0 <= xl < xh <= W
            assert int(H * 0.25) <= yh - yl < int(H * 0.75) and int(W * 0.25) <= xh - xl < int(W * 0.75)
            assert lam == np.float32(1. - (yh - yl) * (xh - xl) / float(H * W))      # (min-max corrects lam whatever correct_lam says)


def test_an_empty_cpu_batch_takes_the_torch_lines():
    m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=10)
    x, t = m(torch.zeros(0, 3, 4, 4), torch.zeros(0, dtype=torch.int64))
    assert x.shape == (0, 3, 4, 4) and t.shape == (0, 10)
    assert sm.mixup._kernel_ok(torch.zeros(0, 3, 4, 4)) is False
