"""Mixup / CutMix of a batch, the reference's ``mixup_fn`` (main.py:505-517 builds ``timm.data.Mixup``; engine.py:46-47 calls
``samples, targets = mixup_fn(samples, targets)`` in every step; the default run is ``--mixup 0.8 --cutmix 1.0 --smoothing 0.1``).

timm is not installed where this package is developed or run, so ``Mixup`` restates timm 0.4.12's ``timm/data/mixup.py`` from its
documented behaviour rather than from its text: the random draws (``np.random`` on the host, in timm's order), the box rule, the
lam correction, the smoothed one-hot targets and -- because bit-equality hangs on it -- where each factor is rounded.

Upstream the images cost a flipped copy and three in-place passes over the whole batch, the targets eight small launches.  Here a
CUDA f32 contiguous batch goes through two kernels: ``smoe_mixup_images`` (one read and one write of each image, in place, any
mix of Mixup / CutMix samples inside a pair) and ``smoe_mixup_target`` (one launch), with the per-sample factors and boxes sent by
ONE non-blocking copy from a persistent pinned buffer: no device-to-host copy, no synchronisation in steady state.  Anything else (CPU tensors, other dtypes or
layouts) takes timm's torch lines -- both paths produce the same bits.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


def one_hot(x: torch.Tensor, num_classes: int, on_value: float = 1., off_value: float = 0.) -> torch.Tensor:
    x = x.long().view(-1, 1)
    return torch.full((x.size(0), num_classes), off_value, device=x.device).scatter_(1, x, on_value)


def mixup_target(target: torch.Tensor, num_classes: int, lam=1., smoothing: float = 0.0) -> torch.Tensor:
    """timm's ``mixup_target`` in torch: ``lam`` a Python float (batch mode) or an f32 [B, 1] tensor (elem / pair mode)."""
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    y1 = one_hot(target, num_classes, on_value=on_value, off_value=off_value)
    y2 = one_hot(target.flip(0), num_classes, on_value=on_value, off_value=off_value)
    return y1 * lam + y2 * (1. - lam)


def rand_bbox(img_shape, lam, count=None):
    """A box of area ratio 1 - lam around a uniformly drawn centre, clipped to the image: (yl, yh, xl, xh)."""
    ratio = np.sqrt(1 - lam)
    img_h, img_w = img_shape[-2:]
    cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
    cy = np.random.randint(0, img_h, size=count)
    cx = np.random.randint(0, img_w, size=count)
    yl = np.clip(cy - cut_h // 2, 0, img_h)
    yh = np.clip(cy + cut_h // 2, 0, img_h)
    xl = np.clip(cx - cut_w // 2, 0, img_w)
    xh = np.clip(cx + cut_w // 2, 0, img_w)
    return yl, yh, xl, xh


def rand_bbox_minmax(img_shape, minmax, count=None):
    """The min-max variant: side lengths drawn between the two fractions of the image's, the box placed wholly inside."""
    assert len(minmax) == 2
    img_h, img_w = img_shape[-2:]
    cut_h = np.random.randint(int(img_h * minmax[0]), int(img_h * minmax[1]), size=count)
    cut_w = np.random.randint(int(img_w * minmax[0]), int(img_w * minmax[1]), size=count)
    yl = np.random.randint(0, img_h - cut_h, size=count)
    xl = np.random.randint(0, img_w - cut_w, size=count)
    return yl, yl + cut_h, xl, xl + cut_w


def cutmix_bbox_and_lam(img_shape, lam, ratio_minmax=None, correct_lam=True, count=None):
    if ratio_minmax is not None:
        yl, yu, xl, xu = rand_bbox_minmax(img_shape, ratio_minmax, count=count)
    else:
        yl, yu, xl, xu = rand_bbox(img_shape, lam, count=count)
    if correct_lam or ratio_minmax is not None:
        bbox_area = (yu - yl) * (xu - xl)
        lam = 1. - bbox_area / float(img_shape[-2] * img_shape[-1])
    return (yl, yu, xl, xu), lam


def _kernel_ok(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and 0 < x.shape[0] <= 131070 and x.is_contiguous()
            and x.data_ptr() % 4 == 0 and x.numel() // x.shape[0] < 2 ** 31)


_RING = 8          # pinned staging buffers per batch size: a buffer is rewritten only after the copy that read it has completed
_staging = {}      # B -> [next slot, [(pinned int32 [8 * B], event or None)] * _RING]


def _send_table(img_lam, img_om, tgt_lam, tgt_om, boxes, device):
    """The call's per-sample tables in ONE non-blocking copy: a flat int32 buffer of 8 * B words -- words [0, B) img_lam, [B, 2B) img_om,
    [2B, 3B) tgt_lam, [3B, 4B) tgt_om (f32 bit patterns), [4B, 8B) the boxes, [B, 4] row-major.  Staged in persistent pinned buffers
    (a ring per batch size; the event of a slot's last copy is waited for before the slot is rewritten -- it completed steps ago):
    no allocation per call and no synchronisation in steady state (the wait is a host wait on an event recorded _RING calls ago).  The
    ring is keyed by B alone, so devices and streams share slots: the per-slot event is what keeps that right.  Returns (img_lam, img_om, tgt_lam, tgt_om f32 [B], boxes i32 [B, 4]) on the device."""
    B = len(img_lam)
    ring = _staging.get(B)
    if ring is None:
        if len(_staging) > 16:
            _staging.clear()
        ring = _staging[B] = [0, [[torch.empty(8 * B, dtype=torch.int32).pin_memory(), None] for _ in range(_RING)]]
    slot = ring[1][ring[0]]
    ring[0] = (ring[0] + 1) % _RING
    host, done = slot
    if done is not None:
        done.synchronize()
    hf = host.view(torch.float32)
    for k, a in enumerate((img_lam, img_om, tgt_lam, tgt_om)):
        hf[k * B:(k + 1) * B] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    host[4 * B:] = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.int32)).reshape(-1)
    dev = host.to(device, non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record(torch.cuda.current_stream(device))
    df = dev.view(torch.float32)
    return df[0:B], df[B:2 * B], df[2 * B:3 * B], df[3 * B:4 * B], dev[4 * B:].view(B, 4)


class Mixup:
    """``timm.data.Mixup``: ``Mixup(mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
    correct_lam=True, label_smoothing=0.1, num_classes=1000)``; ``mixup_fn(x, target) -> (x, target)`` mixes ``x`` [B, C, H, W] IN
    PLACE (sample b with sample B-1-b; B even) and returns the mixed, smoothed targets f32 [B, num_classes].

    ``mode``: 'batch' (one draw for the whole batch), 'pair' (one per pair) or 'elem' (one per sample).  A draw: with probability
    ``prob`` the sample is mixed, by CutMix with probability ``switch_prob`` when both alphas are positive (else by the one that
    is), with ``lam ~ Beta(alpha, alpha)``; an unmixed sample has lam = 1 and is left untouched.  CutMix pastes the partner's pixels
    into a box of area ratio 1 - lam (``cutmix_minmax``: side lengths drawn between two fractions instead) and, with
    ``correct_lam``, sets lam to the share of the image the clipped box really left.  Targets: ``y1 * lam + y2 * (1 - lam)`` of the
    one-hot rows of the sample and its partner with ``off = smoothing / num_classes``, ``on = 1 - smoothing + off``.

    Rounding: in batch mode lam is a Python float and the partner's factor is f32(1.0 - lam), the difference taken in double; in
    elem / pair mode the lam array is f32 and the partner's factor is f32(1) - lam in f32 -- for images and targets alike.

    The last call's draw stays readable: ``lam`` (float, or f32 [B]), ``use_cutmix`` (bool, or bool [B]) and ``boxes`` (int32 [B, 4]:
    yl, yh, xl, xh; zeros where no box was drawn), so a caller can replay it."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0     # the min-max box ignores lam; cutmix is on
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        assert mode in ('batch', 'pair', 'elem'), f"Mixup: unknown mode {mode!r}"
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True       # (set to False to switch the mixing off, as timm's users do at the end of training)
        self.lam, self.use_cutmix, self.boxes = 1., False, None

    # -- the draws (host) ----------------------------------------------------------------------------------------------------
    def _params_per_elem(self, batch_size):
        lam = np.ones(batch_size, dtype=np.float32)
        use_cutmix = np.zeros(batch_size, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand(batch_size) < self.switch_prob
                lam_mix = np.where(use_cutmix, np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size),
                                   np.random.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size))
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size)
            elif self.cutmix_alpha > 0.:
                use_cutmix = np.ones(batch_size, dtype=bool)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size)
            else:
                assert False, "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
            lam = np.where(np.random.rand(batch_size) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _params_per_batch(self):
        lam, use_cutmix = 1., False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = bool(np.random.rand() < self.switch_prob)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.:
                use_cutmix = True
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha)
            else:
                assert False, "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
            lam = float(lam_mix)
        return lam, use_cutmix

    def _draw(self, shape):
        """The whole call's draw, in timm's order.  Returns per-sample tables (what the kernels take, and what the torch lines below
        replay): ``img_lam`` / ``img_om`` f32 [B] (1 / 0 = the image stays as it is), ``tgt_lam`` / ``tgt_om`` f32 [B], ``boxes`` i32 [B, 4]
        (non-empty = CutMix) -- and records ``lam`` / ``use_cutmix`` / ``boxes`` on the object."""
        B = shape[0]
        boxes = np.zeros((B, 4), dtype=np.int32)
        img_lam, img_om = np.ones(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
        if self.mode == 'batch':
            lam, use_cutmix = self._params_per_batch()
            if lam != 1.:
                if use_cutmix:
                    box, lam = cutmix_bbox_and_lam(shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                    lam = float(lam)
                    boxes[:] = [int(v) for v in box]
                else:
                    img_lam[:] = np.float32(lam)
                    img_om[:] = np.float32(1. - lam)         # (the difference in double, rounded once)
            tgt_lam = np.full(B, lam, dtype=np.float32)
            tgt_om = np.full(B, 1. - lam, dtype=np.float32)
        else:
            n = B if self.mode == 'elem' else B // 2
            lam, use_cutmix = self._params_per_elem(n)
            for i in range(n):
                if lam[i] != 1.:
                    if use_cutmix[i]:
                        box, lam_i = cutmix_bbox_and_lam(shape, lam[i], ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                        boxes[i] = [int(v) for v in box]
                        lam[i] = lam_i
                    else:
                        img_lam[i] = lam[i]
                        img_om[i] = np.float32(1) - lam[i]   # (in f32)
            if self.mode == 'pair':
                lam, use_cutmix = np.concatenate((lam, lam[::-1])), np.concatenate((use_cutmix, use_cutmix[::-1]))
                boxes[n:] = boxes[:n][::-1]
                img_lam[n:], img_om[n:] = img_lam[:n][::-1], img_om[:n][::-1]
            tgt_lam = lam.astype(np.float32)
            tgt_om = np.float32(1) - tgt_lam
        empty = (boxes[:, 1] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 2])
        boxes[empty] = 0                                     # a box without area pastes nothing: the image stays as it is
        cut = ~empty
        img_lam[cut], img_om[cut] = 0., 0.                   # (a CutMix sample's factors are not used; lam == 1 would say "untouched")
        self.lam, self.use_cutmix, self.boxes = lam, use_cutmix, boxes
        return img_lam, img_om, tgt_lam, tgt_om, boxes

    # -- timm's torch lines --------------------------------------------------------------------------------------------------
    def _mix_torch(self, x, img_lam, img_om, boxes):
        B = len(x)
        if B == 0:
            return
        if self.mode == 'batch':
            yl, yh, xl, xh = (int(v) for v in boxes[0])
            if yh > yl and xh > xl:
                x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
            elif not self.use_cutmix and self.lam != 1.:
                lam = self.lam
                x_flipped = x.flip(0).mul_(1. - lam)
                x.mul_(lam).add_(x_flipped)
            return
        x_orig = x.clone()
        for i in range(B):
            j = B - i - 1
            yl, yh, xl, xh = (int(v) for v in boxes[i])
            if yh > yl and xh > xl:
                x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
            elif img_lam[i] != 1.:
                x[i] = x[i] * img_lam[i] + x_orig[j] * img_om[i]

    def __call__(self, x: torch.Tensor, target: torch.Tensor):
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        img_lam, img_om, tgt_lam, tgt_om, boxes = self._draw(tuple(x.shape))
        # (batch-mode Mixup with lam within 2^-25 of 1 but not 1: timm multiplies by f32(lam) = 1 and still adds the partner's share,
        # the kernel would read lam == 1 as "untouched" -- once in 10^7 draws, on the torch lines)
        odd = self.mode == 'batch' and not self.use_cutmix and self.lam != 1. and np.float32(self.lam) == 1.
        if _kernel_ok(x) and not odd:
            B = len(x)
            d_lam, d_om, d_tlam, d_tom, d_box = _send_table(img_lam, img_om, tgt_lam, tgt_om, boxes, x.device)
            if bool((img_lam != 1.).any()):                  # (all lam == 1: no image changes)
                ops.mixup_images_(x, d_lam, d_om, d_box)
            labels = target.to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
            assert labels.numel() == B, "Mixup: one label per sample expected"
            off = self.label_smoothing / self.num_classes
            return x, ops.mixup_target(labels, d_tlam, d_tom, 1. - self.label_smoothing + off, off, self.num_classes)
        self._mix_torch(x, img_lam, img_om, boxes)
        if self.mode == 'batch':
            lam = self.lam
        else:
            lam = torch.tensor(self.lam, device=x.device, dtype=x.dtype).unsqueeze(1)
        return x, mixup_target(target, self.num_classes, lam, self.label_smoothing)
