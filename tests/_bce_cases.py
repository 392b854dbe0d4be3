"""The inputs the BCE-with-logits tests share (tests/test_bce_loss_host.py on the CPU, tests/test_gpu_bce_loss.py on the GPU): the same
rows on both sides, so that the float64 reference the GPU bars lean on is itself checked on the host."""
import numpy as np
import torch
import torch.nn.functional as F

import slim_switch_moe_vit_amd as sm

BATCHES = (1, 2, 7, 128)
CLASSES = (1, 3, 10, 100, 1000, 1001, 1008)
KINDS = ("mixup", "mixup_smoothed", "binary", "uniform")
SCALES = (1.0, 30.0, 200.0)
SPECIAL = (-1.0, -0.0, 0.0, 1e-45, 0.1 / 1000, 1.0, float("nan"))      # engine.py:50's `> 0` on these: 0, 0, 0, 1, 1, 1, 0
SPECIAL_BITS = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0)


def targets(kind: str, B: int, C: int) -> torch.Tensor:
    """f32 [B, C] on the CPU.  mixup / mixup_smoothed: ``Mixup``'s own rows at smoothing 0 / 0.1 (an even batch is drawn and cut to B);
    binary: {0, 1}; uniform: U[0, 1)."""
    g = torch.Generator().manual_seed(1000 * B + C)
    if kind in ("mixup", "mixup_smoothed"):
        Be = B + B % 2
        np.random.seed(B * 31 + C)
        m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.0 if kind == "mixup" else 0.1, num_classes=C)
        _, t = m(torch.zeros(Be, 3, 4, 4), torch.randint(0, C, (Be,), generator=g))
        return t[:B].contiguous()
    if kind == "binary":
        return (torch.rand(B, C, generator=g) < 0.3).float()
    assert kind == "uniform"
    return torch.rand(B, C, generator=g)


def logits(B: int, C: int, scale: float, dtype=torch.float32) -> torch.Tensor:
    """[B, C] on the CPU in ``dtype``: N(0, scale^2), rounded to the type (the references start from the rounded values)."""
    g = torch.Generator().manual_seed(7 * B + 13 * C + int(scale))
    return (torch.randn(B, C, generator=g) * scale).to(dtype)


def ref64(x: torch.Tensor, t: torch.Tensor, g: float = 1.0):
    """``F.binary_cross_entropy_with_logits`` in float64 on the host with autograd: (loss, row sums [B], g * d loss / d logits)."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    el = F.binary_cross_entropy_with_logits(x64, t.detach().double().cpu(), reduction="none")
    loss = el.mean()
    (loss * g).backward()
    return loss.detach(), el.detach().sum(1), x64.grad


def emulate64(x: torch.Tensor, t: torch.Tensor, binarize: bool, g: float = 1.0):
    """The kernels' arithmetic written out in float64: the element formula, the row sums, the mean as (sum of rows) / (B C), and the
    two-branch gradient from e = exp(-|x|)."""
    x, t = x.detach().double().cpu(), t.detach().double().cpu()
    if binarize:
        t = torch.where(t > 0, torch.ones_like(t), torch.zeros_like(t))
    el = torch.clamp_min(x, 0) - x * t + torch.log1p(torch.exp(-x.abs()))
    rows = el.sum(1)
    e = torch.exp(-x.abs())
    r = e / (1 + e)
    d = torch.where(x >= 0, (1 - t) - r, r - t)
    return rows.sum() / (x.shape[0] * x.shape[1]), rows, d * (g / (x.shape[0] * x.shape[1]))


def term_scale(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """f64 [B]: per row, sum_c (|x_c| + 1) -- the size of the terms ANY formulation of the element loss handles (torch's own is
    (1 - t) x - log_sigmoid(x)).  Errors of the loss and of the row sums are measured in units of it (of its mean over the elements
    for the loss): the value itself can be as small as exp(-200) while its terms are of size 200, and torch's float64 result has an
    absolute error of an ulp of |x| there (it returns 0 for x = -40, t = 0), so an error relative to the VALUE would measure the
    reference, not the code under test."""
    return (x.detach().double().cpu().abs() + 1.0).sum(1)
