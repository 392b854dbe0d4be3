"""The reference's training criteria (main.py:653-664): ``timm.loss.SoftTargetCrossEntropy`` when Mixup / CutMix is on (targets are
dense rows), ``timm.loss.LabelSmoothingCrossEntropy`` when it is off and ``--smoothing`` > 0; engine.py:54 calls them in every step.

timm is not installed where this package is developed or run: the two modules restate timm 0.4.12's ``timm/loss/cross_entropy.py``
from its documented behaviour.  Upstream each is a torch composition -- log-softmax, multiply, negate, two sums, and their backward:
about ten small launches inside a step whose kernels are all small (profiles/r05_tiny_models.md).  Here CUDA logits go through ONE
``torch.autograd.Function`` over ``smoe_soft_ce_fwd`` / ``smoe_soft_ce_bwd``: two launches forward, one backward, deterministic, no
host sync, capturable (engine.GraphedTrainStep).  Under autocast the 16-bit logits are taken as they are (the kernels compute in
f32); the loss is an f32 scalar.  Anything else (CPU tensors, other dtypes or layouts, targets that need a gradient) takes timm's
torch lines.

``DistillationLoss`` is the reference's ``losses.py`` (main.py:688: every run's criterion is one, ``--distillation-type none`` included): the base
criterion on the class-token logits, blended with a distillation term between the distillation-token logits and a teacher's.  CUDA
logits go through one ``torch.autograd.Function`` over ``smoe_distill_fwd`` / ``smoe_distill_bwd`` -- two launches forward, one backward
(upstream: two log-softmaxes, two divisions, kl_div, sum, two scalings and the blend, and their backward); everything else takes the
reference's torch lines.

``BCEWithLogitsLoss`` is the criterion of ``--bce-loss`` (main.py:663-664 ``torch.nn.BCEWithLogitsLoss()``), a subclass with the upstream
constructor.  CUDA logits go through one ``torch.autograd.Function`` over ``smoe_bce_fwd`` / ``smoe_bce_bwd`` -- two launches forward, one
backward; with ``binarize=True`` the kernels also apply engine.py:49-50's ``targets.gt(0.0)``, and ``engine.train_one_epoch`` leaves
that line (a [B, C] intermediate and two launches) out.  ``weight`` / ``pos_weight`` / other reductions take torch's line.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


class _SoftCrossEntropy(torch.autograd.Function):
    """mean over rows of sum(-t log_softmax(x)); ``dense``: f32 [B, C] target rows, else i64 [B] labels + ``smoothing``."""

    @staticmethod
    def forward(ctx, logits, target, dense: bool, smoothing: float):
        loss, rows = ops.soft_ce_fwd(logits, target if dense else None, None if dense else target, smoothing)
        ctx.save_for_backward(logits, target, rows)
        ctx.dense, ctx.smoothing = dense, smoothing
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target, rows = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.float()
        dx = ops.soft_ce_bwd(logits, rows, g.contiguous(), target if ctx.dense else None, None if ctx.dense else target, ctx.smoothing)
        return dx, None, None, None


def _logits_ok(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype in _DTYPES and x.dim() >= 1 and x.is_contiguous() and x.shape[-1] > 0 and x.data_ptr() % 4 == 0
            and 0 < x.numel() // x.shape[-1] <= 65535)


class SoftTargetCrossEntropy(nn.Module):
    """``timm.loss.SoftTargetCrossEntropy``: ``forward(x, target) = mean(sum(-target * log_softmax(x, dim=-1), dim=-1))``."""

    def __init__(self):
        super().__init__()

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if (_logits_ok(x) and target.shape == x.shape and target.device == x.device and target.is_floating_point()
                and not target.requires_grad):
            C = x.shape[-1]
            t = target.detach().reshape(-1, C)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 4:
                t = t.float().contiguous()
            return _SoftCrossEntropy.apply(x.reshape(-1, C), t, True, 0.0)
        loss = torch.sum(-target * F.log_softmax(x, dim=-1), dim=-1)
        return loss.mean()


class LabelSmoothingCrossEntropy(nn.Module):
    """``timm.loss.LabelSmoothingCrossEntropy(smoothing=0.1)``: ``(1 - smoothing) * nll + smoothing * mean(-log_softmax(x))`` per row,
    averaged; ``smoothing=0`` is plain cross-entropy.  ``x`` [B, C], ``target`` integer labels [B]."""

    def __init__(self, smoothing: float = 0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if (_logits_ok(x) and x.dim() == 2 and target.dim() == 1 and target.numel() == x.shape[0] and target.device == x.device
                and not target.is_floating_point()):
            return _SoftCrossEntropy.apply(x, target.to(torch.int64).contiguous(), False, float(self.smoothing))
        logprobs = F.log_softmax(x, dim=-1)
        nll_loss = -logprobs.gather(dim=-1, index=target.unsqueeze(1))
        nll_loss = nll_loss.squeeze(1)
        smooth_loss = -logprobs.mean(dim=-1)
        loss = self.confidence * nll_loss + self.smoothing * smooth_loss
        return loss.mean()


class _Distill(torch.autograd.Function):
    """``base * (1 - alpha) + distill(student, teacher) * alpha`` (losses.py:53-72) on smoe_distill_fwd / smoe_distill_bwd."""

    @staticmethod
    def forward(ctx, base_loss, student, teacher, mode: str, tau: float, alpha: float):
        loss, _, _, stats, labels = ops.distill_fwd(student, teacher, base_loss.detach().reshape(()), mode, tau, alpha)
        ctx.save_for_backward(student, teacher, stats, labels)
        ctx.mode, ctx.tau, ctx.alpha = mode, tau, alpha
        return loss

    @staticmethod
    def backward(ctx, g):
        student, teacher, stats, labels = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.float()
        g = g.contiguous()
        dx = ops.distill_bwd(student, teacher, stats, labels, g, ctx.mode, ctx.tau, ctx.alpha) if ctx.needs_input_grad[1] else None
        return (g * (1 - ctx.alpha) if ctx.needs_input_grad[0] else None), dx, None, None, None, None


class DistillationLoss(nn.Module):
    """The reference's ``losses.DistillationLoss``: wraps a standard criterion and adds a knowledge-distillation loss that takes a
    teacher model's prediction as additional supervision.  ``forward(inputs, outputs, labels)``: ``inputs`` go to the teacher,
    ``outputs`` is the student's ``(class-token logits, distillation-token logits)`` pair (DistilledVisionTransformer in training
    mode), ``labels`` go to the base criterion.  ``soft``: KL(teacher || student) at temperature ``tau``, summed, times
    ``tau^2 / numel``; ``hard``: cross-entropy against the teacher's argmax; the result is ``base * (1 - alpha) + distill * alpha``."""

    def __init__(self, base_criterion: nn.Module, teacher_model: nn.Module, distillation_type: str, alpha: float, tau: float):
        super().__init__()
        self.base_criterion = base_criterion
        self.teacher_model = teacher_model
        assert distillation_type in ['none', 'soft', 'hard']
        self.distillation_type = distillation_type
        self.alpha = alpha
        self.tau = tau

    def forward(self, inputs, outputs, labels):
        outputs_kd = None
        if not isinstance(outputs, torch.Tensor):
            outputs, outputs_kd = outputs       # the model returns (outputs, outputs_kd)
        base_loss = self.base_criterion(outputs, labels)
        if self.distillation_type == 'none':
            return base_loss
        if outputs_kd is None:
            raise ValueError("When knowledge distillation is enabled, the model is "
                             "expected to return a Tuple[Tensor, Tensor] with the output of the "
                             "class_token and the dist_token")
        with torch.no_grad():                   # no backpropagation through the teacher
            teacher_outputs = self.teacher_model(inputs)
        if self._kernel_ok(base_loss, outputs_kd, teacher_outputs):
            return _Distill.apply(base_loss if base_loss.dtype == torch.float32 else base_loss.float(), outputs_kd, teacher_outputs,
                                  self.distillation_type, float(self.tau), float(self.alpha))
        if self.distillation_type == 'soft':
            T = self.tau
            distillation_loss = F.kl_div(F.log_softmax(outputs_kd / T, dim=1), F.log_softmax(teacher_outputs / T, dim=1),
                                         reduction='sum', log_target=True) * (T * T) / outputs_kd.numel()
        else:
            distillation_loss = F.cross_entropy(outputs_kd, teacher_outputs.argmax(dim=1))
        return base_loss * (1 - self.alpha) + distillation_loss * self.alpha

    def _kernel_ok(self, base_loss, kd, teacher) -> bool:
        return (isinstance(teacher, torch.Tensor) and isinstance(base_loss, torch.Tensor) and _logits_ok(kd) and kd.dim() == 2
                and _logits_ok(teacher) and teacher.shape == kd.shape and teacher.device == kd.device and not teacher.requires_grad
                and base_loss.dim() == 0 and base_loss.device == kd.device and base_loss.is_floating_point()
                and isinstance(self.tau, (int, float)) and self.tau > 0 and isinstance(self.alpha, (int, float)))


class _BCEWithLogits(torch.autograd.Function):
    """mean over all elements of the binary cross-entropy between ``logits`` and f32 ``target`` (read as ``target > 0`` when
    ``binarize``) on smoe_bce_fwd / smoe_bce_bwd."""

    @staticmethod
    def forward(ctx, logits, target, binarize: bool):
        loss, _ = ops.bce_fwd(logits, target, binarize)
        ctx.save_for_backward(logits, target)
        ctx.binarize = binarize
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.float()
        return ops.bce_bwd(logits, target, g.contiguous(), ctx.binarize), None, None


class BCEWithLogitsLoss(nn.BCEWithLogitsLoss):
    """``torch.nn.BCEWithLogitsLoss`` (main.py:663-664, ``--bce-loss``) with one keyword-only extension: ``binarize=True`` scores every
    target as ``target > 0`` -- engine.py:49-50's ``targets = targets.gt(0.0).type(targets.dtype)`` without the intermediate tensor
    (``train_one_epoch`` then leaves that line out).  CUDA logits with a floating-point target of their shape that needs no gradient,
    no ``weight`` / ``pos_weight`` and ``reduction='mean'`` go through the kernels: two launches forward, one backward; the loss is
    an f32 scalar.  Anything else takes torch's line (after the ``gt`` line when ``binarize``)."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction: str = 'mean', pos_weight=None, *,
                 binarize: bool = False):
        super().__init__(weight, size_average, reduce, reduction, pos_weight)
        self.binarize = bool(binarize)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        x = input
        if (self.weight is None and self.pos_weight is None and self.reduction == 'mean' and _logits_ok(x)
                and target.shape == x.shape and target.device == x.device and target.is_floating_point() and not target.requires_grad):
            C = x.shape[-1]
            t = target.detach().reshape(-1, C)
            if t.dtype != torch.float32:      # (binarized in its own dtype: a positive f64 target may round to 0 in f32)
                t = (t.gt(0.0) if self.binarize else t).float()
            if not t.is_contiguous() or t.data_ptr() % 4:
                t = t.contiguous()
            return _BCEWithLogits.apply(x.reshape(-1, C), t, self.binarize)
        if self.binarize:
            target = target.gt(0.0).type(target.dtype)
        return F.binary_cross_entropy_with_logits(input, target, self.weight, pos_weight=self.pos_weight, reduction=self.reduction)
