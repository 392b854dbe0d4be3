"""Optimizer side of the reference's training step on the HIP path.

The reference trains with ``timm.optim.create_optimizer_v2(..., opt="adamw")`` (main.py:729-731; ``--opt adamw``,
``--opt-eps 1e-8``, ``--weight-decay 0.05``) = ``torch.optim.AdamW``, stepped through ``timm.utils.NativeScaler``
(main.py:732, engine.py:68-74):

    loss_scaler(loss, optimizer, clip_grad=max_norm, parameters=model.parameters(), create_graph=is_second_order)

i.e. ``scaler.scale(loss).backward(); scaler.unscale_(optimizer); clip_grad_norm_(parameters, clip_grad);
scaler.step(optimizer); scaler.update()``.  The MoE's expert tensors are ``[E,h,d]`` / ``[E,d,h]`` f32 -- 150 MB per layer
at ViT-B, E = 8 -- and every one of those calls is a full HBM pass (or two) over them and their gradients.  Here the
same step is TWO passes: ``ops``-level kernels ``smoe_grad_sumsq`` (norm + non-finite check on the still-scaled
gradient) and ``smoe_adamw_step`` (the update, reading the gradient times ``inv_scale x clip coefficient``), with the loss
scale, the non-finite flag, the clip coefficient and the step count all living on the device: no host sync in the step.

``AdamW`` and ``NativeScaler`` keep the call signatures, ``state_dict`` keys and numerics of what they replace; CPU
tensors (and non-f32 parameters) fall back to the torch composition, which is also what the tests compare against.

``Lamb`` is ``timm.optim.Lamb`` (the DeiT-III recipes' ``--opt lamb``; the reference hands ``--opt`` to timm's factory) restated, with a
fused step of four launches (csrc/lamb.hip) that keeps the global gradient norm, the trust ratios and the step count on the device; its
global norm comes out of ``NativeScaler``'s own pass over the gradients (``wants_grad_sumsq``), so the step is the same two passes over
the gradients as AdamW's plus one more over the parameters and moments.

``ModelEma`` is ``timm.utils.ModelEma`` (the reference trains with ``--model-ema`` on: main.py:81-84, 599-606; engine.py:77-78) with
its per-step update -- four torch launches per state-dict entry upstream -- as ONE launch of ``smoe_ema_update_multi``, bit-equal to
timm's line and skippable from the device, so that the graphed training step can capture it.
"""
from __future__ import annotations

from typing import Iterable, NamedTuple, Optional

import torch

import os

from . import _lib, ops
from ._cache import param_version, shadow_of

# the fused step also writes the 16-bit operand images of the weights it updates (A/B: SLIMMOE_ADAMW_SHADOW=0)
SHADOW_STEP = os.environ.get("SLIMMOE_ADAMW_SHADOW", "1") != "0"


def _hip_ok(p: torch.Tensor) -> bool:
    return p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()


SUMSQ_BLOCK = 16384   # elements per workgroup of every multi-tensor kernel: OPT_BLOCK of csrc/optim_table.h
_size_cache = {}      # (device, numels) -> [blk, nb, first]: what the multi-tensor launches need that depends on the tensor sizes only


def _size_tables(numels, device):
    """The cache entry of these tensor sizes: blk = int32 [2, n_blocks] on the device (tensor of workgroup b, 16K-element block inside
    it), nb = blocks per tensor, first = None until ``_first_block_table`` asks for it."""
    key = (str(device), tuple(numels))
    hit = _size_cache.get(key)
    if hit is None:
        import numpy as np
        nb = [(n + SUMSQ_BLOCK - 1) // SUMSQ_BLOCK for n in numels]
        tens = np.repeat(np.arange(len(numels), dtype=np.int32), nb)
        first = np.cumsum([0] + nb[:-1]) if nb else np.zeros(0, dtype=np.int64)
        index = (np.arange(int(sum(nb)), dtype=np.int64) - np.repeat(first, nb)).astype(np.int32)
        blk = torch.from_numpy(np.stack([tens, index]) if len(tens) else np.zeros((2, 0), dtype=np.int32)).to(device)
        if len(_size_cache) > 16:
            _size_cache.clear()
        hit = _size_cache[key] = [blk.contiguous(), nb, None]
    return hit


def _block_table(numels, device):
    """Workgroup -> (tensor, 16K-element block) map of the multi-tensor kernels and the blocks per tensor; cached."""
    return tuple(_size_tables(numels, device)[:2])


def _first_block_table(numels, device):
    """int32 [n_t + 1] on the device: first 16K-element block of every tensor in ``_block_table``'s order, the block count at the end
    (what smoe_lamb_trust_multi walks a tensor's block partials by).  The same cache entry."""
    hit = _size_tables(numels, device)
    if hit[2] is None:
        hit[2] = torch.tensor([sum(hit[1][:t]) for t in range(len(hit[1]) + 1)], dtype=torch.int32).to(device)
    return hit[2]


_staging = []          # pinned staging buffers of tables copied to the device while a HIP graph was being captured: kept for good
_staging_ring = []     # ... and of the eager steps: the last few (the copy is asynchronous)


def _host_table(rows, dtype, device):
    """A small table (addresses, element counts, per-tensor hyper-parameters) on the device.  The values change with every backward,
    so this is one small host-to-device copy per step -- from PINNED memory, asynchronously: it costs the host no wait, and it can be
    captured (a HIP graph of the whole training step replays the copy from the same pinned buffer, which therefore must outlive the
    graph: buffers staged during a capture are never released)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return torch.tensor(rows, dtype=dtype, device=dev)
    host = torch.tensor(rows, dtype=dtype).pin_memory()
    if torch.cuda.is_current_stream_capturing():
        _staging.append(host)
    else:
        _staging_ring.append(host)
        if len(_staging_ring) > 64:
            del _staging_ring[:32]
    return host.to(dev, non_blocking=True)


def _pointer_table(rows, device):
    """int64 [len(rows), n_t] on the device (addresses and element counts)."""
    return _host_table(rows, torch.int64, device)


class _Item(NamedTuple):
    # one parameter of a fused step: its group (lr, weight decay, ...), the parameter, its gradient and its two moments
    group: dict
    p: torch.Tensor
    g: torch.Tensor
    exp_avg: torch.Tensor
    exp_avg_sq: torch.Tensor


def _closure_loss(closure):
    with torch.enable_grad():
        return closure() if closure is not None else None


def _moment_state(state, p, with_step: bool):
    """state[p] with exp_avg / exp_avg_sq made at the parameter's first step (``with_step``: and torch.optim.AdamW's ``step`` = 0)."""
    st = state[p]
    if not st:
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if with_step:
            st["step"] = 0
    return st


def _step_tables(items, hyp_rows, dev):
    """One multi-tensor step launch's tab int64 [5][n_t] (p, g, exp_avg, exp_avg_sq addresses and n), hyp f32 [len(hyp_rows)][n_t] and
    shadow table int64 [2][n_t] (address / dtype of every 16-bit operand image that is current NOW, None without any: the kernel writes
    them in the same pass, so no cast pass over every weight follows the step), and the images to stamp: [(p, (cache, key, image))]."""
    tab = _pointer_table([[it.p.data_ptr() for it in items], [it.g.data_ptr() for it in items], [it.exp_avg.data_ptr() for it in items],
                          [it.exp_avg_sq.data_ptr() for it in items], [it.p.numel() for it in items]], dev)
    hyp = _host_table(hyp_rows, torch.float32, dev)
    shadows = [shadow_of(it.p) if SHADOW_STEP else None for it in items]
    sh_tab = None
    if any(sh is not None for sh in shadows):
        sh_tab = _pointer_table([[sh[2].data_ptr() if sh is not None else 0 for sh in shadows],
                                 [ops.dtype_code(sh[2].dtype) if sh is not None else 0 for sh in shadows]], dev)
    return tab, hyp, sh_tab, [(it.p, sh) for it, sh in zip(items, shadows) if sh is not None]


def _finish_step(params, images) -> None:
    """The kernels wrote the parameters through raw pointers: autograd's version counters did not move, and every derived tensor keyed
    on them (16-bit weight shadows, zero-row constants) would go on serving the OLD weights.  Bump the versions, as an in-place torch
    op would have; the images the step wrote itself belong to the NEW version of their parameter."""
    _bump_versions(params)
    for p, (cache, key, img) in images:
        cache.refresh(key, img, param_version(p))


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW(params, lr, betas, eps, weight_decay)`` (no amsgrad / maximize) with a fused HIP step.

    ``step(grad_mult=None, found_inf=None)``: optional device scalars (f32[1]) -- every gradient is multiplied by
    ``grad_mult`` on the fly, and the whole step (including the step count) is skipped when ``found_inf`` is non-zero;
    this is how ``NativeScaler`` drives it without unscaling gradients in memory or asking the host."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("AdamW: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._step_dev = {}       # device -> f32[1] number of updates applied so far (advanced on the device)
        self._step_restore = {}   # device -> count loaded from a checkpoint, applied when the counter is (re)created

    supports_device_scalars = True
    _slimmoe_refreshes_images = True     # (_foreign_step_hook: this step bumps the versions / refreshes the 16-bit images itself)

    def _step_counter(self, device) -> torch.Tensor:
        t = self._step_dev.get(device)
        if t is None:
            t = self._step_dev[device] = torch.full((1,), float(self._step_restore.pop(device, 0.0)), dtype=torch.float32,
                                                    device=device)
        return t

    def _on_hip_path(self, p) -> bool:
        return _hip_ok(p)

    # -- checkpoints (the reference saves / restores `optimizer.state_dict()`: main.py:898, 717) -------------------------------
    def state_dict(self):
        """torch.optim.AdamW's layout.  ``state[p]['step']`` is the number of updates APPLIED to p (the bias-correction
        t): for parameters on the HIP path that is the device-side counter (steps skipped for non-finite gradients are
        not counted), read back here -- a checkpoint is the one place where the host may ask."""
        for dev, t in self._step_dev.items():
            n = int(float(t))
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st and p.device == dev and self._on_hip_path(p):
                        st["step"] = n
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Restores exp_avg / exp_avg_sq AND the step count the kernels' bias correction uses (a ``torch.optim.AdamW``
        checkpoint carries ``step`` as a tensor per parameter, this class's own as an int: both load)."""
        super().load_state_dict(state_dict)
        self._step_dev, self._step_restore = {}, {}
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if not st or "step" not in st:
                    continue
                n = float(st["step"])          # tensor or number
                st["step"] = int(n)
                if self._on_hip_path(p):       # one counter per device: every tensor of a step shares t
                    self._step_restore[p.device] = max(self._step_restore.get(p.device, 0.0), n)

    @torch.no_grad()
    def step(self, closure=None, grad_mult: Optional[torch.Tensor] = None, found_inf: Optional[torch.Tensor] = None):
        loss = _closure_loss(closure)
        advanced = set()
        images = []    # [(parameter, (cache, key, image))]: 16-bit images the fused step wrote
        batches = {}   # (device, grad dtype, betas, eps) -> [_Item]: one launch each
        for group in self.param_groups:
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = _moment_state(self.state, p, with_step=True)
                g = p.grad
                if _hip_ok(p) and g.is_cuda and g.is_contiguous() and g.dtype in ops._DT:
                    batches.setdefault((p.device, g.dtype, float(b1), float(b2), float(eps)), []).append(
                        _Item(group, p, g, st["exp_avg"], st["exp_avg_sq"]))
                else:                 # torch composition (CPU tensors, other dtypes): same arithmetic
                    if found_inf is not None and float(found_inf) != 0.0:
                        continue
                    gg = g.float() * (float(grad_mult) if grad_mult is not None else 1.0)
                    st["step"] += 1
                    t = st["step"]
                    p.mul_(1 - lr * wd)
                    st["exp_avg"].lerp_(gg, 1 - b1)
                    st["exp_avg_sq"].mul_(b2).addcmul_(gg, gg, value=1 - b2)
                    denom = (st["exp_avg_sq"].sqrt() / (1 - b2 ** t) ** 0.5).add_(eps)
                    p.addcdiv_(st["exp_avg"], denom, value=-lr / (1 - b1 ** t))
        lib = _lib.load() if batches else None
        for (dev, gdt, b1, b2, eps), items in batches.items():
            lrs, wds = [float(it.group["lr"]) for it in items], [float(it.group["weight_decay"]) for it in items]
            step_t = self._step_counter(dev)
            stream = ops._stream(items[0].p)
            if dev not in advanced:   # one counter per device: every parameter of a step sees the same t
                _lib.check(lib.smoe_step_advance(step_t.data_ptr(), ops._ptr(found_inf), stream), "smoe_step_advance")
                advanced.add(dev)
            if len(items) == 1:
                it = items[0]
                rc = lib.smoe_adamw_step(it.p.data_ptr(), it.g.data_ptr(), ops.dtype_code(gdt), it.exp_avg.data_ptr(),
                                         it.exp_avg_sq.data_ptr(), it.p.numel(), lrs[0], b1, b2, eps, wds[0], step_t.data_ptr(),
                                         ops._ptr(grad_mult), ops._ptr(found_inf), stream)
                _lib.check(rc, "smoe_adamw_step")
                continue
            # every tensor of the batch in ONE launch (a ViT-B/16 MoE has ~180 parameter tensors)
            blk, nb = _block_table([it.p.numel() for it in items], dev)
            tab, hyp, sh_tab, written = _step_tables(items, [lrs, wds], dev)
            rc = lib.smoe_adamw_step_multi(tab.data_ptr(), hyp.data_ptr(), len(items), blk.data_ptr(), sum(nb), ops.dtype_code(gdt),
                                           b1, b2, eps, step_t.data_ptr(), ops._ptr(grad_mult), ops._ptr(found_inf), ops._ptr(sh_tab),
                                           stream)
            _lib.check(rc, "smoe_adamw_step_multi")
            images.extend(written)
        _finish_step([it.p for items in batches.values() for it in items], images)
        return loss


def _bump_versions(tensors) -> None:
    """``torch._C._increment_version`` is private API: newer releases take a list, older ones a single tensor.  If neither form
    works the derived-tensor caches are dropped wholesale -- slower (every shadow is re-cast on its next use), never stale."""
    try:
        torch._C._increment_version(tensors)
        return
    except (TypeError, AttributeError):
        pass
    try:
        for t in tensors:
            torch._C._increment_version(t)
    except (TypeError, AttributeError):
        from ._cache import invalidate_all
        invalidate_all()


def _grad_sumsq_launch(grads, mul, found_inf, device):
    """One ``smoe_grad_sumsq_multi`` launch per gradient dtype over the non-empty device tensors ``grads``: per dtype, ``(partials,
    gradients in launch order, blocks per gradient)``, partials = the 16K-element block sums of (g * *mul)^2; ``mul`` / ``found_inf``: f32[1] or None."""
    lib = _lib.load()
    by_dtype = {}
    for g in grads:
        if g.numel():
            by_dtype.setdefault(g.dtype, []).append(g)
    out = []
    for gdt, gs in by_dtype.items():
        numels = [g.numel() for g in gs]
        blk, nb = _block_table(numels, device)
        zeros = [0] * len(gs)
        tab = _pointer_table([zeros, [g.data_ptr() for g in gs], zeros, zeros, numels], device)
        part = torch.empty(sum(nb), dtype=torch.float32, device=device)
        rc = lib.smoe_grad_sumsq_multi(tab.data_ptr(), len(gs), blk.data_ptr(), sum(nb), ops.dtype_code(gdt), ops._ptr(mul),
                                       part.data_ptr(), ops._ptr(found_inf), ops._stream(part))
        _lib.check(rc, "smoe_grad_sumsq_multi")
        out.append((part, gs, nb))
    return out


def _grad_sumsq_partials(grads, mul, found_inf, device):
    # (the block partials alone, one tensor per gradient dtype)
    return [part for part, _, _ in _grad_sumsq_launch(grads, mul, found_inf, device)]


class Lamb(torch.optim.Optimizer):
    """``timm.optim.Lamb`` (timm 0.4.12 / 0.5: the DeiT-III recipes' ``--opt lamb``; main.py:90-96, 729-731) with a fused HIP step.

        G    = sqrt(sum over every p with a gradient, all groups, of sum(grad^2));   clip = G / max_grad_norm if G > max_grad_norm else 1
        per group: step += 1; beta3 = 1 - beta1 if grad_averaging else 1; bc1, bc2 = 1 - beta1^step, 1 - beta2^step (1 without bias_correction)
        per p:     g = grad / clip;  exp_avg = exp_avg * beta1 + beta3 * g;  exp_avg_sq = exp_avg_sq * beta2 + (1 - beta2) * g * g
                   u = (exp_avg / bc1) / (sqrt(exp_avg_sq) / sqrt(bc2) + eps) + weight_decay * p
                   if weight_decay != 0 or always_adapt:  r = ||p|| / ||u|| (1 where either is 0; at most 1 with trust_clip);  u *= r
                   p -= lr * u

    State per parameter: ``exp_avg``, ``exp_avg_sq``; the step count is ``param_groups[i]['step']`` (timm's layout, which checkpoints
    keep).  ``max_grad_norm`` is read from the defaults, as timm does.

    f32 contiguous parameters on one GPU with contiguous f32 / f16 / bf16 gradients take four launches per (gradient dtype, betas, eps)
    batch -- ``smoe_lamb_clip``, ``smoe_lamb_stage1_multi``, ``smoe_lamb_trust_multi``, ``smoe_lamb_stage2_multi`` (csrc/lamb.hip) --
    with G, the clip factor, the trust ratios and the step count on the device: no host sync, so the step can be captured.  The 16-bit
    operand images of the weights are written by the last launch.  If ANY tensor of the step is not of that kind (CPU tensors, non-f32
    parameters, non-contiguous gradients, several devices) the whole step is the rule above in f32 torch ops.

    ``step(grad_mult=None, found_inf=None, grad_sumsq=None)``: device f32[1] scalars as for ``AdamW`` -- every gradient counts times
    ``grad_mult``, a non-zero ``found_inf`` skips the step and its count.  ``grad_sumsq = (partials, taken_with)``: block partials of
    ``smoe_grad_sumsq_multi`` over every gradient of this optimizer, taken with the multiplier ``taken_with`` -- ``NativeScaler`` hands
    over the ones of its own non-finite / clipping pass (``wants_grad_sumsq``), so that G costs no second pass over the gradients; G is
    then ``grad_mult / taken_with`` times the root of their sum, the norm of the gradients a stock optimizer would see after unscale
    and clip.  Called bare, the step makes the norm pass itself.  ``last_grad_norm`` (f32[2] on the device: clip, G) and
    ``trust_ratios()`` expose what the last applied step used.

    The global norm is over THIS process's gradients, as timm's is: expert-parallel models (rank-private experts) get a rank-local
    norm, which is not what a single-process run of the same model computes."""

    supports_device_scalars = True
    _slimmoe_refreshes_images = True     # (_foreign_step_hook: this step bumps the versions / refreshes the 16-bit images itself)
    wants_grad_sumsq = True              # NativeScaler: pass the norm pass's block partials to step()

    def __init__(self, params, lr: float = 1e-3, bias_correction: bool = True, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, grad_averaging: bool = True, max_grad_norm: Optional[float] = 1.0,
                 trust_clip: bool = False, always_adapt: bool = False):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("Lamb: invalid hyper-parameter")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("Lamb: max_grad_norm must be positive (or None: no clipping)")
        super().__init__(params, dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay,
                                      grad_averaging=grad_averaging, max_grad_norm=max_grad_norm, trust_clip=trust_clip,
                                      always_adapt=always_adapt))
        self._step_dev = {}       # device -> f32[1] number of updates applied so far (advanced on the device)
        self._norm_dev = {}       # device -> f32[2]: clip, G of the last applied step
        self._trust = []          # [(parameters, f32 [n] trust ratios on the device or a list of floats)] of the last step
        self.last_grad_norm = None

    def _slimmoe_baked_hyper(self):
        """What a captured step bakes in besides lr / weight decay / betas / eps (engine.GraphedTrainStep._hyper)."""
        return (self.defaults["max_grad_norm"],) + tuple(
            (g["bias_correction"], g["grad_averaging"], g["trust_clip"], g["always_adapt"]) for g in self.param_groups)

    def _group_steps(self) -> int:
        return max([int(g.get("step", 0)) for g in self.param_groups] or [0])

    def _step_counter(self, device) -> torch.Tensor:
        t = self._step_dev.get(device)
        if t is None:        # (created from the groups' count: a loaded checkpoint, or earlier steps on the torch composition)
            t = self._step_dev[device] = torch.full((1,), float(self._group_steps()), dtype=torch.float32, device=device)
        return t

    def _steps_to_groups(self) -> None:
        """param_groups[i]['step'] = the device-side count (steps skipped for non-finite gradients are not counted)."""
        for t in self._step_dev.values():
            n = int(float(t))
            for group in self.param_groups:
                if n or "step" in group:
                    group["step"] = n

    def state_dict(self):
        """timm's layout: ``state[i] = {exp_avg, exp_avg_sq}``, ``param_groups[i]['step']``.  On the HIP path the count is read back
        from the device here -- a checkpoint is the one place where the host may ask."""
        self._steps_to_groups()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Restores the moments and the step count the bias correction uses (from ``param_groups[i]['step']``)."""
        super().load_state_dict(state_dict)
        self._step_dev = {}       # (re-created from the loaded groups at the next fused step)

    def trust_ratios(self):
        """{parameter: trust ratio the last applied step multiplied its update by} (asks the host)."""
        out = {}
        for params, r in self._trust:
            vals = r.tolist() if isinstance(r, torch.Tensor) else r
            out.update(zip(params, vals))
        return out

    @staticmethod
    def _fusable(p, g, m, v) -> bool:
        return (_hip_ok(p) and g.is_cuda and g.device == p.device and g.is_contiguous() and g.dtype in ops._DT
                and m.dtype == torch.float32 and v.dtype == torch.float32 and m.is_contiguous() and v.is_contiguous()
                and m.device == p.device and v.device == p.device
                and p.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
                and g.data_ptr() % (4 * g.element_size()) == 0)

    @torch.no_grad()
    def step(self, closure=None, grad_mult: Optional[torch.Tensor] = None, found_inf: Optional[torch.Tensor] = None,
             grad_sumsq=None):
        loss = _closure_loss(closure)
        entries = []      # _Item of every non-empty parameter with a gradient
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Lamb does not support sparse gradients, consider SparseAdam instead.")
                st = _moment_state(self.state, p, with_step=False)
                if p.numel():
                    entries.append(_Item(group, p, p.grad, st["exp_avg"], st["exp_avg_sq"]))
        if not entries:
            return loss
        dev = entries[0].p.device
        if all(it.p.device == dev and self._fusable(it.p, it.g, it.exp_avg, it.exp_avg_sq) for it in entries):
            self._fused_step(entries, dev, grad_mult, found_inf, grad_sumsq)
        else:
            self._torch_step(entries, grad_mult, found_inf)
        return loss

    def _torch_step(self, entries, grad_mult, found_inf) -> None:
        """The rule in f32 torch ops (CPU tensors, other dtypes, non-contiguous gradients)."""
        import math
        if self._step_dev:                  # earlier steps ran fused: carry their count over
            self._steps_to_groups()
            self._step_dev = {}
        if found_inf is not None and float(found_inf) != 0.0:
            return
        gm = float(grad_mult) if grad_mult is not None else 1.0
        grads = [it.g.float() * gm for it in entries]
        G = math.sqrt(sum(float(gg.pow(2).sum()) for gg in grads))
        mgn = self.defaults["max_grad_norm"]
        clip = G / mgn if (mgn is not None and G > mgn) else 1.0
        self.last_grad_norm = torch.tensor([clip, G], dtype=torch.float32)
        stepped, params, ratios = set(), [], []
        for (group, p, _, m, v), gg in zip(entries, grads):
            if id(group) not in stepped:
                group["step"] = int(group.get("step", 0)) + 1
                stepped.add(id(group))
            b1, b2 = group["betas"]
            beta3 = 1 - b1 if group["grad_averaging"] else 1.0
            t = group["step"]
            bc1, bc2 = (1 - b1 ** t, 1 - b2 ** t) if group["bias_correction"] else (1.0, 1.0)
            lr, wd = group["lr"], group["weight_decay"]
            p32, m32, v32 = p.float(), m.float(), v.float()      # (of an f32 tensor: the tensor itself, updated in place)
            gg = gg / clip
            m32.mul_(b1).add_(gg, alpha=beta3)
            v32.mul_(b2).addcmul_(gg, gg, value=1 - b2)
            u = (m32 / bc1).div_((v32.sqrt() / math.sqrt(bc2)).add_(group["eps"]))
            if wd != 0:
                u.add_(p32, alpha=wd)
            r = 1.0
            if wd != 0 or group["always_adapt"]:
                w_norm, u_norm = float(p32.norm(2.0)), float(u.norm(2.0))
                if w_norm > 0 and u_norm > 0:
                    r = w_norm / u_norm
                if group["trust_clip"]:
                    r = min(r, 1.0)
                u.mul_(r)
            p32.add_(u, alpha=-lr)
            if m32 is not m:
                m.copy_(m32)
            if v32 is not v:
                v.copy_(v32)
            if p32 is not p:
                p.copy_(p32)
            params.append(p)
            ratios.append(r)
        self._trust = [(params, ratios)]

    def _fused_step(self, entries, dev, grad_mult, found_inf, grad_sumsq) -> None:
        lib = _lib.load()
        stream = ops._stream(entries[0].p)
        step_t = self._step_counter(dev)
        # G and the clip factor, from the norm pass's block partials (the scaler's, or a pass of this step's own)
        if grad_sumsq is not None:
            partials, num, den = list(grad_sumsq[0]), grad_mult, grad_sumsq[1]
        else:
            partials, num, den = _grad_sumsq_partials([it.g for it in entries], grad_mult, None, dev), None, None
        part = partials[0] if len(partials) == 1 else torch.cat(partials)
        out = self._norm_dev.get(dev)
        if out is None:
            out = self._norm_dev[dev] = torch.tensor([1.0, 0.0], dtype=torch.float32, device=dev)
        mgn = self.defaults["max_grad_norm"]
        rc = lib.smoe_lamb_clip(part.data_ptr(), part.numel(), ops._ptr(num), ops._ptr(den), float(mgn) if mgn is not None else 0.0,
                                ops._ptr(found_inf), out.data_ptr(), stream)
        _lib.check(rc, "smoe_lamb_clip")
        self.last_grad_norm = out
        _lib.check(lib.smoe_step_advance(step_t.data_ptr(), ops._ptr(found_inf), stream), "smoe_step_advance")
        batches = {}      # (grad dtype, betas, eps, bias_correction, grad_averaging, trust_clip) -> entries: four launches each
        for it in entries:
            group = it.group
            b1, b2 = group["betas"]
            batches.setdefault((it.g.dtype, float(b1), float(b2), float(group["eps"]), bool(group["bias_correction"]),
                                bool(group["grad_averaging"]), bool(group["trust_clip"])), []).append(it)
        images = []
        self._trust = []
        for (gdt, b1, b2, eps, bias, averaging, trust_clip), items in batches.items():
            numels = [it.p.numel() for it in items]
            blk, nb = _block_table(numels, dev)
            first = _first_block_table(numels, dev)
            n_blocks = sum(nb)
            groups = [it.group for it in items]
            tab, hyp, sh_tab, written = _step_tables(
                items, [[float(gr["lr"]) for gr in groups], [float(gr["weight_decay"]) for gr in groups],
                        [1.0 if (gr["weight_decay"] != 0 or gr["always_adapt"]) else 0.0 for gr in groups]], dev)
            norms = torch.empty((2, n_blocks), dtype=torch.float32, device=dev)
            trust = torch.ones(len(items), dtype=torch.float32, device=dev)
            rc = lib.smoe_lamb_stage1_multi(tab.data_ptr(), hyp.data_ptr(), len(items), blk.data_ptr(), n_blocks, ops.dtype_code(gdt),
                                            b1, b2, (1.0 - b1) if averaging else 1.0, eps, int(bias), step_t.data_ptr(),
                                            ops._ptr(grad_mult), out.data_ptr(), ops._ptr(found_inf), norms.data_ptr(), stream)
            _lib.check(rc, "smoe_lamb_stage1_multi")
            rc = lib.smoe_lamb_trust_multi(norms.data_ptr(), n_blocks, first.data_ptr(), hyp.data_ptr(), len(items), int(trust_clip),
                                           ops._ptr(found_inf), trust.data_ptr(), stream)
            _lib.check(rc, "smoe_lamb_trust_multi")
            rc = lib.smoe_lamb_stage2_multi(tab.data_ptr(), hyp.data_ptr(), len(items), blk.data_ptr(), n_blocks, b1, b2, eps, int(bias),
                                            step_t.data_ptr(), trust.data_ptr(), ops._ptr(found_inf), ops._ptr(sh_tab), stream)
            _lib.check(rc, "smoe_lamb_stage2_multi")
            self._trust.append(([it.p for it in items], trust))
            images.extend(written)
        _finish_step([it.p for it in entries], images)


def _foreign_step_hook(optimizer, args, kwargs) -> None:
    """Global optimizer step post-hook (registered on import, below).  The modules keep 16-bit operand images of their f32
    weights, keyed on ``(param._version, data_ptr, dtype)`` (_cache.param_version).  An optimizer that updates through
    ``p.data`` -- every timm-native optimizer reachable from the reference's ``--opt`` (main.py:90-96, 729-731) does -- moves the
    weights WITHOUT moving ``_version``, and the next forward would go on reading the old images: training on stale weights, no
    error, no warning.  After ANY optimizer's step other than this module's AdamW (whose fused step refreshes the images itself)
    the version counters of its parameters are therefore bumped here, as an in-place torch op would have: the images are re-cast
    on their next use.  (A hand-written update outside a torch.optim.Optimizer -- ``p.data.add_(...)`` in a loop -- cannot be seen:
    call ``slim_switch_moe_vit_amd.invalidate_weight_images()`` after it.)"""
    if getattr(optimizer, "_slimmoe_refreshes_images", False):
        return
    params = [p for group in optimizer.param_groups for p in group["params"] if isinstance(p, torch.Tensor)]
    if params:
        _bump_versions(params)


def invalidate_weight_images() -> None:
    """Drop every derived tensor (16-bit weight images, transposed images, zero-row constants): call after changing parameters
    behind autograd's back (``p.data`` writes outside an optimizer, raw-pointer writes)."""
    from ._cache import invalidate_all
    invalidate_all()


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_post
    _FOREIGN_HOOK = _reg_post(_foreign_step_hook)
except ImportError:      # (a torch without global optimizer hooks: the documented invalidate_weight_images() remains)
    _FOREIGN_HOOK = None


class NativeScaler:
    """``timm.utils.NativeScaler`` (main.py:732; called at engine.py:68-74) on device-side state.

    ``__call__(loss, optimizer, clip_grad=None, parameters=None, create_graph=False)``: scaled backward, gradient-norm
    clipping to ``clip_grad`` when it is not None (``parameters`` then required, as in timm), optimizer step skipped on
    non-finite gradients, scale update (growth 2.0 every 2000 clean steps, backoff 0.5) -- ``torch.cuda.amp.GradScaler``
    defaults.  With an optimizer that takes device scalars (``optim.AdamW``) nothing in the step syncs with the host and
    the gradients stay SCALED in ``.grad`` (``grad_multiplier`` holds ``inv_scale x clip coefficient``); one that sets ``wants_grad_sumsq``
    (``optim.Lamb``) is also handed the block partials of this step's pass over the gradients: ``step(..., grad_sumsq=(partials, inv_scale))``;
    any other optimizer gets the stock sequence (unscale in place, ``clip_grad_norm_``, host-checked step).
    ``state_dict()`` has GradScaler's keys (main.py:903 saves it, 723 loads it)."""

    state_dict_key = "amp_scaler"

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, enabled: bool = True):
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        self.enabled = enabled
        self._init_scale = float(init_scale)
        self._scale = None            # f32[1] on the device, created at the first call
        self._growth_tracker = None   # f32[1]
        self.grad_multiplier = None   # f32[1]: what the last step multiplied the stored gradients by
        self.last_grad_norm = None    # f32[1]: total norm of the unscaled gradients of the last clipped step

    def _lazy(self, device):
        if self._scale is None or self._scale.device != device:
            s = self._init_scale if self._scale is None else float(self._scale)
            t = 0.0 if self._growth_tracker is None else float(self._growth_tracker)
            self._scale = torch.full((1,), s, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((1,), t, dtype=torch.float32, device=device)

    def get_scale(self) -> float:
        return self._init_scale if self._scale is None else float(self._scale)

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval,
                "_growth_tracker": 0 if self._growth_tracker is None else int(self._growth_tracker)}

    def load_state_dict(self, sd):
        self.growth_factor, self.backoff_factor = sd["growth_factor"], sd["backoff_factor"]
        self.growth_interval = sd["growth_interval"]
        self._init_scale = float(sd["scale"])
        dev = None if self._scale is None else self._scale.device
        self._scale = self._growth_tracker = None
        if dev is not None:
            self._lazy(dev)
        if self._growth_tracker is not None:
            self._growth_tracker.fill_(float(sd["_growth_tracker"]))
        else:
            self._pending_tracker = float(sd["_growth_tracker"])

    def __call__(self, loss, optimizer, clip_grad=None, parameters: Optional[Iterable] = None, create_graph: bool = False):
        if not self.enabled:
            loss.backward(create_graph=create_graph)
            if clip_grad is not None:
                assert parameters is not None
                torch.nn.utils.clip_grad_norm_(parameters, clip_grad)
            optimizer.step()
            return
        dev = loss.device
        self._lazy(dev)
        if getattr(self, "_pending_tracker", None) is not None:
            self._growth_tracker.fill_(self._pending_tracker)
            self._pending_tracker = None
        (loss * self._scale[0]).backward(create_graph=create_graph)
        params = [p for g in optimizer.param_groups for p in g["params"] if p.grad is not None]
        fused = bool(getattr(optimizer, "supports_device_scalars", False)) and dev.type == "cuda" and all(
            p.grad.is_cuda and p.grad.is_contiguous() and p.grad.dtype in ops._DT for p in params)
        if not fused:
            self._stock_step(optimizer, params, clip_grad, parameters)
            return
        lib = _lib.load()
        found_inf = torch.zeros(1, dtype=torch.float32, device=dev)
        inv_scale = self._scale.reciprocal()
        clip_over = list(parameters) if (clip_grad is not None and parameters is not None) else None
        if clip_grad is not None:
            assert parameters is not None, "clip_grad needs `parameters` (timm NativeScaler)"
        # pass 1 over every gradient the optimizer will use: non-finite check (+ the norm's partial sums where clipped)
        # (one launch per gradient dtype over every gradient: partials in parameter order, 16K-element blocks)
        clipped = {id(p.grad) for p in clip_over if p.grad is not None} if clip_over is not None else set()
        partials, masks = [], []
        for part, gs, nb in _grad_sumsq_launch([p.grad for p in params], inv_scale, found_inf, dev):
            partials.append(part)
            if clip_grad is not None:
                masks.append(self._clip_mask([id(g) in clipped for g in gs], nb, dev))
        mult = inv_scale
        if clip_grad is not None:
            total = torch.zeros((), dtype=torch.float32, device=dev)
            for part, mask in zip(partials, masks):
                if mask is not None:
                    total = total + torch.where(mask, part, part.new_zeros(())).sum()
            total = total.sqrt()
            self.last_grad_norm = total.reshape(1)
            coef = (float(clip_grad) / (total + 1e-6)).clamp(max=1.0)      # torch.nn.utils.clip_grad_norm_
            mult = inv_scale * coef
        self.grad_multiplier = mult.reshape(1).contiguous()
        if getattr(optimizer, "wants_grad_sumsq", False):
            # (optim.Lamb: its global gradient norm comes out of THIS pass's partials, taken with inv_scale -- no second pass)
            optimizer.step(grad_mult=self.grad_multiplier, found_inf=found_inf, grad_sumsq=(partials, inv_scale))
        else:
            optimizer.step(grad_mult=self.grad_multiplier, found_inf=found_inf)
        rc = lib.smoe_amp_update(self._scale.data_ptr(), self._growth_tracker.data_ptr(), found_inf.data_ptr(),
                                 float(self.growth_factor), float(self.backoff_factor), int(self.growth_interval),
                                 ops._stream(self._scale))
        _lib.check(rc, "smoe_amp_update")

    def _clip_mask(self, clipped, nb, dev):
        """bool [n_blocks]: True for the partial sums of gradients that count towards the clipped norm (cached: the pattern
        only changes with the parameter list); None when nothing is clipped."""
        if not any(clipped):
            return None
        key = (str(dev), tuple(clipped), tuple(nb))
        cache = self.__dict__.setdefault("_mask_cache", {})
        m = cache.get(key)
        if m is None:
            if len(cache) > 8:
                cache.clear()
            m = cache[key] = torch.repeat_interleave(torch.tensor(clipped, dtype=torch.bool), torch.tensor(nb)).to(dev)
        return m

    def _stock_step(self, optimizer, params, clip_grad, parameters):
        """GradScaler's sequence for optimizers that know nothing of device scalars (and for CPU tensors)."""
        inv = 1.0 / float(self._scale)
        finite = True
        for p in params:
            p.grad.mul_(inv)
            finite = finite and bool(torch.isfinite(p.grad).all())
        if clip_grad is not None:
            assert parameters is not None, "clip_grad needs `parameters` (timm NativeScaler)"
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(parameters, clip_grad).reshape(1)
        self.grad_multiplier = None
        if finite:
            optimizer.step()
            self._growth_tracker += 1
            if int(self._growth_tracker) >= self.growth_interval:
                self._scale *= self.growth_factor
                self._growth_tracker.zero_()
        else:
            self._scale *= self.backoff_factor
            self._growth_tracker.zero_()


# -- weight EMA -----------------------------------------------------------------------------------------------------------------
# module attributes that hold per-process GPU plumbing rather than model state: an EMA copy starts without them (re-made lazily)
_TRANSIENT_ATTRS = ("_side_streams", "_ep_static_agreed", "_ep_slots", "_ep_last_stats")


def _independent_copy(model: torch.nn.Module) -> torch.nn.Module:
    """``copy.deepcopy(model)`` whose derived-tensor caches are its OWN and empty.  A plain deepcopy would carry the original's
    ``StreamCache`` objects over -- 16-bit weight images, zero-row constants, the events behind them -- as copies that no
    ``invalidate_weight_images()`` reaches (they are not in ``_cache._ALL``).  Each cache of the original is mapped to a fresh one of
    the same class (the load_state_dict post-hooks that invalidate it find it under the same attribute); the side streams and the
    exchange state are left out (made again on first use)."""
    import copy
    from ._cache import StreamCache
    memo = {}
    for m in model.modules():
        for k, v in m.__dict__.items():
            if isinstance(v, StreamCache):
                memo[id(v)] = type(v)()
            elif k in _TRANSIENT_ATTRS:
                memo[id(v)] = None
    ema = copy.deepcopy(model, memo)
    for m in ema.modules():
        for k in _TRANSIENT_ATTRS:
            if k in m.__dict__ and m.__dict__[k] is None:
                del m.__dict__[k]
    return ema


def _ema_kernel_ok(e: torch.Tensor, m: torch.Tensor) -> bool:
    return (e.is_cuda and e.dtype == torch.float32 and m.dtype == torch.float32 and m.device == e.device and e.shape == m.shape
            and e.is_contiguous() and m.is_contiguous() and e.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0)


class ModelEma:
    """``timm.utils.ModelEma`` (timm 0.4 / 0.5; main.py:599-606, engine.py:77-78) with the update in ONE HIP launch.

    ``ModelEma(model, decay=0.9999, device='', resume='')``: ``.ema`` is an independent copy of ``model`` (eval mode, no grad, its own
    empty weight-image caches), kept on ``device`` when that is given (``'cpu'``: ``--model-ema-force-cpu``).  ``update(model)``
    applies timm's ``ema_v.copy_(ema_v * decay + (1. - decay) * model_v)`` to every ``state_dict()`` entry of the EMA (buffers too),
    in ``ema.state_dict()`` order, reading a DataParallel / DDP-wrapped ``model`` under its ``module.`` keys as timm does.  f32 device
    entries go through ``smoe_ema_update_multi`` -- one launch, bit-equal to torch's line, no host-to-device copy once the pointer
    table is cached, so it can be captured (engine.GraphedTrainStep); everything else (CPU, 16-bit, integer or mismatched entries, and
    tied weights: one storage under several keys, which timm updates once per key) takes timm's line itself.  Keyword-only ``skip``: a device f32 flag; non-zero = this update changes nothing (the harness passes
    "the loss was non-finite" without asking the host).

    Checkpoints: ``_load_checkpoint(path_or_file)`` reads ``state_dict_ema`` (utils._load_checkpoint_for_ema hands it a BytesIO);
    ``state_dict()`` / ``load_state_dict()`` are the unwrapped EMA model's, so ``timm.utils.get_state_dict(model_ema)`` works unchanged
    (this class deliberately has no ``.module``).  Expert-parallel models are refused."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, device="", resume: str = ""):
        ep = [n for n, m in model.named_modules() if callable(getattr(m, "ep_active", None)) and m.ep_active()]
        if ep:
            raise ValueError(f"ModelEma: expert-parallel MoE layers ({', '.join(ep[:3])}{', ...' if len(ep) > 3 else ''}) are not "
                             "supported: their experts are rank-private and the copy would share the communicator state")
        self.ema = _independent_copy(model)
        self.ema.eval()
        self.decay = decay
        self.device = device
        if device:
            self.ema.to(device=device)
        self.ema_has_module = hasattr(self.ema, "module")
        self._tables = {}      # device -> (entry key, device table, blk, blocks): the kernel's pointer table
        self._captured = []    # tables a captured graph launches with: kept alive as long as this object
        if resume:
            self._load_checkpoint(resume)
        for p in self.ema.parameters():
            p.requires_grad_(False)

    def _unwrapped(self) -> torch.nn.Module:
        return self.ema.module if self.ema_has_module else self.ema

    def _load_checkpoint(self, checkpoint_path) -> None:
        from collections import OrderedDict
        import logging
        checkpoint = torch.load(checkpoint_path, map_location="cpu")
        assert isinstance(checkpoint, dict)
        if "state_dict_ema" in checkpoint:
            new_state_dict = OrderedDict()
            for k, v in checkpoint["state_dict_ema"].items():
                # ema model may have been wrapped by DataParallel, and need module prefix
                if self.ema_has_module:
                    name = "module." + k if not k.startswith("module") else k
                else:
                    name = k
                new_state_dict[name] = v
            self.ema.load_state_dict(new_state_dict)
            logging.getLogger(__name__).info("Loaded state_dict_ema")
        else:
            logging.getLogger(__name__).warning("Failed to find state_dict_ema, starting from loaded model weights")

    def state_dict(self, *args, **kwargs):
        return self._unwrapped().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True):
        return self._unwrapped().load_state_dict(state_dict, strict=strict)

    def tensors(self):
        """The EMA model's parameters and buffers (what ``update`` writes)."""
        return list(self.ema.parameters()) + list(self.ema.buffers())

    @torch.no_grad()
    def update(self, model: torch.nn.Module, *, skip: Optional[torch.Tensor] = None) -> None:
        needs_module = hasattr(model, "module") and not self.ema_has_module
        msd = model.state_dict()
        entries = []
        for k, ema_v in self.ema.state_dict().items():
            if needs_module:
                k = "module." + k
            model_v = msd[k].detach()
            if self.device:
                model_v = model_v.to(device=self.device)
            entries.append((ema_v, model_v))
        # an EMA storage under two keys (tied weights) gets timm's line once per key, one after the other: such entries take the torch
        # path in state-dict order (inside one launch, two workgroups would read and write the same memory at the same time)
        owners = {}
        for ema_v, _ in entries:
            if ema_v.numel():
                s = (ema_v.device, ema_v.untyped_storage().data_ptr())
                owners[s] = owners.get(s, 0) + 1
        fused, rest = {}, []
        for ema_v, model_v in entries:
            shared = ema_v.numel() and owners[(ema_v.device, ema_v.untyped_storage().data_ptr())] > 1
            if not shared and _ema_kernel_ok(ema_v, model_v):
                fused.setdefault(ema_v.device, []).append((ema_v, model_v))
            else:
                rest.append((ema_v, model_v))
        for dev, pairs in fused.items():
            self._launch(dev, pairs, skip)
        keep = {}      # device -> the skip flag as a bool there (one copy per device, not one per entry)
        for ema_v, model_v in rest:        # timm's line
            new = ema_v * self.decay + (1. - self.decay) * model_v
            if skip is not None:
                if ema_v.device not in keep:
                    keep[ema_v.device] = skip.to(ema_v.device).reshape(()) != 0
                new = torch.where(keep[ema_v.device], ema_v, new)
            ema_v.copy_(new)
        if fused:
            # the kernel wrote through raw pointers: move the version counters, so that the EMA model's 16-bit weight images are
            # re-cast on its next forward (state_dict() entries share their parameter's counter)
            _bump_versions([e for pairs in fused.values() for e, _ in pairs])

    def _launch(self, dev, pairs, skip) -> None:
        key = tuple((e.data_ptr(), m.data_ptr(), e.numel()) for e, m in pairs)
        hit = self._tables.get(dev)
        if hit is None or hit[0] != key:
            hit = (key,) + _ema_table(pairs, dev)
            if not torch.cuda.is_current_stream_capturing():   # (a table made inside a capture lives in the graph's pool)
                self._tables[dev] = hit
        if torch.cuda.is_current_stream_capturing():
            self._captured.append(hit)
        _ema_launch(hit[1:], len(pairs), self.decay, skip)


def _ema_table(pairs, dev):
    """(tab int64 [3][n_t]: ema, model, n; blk; number of blocks) of smoe_ema_update_multi on the device."""
    blk, nb = _block_table([e.numel() for e, _ in pairs], dev)
    tab = _pointer_table([[e.data_ptr() for e, _ in pairs], [m.data_ptr() for _, m in pairs], [e.numel() for e, _ in pairs]], dev)
    return tab, blk, sum(nb)


def _ema_launch(table, n_tensors: int, decay: float, skip: Optional[torch.Tensor]) -> None:
    tab, blk, n_blocks = table
    if skip is not None:
        assert skip.device == tab.device and skip.dtype == torch.float32 and skip.numel() == 1, "skip is a device f32 flag"
    decay = float(decay)
    # the factors torch's `ema * decay + (1. - decay) * model` multiplies by: f32(decay) and f32(1 - decay), the difference in double
    rc = _lib.load().smoe_ema_update_multi(tab.data_ptr(), n_tensors, blk.data_ptr(), n_blocks, decay, 1.0 - decay, ops._ptr(skip),
                                           ops._stream(tab))
    _lib.check(rc, "smoe_ema_update_multi")


@torch.no_grad()
def ema_update_(emas, models, decay: float, skip: Optional[torch.Tensor] = None) -> None:
    """``e.copy_(e * decay + (1. - decay) * m)`` for every pair, in ONE launch of smoe_ema_update_multi, bit-equal to torch's line:
    f32 device tensors of equal shapes, contiguous, 16-byte aligned (ModelEma.update checks that and routes other entries to torch).
    ``skip``: optional device f32 flag, non-zero = nothing is written.  Moves the version counters of ``emas``."""
    pairs = list(zip(emas, models))
    if not pairs:
        return
    if not all(_ema_kernel_ok(e, m) for e, m in pairs) or len({e.device for e, _ in pairs}) != 1:
        raise ValueError("ema_update_: f32 contiguous 16-byte aligned tensor pairs of equal shapes on one GPU expected")
    _ema_launch(_ema_table(pairs, pairs[0][0].device), len(pairs), decay, skip)
    _bump_versions([e for e, _ in pairs])
