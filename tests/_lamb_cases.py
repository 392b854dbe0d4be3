"""Shared by tests/test_lamb_host.py and tests/test_gpu_lamb.py: the LAMB rule of timm.optim.Lamb (0.4.12 / 0.5) restated on plain
lists of tensors -- no optimizer class -- and the case set both files step through.

    G    = sqrt(sum over every tensor of sum(grad^2));  clip = G / max_grad_norm if G > max_grad_norm else 1   (None: 1)
    per group: step += 1; beta3 = 1 - beta1 if grad_averaging else 1; bc1, bc2 = 1 - beta1^step, 1 - beta2^step
    per p: g = grad / clip; m = m * beta1 + beta3 * g; v = v * beta2 + (1 - beta2) * g * g
           u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) (+ wd * p);  if wd != 0 or always_adapt: u *= r, r = ||p|| / ||u|| (1 if either is 0)
           p -= lr * u

The case set: two parameter groups, 12 steps, gradients N(0,1) x a gradient scale rounded to f16.  The shapes are where the kernels'
block walk can go wrong (one element, a tail that is no multiple of 4, exactly one 16K block, one block plus one element, two blocks
plus one vector); the weight scales put the trust ratios far from 1 (~0.02, ~5, and w = 0 -> 1)."""
import functools
import math

import torch

STEPS = 12
GROUPS = [
    dict(shapes=[(8, 96, 64), (8, 64, 96), (8, 96), (3, 7), (1,), (40001,)], lr=3e-3, weight_decay=0.05, betas=(0.9, 0.95), eps=1e-6,
         weight_scales=[0.02, 5.0, 1.0, 0.02, 5.0, 0.02]),
    dict(shapes=[(16384,), (16385,), (2 * 16384 + 4,)], lr=5e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-6,
         weight_scales=[0.0, 1.0, 5.0]),
]
SHAPES = [s for g in GROUPS for s in g["shapes"]]
GROUP_OF = [i for i, g in enumerate(GROUPS) for _ in g["shapes"]]
HYPER = [dict(lr=g["lr"], weight_decay=g["weight_decay"], betas=g["betas"], eps=g["eps"]) for g in GROUPS]
# (max_grad_norm, gradient scale, trust_clip, always_adapt)
SETTINGS = [(1.0, 1.0, False, False),     # the global clip engages
            (1.0, 1e-3, False, True),     # it does not (G ~ 0.45), and the wd = 0 group adapts
            (None, 1.0, True, True),
            (1.0, 1.0, True, False)]


def initial_weights():
    """f32 tensors, N(0,1) x the tensor's weight scale (seeded)."""
    g = torch.Generator().manual_seed(1234)
    scales = [s for grp in GROUPS for s in grp["weight_scales"]]
    return [torch.randn(shape, generator=g) * scale for shape, scale in zip(SHAPES, scales)]


@functools.lru_cache(maxsize=None)
def gradients(grad_scale: float, dtype=torch.float16):
    """STEPS lists of f32 tensors whose values are exactly representable in ``dtype`` (f16 first, as the issue's trial did)."""
    out = []
    for it in range(STEPS):
        g = torch.Generator().manual_seed(5000 + it)
        out.append([(torch.randn(shape, generator=g) * grad_scale).half().to(dtype).float() for shape in SHAPES])
    return out


def lamb_steps(params, grads_seq, group_of, hyper, *, max_grad_norm=1.0, trust_clip=False, always_adapt=False, bias_correction=True,
               grad_averaging=True, dtype=torch.float64, exp_avg=None, exp_avg_sq=None, first_step=1):
    """The rule above over ``len(grads_seq)`` steps in ``dtype`` torch ops.  ``params`` / ``grads_seq[i]``: lists of tensors (not
    modified); ``group_of[j]``: index into ``hyper`` (dicts of lr, weight_decay, betas, eps) of tensor j.  Returns a dict: params, exp_avg,
    exp_avg_sq (lists), G and clip (one float per step), trust (one list of floats per step)."""
    p = [t.detach().clone().to(dtype) for t in params]
    m = [torch.zeros_like(t) if exp_avg is None else exp_avg[j].detach().clone().to(dtype) for j, t in enumerate(p)]
    v = [torch.zeros_like(t) if exp_avg_sq is None else exp_avg_sq[j].detach().clone().to(dtype) for j, t in enumerate(p)]
    Gs, clips, trusts = [], [], []
    for it, grads in enumerate(grads_seq):
        step = first_step + it
        gs = [g.detach().to(dtype) for g in grads]
        G = math.sqrt(sum(float(g.pow(2).sum()) for g in gs))
        clip = G / max_grad_norm if (max_grad_norm is not None and G > max_grad_norm) else 1.0
        trust = []
        for j, g in enumerate(gs):
            h = hyper[group_of[j]]
            b1, b2 = h["betas"]
            beta3 = 1 - b1 if grad_averaging else 1.0
            bc1, bc2 = (1 - b1 ** step, 1 - b2 ** step) if bias_correction else (1.0, 1.0)
            g = g / clip
            m[j].mul_(b1).add_(g, alpha=beta3)
            v[j].mul_(b2).addcmul_(g, g, value=1 - b2)
            u = (m[j] / bc1) / (v[j].sqrt() / math.sqrt(bc2) + h["eps"])
            if h["weight_decay"] != 0:
                u = u + h["weight_decay"] * p[j]
            r = 1.0
            if h["weight_decay"] != 0 or always_adapt:
                w_norm, u_norm = float(p[j].norm(2.0)), float(u.norm(2.0))
                if w_norm > 0 and u_norm > 0:
                    r = w_norm / u_norm
                if trust_clip:
                    r = min(r, 1.0)
                u = u * r
            p[j].add_(u, alpha=-h["lr"])
            trust.append(r)
        Gs.append(G)
        clips.append(clip)
        trusts.append(trust)
    return dict(params=p, exp_avg=m, exp_avg_sq=v, G=Gs, clip=clips, trust=trusts)


@functools.lru_cache(maxsize=None)
def reference(setting: int, grad_dtype=torch.float16):
    """The float64 run of SETTINGS[setting] over the case set (computed once per process; treat as read-only)."""
    mgn, gscale, trust_clip, always_adapt = SETTINGS[setting]
    return lamb_steps(initial_weights(), gradients(gscale, grad_dtype), GROUP_OF, HYPER, max_grad_norm=mgn, trust_clip=trust_clip,
                      always_adapt=always_adapt)


def rel_err(got, ref) -> float:
    """max |got - ref| relative to max(1, max |ref|), over lists of tensors (compared in float64 on the CPU)."""
    worst = 0.0
    for a, b in zip(got, ref):
        b = b.detach().double().cpu()
        worst = max(worst, float((a.detach().double().cpu() - b).abs().max()) / max(1.0, float(b.abs().max())))
    return worst


def make_optimizer(cls, params, setting: int, **kw):
    """``cls`` (sm.Lamb, or timm's) over ``params`` (in SHAPES order) with the case set's two groups and SETTINGS[setting]."""
    mgn, _, trust_clip, always_adapt = SETTINGS[setting]
    groups, at = [], 0
    for g, h in zip(GROUPS, HYPER):
        groups.append(dict(params=list(params[at:at + len(g["shapes"])]), **h))
        at += len(g["shapes"])
    return cls(groups, max_grad_norm=mgn, trust_clip=trust_clip, always_adapt=always_adapt, **kw)
