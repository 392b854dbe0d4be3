"""Fixture from the reference's OWN criterion: ``DistillationLoss`` (losses.py) run on small stored inputs.

The reference module needs only torch, so it is imported from its file at run time; nothing of it is copied here and only arrays are
stored.  Per case (soft at tau 1 and 3, hard; alpha 0.5 and 0.1; [B, C] = [5, 37] and [3, 1000]): the f32 inputs (class-token logits,
distillation-token logits, teacher logits, integer labels), the loss and the gradients with respect to both student logit tensors as
the reference computes them in f32, and the same three in float64 (the tight reference).  The teacher is a lambda returning the stored
tensor, the base criterion ``F.cross_entropy``.  The teacher rows of the hard cases carry two exact ties (torch.argmax takes the
first index).

    python tests/golden/distill/make_golden_distill.py          # -> tests/golden/distill/ref_distill_loss.npz
"""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

REF_LOSSES = os.path.join(os.environ.get("SLIMMOE_REFERENCE", "/root/reference"), "losses.py")
OUT_DIR = os.environ.get("SLIMMOE_GOLDEN_OUT", os.path.dirname(os.path.abspath(__file__)))

CASES = [("soft", 1.0), ("soft", 3.0), ("hard", 1.0)]
ALPHAS = [0.5, 0.1]
SHAPES = [(5, 37), (3, 1000)]


def case_name(kind, tau, alpha, B, C):
    return f"{kind}_tau{tau:g}_alpha{alpha:g}_{B}x{C}"


def inputs(kind, B, C, seed):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(B, C, generator=g) * 2
    kd = torch.randn(B, C, generator=g) * 2
    teacher = torch.randn(B, C, generator=g) * 3
    labels = torch.randint(0, C, (B,), generator=g)
    if kind == "hard":                       # two exact ties at the row maximum: rows 0 and 1 (the later index is the tie's second)
        for row, (a, b) in ((0, (C - 2, 3)), (1, (7, 5))):
            top = teacher[row].max() + 1.0
            teacher[row, a] = top
            teacher[row, b] = top
    return cls, kd, teacher, labels


def run(ref_cls, kind, tau, alpha, cls, kd, teacher, labels, dtype):
    cls = cls.detach().clone().to(dtype).requires_grad_(True)
    kd = kd.detach().clone().to(dtype).requires_grad_(True)
    t = teacher.to(dtype)
    crit = ref_cls(F.cross_entropy, lambda inp: t, kind, alpha, tau)
    loss = crit(torch.zeros(1), (cls, kd), labels)
    loss.backward()
    return loss.detach().numpy(), cls.grad.numpy(), kd.grad.numpy()


def main():
    spec = importlib.util.spec_from_file_location("ref_losses", REF_LOSSES)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(1)                  # one summation order whatever the machine
    out = {}
    seed = 0
    for kind, tau in CASES:
        for alpha in ALPHAS:
            for B, C in SHAPES:
                seed += 1
                name = case_name(kind, tau, alpha, B, C)
                cls, kd, teacher, labels = inputs(kind, B, C, seed)
                out[name + "/cls"], out[name + "/kd"], out[name + "/teacher"] = cls.numpy(), kd.numpy(), teacher.numpy()
                out[name + "/labels"] = labels.numpy()
                for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                    loss, gc, gk = run(mod.DistillationLoss, kind, tau, alpha, cls, kd, teacher, labels, dt)
                    out[f"{name}/loss_{tag}"], out[f"{name}/dcls_{tag}"], out[f"{name}/dkd_{tag}"] = loss, gc, gk
    path = os.path.join(OUT_DIR, "ref_distill_loss.npz")
    np.savez(path, **out)
    print(path, len(out), "arrays")


if __name__ == "__main__":
    main()
