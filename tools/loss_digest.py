#!/usr/bin/env python3
"""One sha256 per output tensor of the loss family's entry points (csrc/loss.hip: Mixup, soft-target / label-smoothing cross-entropy,
distillation, evaluation metrics, BCE) over a fixed grid of seeded inputs.  Run it once per build of the library on the same device
(SLIMMOE_LIB selects another build) and compare the two outputs line by line: equal lines = equal bits.
usage: loss_digest.py [--out FILE]"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CS = (1, 8, 1000, 1001, 2048, 2056, 4099)
BS = (1, 255, 257)
LINES = []


def emit(name, **tensors):
    for k, t in tensors.items():
        raw = t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()
        LINES.append(f"{name} {k} {hashlib.sha256(raw).hexdigest()}")


def place(x, off):
    """x on the device, its base 16-byte aligned (off = 0) or ``off`` bytes past such a base."""
    if off == 0:
        y = x.to(DEV).contiguous()
        assert y.data_ptr() % 16 == 0
        return y
    e = off // x.element_size()
    store = torch.zeros(x.numel() + 16, dtype=x.dtype, device=DEV)
    y = store[e:e + x.numel()].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 == off
    return y


def inputs(B, C, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * scale
    y = torch.randn(B, C, generator=g) * scale
    labels = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, 1, generator=g)
    return x, y, labels, lam


def dense_target(labels, lam, C, smoothing):
    off = smoothing / C
    one = lambda l: torch.full((l.numel(), C), off).scatter_(1, l.view(-1, 1), 1.0 - smoothing + off)
    return one(labels) * lam + one(labels.flip(0)) * (1 - lam)


def scalar(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def soft_ce(tag, x, t, labels, smoothing):
    loss, rows = ops.soft_ce_fwd(x, t, labels, smoothing)
    emit(tag, loss=loss, rows=rows, dx=ops.soft_ce_bwd(x, rows, scalar(3.0), t, labels, smoothing))


def distill(tag, s, t, mode, tau):
    loss, dl, rows, stats, labels = ops.distill_fwd(s, t, scalar(2.5), mode, tau, 0.3)
    emit(tag, loss=loss, distill=dl, rows=rows, stats=stats, labels=labels,
         dx=ops.distill_bwd(s, t, stats, labels, scalar(3.0), mode, tau, 0.3))


def bce(tag, x, t, binarize):
    loss, rows = ops.bce_fwd(x, t, binarize)
    emit(tag, loss=loss, rows=rows, dx=ops.bce_bwd(x, t, scalar(512.0), binarize))


def evalm(tag, x, labels, topk):
    acc = torch.zeros(2 + len(topk), dtype=torch.float64, device=DEV)
    batch, row_loss, row_rank = ops.eval_metrics(x, labels, acc, topk)
    emit(tag, batch=batch, row_loss=row_loss, row_rank=row_rank)
    batch2, _, _ = ops.eval_metrics(x.flip(0).contiguous(), labels, acc, topk)
    emit(tag, batch2=batch2, acc=acc)


MODES = (("soft", 1.0), ("soft", 3.0), ("hard", 1.0))
TOPKS = ((1,), (1, 5), (1, 2, 3, 4))


def grid():
    for dn, dt in DTYPES.items():
        for C in CS:
            for B in BS:
                x32, y32, labels, lam = inputs(B, C, 1000 * B + C)
                lab = labels.to(DEV)
                for off in (0, 4):
                    x, y = place(x32.to(dt), off), place(y32.to(dt), 0)
                    tag = f"{dn} B{B} C{C} off{off}"
                    for sm_ in (0.0, 0.1):
                        soft_ce(f"soft_ce dense s{sm_} {tag}", x, place(dense_target(labels, lam, C, sm_), 0), None, sm_)
                        soft_ce(f"soft_ce labels s{sm_} {tag}", x, None, lab, sm_)
                    for mode, tau in MODES:
                        distill(f"distill {mode} tau{tau} {tag}", x, y, mode, tau)
                    tm = place(dense_target(labels, lam, C, 0.0), 0)
                    for b in (False, True):
                        bce(f"bce bin{int(b)} {tag}", x, tm, b)
                    for tk in TOPKS:
                        evalm(f"eval topk{'_'.join(map(str, tk))} {tag}", x, lab, tk)


def pairs():
    B, C = 255, 1001
    x32, y32, _, _ = inputs(B, C, 5)
    for sn, sd in DTYPES.items():
        for tn, td in DTYPES.items():
            for C2 in (C, 1000):          # (the element path and the 8-per-lane path)
                for mode, tau in MODES:
                    distill(f"distill pair {sn}/{tn} {mode} tau{tau} C{C2}", place(x32[:, :C2].contiguous().to(sd), 0),
                            place(y32[:, :C2].contiguous().to(td), 0), mode, tau)


def planted():
    """Row 0 a NaN logit, row 1 +inf, row 2 -inf, row 3 a label outside [0, C); rows 4.. clean."""
    for dn, dt in DTYPES.items():
        for C in (1000, 1001):
            B = 6
            x32, y32, labels, lam = inputs(B, C, 77 + C)
            x32[0, 5], x32[1, C - 1], x32[2, C // 2] = float("nan"), float("inf"), float("-inf")
            bad = labels.clone()
            bad[3] = C
            x, y, tag = place(x32.to(dt), 0), place(y32.to(dt), 0), f"planted {dn} C{C}"
            t = place(dense_target(labels, lam, C, 0.1), 0)
            soft_ce(f"soft_ce dense {tag}", x, t, None, 0.1)
            soft_ce(f"soft_ce labels {tag}", x, None, bad.to(DEV), 0.1)
            evalm(f"eval {tag}", x, bad.to(DEV), (1, 5))
            for b in (False, True):
                bce(f"bce bin{int(b)} {tag}", x, t, b)
            for mode, tau in MODES:
                distill(f"distill student {mode} tau{tau} {tag}", x, y, mode, tau)
                distill(f"distill teacher {mode} tau{tau} {tag}", y, x, mode, tau)


def mixup():
    for mode in ("batch", "pair", "elem"):
        for shape in ((8, 3, 30, 34), (6, 3, 5, 7)):
            np.random.seed(shape[0])
            m = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=0.1, num_classes=1000)
            g = torch.Generator().manual_seed(shape[2])
            for call in range(4):          # (several draws: Mixup, CutMix and untouched samples)
                x = torch.randn(shape, generator=g).to(DEV)
                labels = torch.randint(0, 1000, (shape[0],), generator=g).to(DEV)
                xo, t = m(x, labels)
                emit(f"mixup {mode} {shape} call{call}", images=xo, target=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "loss_digest.py needs the GPU"
    for part in (grid, pairs, planted, mixup):
        part()
        torch.cuda.synchronize()
    text = "\n".join(LINES)
    print(text)
    print(f"# {len(LINES)} lines, library {sm._lib.binary_build_id()}", file=sys.stderr)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
