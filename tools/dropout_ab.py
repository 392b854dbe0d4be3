#!/usr/bin/env python3
"""The counter-based dropout kernel beside a plain scaling pass (profiles/r24_dropout.md).

smoe_dropout in place on f16 [50432, 3072] and [25216, 768] beside an in-place mul_ by a scalar on the same tensors (the same bytes, no
generator): interleaved rounds in one process, median and min per launch, the ratio, and the fraction of the 6.3 TB/s copy rate.

usage: dropout_ab.py"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.3e12      # bytes / s, the chip's measured copy rate (read + write)


def _events_ms(fn, n):
    import torch
    e = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    e[0].record()
    for i in range(n):
        fn()
        e[i + 1].record()
    torch.cuda.synchronize()
    return [e[i].elapsed_time(e[i + 1]) for i in range(n)]


def kernel():
    import torch
    sys.path.insert(0, ROOT)
    from slim_switch_moe_vit_amd import ops
    dev = torch.device("cuda", 0)
    out = {}
    for rows, cols in ((50432, 3072), (25216, 768)):
        x = torch.randn(rows, cols, device=dev).half()
        key = ops.dropout_key(dev)
        arms = {"dropout": lambda: ops.dropout(x, key, 0.1, out=x), "mul_": lambda: x.mul_(1.0009765625)}
        ms = {k: [] for k in arms}
        for k, fn in arms.items():
            for _ in range(5):
                fn()
        for _ in range(6):
            for k, fn in arms.items():
                x.normal_()
                ms[k] += _events_ms(fn, 20)
        byts = 2 * x.numel() * 2
        r = {}
        for k, v in ms.items():
            med = statistics.median(v)
            r[k] = {"us_median": round(med * 1e3, 2), "us_min": round(min(v) * 1e3, 2), "TB_per_s": round(byts / (med * 1e-3) / 1e12, 3),
                    "of_copy_rate": round(byts / (med * 1e-3) / COPY_RATE, 3)}
        r["dropout_over_mul"] = round(r["dropout"]["us_median"] / r["mul_"]["us_median"], 3)
        out[f"f16 [{rows}, {cols}]"] = r
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    kernel()
