#!/usr/bin/env python3
"""The --bce-loss criterion (loss.BCEWithLogitsLoss over smoe_bce_fwd / smoe_bce_bwd; main.py:663-664, engine.py:49-50) on the GPU,
beside the path the recipe took before it: engine.py:50's `targets.gt(0.0).type(targets.dtype)` + torch.nn.BCEWithLogitsLoss.

(a) the criterion alone, forward + backward, at [128, 10] (the reference's CIFAR-10 scripts), [128, 1000] and [192, 1000], f32 and f16
    logits, raw Mixup targets: launches per pass (torch.profiler kernel rows) and us per pass (device events around back-to-back
    passes, the two sides alternating on one device).
(b) deit_tiny_patch16_224, batch 128, train_one_epoch with args.bce_loss and Mixup, eager and hip_graph=True, old criterion against
    new (device events the loader records as it hands out each batch, configurations alternating).
The shader clock level rocm-smi reports is sampled right after each timed part.
usage: bce_bench.py [--out FILE.md] [--rounds N] [--steps K] [--parts ab]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402

DEV = torch.device("cuda", 0)


def clock_note():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=10).stdout
        d = json.loads(out)
        card = d[sorted(k for k in d if k.startswith("card"))[0]]
        return "; ".join(f"{k}: {v}" for k, v in card.items() if k.startswith("sclk")) or "rocm-smi reports no sclk"
    except Exception as exc:  # noqa: BLE001
        return f"not read ({type(exc).__name__})"


def one_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def interleaved_us(fns, rounds, inner, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            res[n].append(one_us(lambda: [fn() for _ in range(inner)]) / inner)
    return res


def fmt(v):
    return f"{statistics.median(v):.1f} | {min(v):.1f} - {max(v):.1f}"


def _launches(fn):
    from torch.profiler import profile, ProfilerActivity
    for _attempt in range(3):      # (a pass that already completed outside the profiler; repeated only when the trace came back empty)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.count) for e in prof.key_averages() if not e.key.startswith("hip") and "Memcpy" not in e.key and "Memset" not in e.key]
        if rows:
            return rows
    return []


def _mixup_targets(B, C):
    np.random.seed(B + C)
    mix = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.0, num_classes=C)
    g = torch.Generator(device=DEV).manual_seed(C)
    return mix(torch.zeros(B, 3, 8, 8, device=DEV), torch.randint(0, C, (B,), generator=g, device=DEV))[1]


def loss_part(lines, rounds):
    lines += ["## (a) the criterion alone, forward + backward", "",
              "old = `targets.gt(0.0).type(targets.dtype)` + `torch.nn.BCEWithLogitsLoss()`; new = `BCEWithLogitsLoss(binarize=True)` on "
              "the raw Mixup targets.  Loss x 65536 before the backward (the multiplication and autograd's seed are on both sides); "
              f"device events around 20 back-to-back passes, {rounds} rounds, the two alternating; launches = kernel rows of one pass "
              "under torch.profiler.", "",
              "| logits | new us (median) | range | new launches | old us (median) | range | old launches | new / old |",
              "|---|---|---|---|---|---|---|---|"]
    scale = torch.tensor(65536.0, device=DEV)
    old_crit, new_crit = torch.nn.BCEWithLogitsLoss(), sm.BCEWithLogitsLoss(binarize=True)
    detail = None
    for B, C in ((128, 10), (128, 1000), (192, 1000)):
        t = _mixup_targets(B, C)
        for dtype in (torch.float32, torch.float16):
            g = torch.Generator(device=DEV).manual_seed(B)
            logits = (torch.randn(B, C, generator=g, device=DEV) * 4).to(dtype)

            def new():
                x = logits.detach().requires_grad_(True)
                (new_crit(x, t) * scale).backward()
                return x.grad

            def old():
                x = logits.detach().requires_grad_(True)
                tb = t.gt(0.0).type(t.dtype)
                with torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16):   # (f16 logits reach it under autocast)
                    loss = old_crit(x, tb)
                (loss * scale).backward()
                return x.grad
            res = interleaved_us({"new": new, "old": old}, rounds, 20)
            ln, lo = _launches(new), _launches(old)
            nn_, no = sum(c for _, c in ln), sum(c for _, c in lo)
            mn, mo = statistics.median(res["new"]), statistics.median(res["old"])
            name = "f16" if dtype == torch.float16 else "f32"
            lines.append(f"| [{B}, {C}] {name} | {fmt(res['new'])} | {nn_} | {fmt(res['old'])} | {no} | {mn / mo:.2f} |")
            if detail is None or (B, C, name) == (128, 1000, "f16"):
                detail = (B, C, name, ln, lo)
    B, C, name, ln, lo = detail
    lines += ["", f"Kernels of one forward + backward at [{B}, {C}] {name} (name x count):", "",
              "- new: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in ln),
              "- old: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in lo), "",
              f"Shader clock after the part: {clock_note()}", ""]


class EventLoader:
    """``n`` times the same batch; records an event on the current stream as each batch is handed out and one after the last step."""

    def __init__(self, batch, n):
        self.batch, self.n, self.events = batch, n, []

    def __iter__(self):
        self.events = []
        for _ in range(self.n):
            self.events.append(torch.cuda.Event(enable_timing=True))
            self.events[-1].record()
            yield self.batch[0].clone(), self.batch[1]       # (Mixup works in place)
        self.events.append(torch.cuda.Event(enable_timing=True))
        self.events[-1].record()


def step_ms(own, graph, batch, w, k):
    torch.manual_seed(0)
    np.random.seed(0)
    model = sm.create_model("deit_tiny_patch16_224").to(DEV)
    opt = sm.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    crit = sm.BCEWithLogitsLoss(binarize=True) if own else torch.nn.BCEWithLogitsLoss()
    mix = sm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=1000)
    loader = EventLoader(batch, w + k)
    st = sm.train_one_epoch(model, crit, loader, opt, DEV, 0, sm.NativeScaler(), None, None, mix, args=SimpleNamespace(bce_loss=True),
                            hip_graph=graph)
    torch.cuda.synchronize()
    return loader.events[w].elapsed_time(loader.events[w + k]) / k, st["hip_graph_steps"]


def harness_part(lines, rounds, k):
    g = torch.Generator(device=DEV).manual_seed(1)
    batch = (torch.randn(128, 3, 224, 224, device=DEV, generator=g), torch.randint(0, 1000, (128,), device=DEV, generator=g))
    w = 8
    cfgs = [(f"{'new: BCEWithLogitsLoss(binarize=True)' if own else 'old: gt line + torch.nn.BCEWithLogitsLoss'}, "
             f"{'hip_graph=True' if gr else 'eager'}", own, gr) for gr in (False, True) for own in (False, True)]
    res, graphed = {n: [] for n, _, _ in cfgs}, {}
    step_ms(True, True, batch, 4, 4)                # first-use costs outside the table
    for _ in range(rounds):
        for n, own, gr in cfgs:
            ms, gs = step_ms(own, gr, batch, w, k)
            res[n].append(ms)
            graphed[n] = gs
    lines += ["## (b) train_one_epoch with args.bce_loss, deit_tiny_patch16_224, batch 128", "",
              "AdamW + NativeScaler, autocast f16, Mixup 0.8 / CutMix 1.0 / smoothing 0.1 (the batch is cloned per step: Mixup works in "
              f"place); ms per step = device events from the start of step {w} to the end of step {w + k - 1} of an epoch of {w + k} "
              f"steps, over {k}; {rounds} rounds, configurations alternating.", "",
              "| configuration | ms per step (median) | range | graphed steps in the epoch |", "|---|---|---|---|"]
    for n, _, _ in cfgs:
        v = res[n]
        lines.append(f"| {n} | {statistics.median(v):.3f} | {min(v):.3f} - {max(v):.3f} | {graphed[n]} |")
    lines += ["", f"Shader clock after the part: {clock_note()}", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--parts", default="ab")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bce_bench.py needs the GPU"
    lines = ["# BCE-with-logits criterion on the GPU (tools/bce_bench.py)", "", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    if "a" in a.parts:
        loss_part(lines, a.rounds)
        print("\n".join(lines), flush=True)
    if "b" in a.parts:
        harness_part(lines, a.rounds, a.steps)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
