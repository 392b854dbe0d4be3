#!/usr/bin/env python3
"""The evaluation loop's metrics (ops.eval_metrics / engine.EvalMeter: smoe_eval_metrics) on the GPU, beside the reference's lines
(engine.py:99-113: CrossEntropyLoss, timm's accuracy, three .item() reads per batch), alternating the two inside one process.

(a) the metrics alone at [192, 1000] and [384, 1000], f32 and f16 logits: ops.eval_metrics with an accumulator (two launches, no host
    read) against the torch composition with its three reads (and, for information, without them): us per call from device events
    around back-to-back calls, launches per call (torch.profiler kernel rows).
(b) engine.evaluate() on resmoe_tiny_patch16_224_expert8 (1000 classes), batch 192, hip_graph on, metrics="device" against
    metrics="torch": ms per batch from a host clock around the call (it ends in a synchronise).  The batches live on the device.
usage: eval_metrics_bench.py [--out FILE.md] [--rounds N] [--calls K] [--batches M] [--parts ab]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import engine, ops  # noqa: E402

DEV = torch.device("cuda", 0)


def events_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    for _attempt in range(3):      # (a call that already completed outside the profiler; repeated only when the trace came back empty)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.count) for e in prof.key_averages() if not e.key.startswith("hip") and "Memcpy" not in e.key and "Memset" not in e.key]
        if rows:
            return rows
    return []


def fmt(v, digits=1):
    return f"{statistics.median(v):.{digits}f} | {min(v):.{digits}f} - {max(v):.{digits}f}"


def metrics_part(lines, rounds, calls):
    lines += ["## (a) the metrics of one batch", "",
              f"Device events around {calls} back-to-back calls, {rounds} rounds, the paths alternating inside each round, every shape warmed "
              "up first.  own = `ops.eval_metrics(logits, labels, acc, (1, 5))`: no host read.  torch = `CrossEntropyLoss` + timm's "
              "`accuracy(topk=(1, 5))` + the three `.item()` reads of the reference's loop; the column without reads is the same lines "
              "with the reads left out (what the device alone does).  Launches = kernel rows of one call under torch.profiler.", "",
              "| logits | own us (median) | range | own launches | torch us (median) | range | torch launches | torch without reads us (median) | range | own / torch |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    crit = torch.nn.CrossEntropyLoss()
    detail = None
    for B in (192, 384):
        for dtype in (torch.float32, torch.float16):
            g = torch.Generator(device=DEV).manual_seed(B)
            x = (torch.randn(B, 1000, generator=g, device=DEV) * 3).to(dtype)
            labels = torch.randint(0, 1000, (B,), generator=g, device=DEV)
            acc = torch.zeros(4, dtype=torch.float64, device=DEV)

            def own():
                return ops.eval_metrics(x, labels, acc, (1, 5))

            def torch_noread():
                loss = crit(x, labels)
                a1, a5 = engine._accuracy_torch(x, labels, (1, 5))
                return loss, a1, a5

            def torch_lines():
                loss, a1, a5 = torch_noread()
                return loss.item(), a1.item(), a5.item()
            fns = {"own": own, "torch": torch_lines, "noread": torch_noread}
            for fn in fns.values():
                for _ in range(20):
                    fn()
            res = {n: [] for n in fns}
            for _ in range(rounds):
                for n, fn in fns.items():
                    res[n].append(events_us(fn, calls))
            lo, lt = launches(own), launches(torch_noread)
            no, nt = sum(c for _, c in lo), sum(c for _, c in lt)
            name = "f16" if dtype == torch.float16 else "f32"
            lines.append(f"| [{B}, 1000] {name} | {fmt(res['own'])} | {no} | {fmt(res['torch'])} | {nt} | {fmt(res['noread'])} | "
                         f"{statistics.median(res['own']) / statistics.median(res['torch']):.2f} |")
            if detail is None:
                detail = (B, name, lo, lt)
    B, name, lo, lt = detail
    lines += ["", f"Kernels of one call at [{B}, 1000] {name} (name x count):", "",
              "- own: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in lo),
              "- torch: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in lt), ""]


def evaluate_part(lines, rounds, batches):
    torch.manual_seed(0)
    model = sm.create_model("resmoe_tiny_patch16_224_expert8", num_classes=1000).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    batch = (torch.randn(192, 3, 224, 224, device=DEV, generator=g), torch.randint(0, 1000, (192,), device=DEV, generator=g))
    loader = [batch] * batches

    def run(metrics):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sm.evaluate(loader, model, DEV, hip_graph=True, metrics=metrics)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / batches, res
    for m in ("device", "torch"):                    # first-use costs outside the table
        run(m)
    ms = {"device": [], "torch": []}
    last = {}
    for _ in range(rounds):
        for m in ms:
            t, last[m] = run(m)
            ms[m].append(t)
    lines += ["## (b) engine.evaluate(), resmoe_tiny_patch16_224_expert8, 1000 classes, batch 192, fp16 autocast, hip_graph on", "",
              f"{batches} batches per call (the same device-resident batch: no host-to-device copy in the loop), ms per batch = a host "
              f"clock around the call, which ends in a synchronise, over {batches}; every call captures its graph afresh, so that cost is "
              f"inside both figures; {rounds} rounds, the two paths alternating.", "",
              "| metrics | ms per batch (median) | range | hip_graph | loss | acc1 | acc5 |", "|---|---|---|---|---|---|---|"]
    for m in ms:
        r = last[m]
        lines.append(f"| {m} | {fmt(ms[m], 3)} | {r['hip_graph']} | {r['loss']!r} | {r['acc1']!r} | {r['acc5']!r} |")
    d, t = statistics.median(ms["device"]), statistics.median(ms["torch"])
    spread = max(max(v) - min(v) for v in ms.values())
    lines += ["", f"device - torch = {d - t:+.3f} ms per batch (medians); the larger of the two ranges is {spread:.3f} ms.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--parts", default="ab")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_metrics_bench.py needs the GPU"
    assert a.rounds >= 3 and a.calls >= 200 and a.batches >= 50
    lines = ["# Evaluation metrics on the GPU (tools/eval_metrics_bench.py)", "", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    if "a" in a.parts:
        metrics_part(lines, a.rounds, a.calls)
        print("\n".join(lines), flush=True)
    if "b" in a.parts:
        evaluate_part(lines, a.rounds, a.batches)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
