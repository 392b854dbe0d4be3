#!/usr/bin/env python3
"""Weight EMA (optim.ModelEma, the timm.utils.ModelEma surface of main.py:599-606 / engine.py:77-78) on the GPU.

(a) smoe_ema_update_multi over ViT-B/16 E = 8's state (moe_base_patch16_224_expert8_top1: 176 f32 entries): time per update and
    effective rate at 12 bytes per value (read ema, read model, write ema), beside timm's torch line per entry.
(b) resmoe_tiny_patch16_224_expert8 (the reference's model), batch 128, train_one_epoch steady-state ms per step:
    timm-style torch EMA eager (as a user gets it today), ModelEma eager, ModelEma hip_graph=True, no EMA hip_graph=True (and, for
    context, no EMA eager).
    Steady state = device time from the start of step W to the end of step W + K of one epoch (events recorded on the compute stream
    by the data loader as it hands out each batch: an eager, host-bound step's GPU idles as long as the host takes), after the eager
    warm-up and the capture.  Each configuration is measured ROUNDS times, the configurations interleaved; the table gives the median
    and the range.
usage: ema_bench.py [--out FILE.md] [--rounds N] [--steps K]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import optim as smo  # noqa: E402

DEV = torch.device("cuda", 0)


class TimmModelEma:
    """timm.utils.ModelEma (0.4 / 0.5), restated: timm is not a dependency of this package."""

    def __init__(self, model, decay=0.9999):
        import copy
        self.ema = copy.deepcopy(model)
        self.ema.eval()
        self.decay = decay
        for p in self.ema.parameters():
            p.requires_grad_(False)

    def update(self, model):
        with torch.no_grad():
            msd = model.state_dict()
            for k, ema_v in self.ema.state_dict().items():
                model_v = msd[k].detach()
                ema_v.copy_(ema_v * self.decay + (1. - self.decay) * model_v)


def events_ms(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_part(lines):
    cpu = sm.create_model("moe_base_patch16_224_expert8_top1")
    shapes = [v.shape for v in cpu.state_dict().values()]
    del cpu
    g = torch.Generator(device=DEV).manual_seed(0)
    emas = [torch.randn(s, device=DEV, generator=g) for s in shapes]
    models = [torch.randn(s, device=DEV, generator=g) for s in shapes]
    n = sum(e.numel() for e in emas)
    decay = 0.99996
    pairs = list(zip(emas, models))
    table = smo._ema_table(pairs, DEV)
    ms = events_ms(lambda: smo._ema_launch(table, len(pairs), decay, None), 50)
    rate = 12.0 * n / (ms * 1e-3) / 1e12

    def torch_line():
        for e, m in pairs:
            e.copy_(e * decay + (1. - decay) * m)
    ms_t = events_ms(torch_line, 10)
    lines += ["## (a) smoe_ema_update_multi on ViT-B/16 E = 8's state", "",
              f"{len(shapes)} f32 entries, {n / 1e6:.1f} M values, {12.0 * n / 1e9:.2f} GB moved per update at 12 B per value "
              "(read ema, read model, write ema); device events around 50 back-to-back updates after 3 warm-up updates.", "",
              "| update | ms per update | effective TB/s (12 B per value) |", "|---|---|---|",
              f"| smoe_ema_update_multi (one launch) | {ms:.3f} | {rate:.2f} |",
              f"| timm's line, torch, per entry ({4 * len(shapes)} launches) | {ms_t:.3f} | {12.0 * n / (ms_t * 1e-3) / 1e12:.2f} |", ""]
    del emas, models, pairs, table
    torch.cuda.empty_cache()
    return ms, rate


def make_model():
    torch.manual_seed(0)
    model = sm.create_model("resmoe_tiny_patch16_224_expert8")
    return model.to(DEV)


class EventLoader:
    """``n`` times the same (images, labels) batch; records an event on the current stream as each batch is handed out (= after
    everything the previous step enqueued) and one after the last step."""

    def __init__(self, batch, n):
        self.batch, self.n, self.events = batch, n, []

    def __iter__(self):
        self.events = []
        for _ in range(self.n):
            self.events.append(torch.cuda.Event(enable_timing=True))
            self.events[-1].record()
            yield self.batch
        self.events.append(torch.cuda.Event(enable_timing=True))
        self.events[-1].record()


def step_ms(cfg, batch, w, k):
    """ms per step over steps w .. w + k - 1 of one epoch of w + k steps."""
    model = make_model()
    opt = sm.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    scaler = sm.NativeScaler()
    ema = None if cfg["ema"] is None else cfg["ema"](model, 0.99996)
    loader = EventLoader(batch, w + k)
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), loader, opt, DEV, 0, scaler, None, ema, hip_graph=cfg["graph"])
    torch.cuda.synchronize()
    return loader.events[w].elapsed_time(loader.events[w + k]) / k, st["hip_graph_steps"]


def harness_part(lines, rounds, k):
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(128, 3, 224, 224, device=DEV, generator=g)
    y = torch.randint(0, 1000, (128,), device=DEV, generator=g)
    w = 8       # 3 eager warm steps, the capture, 4 replays
    cfgs = [dict(name="timm-style torch EMA, eager (today)", ema=TimmModelEma, graph=False),
            dict(name="ModelEma, eager", ema=sm.ModelEma, graph=False),
            dict(name="ModelEma, hip_graph=True", ema=sm.ModelEma, graph=True),
            dict(name="no EMA, hip_graph=True (yardstick)", ema=None, graph=True),
            dict(name="no EMA, eager (context)", ema=None, graph=False)]
    res = {c["name"]: [] for c in cfgs}
    graphed = {}
    step_ms(cfgs[3], (x, y), 4, 4)                 # first-use costs (code objects, allocator) outside the table
    for _ in range(rounds):
        for c in cfgs:
            ms, gs = step_ms(c, (x, y), w, k)
            res[c["name"]].append(ms)
            graphed[c["name"]] = gs
    lines += ["## (b) train_one_epoch, resmoe_tiny_patch16_224_expert8, batch 128", "",
              f"AdamW + NativeScaler, autocast f16, decay 0.99996.  ms per step = device events from the start of step {w} to the end "
              f"of step {w + k - 1} of an epoch of {w + k} steps, over {k}; {rounds} rounds, configurations interleaved.", "",
              "| configuration | ms per step (median) | range | every round | graphed steps in the epoch |",
              "|---|---|---|---|---|"]
    for c in cfgs:
        v = res[c["name"]]
        lines.append(f"| {c['name']} | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} | "
                     f"{', '.join('%.2f' % t for t in v)} | {graphed[c['name']]} |")
    # what the EMA adds to the GPU's work per step: the kernel alone over this model's state (device events, no host in the loop)
    model = make_model()
    ema = sm.ModelEma(model, 0.99996)
    pairs = list(zip(ema.state_dict().values(), model.state_dict().values()))
    table = smo._ema_table(pairs, DEV)
    ms = events_ms(lambda: smo._ema_launch(table, len(pairs), 0.99996, None), 200)
    n = sum(e.numel() for e, _ in pairs)
    lines += ["", f"The update kernel alone over this model's state ({len(pairs)} entries, {n / 1e6:.1f} M values): {ms:.3f} ms "
              f"({12.0 * n / (ms * 1e-3) / 1e12:.2f} TB/s; device events around 200 back-to-back launches).", ""]
    return {n: statistics.median(v) for n, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench.py needs the GPU"
    lines = ["# Weight EMA on the GPU (tools/ema_bench.py)", "", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    ms, rate = kernel_part(lines)
    print("\n".join(lines), flush=True)
    med = harness_part(lines, a.rounds, a.steps)
    gap = med["ModelEma, hip_graph=True"] - med["no EMA, hip_graph=True (yardstick)"]
    lines += ["## Against the targets", "",
              f"- kernel: {rate:.2f} TB/s effective ({ms:.3f} ms per update; target >= 5.0 TB/s, <= 1.16 ms)",
              f"- graphed step with ModelEma - graphed step without EMA: {gap:+.2f} ms (target within 0.3 ms)", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
