#!/usr/bin/env python3
"""DeiT distillation (loss.DistillationLoss, vit.DistilledVisionTransformer: the reference's losses.py and models/model.py:32-77) on the
GPU, beside the torch composition of losses.py's lines restated here.

(a) the loss alone, forward + backward, at [128, 1000] and [256, 1000], f16 and f32 logits, soft (tau 3) and hard, own against the torch
    composition: us per forward + backward (device events around back-to-back passes, rounds interleaved) and launches per pass
    (torch.profiler kernel rows); max errors against float64 on f32 logits.
(b) deit_tiny_distilled_patch16_224, batch 128, frozen deit_tiny_patch16_224 teacher, train_one_epoch steady state, eager and
    hip_graph=True, own criterion against the torch composition (device events the loader records as it hands out each batch).
(c) the distilled eval forward (fp16 autocast, batch 128) against the non-distilled deit_tiny_patch16_224: one token in 197 and one head more.
usage: distill_bench.py [--out FILE.md] [--rounds N] [--steps K] [--parts abc]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402

DEV = torch.device("cuda", 0)


class TorchDistillationLoss(torch.nn.Module):
    """losses.py:28-73 restated: the composition the own criterion replaces."""

    def __init__(self, base, teacher, kind, alpha, tau):
        super().__init__()
        self.base, self.teacher, self.kind, self.alpha, self.tau = base, teacher, kind, alpha, tau

    def forward(self, inputs, outputs, labels):
        out, kd = outputs
        base = self.base(out, labels)
        with torch.no_grad():
            te = self.teacher(inputs)
        if self.kind == "soft":
            T = self.tau
            d = F.kl_div(F.log_softmax(kd / T, dim=1), F.log_softmax(te / T, dim=1), reduction='sum', log_target=True) * (T * T) / kd.numel()
        else:
            d = F.cross_entropy(kd, te.argmax(dim=1))
        return base * (1 - self.alpha) + d * self.alpha


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


def loss_part(lines, rounds):
    lines += ["## (a) the distillation term and its blend, forward + backward", "",
              "The base loss is a device scalar made once (its own cost is the same on both sides and outside the loop); teacher = a stored "
              "tensor; loss x 65536 before the backward; device events around 20 back-to-back passes, "
              f"{rounds} rounds, the two interleaved; launches = kernel rows of one pass under torch.profiler.", "",
              "| logits | mode | own us (median) | range | own launches | torch us (median) | range | torch launches | own / torch |",
              "|---|---|---|---|---|---|---|---|---|"]
    scale = torch.tensor(65536.0, device=DEV)
    detail = None
    for B in (128, 256):
        for dtype in (torch.float16, torch.float32):
            g = torch.Generator(device=DEV).manual_seed(B)
            kd = (torch.randn(B, 1000, generator=g, device=DEV) * 4).to(dtype)
            te = (torch.randn(B, 1000, generator=g, device=DEV) * 4).to(dtype)
            base = torch.tensor(2.0, device=DEV)
            for kind in ("soft", "hard"):
                own = sm.DistillationLoss(lambda o, l: base, lambda i: te, kind, 0.5, 3.0)
                ref = TorchDistillationLoss(lambda o, l: base, lambda i: te, kind, 0.5, 3.0)

                def run(crit):
                    x = kd.detach().requires_grad_(True)
                    (crit(None, (x, x), None) * scale).backward()
                    return x.grad
                res = interleaved_us({"own": lambda: run(own), "torch": lambda: run(ref)}, rounds, 20)
                lo, lt = _launches(lambda: run(own)), _launches(lambda: run(ref))
                no, nt = sum(c for _, c in lo), sum(c for _, c in lt)
                mo, mt = statistics.median(res["own"]), statistics.median(res["torch"])
                name = "f16" if dtype == torch.float16 else "f32"
                lines.append(f"| [{B}, 1000] {name} | {kind} | {fmt(res['own'])} | {no} | {fmt(res['torch'])} | {nt} | {mo / mt:.2f} |")
                if detail is None:
                    detail = (B, name, kind, lo, lt)
    B, name, kind, lo, lt = detail
    lines += ["", f"Kernels of one forward + backward at [{B}, 1000] {name}, {kind} (name x count):", "",
              "- own: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in lo),
              "- torch: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in lt), "",
              "Max error against float64 on f32 logits [128, 1000], distillation loss and its dlogits:", "",
              "| mode | logit scale | loss: own | loss: torch f32 | dlogits: own | dlogits: torch f32 |", "|---|---|---|---|---|---|"]
    for kind in ("soft", "hard"):
        for s in (1.0, 4.0, 12.0):
            g = torch.Generator(device=DEV).manual_seed(int(s))
            kd, te = torch.randn(128, 1000, generator=g, device=DEV) * s, torch.randn(128, 1000, generator=g, device=DEV) * s
            zero = torch.zeros((), device=DEV)
            outs = {}
            for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
                x = kd.to(dt).requires_grad_(True)
                loss = TorchDistillationLoss(lambda o, l: zero.to(dt), lambda i: te.to(dt), kind, 1.0, 3.0)(None, (x, x), None)
                loss.backward()
                outs[tag] = (loss.detach().double(), x.grad.double())
            loss, _, _, stats, labels = ops.distill_fwd(kd, te, zero, kind, 3.0, 1.0)
            dx = ops.distill_bwd(kd, te, stats, labels, torch.ones((), device=DEV), kind, 3.0, 1.0)
            l64, g64 = outs["f64"]
            lines.append(f"| {kind} | {s:g} | {abs(loss.double().item() - l64.item()):.2e} | {abs(outs['f32'][0].item() - l64.item()):.2e} | "
                         f"{(dx.double() - g64).abs().max().item():.2e} | {(outs['f32'][1] - g64).abs().max().item():.2e} |")
    lines.append("")


class EventLoader:
    """``n`` times the same batch; records an event on the current stream as each batch is handed out and one after the last step."""

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


def step_ms(own, graph, batch, w, k):
    torch.manual_seed(0)
    model = sm.create_model("deit_tiny_distilled_patch16_224").to(DEV)
    teacher = sm.create_model("deit_tiny_patch16_224").to(DEV).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    opt = sm.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    base = sm.LabelSmoothingCrossEntropy(0.1)
    crit = (sm.DistillationLoss if own else TorchDistillationLoss)(base, teacher, "soft", 0.5, 3.0)
    loader = EventLoader(batch, w + k)
    st = sm.train_one_epoch(model, crit, loader, opt, DEV, 0, sm.NativeScaler(), None, None, None, hip_graph=graph)
    torch.cuda.synchronize()
    return loader.events[w].elapsed_time(loader.events[w + k]) / k, st["hip_graph_steps"]


def harness_part(lines, rounds, k):
    g = torch.Generator(device=DEV).manual_seed(1)
    batch = (torch.randn(128, 3, 224, 224, device=DEV, generator=g), torch.randint(0, 1000, (128,), device=DEV, generator=g))
    w = 8
    cfgs = [(f"{'own DistillationLoss' if own else 'torch composition'}, {'hip_graph=True' if gr else 'eager'}", own, gr)
            for gr in (False, True) for own in (False, True)]
    res, graphed = {n: [] for n, _, _ in cfgs}, {}
    step_ms(True, True, batch, 4, 4)                # first-use costs outside the table
    for _ in range(rounds):
        for n, own, gr in cfgs:
            ms, gs = step_ms(own, gr, batch, w, k)
            res[n].append(ms)
            graphed[n] = gs
    lines += ["## (b) train_one_epoch, deit_tiny_distilled_patch16_224, batch 128, frozen deit_tiny_patch16_224 teacher", "",
              "AdamW + NativeScaler, autocast f16, soft distillation (alpha 0.5, tau 3) over LabelSmoothingCrossEntropy(0.1); ms per step = "
              f"device events from the start of step {w} to the end of step {w + k - 1} of an epoch of {w + k} steps, over {k}; {rounds} "
              "rounds, configurations interleaved.", "",
              "| configuration | ms per step (median) | range | graphed steps in the epoch |", "|---|---|---|---|"]
    for n, _, _ in cfgs:
        v = res[n]
        lines.append(f"| {n} | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} | {graphed[n]} |")
    lines.append("")


def eval_part(lines, rounds):
    torch.manual_seed(0)
    dist = sm.create_model("deit_tiny_distilled_patch16_224").to(DEV).eval()
    plain = sm.create_model("deit_tiny_patch16_224").to(DEV).eval()
    x = torch.randn(128, 3, 224, 224, device=DEV)

    def fwd(m):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return m(x)
    gd, gp = sm.GraphedForward(dist), sm.GraphedForward(plain)
    res = interleaved_us({"distilled eager": lambda: fwd(dist), "plain eager": lambda: fwd(plain),
                          "distilled graph": lambda: gd(x), "plain graph": lambda: gp(x)}, rounds, 10)
    ld, lp = _launches(lambda: fwd(dist)), _launches(lambda: fwd(plain))
    lines += ["## (c) eval forward, batch 128, fp16 autocast: distilled against deit_tiny_patch16_224", "",
              "Expected cost of the distilled model: 198 tokens instead of 197, a second head GEMM, a second final-norm launch and the "
              "two torch launches of `(x + x_dist) / 2`.", "",
              "| model | us per forward (median) | range | launches |", "|---|---|---|---|"]
    for n, l in (("distilled eager", sum(c for _, c in ld)), ("plain eager", sum(c for _, c in lp)), ("distilled graph", "-"), ("plain graph", "-")):
        lines.append(f"| {n} | {fmt(res[n])} | {l} |")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "distill_bench.py needs the GPU"
    lines = ["# DeiT distillation on the GPU (tools/distill_bench.py)", "", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    if "a" in a.parts:
        loss_part(lines, a.rounds)
        print("\n".join(lines), flush=True)
    if "b" in a.parts:
        harness_part(lines, a.rounds, a.steps)
    if "c" in a.parts:
        eval_part(lines, a.rounds)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
