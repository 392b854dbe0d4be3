#!/usr/bin/env python3
"""The noisy top-k gate (fmoe.NoisyGate) on the GPU.

(a) The gate side alone at T = 128 x 197 and 256 x 197, E = 8 and 32, k = 2: smoe_noisy_gate_fwd (two launches) and smoe_noisy_gate_bwd
    (one) on given logits2 = [clean | raw], against the same rule as torch ops on the device (autograd for the backward).  Device-event
    time per call, the two sides alternating in one process, and the launch counts, asserted from the profiler's kernel records.
(b) The router over the [2E, d] stack against the router over the [E, d] weight (d = 192, f16 rows, logits stored in both): what the
    unchanged router costs when it delivers clean and raw logits in one call.
(c) moe_tiny_patch16_224_expert8 (DeiT-Tiny, E = 8, top-2), batch 128, train_one_epoch(hip_graph=True) steady-state ms per step:
    gate="noisy" (0.01 x the loss) against gate="naive" on the same commit; arms alternating on one device, median and range.
usage: noisy_gate_bench.py [--out FILE.md] [--rounds N] [--steps K] [--skip-harness]"""
import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402

DEV = torch.device("cuda", 0)
MODEL = "moe_tiny_patch16_224_expert8"
fmt = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"      # noqa: E731


def alternate_ms(fns, n=20, rounds=5, warm=3):
    """{name: [ms per call, one per round]}: ``n`` back-to-back calls between two device events, the sides alternating per round."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / n)
    return out


def launches(fn):
    """number of device kernels one call of ``fn`` launches"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name)


def torch_rule(logits2, eps, k, w, aux_w):
    """the rule and its backward as torch ops on the device: what a port of the gate's python lines does"""
    l = logits2.detach().requires_grad_(True)
    E = l.shape[1] // 2
    clean, raw = l[:, :E], l[:, E:]
    sigma = torch.nn.functional.softplus(raw) + 1e-2
    noisy = clean + eps * sigma
    val, idx = noisy.topk(k + 1, dim=1)
    score = torch.softmax(val[:, :k], dim=-1)
    imp = torch.zeros(E, device=l.device).scatter_add(0, idx[:, :k].reshape(-1), score.reshape(-1))
    thr = torch.where(noisy > val[:, k:k + 1], val[:, k:k + 1], val[:, k - 1:k])
    load = (0.5 * (1.0 + torch.erf((clean - thr) / sigma * 0.7071067811865476))).sum(0)
    cv2 = lambda v: v.var(unbiased=True) / (v.mean() ** 2 + 1e-10)      # noqa: E731
    aux = cv2(imp) + cv2(load)
    ((score * w).sum() + aux_w * aux).backward()
    return idx[:, :k], aux, l.grad


def gate_part(lines, rounds):
    lines += ["## (a) The gate side alone", "",
              "Forward + backward on given logits2 (Gaussian clean and raw, k = 2), 20 back-to-back calls between device events after 3 "
              f"warm-up calls, {rounds} rounds, sides alternating.  ms: median (range).", "",
              "| T | E | own forward | own backward | own both | launches (fwd + bwd) | torch ops, both | launches |", "|---|---|---|---|---|---|---|---|"]
    for B in (128, 256):
        for E in (8, 32):
            T, k = B * 197, 2
            g = torch.Generator(device=DEV).manual_seed(E + B)
            logits2 = torch.randn(T, 2 * E, device=DEV, generator=g)
            eps = torch.randn(T, E, device=DEV, generator=g)
            w = torch.randn(T, k, device=DEV, generator=g)
            scale = torch.tensor([0.01], device=DEV)

            def fwd():
                return ops.noisy_gate_fwd(logits2, eps, k, True)

            r = fwd()

            def bwd():
                return ops.noisy_gate_bwd(logits2, eps, r["idx"], r["keep"], r["next"], w, r["coef_imp"], r["coef_load"], scale, True)

            def own():
                fwd()
                return bwd()

            def other():
                return torch_rule(logits2, eps, k, w, 0.01)

            b = other()
            same = (r["idx"] == b[0]).all(1).float().mean()
            assert float(same) > 0.9999, "the two sides route differently"
            assert float((bwd() - b[2]).abs().max()) <= 1e-4 * max(1.0, float(b[2].abs().max()))
            n_f, n_b = launches(fwd), launches(bwd)
            assert n_f == 2 and n_b == 1, (n_f, n_b)          # the design's launch counts
            n_o = launches(other)
            ms = alternate_ms({"fwd": fwd, "bwd": bwd, "own": own, "torch": other}, rounds=rounds)
            lines.append(f"| {T} | {E} | {fmt(ms['fwd'])} | {fmt(ms['bwd'])} | {fmt(ms['own'])} | {n_f} + {n_b} | {fmt(ms['torch'])} | {n_o} |")
    lines.append("")


def router_part(lines, rounds):
    lines += ["## (b) The router over 2E columns against E columns", "",
              "ops.router_topk(x f16 [T, 192], W f32, want_logits=True): k = 2 over [E, d] (the NaiveGate's call in training) against "
              "k = 1 over [2E, d] (the NoisyGate's).  ms: median (range).", "",
              "| T | E | E columns | 2E columns | extra |", "|---|---|---|---|---|"]
    for B in (128, 256):
        for E in (8, 32):
            T, d = B * 197, 192
            g = torch.Generator(device=DEV).manual_seed(E + B)
            x = torch.randn(T, d, device=DEV, generator=g).half()
            w1 = torch.randn(E, d, device=DEV, generator=g) * 0.1
            w2 = torch.randn(2 * E, d, device=DEV, generator=g) * 0.1
            ms = alternate_ms({"E": lambda: ops.router_topk(x, w1, None, 2, ops.GATE_NAIVE, None, want_logits=True),
                               "2E": lambda: ops.router_topk(x, w2, None, 1, ops.GATE_NAIVE, None, want_logits=True)}, rounds=rounds)
            lines.append(f"| {T} | {E} | {fmt(ms['E'])} | {fmt(ms['2E'])} | {statistics.median(ms['2E']) - statistics.median(ms['E']):+.3f} |")
    lines.append("")


class EventLoader:
    """``n`` times the same batch; an event on the current stream as each batch is handed out and one after the last step."""

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


def step_ms(gate, batch, w, k):
    torch.manual_seed(0)
    model = sm.create_model(MODEL, gate=gate).to(DEV)
    opt = sm.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    loader = EventLoader(batch, w + k)
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), loader, opt, DEV, 0, sm.NativeScaler(), None, hip_graph=True,
                            aux_loss_weight=0.01 if gate == "noisy" else 0.0)
    torch.cuda.synchronize()
    return loader.events[w].elapsed_time(loader.events[w + k]) / k, st["hip_graph_steps"]


def harness_part(lines, rounds, k):
    g = torch.Generator(device=DEV).manual_seed(1)
    batch = (torch.randn(128, 3, 224, 224, device=DEV, generator=g), torch.randint(0, 1000, (128,), device=DEV, generator=g))
    W = 8       # 3 eager warm steps, the capture, 4 replays
    step_ms("noisy", batch, 4, 4)                       # first-use costs outside the table
    res, graphed = {"naive": [], "noisy": []}, {}
    for _ in range(rounds):
        for gate in res:
            ms, graphed[gate] = step_ms(gate, batch, W, k)
            res[gate].append(ms)
    lines += [f"## (c) train_one_epoch(hip_graph=True), {MODEL}, batch 128", "",
              f"NativeScaler, autocast f16, AdamW; the noisy arm adds 0.01 x the gates' losses.  ms per step = device events from the start "
              f"of step {W} to the end of step {W + k - 1} of an epoch of {W + k} steps, over {k}; {rounds} rounds, arms alternating.", "",
              "| gate | ms per step (median) | range | graphed steps in the epoch |", "|---|---|---|---|"]
    for gate, v in res.items():
        lines.append(f"| {gate} | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} | {graphed[gate]} |")
    lines += ["", f"- the price of the gate: {statistics.median(res['noisy']) - statistics.median(res['naive']):+.2f} ms per step", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-harness", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "noisy_gate_bench.py needs the GPU"
    lines = ["# The noisy top-k gate on the GPU (tools/noisy_gate_bench.py)", "", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    gate_part(lines, max(a.rounds, 5))
    router_part(lines, max(a.rounds, 5))
    print("\n".join(lines), flush=True)
    if not a.skip_harness:
        n = len(lines)
        harness_part(lines, a.rounds, a.steps)
        print("\n".join(lines[n:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
