#!/usr/bin/env python3
"""The GShard gate (fmoe.GShardGate) on the GPU.

(a) The gate side alone at T = 128 x 197 and 256 x 197, E = 8 and 32: smoe_gshard_prune + smoe_gshard_aux + smoe_gshard_gate_bwd against
    the same rule as torch ops on the device (one-hot cumulative sum for the capacity rank, autograd for the backward).  Device-event
    time per call, the two sides alternating in one process, and the launch counts -- the design's: at most 2 (prune), 2 (aux), 1
    (backward), asserted here from the kernel records of the profiler.
(b) moe_tiny_patch16_224_expert8 (DeiT-Tiny, E = 8, top-2), batch 128, train_one_epoch steady-state ms per step: gate="gshard" at
    rate 1.2 against the NaiveGate on the same commit, eager and hip_graph=True; arms interleaved, median and range.
(c) The same model with force_ep on a one-rank group: the GShard gate's static exchange by capacity against the NaiveGate's
    speculative one; count read-backs per step, and ms per step.
With --parent DIR (a built checkout of the parent commit) the NaiveGate arms of (b) also run from that tree, in child processes
alternating with this tree's, twice each: the difference between the parent's two runs is the margin the NaiveGate arm is held to.
usage: gshard_bench.py [--out FILE.md] [--rounds N] [--steps K] [--parent DIR] [--skip-harness]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("GSHARD_BENCH_ROOT", HERE)       # the tree the package is imported from (a child run of --parent sets it)
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402

DEV = torch.device("cuda", 0)
MODEL = "moe_tiny_patch16_224_expert8"


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


def torch_rule(logits, idx, score, u, E, cap, num_expert, w, aux_w):
    """rules 2-4 and the backward as torch ops on the device: what a port of the gate's python lines does."""
    T = idx.shape[0]
    flat = idx.reshape(-1)
    onehot = torch.nn.functional.one_hot(flat, E)
    rank = (onehot.cumsum(0) - onehot).gather(1, flat.unsqueeze(1)).squeeze(1)
    keep = rank < cap
    keep = keep & ~torch.stack([torch.zeros_like(u, dtype=torch.bool), 2.0 * score[:, 1] < u], 1).reshape(-1)
    idx_out = torch.where(keep, flat, torch.full_like(flat, -1)).reshape(T, 2)
    l = logits.detach().requires_grad_(True)
    s = torch.softmax(l.gather(1, idx), dim=-1)
    c = torch.bincount(idx[:, 0], minlength=E).float() / T
    aux = (c * torch.softmax(l, dim=1).mean(0)).mean() * num_expert ** 2
    ((s * w * (idx_out >= 0)).sum() + aux_w * aux).backward()
    return idx_out, aux, l.grad


def gate_part(lines, rounds):
    from slim_switch_moe_vit_amd import ops
    lines += ["## (a) The gate side alone", "",
              "prune + aux + backward on given router outputs (f32 logits with an expert-0 offset of 2, rate 1.2, random routing on), "
              f"20 back-to-back calls between device events after 3 warm-up calls, {rounds} rounds, sides alternating.", "",
              "| T | E | own kernels: ms (median, range) | launches (prune + aux + bwd) | torch ops: ms (median, range) | launches |",
              "|---|---|---|---|---|---|"]
    for B in (128, 256):
        for E in (8, 32):
            T = B * 197
            g = torch.Generator(device=DEV).manual_seed(E + B)
            logits = torch.randn(T, E, device=DEV, generator=g)
            logits[:, 0] += 2.0
            val, idx = torch.topk(logits, 2, dim=1)
            score = torch.softmax(val, dim=-1)
            u = torch.rand(T, device=DEV, generator=g)
            w = torch.randn(T, 2, device=DEV, generator=g)
            cap = (int(math.ceil(1.2 * T)) * 2) // E
            scale = torch.tensor([0.01], device=DEV)

            def own():
                idx_out, top1 = ops.gshard_prune(idx, score, u, E, cap)
                aux, coef = ops.gshard_aux(logits, top1, E)
                return idx_out, aux, ops.gshard_gate_bwd(logits, idx, idx_out, score, w, coef, scale)

            def other():
                return torch_rule(logits, idx, score, u, E, cap, E, w, 0.01)

            a, b = own(), other()
            assert torch.equal(a[0], b[0]), "the two sides route differently"
            assert float((a[2] - b[2]).abs().max()) <= 1e-5 * max(1.0, float(b[2].abs().max()))
            n_p = launches(lambda: ops.gshard_prune(idx, score, u, E, cap))
            top1 = ops.gshard_prune(idx, score, u, E, cap)[1]
            n_a = launches(lambda: ops.gshard_aux(logits, top1, E))
            coef = ops.gshard_aux(logits, top1, E)[1]
            n_b = launches(lambda: ops.gshard_gate_bwd(logits, idx, a[0], score, w, coef, scale))
            assert n_p <= 2 and n_a <= 2 and n_b == 1, (n_p, n_a, n_b)          # the design's launch counts
            n_o = launches(other)
            ms = alternate_ms({"own": own, "torch": other}, rounds=rounds)
            fmt = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"
            lines.append(f"| {T} | {E} | {fmt(ms['own'])} | {n_p} + {n_a} + {n_b} | {fmt(ms['torch'])} | {n_o} |")
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


def step_ms(gate, graph, batch, w, k, force_ep=False, counter=None):
    """ms per step over steps w .. w + k - 1 of one epoch of w + k steps (and the count read-backs per step of that window)."""
    torch.manual_seed(0)
    kw = dict(gate="gshard", capacity_factor=1.2) if gate == "gshard" else {}
    model = sm.create_model(MODEL, **kw).to(DEV)
    if force_ep:
        for m in model.modules():
            if isinstance(m, sm.FMoETransformerMLP):
                m.force_ep = True
    opt = sm.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    loader = EventLoader(batch, w + k)
    if counter is not None:
        counter["n"] = 0
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), loader, opt, DEV, 0, sm.NativeScaler(), None, hip_graph=graph,
                            aux_loss_weight=0.01 if gate == "gshard" else 0.0)
    torch.cuda.synchronize()
    reads = None if counter is None else counter["n"] / (w + k)
    return loader.events[w].elapsed_time(loader.events[w + k]) / k, st["hip_graph_steps"], reads


def _batch():
    g = torch.Generator(device=DEV).manual_seed(1)
    return torch.randn(128, 3, 224, 224, device=DEV, generator=g), torch.randint(0, 1000, (128,), device=DEV, generator=g)


ARMS = [("NaiveGate, eager", "naive", False), ("NaiveGate, hip_graph=True", "naive", True),
        ("GShardGate rate 1.2, eager", "gshard", False), ("GShardGate rate 1.2, hip_graph=True", "gshard", True)]
W_STEPS = 8       # 3 eager warm steps, the capture, 4 replays


def naive_json(rounds, k):
    """the NaiveGate arms alone, as JSON on the last line (what a --parent child run prints)"""
    batch = _batch()
    step_ms("naive", True, batch, 4, 4)
    res = {name: [step_ms(gate, graph, batch, W_STEPS, k)[0] for _ in range(rounds)] for name, gate, graph in ARMS[:2]}
    print(json.dumps(res))


def harness_part(lines, rounds, k, parent):
    batch = _batch()
    step_ms("gshard", True, batch, 4, 4)                 # first-use costs outside the table
    res, graphed = {a[0]: [] for a in ARMS}, {}
    for _ in range(rounds):
        for name, gate, graph in ARMS:
            ms, gs, _ = step_ms(gate, graph, batch, W_STEPS, k)
            res[name].append(ms)
            graphed[name] = gs
    lines += [f"## (b) train_one_epoch, {MODEL}, batch 128", "",
              f"NativeScaler, autocast f16, AdamW; the GShard arms add 0.01 x the balance losses.  ms per step = device events from the "
              f"start of step {W_STEPS} to the end of step {W_STEPS + k - 1} of an epoch of {W_STEPS + k} steps, over {k}; {rounds} rounds, "
              "arms interleaved.", "", "| arm | ms per step (median) | range | graphed steps in the epoch |", "|---|---|---|---|"]
    for name, _, _ in ARMS:
        v = res[name]
        lines.append(f"| {name} | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} | {graphed[name]} |")
    lines.append("")
    for a, b in ((ARMS[2][0], ARMS[0][0]), (ARMS[3][0], ARMS[1][0])):
        lines.append(f"- the price of the gate, {a} minus {b}: {statistics.median(res[a]) - statistics.median(res[b]):+.2f} ms per step")
    lines.append("")
    if parent:
        runs = {"parent": [], "this": []}
        for _ in range(2):
            for who, root in (("parent", parent), ("this", HERE)):
                env = dict(os.environ, GSHARD_BENCH_ROOT=os.path.abspath(root))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--naive-json", "--rounds", "2", "--steps", str(k)],
                                   env=env, capture_output=True, text=True, timeout=900)
                assert r.returncode == 0, r.stderr[-2000:]
                runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
        lines += ["### The NaiveGate arms against the parent commit", "",
                  "Child processes alternating parent, this, parent, this; 2 rounds each; the median of each run.", "",
                  "| arm | parent run 1 | parent run 2 | this run 1 | this run 2 | parent's own spread | this minus parent (means) |",
                  "|---|---|---|---|---|---|---|"]
        for name in (ARMS[0][0], ARMS[1][0]):
            p = [statistics.median(r[name]) for r in runs["parent"]]
            t = [statistics.median(r[name]) for r in runs["this"]]
            lines.append(f"| {name} | {p[0]:.2f} | {p[1]:.2f} | {t[0]:.2f} | {t[1]:.2f} | {abs(p[0] - p[1]):.2f} | "
                         f"{sum(t) / 2 - sum(p) / 2:+.2f} |")
        lines.append("")


def ep_part(lines, rounds, k):
    import socket
    import torch.distributed as dist
    from slim_switch_moe_vit_amd import ep
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=DEV)
    counter = {"n": 0}
    real, real_t = ep.PendingCounts.finish_rows, ep.PendingCounts.finish

    def counting(self):
        counter["n"] += 1
        return real(self)

    def counting_t(self):
        counter["n"] += 1
        return real_t(self)
    ep.PendingCounts.finish_rows, ep.PendingCounts.finish = counting, counting_t
    try:
        batch = _batch()
        arms = [("NaiveGate, speculative static exchange (train_one_epoch's default)", "naive"),
                ("GShardGate rate 1.2, static exchange by capacity", "gshard")]
        res = {a[0]: [] for a in arms}
        reads = {}
        for _ in range(rounds):
            for name, gate in arms:
                ms, _, rd = step_ms(gate, False, batch, W_STEPS, k, force_ep=True, counter=counter)
                res[name].append(ms)
                reads[name] = rd
        kinds = {}
        for name, gate in arms:
            kw = dict(gate="gshard", capacity_factor=1.2) if gate == "gshard" else {}
            m = next(m for m in sm.create_model(MODEL, **kw).modules() if isinstance(m, sm.FMoETransformerMLP))
            m.force_ep = True
            kinds[name] = ep.static_kind(m.train(), torch.float16)
        lines += [f"## (c) The same model through force_ep on a one-rank group, eager", "",
                  "Count read-backs = host waits for a count matrix (the counted exchange's; a speculative step that overflowed is "
                  "repeated on it), per step over the whole epoch.  The speculative exchange also reads its overflow report once per "
                  "step before the backward; the capacity gate's exchange reads nothing.", "",
                  "| arm | static_kind before the harness opts in | ms per step (median) | range | count read-backs per step |",
                  "|---|---|---|---|---|"]
        for name, _ in arms:
            v = res[name]
            lines.append(f"| {name} | {kinds[name]} | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} | {reads[name]:.2f} |")
        lines.append("")
    finally:
        ep.PendingCounts.finish_rows, ep.PendingCounts.finish = real, real_t
        torch.cuda.synchronize()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--skip-harness", action="store_true")
    ap.add_argument("--naive-json", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gshard_bench.py needs the GPU"
    if a.naive_json:
        return naive_json(a.rounds, a.steps)
    lines = ["# The GShard gate on the GPU (tools/gshard_bench.py)", "", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    gate_part(lines, max(a.rounds, 5))
    print("\n".join(lines), flush=True)
    if not a.skip_harness:
        n = len(lines)
        harness_part(lines, a.rounds, a.steps, a.parent)
        print("\n".join(lines[n:]), flush=True)
        n = len(lines)
        ep_part(lines, a.rounds, a.steps)
        print("\n".join(lines[n:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
