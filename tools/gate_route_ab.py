#!/usr/bin/env python3
"""Parent tree against this tree for a change of the Python host path (profiles/gate_route_ab.md): both trees run the SAME build of the
library (this tree's, through SLIMMOE_LIB), each figure comes from a fresh child process started in its tree, the trees alternate over
the rounds and which one goes first alternates per round.  Per round and tree: bench.py --steps 30 --warmup 5 --no-cpu-baseline,
tools/host_overhead.py without and with --force-ep (host enqueue time of one forward), and tools/train_bench.py model 64 10 with
TRAIN_BENCH_GRAPH=1 (eager and one-graph training step).  A child that fails ends the run.
usage: gate_route_ab.py PARENT_TREE [--rounds 5] [--out FILE.md]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "slim-switch-moe-vit_amd", "libslimmoe_hip.so")


def run(cmd, tree, limit, **env):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, capture_output=True, text=True, cwd=tree,
                       env=dict(os.environ, SLIMMOE_LIB=LIB, **env))
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}): {cmd} in {tree}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout


def one_side(tree):
    got = {}
    text = run(["bench.py", "--gpus", "1", "--steps", "30", "--warmup", "5", "--no-cpu-baseline"], tree, 300)
    j = json.loads([ln for ln in text.split("\n") if ln.startswith("{")][-1])
    got["bench.py ms_per_step_median, ms"], got["bench.py images/s"] = j["ms_per_step_median"], j["value"]
    for flag, word in (([], "single rank"), (["--force-ep"], "--force-ep")):
        m = re.search(r"host enqueue ([0-9.]+) ms, step ([0-9.]+) ms", run(["tools/host_overhead.py"] + flag, tree, 200))
        got[f"host_overhead.py {word}, host enqueue, ms"] = float(m.group(1))
        got[f"host_overhead.py {word}, step, ms"] = float(m.group(2))
    text = run(["tools/train_bench.py", "model", "64", "10"], tree, 300, TRAIN_BENCH_GRAPH="1")
    eager = re.search(r"train step \(fwd \+ bwd \+ clip \+ AdamW\), batch 64: ([0-9.]+) ms", text)
    graph = re.search(r"train step replayed from one HIP graph, batch 64: ([0-9.]+) ms", text)
    got["train_bench.py model 64 10, eager, ms per step"] = float(eager.group(1))
    got["train_bench.py model 64 10, one HIP graph, ms per step"] = float(graph.group(1))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    trees = (("parent", os.path.abspath(a.parent)), ("change", ROOT))
    res = {s: {} for s, _ in trees}
    t0 = time.time()
    for rnd in range(a.rounds):
        for side, tree in (trees if rnd % 2 == 0 else trees[::-1]):          # (who goes first alternates too)
            for k, v in one_side(tree).items():
                res[side].setdefault(k, []).append(v)
            print(f"round {rnd} {side} done after {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
    lines = ["| measurement | parent, rounds | parent min - max | parent median | change, rounds | change median | change median vs parent spread |",
             "|---|---|---|---|---|---|---|"]
    for k, p in res["parent"].items():
        c, up = res["change"][k], "images/s" in k
        lo, hi, pm, cm = min(p), max(p), statistics.median(p), statistics.median(c)
        verdict = "inside" if lo <= cm <= hi else ("outside: better" if (cm > hi) == up else "OUTSIDE: WORSE")
        f = (lambda v: f"{v:.0f}") if up else (lambda v: f"{v:.3f}")
        lines.append(f"| {k} | {' '.join(map(f, p))} | {f(lo)} - {f(hi)} | {f(pm)} | {' '.join(map(f, c))} | {f(cm)} | {verdict} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
