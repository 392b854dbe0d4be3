#!/usr/bin/env python3
"""Parent against change for the csrc/optim_table.h refactor (profiles/optim_table_ab.md): two builds of the library, each figure from
a fresh child process (SLIMMOE_LIB selects the build), the sides alternating over the rounds, and which side goes first alternating
per round.  Per round and side: tools/adamw_ab.py --json (the one-launch AdamW step and LAMB's three launches over ViT-B/16 E = 8's
parameter set), the EMA launch (tools/ema_bench.py's kernel part), tools/train_bench.py model 64 10 with TRAIN_BENCH_GRAPH=1 (eager
and one-graph harness) under AdamW and under --opt lamb, and tools/ab_bench.py (the forward benchmark; its kernels are untouched).
--state FILE keeps every figure measured so far: a later call with the same file goes on from the round it stopped in, so the rounds
may be spread over several calls; --deadline SECONDS starts no round that, going by the longest one so far, would end later than
that.  A child that fails ends the run.
usage: optim_table_ab.py PARENT_LIB.so [CHANGE_LIB.so] [--rounds 5] [--state FILE.json] [--deadline SECONDS] [--out FILE.md]"""
import argparse
import importlib.util
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ema_child():
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location("ema_bench", os.path.join(ROOT, "tools", "ema_bench.py"))
    eb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eb)
    ms, _ = eb.kernel_part([])
    print(json.dumps({"ema_ms": round(ms, 4)}))


def run(cmd, lib, limit, **env):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, SLIMMOE_LIB=lib, SMOE_LIB=lib, **env))
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}): {cmd} with {lib}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout


def last_json(text):
    return json.loads([ln for ln in text.split("\n") if ln.startswith("{")][-1])


def one_side(lib):
    got = {}
    j = last_json(run(["tools/adamw_ab.py", "--json", "--rounds", "5"], lib, 200))
    got["smoe_adamw_step_multi, ViT-B/16 E = 8 set, ms"] = j["adamw_ms"]
    got["smoe_lamb_stage1 + trust + stage2, same set, ms"] = j["lamb_ms"]
    got["smoe_ema_update_multi, ViT-B/16 E = 8 state, ms"] = last_json(run([os.path.abspath(__file__), "--ema-child"], lib, 200))["ema_ms"]
    for opt, word in (("adamw", "AdamW"), ("lamb", "LAMB")):
        text = run(["tools/train_bench.py", "model", "64", "10", "--opt", opt], lib, 300, TRAIN_BENCH_GRAPH="1")
        eager = re.search(r"train step \(fwd \+ bwd \+ clip \+ %s\), batch 64: ([0-9.]+) ms" % word, text)
        graph = re.search(r"train step replayed from one HIP graph, batch 64: ([0-9.]+) ms", text)
        got[f"train_bench.py model 64 10, {word}, eager, ms per step"] = float(eager.group(1))
        got[f"train_bench.py model 64 10, {word}, one HIP graph, ms per step"] = float(graph.group(1))
    j = last_json(run(["tools/ab_bench.py"], lib, 200))
    got["bench.py ms_per_step_median, ms"], got["bench.py images/s"] = j["ms_per_step_median"], j["value"]
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change", nargs="?", default=os.path.join(ROOT, "slim-switch-moe-vit_amd", "libslimmoe_hip.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--state")
    ap.add_argument("--deadline", type=float, default=None)
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = (("parent", os.path.abspath(a.parent)), ("change", os.path.abspath(a.change)))
    done = []          # [[round, side, {measurement: figure}]]
    if a.state and os.path.exists(a.state):
        done = json.load(open(a.state))
    t0, longest = time.time(), 0.0
    for rnd in range(a.rounds):
        t_round = time.time()
        if a.deadline is not None and t_round - t0 + longest > a.deadline:
            print(f"stopped before round {rnd}: {t_round - t0:.0f} s used, the longest round took {longest:.0f} s", file=sys.stderr, flush=True)
            break
        for side, lib in (libs if rnd % 2 == 0 else libs[::-1]):          # (who goes first alternates too)
            if any(r == rnd and s == side for r, s, _ in done):
                continue
            done.append([rnd, side, one_side(lib)])
            if a.state:
                os.makedirs(os.path.dirname(os.path.abspath(a.state)), exist_ok=True)
                json.dump(done, open(a.state, "w"))
            print(f"round {rnd} {side} done", file=sys.stderr, flush=True)
        longest = max(longest, time.time() - t_round)
    res = {s: {} for s, _ in libs}
    whole = [r for r in range(a.rounds) if sum(1 for rr, _, _ in done if rr == r) == 2]
    for _, side, got in sorted((d for d in done if d[0] in whole), key=lambda d: d[0]):
        for k, v in got.items():
            res[side].setdefault(k, []).append(v)
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
    ema_child() if "--ema-child" in sys.argv else main()
