#!/usr/bin/env python3
"""Parent against change for the csrc/wave_row4.h refactor (profiles/wave_row4_ab.md): two builds of the library, each figure from a
fresh child process (SLIMMOE_LIB selects the build), the sides alternating over the rounds (and which side goes first, per round).  Per round and side: the kernel times of
the LayerNorm family (the timing loop of tools/switch_ln_bench.py over its six SwitchableLayerNorm shapes, and at the two K = 1 shapes
smoe_layernorm_bwd -- f32 dy, and tools/dispatch_prof.py's call: f16 dy with dres --, smoe_gate_ln_bwd and smoe_soft_gate_ln_fwd),
tools/ab_bench.py (bench.py --steps 30 --warmup 5) and tools/train_bench.py model 64 10.  Prints the table in the layout of
profiles/attention_tile_ab.md; a child that fails ends the run.
usage: wave_row4_ab.py PARENT_LIB.so [CHANGE_LIB.so] [--rounds 5] [--out FILE.md]"""
import argparse
import importlib.util
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    import torch
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location("slb", os.path.join(ROOT, "tools", "switch_ln_bench.py"))
    slb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(slb)
    from slim_switch_moe_vit_amd import ops
    dev, fns = slb.DEV, {}
    for T, d, K in slb.SHAPES:
        g = torch.Generator().manual_seed(T + d + K)
        cent = torch.randn(K, d, generator=g)
        x = (cent[torch.randint(0, K, (T,), generator=g)] + 0.5 * torch.randn(T, d, generator=g)).to(dev)
        cent = cent.to(dev)
        w, b = (1.0 + 0.25 * torch.randn(K, d, generator=g)).to(dev), (0.25 * torch.randn(K, d, generator=g)).to(dev)
        dy = torch.randn(T, d, generator=g).to(dev)
        _, bk = ops.switch_ln(x, w, b, cent, 1e-5)
        fns[f"smoe_switch_ln_fwd T{T} d{d} K{K}"] = lambda x=x, w=w, b=b, cent=cent: ops.switch_ln(x, w, b, cent, 1e-5)
        fns[f"smoe_switch_ln_bwd T{T} d{d} K{K}"] = lambda x=x, dy=dy, w=w, bk=bk: ops.switch_ln_bwd(x, dy, w, bk, 1e-5)
        if K != 1:
            continue
        dy16, gw, gb = dy.half(), torch.randn(d, generator=g).to(dev) * 0.05, torch.zeros(1, device=dev)
        mask = torch.rand(T, 2, generator=g).to(dev)
        fns[f"smoe_layernorm_bwd T{T} d{d} dy f32"] = lambda x=x, dy=dy, w=w: ops.layernorm_bwd(x, dy, w[0], 1e-5)
        fns[f"smoe_layernorm_bwd T{T} d{d} dy f16 + dres"] = lambda x=x, dy16=dy16, w=w: ops.layernorm_bwd(x, dy16, w[0], 1e-6, dres=x)
        fns[f"smoe_gate_ln_bwd T{T} d{d} g_f f16 hard gate + g_out"] = (
            lambda x=x, dy16=dy16, dy=dy, w=w, b=b, gw=gw, gb=gb, mask=mask:
            ops.gate_ln_bwd(x, dy16, dy, w[0], b[0], 1e-6, gw, gb, mask, gate_on=True))
        fns[f"smoe_soft_gate_ln_fwd T{T} d{d} LN f16"] = (
            lambda x=x, w=w, b=b, gw=gw, gb=gb:
            ops.soft_gate_ln(x, gw, gb, ln=(w[0], b[0], 1e-6), xn16_dtype=torch.float16, want_xn32=True, want_mask=True))
    with torch.no_grad():
        r = slb.alternate_us(fns, n=20, rounds=5)
    print(json.dumps({k + ", us": round(statistics.median(v), 2) for k, v in r.items()}))


def run(cmd, lib, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, env=dict(os.environ, SLIMMOE_LIB=lib, SMOE_LIB=lib),
                       capture_output=True, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}): {cmd} with {lib}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change", nargs="?", default=os.path.join(ROOT, "slim-switch-moe-vit_amd", "libslimmoe_hip.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = (("parent", os.path.abspath(a.parent)), ("change", os.path.abspath(a.change)))
    res = {s: {} for s, _ in libs}
    for rnd in range(a.rounds):
        for side, lib in (libs if rnd % 2 == 0 else libs[::-1]):          # (who goes first alternates too)
            got = json.loads(run([os.path.abspath(__file__), "--child"], lib, 150).strip().split("\n")[-1])
            j = json.loads([ln for ln in run(["tools/ab_bench.py"], lib, 200).split("\n") if ln.startswith("{")][-1])
            got["bench.py ms_per_step_median, ms"], got["bench.py images/s"] = j["ms_per_step_median"], j["value"]
            m = re.search(r"train step \(fwd \+ bwd \+ clip \+ AdamW\), batch 64: ([0-9.]+) ms", run(["tools/train_bench.py", "model", "64", "10"], lib, 200))
            got["train_bench.py model, batch 64, ms per step"] = float(m.group(1))
            for k, v in got.items():
                res[side].setdefault(k, []).append(v)
            print(f"round {rnd} {side} done", file=sys.stderr, flush=True)
    lines = ["| measurement | parent, rounds | parent min - max | parent median | change, rounds | change median | change median vs parent spread |",
             "|---|---|---|---|---|---|---|"]
    for k, p in res["parent"].items():
        c, up = res["change"][k], "images/s" in k
        lo, hi, pm, cm = min(p), max(p), statistics.median(p), statistics.median(c)
        verdict = "inside" if lo <= cm <= hi else ("outside: better" if (cm > hi) == up else "OUTSIDE: WORSE")
        f = (lambda v: f"{v:.0f}") if up else (lambda v: f"{v:.2f}")
        lines.append(f"| {k} | {' '.join(map(f, p))} | {f(lo)} - {f(hi)} | {f(pm)} | {' '.join(map(f, c))} | {f(cm)} | {verdict} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
