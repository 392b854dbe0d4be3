#!/usr/bin/env python3
"""SwitchableLayerNorm on the GPU (profiles/r22_switch_ln.md).

(a) Forward kernel at [128*197, 192] with K in {1, 4, 8} and [256*197, 768] with K in {1, 8, 32}: smoe_switch_ln_fwd against
    smoe_layernorm (f32 in, f32 out: the same bytes, the floor) and against the module's torch composition on the device.
(b) Backward at the same shapes: smoe_switch_ln_bwd against smoe_layernorm_bwd.
(c) deit_sw_tiny_patch16_224 (buckets 4, centroids set) against deit_tiny_patch16_224 at batch 128: eval per batch from
    evaluate()'s graph (GraphedForward), training per step of train_one_epoch(hip_graph=True) (the difference of two epoch lengths).
Device-event time per call, the sides alternating in one process, median and range over the rounds; launch counts from the
profiler's kernel records.
usage: switch_ln_bench.py [--out FILE.md] [--rounds N] [--skip-model]"""
import argparse
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402

DEV = torch.device("cuda", 0)
fmt = lambda v: f"{statistics.median(v):.1f} ({min(v):.1f} - {max(v):.1f})"      # noqa: E731
SHAPES = [(128 * 197, 192, 1), (128 * 197, 192, 4), (128 * 197, 192, 8), (256 * 197, 768, 1), (256 * 197, 768, 8), (256 * 197, 768, 32)]


def alternate_us(fns, n=20, rounds=5, warm=3):
    """{name: [us per call, one per round]}: ``n`` back-to-back calls between two device events, the sides alternating per round."""
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
            out[name].append(1e3 * e0.elapsed_time(e1) / n)
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


def kernels(rounds, lines):
    lines += ["## Kernels (us per call: median (min - max) over the rounds)", "",
              "| T x d | K | switch_ln fwd | layernorm f32->f32 | ratio | torch composition | ratio | launches own / composition |"
              " switch_ln bwd | layernorm_bwd | ratio | launches |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for T, d, K in SHAPES:
        g = torch.Generator().manual_seed(T + d + K)
        cent = torch.randn(K, d, generator=g)
        x = (cent[torch.randint(0, K, (T,), generator=g)] + 0.5 * torch.randn(T, d, generator=g)).to(DEV)
        cent = cent.to(DEV)
        w = (1.0 + 0.25 * torch.randn(K, d, generator=g)).to(DEV)
        b = (0.25 * torch.randn(K, d, generator=g)).to(DEV)
        dy = torch.randn(T, d, generator=g).to(DEV)
        _, bk = ops.switch_ln(x, w, b, cent, 1e-5)
        fwd = {"own": lambda: ops.switch_ln(x, w, b, cent, 1e-5),
               "ln": lambda: ops.layernorm(x, w[0], b[0], 1e-5, torch.float32),
               "compose": lambda: sm.switch_ln_compose(x, 1e-5, w, b, cent, None, K)}
        with torch.no_grad():
            f = alternate_us(fwd, rounds=rounds)
            nf = (launches(fwd["own"]), launches(fwd["compose"]))
        bwd = {"own": lambda: ops.switch_ln_bwd(x, dy, w, bk, 1e-5), "ln": lambda: ops.layernorm_bwd(x, dy, w[0], 1e-5)}
        r = alternate_us(bwd, rounds=rounds)
        nb = launches(bwd["own"])
        med = statistics.median
        lines.append(f"| {T} x {d} | {K} | {fmt(f['own'])} | {fmt(f['ln'])} | {med(f['own']) / med(f['ln']):.2f} | {fmt(f['compose'])} | "
                     f"{med(f['compose']) / med(f['own']):.1f}x | {nf[0]} / {nf[1]} | {fmt(r['own'])} | {fmt(r['ln'])} | "
                     f"{med(r['own']) / med(r['ln']):.2f} | {nb} |")
        print(lines[-1], flush=True)
    lines.append("")


def model(rounds, lines):
    B = 128
    torch.manual_seed(0)
    sw = sm.create_model("deit_sw_tiny_patch16_224", buckets=4, num_classes=1000).to(DEV)
    sw.router.set_centroids(0.05 * torch.randn(4, 192))
    plain = sm.create_model("deit_tiny_patch16_224", num_classes=1000).to(DEV)
    img = torch.randn(B, 3, 224, 224, device=DEV)
    ev = {}
    for name, m in (("sw", sw), ("plain", plain)):
        m.eval()
        gf = sm.GraphedForward(m)
        gf(img)
        assert gf.failed is None and gf.captures == 1, (name, gf.failed)
        ev[name] = (lambda gf=gf: gf(img))
    e = alternate_us(ev, n=10, rounds=rounds)
    lines += ["## Model, batch 128 (DeiT-Tiny; sw = deit_sw_tiny_patch16_224 with 4 buckets, centroids set)", "",
              f"- eval, per batch from evaluate()'s graph: sw {fmt(e['sw'])} us, plain {fmt(e['plain'])} us, "
              f"difference {statistics.median(e['sw']) - statistics.median(e['plain']):+.1f} us"]
    print(lines[-1], flush=True)
    labels = torch.randint(0, 1000, (B,))
    cpu = img.cpu()
    warm = sm.GraphedTrainStep.WARM

    def epoch_ms(m, n):
        opt = sm.AdamW(m.parameters(), lr=1e-4, weight_decay=0.05)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = sm.train_one_epoch(m, torch.nn.CrossEntropyLoss(), [(cpu, labels)] * n, opt, DEV, 0, sm.NativeScaler(), 1.0, hip_graph=True)
        torch.cuda.synchronize()
        assert st["hip_graph_steps"] == n - warm, st
        return 1e3 * (time.perf_counter() - t0)
    tr = {"sw": [], "plain": []}
    for _ in range(max(3, rounds // 2 + 1)):
        for name, m in (("sw", sw), ("plain", plain)):
            short, long_ = epoch_ms(m, warm + 4), epoch_ms(m, warm + 24)
            tr[name].append(1e3 * (long_ - short) / 20)
    lines.append(f"- training, per step of train_one_epoch(hip_graph=True) (20 replayed steps, wall clock incl. the host-to-device copy of "
                 f"the batch): sw {fmt(tr['sw'])} us, plain {fmt(tr['plain'])} us (median (min - max) over {len(tr['sw'])} rounds); the "
                 f"medians differ by {statistics.median(tr['sw']) - statistics.median(tr['plain']):+.1f} us")
    print(lines[-1], flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}", ""]
    kernels(a.rounds, lines)
    if not a.skip_model:
        model(a.rounds, lines)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
