#!/usr/bin/env python3
"""A/B inside ONE process on one device: VisionTransformer.skip_aware_attention off / on at forced bypass shares.

Models: resmoe_tiny_patch16_224_expert8 at batch 128 and resmoe_base_patch16_224_expert8_top1 (ViT-B) at batch 256.  For every
share in SHARES each gate's threshold is set to the matching quantile of its OWN p on a seeded calibration batch (one composed f32
forward whose gates set their threshold as they are reached), then flag off / flag on alternate R times: S eager steps and S
replays of evaluate()'s HIP graph each, timed with HIP events after a warm-up; medians with min / max.  Two profiled eager steps per
mode give the per-kernel table of the attention half (ops.profile_begin).  A last section times smoe_attention_fwd_varlen alone
under its four flag combinations (weight on the probability / on the score, key-tile tiers on / off) on a synthetic plan.

    python tools/skip_attention_bench.py [rounds=3] [steps=10] [models=tiny,base]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops, resmoe  # noqa: E402

SHARES = (0.0, 0.25, 0.5, 0.75, 0.95)
MODELS = {"tiny": ("resmoe_tiny_patch16_224_expert8", 128), "base": ("resmoe_base_patch16_224_expert8_top1", 256)}
HALF_KERNELS = ("gate_ln", "qkv_gemm", "attention", "attn_proj_gemm", "skip_plan", "qkv_gemm_skip", "attention_varlen",
                "attn_proj_gemm_skip", "skip_expand")
DEV = torch.device("cuda", 0)


def gates(model):
    return [m for m in model.modules() if isinstance(m, resmoe.Gate)]


def calibrate(model, share: float, images):
    """Every gate's threshold <- the (1 - share) quantile of its own p on ``images`` (composed f32 forward, in block order)."""
    def hook(g, args):
        p = torch.sigmoid(g.head(args[0])).flatten().float()
        g.threshold.fill_(float(torch.quantile(p[torch.randperm(p.numel(), device=p.device)[:1 << 20]], 1.0 - share)))
    hs = [g.register_forward_pre_hook(hook) for g in gates(model)]
    with torch.no_grad():
        model(images)
    for h in hs:
        h.remove()


def median(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def timed(fn, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]


def run_model(tag, rounds, steps):
    name, batch = MODELS[tag]
    torch.manual_seed(0)
    model = sm.create_model(name, num_classes=1000).eval().to(DEV)
    images = torch.randn(batch, 3, 224, 224, generator=torch.Generator().manual_seed(100)).to(DEV)
    calib = torch.randn(16, 3, 224, 224, generator=torch.Generator().manual_seed(101)).to(DEV)
    out = {"model": name, "batch": batch, "shares": {}}

    def eager():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return model(images)

    for share in SHARES:
        calibrate(model, share, calib)
        res = {f: {"eager": [], "graph": [], "kern": {}} for f in (False, True)}
        graphed = {}
        for flag in (False, True):
            model.skip_aware_attention = flag
            graphed[flag] = sm.GraphedForward(model)
            graphed[flag](images)
        got = {}
        for _ in range(rounds):
            for flag in (False, True):
                model.skip_aware_attention = flag
                for g in gates(model):
                    g._total_tokens, g._skipped_tokens = 0, 0
                for _ in range(3):
                    eager()
                torch.cuda.synchronize()
                dg = [g for n, g in model.named_modules() if n.endswith("dense_gate")]
                got[flag] = sum(g._skipped_tokens for g in dg) / max(1, sum(g._total_tokens for g in dg))
                res[flag]["eager"] += timed(eager, steps)
                graphed[flag](images)
                res[flag]["graph"] += timed(lambda: graphed[flag](images), steps)
                ops.profile_begin(only=HALF_KERNELS)
                for _ in range(2):
                    eager()
                torch.cuda.synchronize()
                for nm, _, ms in ops.profile_end():
                    a = res[flag]["kern"].setdefault(nm, [0, 0.0])
                    a[0] += 1
                    a[1] += ms
        row = {}
        for flag in (False, True):
            r = res[flag]
            row["flag_on" if flag else "flag_off"] = {
                "dense_gate_bypass_share": round(got[flag], 4), "eager": median(r["eager"]), "graph_replay": median(r["graph"]),
                "attention_half_kernels_us_per_launch": {k: round(v[1] / v[0] * 1e3, 2) for k, v in sorted(r["kern"].items())},
                "attention_half_us_per_block": round(sum(v[1] for v in r["kern"].values()) / (2 * rounds * len(model.blocks)) * 1e3, 2)}
        row["graph_replay_on_minus_off_us"] = round((row["flag_on"]["graph_replay"]["median_ms"]
                                                     - row["flag_off"]["graph_replay"]["median_ms"]) * 1e3, 1)
        out["shares"][str(share)] = row
        print(json.dumps({tag: {str(share): row}}), flush=True)
    model.skip_aware_attention = False
    return out


def varlen_ab(B=256, H=12, N=197, reps=20):
    """smoe_attention_fwd_varlen alone, per bypass share and flag combination, against smoe_attention_fwd over all B*N rows."""
    out = {}
    g = torch.Generator().manual_seed(7)
    full = torch.randn(B * N, 3 * H * 64, generator=g).half().to(DEV)
    t_full = median(timed(lambda: ops.attention(full, B, N, H, 64, 0.125), reps))
    out["smoe_attention_fwd (all rows)"] = t_full
    for share in SHARES:
        byp = torch.rand(B, N, generator=g) < share
        n = (~byp).sum(dim=1)
        m = N - n
        length = (n + (m > 0)).to(torch.int32)
        rs = (torch.cumsum(length, 0) - length).to(torch.int32)
        args = (rs.to(DEV), length.to(DEV), m.to(torch.int32).to(DEV))
        for flags, nm in ((0, "probability, tiers"), (ops.VARLEN_WEIGHT_SCORE, "score, tiers"), (ops.VARLEN_NO_TIERS, "probability, no tiers"),
                          (ops.VARLEN_WEIGHT_SCORE | ops.VARLEN_NO_TIERS, "score, no tiers")):
            ops.attention_varlen(full, *args, N, H, 64, 0.125, flags=flags)
            out[f"share {share}: {nm}"] = median(timed(lambda: ops.attention_varlen(full, *args, N, H, 64, 0.125, flags=flags), reps))
    return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    tags = (sys.argv[3] if len(sys.argv) > 3 else "tiny,base").split(",")
    res = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "steps": steps}
    res["varlen_kernel_ab"] = varlen_ab()
    print(json.dumps({"varlen_kernel_ab": res["varlen_kernel_ab"]}), flush=True)
    for tag in tags:
        res[tag] = run_model(tag, rounds, steps)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
