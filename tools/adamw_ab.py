#!/usr/bin/env python3
"""The fused AdamW step (one smoe_adamw_step_multi launch) and the fused LAMB step (smoe_lamb_stage1_multi, smoe_lamb_trust_multi,
smoe_lamb_stage2_multi) over ViT-B/16 E = 8's parameter set, this tree's library against ANOTHER build of it, alternated on one
device: the setting of profiles/r17_lamb.md (moe_base_patch16_224_expert8_top1, f16 gradients, timm's weight-decay split, no 16-bit
images).  Without --other: the one library that SLIMMOE_LIB (or the tree) names; --json prints its medians as one JSON line, which is
how tools/optim_table_ab.py takes each figure from a fresh process.

Both libraries are driven through the C entry point directly, so the other build may be of another ABI: up to ABI 29 the entry point
takes its betas as floats, from ABI 30 on as doubles.  One launch per gradient dtype is the whole step here (smoe_step_advance is a
one-thread launch and is left out); 26 B of algorithmic traffic per element (gradient 2, p / exp_avg / exp_avg_sq read and written 24).

usage: adamw_ab.py [--other PATH/libslimmoe_hip.so] [--rounds N] [--steps K] [--json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import _lib, ops, optim  # noqa: E402

DEV = torch.device("cuda", 0)


def entry(path):
    """({entry point: callable taking the launch's arguments}, ABI number) of the build at `path`."""
    lib = ctypes.CDLL(path)
    lib.smoe_abi_version.restype = ctypes.c_int
    abi = lib.smoe_abi_version()
    beta = ctypes.c_double if abi >= 30 else ctypes.c_float
    v, f, i, i64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    protos = {"smoe_adamw_step_multi": [v, v, i, v, i64, i, beta, beta, f, v, v, v, v, v],
              "smoe_lamb_stage1_multi": [v, v, i, v, i64, i, beta, beta, f, f, i, v, v, v, v, v, v],
              "smoe_lamb_trust_multi": [v, i64, v, v, i, i, v, v, v],
              "smoe_lamb_stage2_multi": [v, v, i, v, i64, beta, beta, f, i, v, v, v, v, v]}
    fns = {}
    for name, argtypes in protos.items():
        fns[name] = getattr(lib, name)
        fns[name].restype, fns[name].argtypes = ctypes.c_int, argtypes
    return fns, abi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "adamw_ab.py needs the GPU"
    cpu = sm.create_model("moe_base_patch16_224_expert8_top1")
    shapes = [p.shape for p in cpu.parameters()]
    del cpu
    g = torch.Generator(device=DEV).manual_seed(0)
    ps = [torch.randn(s, device=DEV, generator=g) * 0.02 for s in shapes]
    gs = [(torch.randn(s, device=DEV, generator=g) * 1e-2).half() for s in shapes]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    numels = [p.numel() for p in ps]
    n = sum(numels)
    blk, nb = optim._block_table(numels, DEV)
    tab = torch.tensor([[t.data_ptr() for t in ts] for ts in (ps, gs, ms, vs)] + [numels], dtype=torch.int64, device=DEV)
    wds = [0.05 if p.ndim > 1 else 0.0 for p in ps]
    hyp = torch.tensor([[1e-3] * len(ps), wds, [float(wd != 0) for wd in wds]], dtype=torch.float32, device=DEV)   # (AdamW reads two rows)
    step = torch.tensor([100.0], device=DEV)
    first = optim._first_block_table(numels, DEV)
    norms, trust = torch.zeros((2, sum(nb)), device=DEV), torch.ones(len(ps), device=DEV)
    arms = {"this tree": entry(_lib.LIB_PATH)}
    if a.other:
        arms["other"] = entry(a.other)
    f16 = ops.dtype_code(torch.float16)

    def adamw(fns):
        rc = fns["smoe_adamw_step_multi"](tab.data_ptr(), hyp.data_ptr(), len(ps), blk.data_ptr(), sum(nb), f16, 0.9, 0.999, 1e-8,
                                          step.data_ptr(), None, None, None, None)
        assert rc == 0, rc

    def lamb(fns):
        rc = fns["smoe_lamb_stage1_multi"](tab.data_ptr(), hyp.data_ptr(), len(ps), blk.data_ptr(), sum(nb), f16, 0.9, 0.999, 0.1, 1e-6, 1,
                                           step.data_ptr(), None, None, None, norms.data_ptr(), None)
        assert rc == 0, rc
        rc = fns["smoe_lamb_trust_multi"](norms.data_ptr(), sum(nb), first.data_ptr(), hyp.data_ptr(), len(ps), 0, None, trust.data_ptr(), None)
        assert rc == 0, rc
        rc = fns["smoe_lamb_stage2_multi"](tab.data_ptr(), hyp.data_ptr(), len(ps), blk.data_ptr(), sum(nb), 0.9, 0.999, 1e-6, 1,
                                           step.data_ptr(), trust.data_ptr(), None, None, None)
        assert rc == 0, rc

    def ms_per_step(launch, fns):
        for _ in range(3):
            launch(fns)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            launch(fns)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    res, res_lamb = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (fns, _) in arms.items():
            res[k].append(ms_per_step(adamw, fns))
            res_lamb[k].append(ms_per_step(lamb, fns))
    if a.json:
        print(json.dumps({"adamw_ms": round(statistics.median(res["this tree"]), 4), "lamb_ms": round(statistics.median(res_lamb["this tree"]), 4)}))
        return
    moved = 26.0 * n
    print(f"# fused AdamW step, {len(ps)} tensors, {n / 1e6:.1f} M values, f16 gradients, {moved / 1e9:.2f} GB per step; torch {torch.__version__}, "
          f"{torch.cuda.get_device_name(0)}; {a.rounds} rounds of {a.steps} steps after 3, arms alternated")
    print("| arm | ABI | ms per step (median) | range | TB/s at the median | every round |")
    print("|---|---|---|---|---|---|")
    for k, v in res.items():
        med = statistics.median(v)
        print(f"| {k} | {arms[k][1]} | {med:.3f} | {min(v):.3f} - {max(v):.3f} | {moved / (med * 1e-3) / 1e12:.2f} | {', '.join('%.3f' % t for t in v)} |")
    print()
    print("# fused LAMB step (stage 1, trust ratios, stage 2) over the same set")
    print("| arm | ABI | ms per step (median) | range | every round |")
    print("|---|---|---|---|---|")
    for k, v in res_lamb.items():
        print(f"| {k} | {arms[k][1]} | {statistics.median(v):.3f} | {min(v):.3f} - {max(v):.3f} | {', '.join('%.3f' % t for t in v)} |")
    if not a.other:
        return
    for what, r in (("AdamW", res), ("LAMB", res_lamb)):
        gap = statistics.median(r["this tree"]) - statistics.median(r["other"])
        spread = max(max(v) - min(v) for v in r.values())
        print(f"{what}: this tree minus other: {gap:+.4f} ms; the wider range of the two arms is {spread:.4f} ms: "
              + ("inside the measured spread" if abs(gap) <= spread else "outside the measured spread"))


if __name__ == "__main__":
    main()
