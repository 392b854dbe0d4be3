#!/usr/bin/env python3
"""One sha256 per output tensor of the entry points whose kernels sit on csrc/wave_row4.h or take smoe_common.h's wave_sum -- the two
LayerNorm backwards, the soft gate's forward, SwitchableLayerNorm forward and backward, and the kernels that only had their butterfly
replaced (generic router, gradient norm, the 8-wide wave-per-row LayerNorms) -- over a fixed grid of seeded inputs.  Run it once per
build of the library on the same device (SLIMMOE_LIB selects another build) and compare the two outputs line by line: equal lines =
equal bits.  The grid: d = one chunk / NJ 1 full / one chunk into NJ 2 / NJ 3 full / NJ 4 full, T = 1, 2, 17 partial rows and one past
the grid cap.
usage: wave_row4_digest.py [--out FILE]"""
import argparse
import hashlib
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops, optim  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DS = (4, 192, 260, 768, 1024)
SOFT_DS = (192, 384, 768, 1024)
LINES = []


def emit(name, **tensors):
    for k, t in tensors.items():
        if t is None:
            continue
        raw = t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()
        LINES.append(f"{name} {k} {hashlib.sha256(raw).hexdigest()}")


def rows(cap_rows):
    return (1, 5, 67, cap_rows + 4)


def rnd(g, *shape, scale=1.0, dt=torch.float32):
    return (torch.randn(*shape, generator=g) * scale).to(dt).to(DEV)


def layernorm_bwd(cus):
    for d, T in itertools.product(DS, rows(cus * 16)):
        g = torch.Generator().manual_seed(d * 100003 + T)
        x, dres, gamma = rnd(g, T, d, scale=2.0) + 0.5, rnd(g, T, d), 1 + 0.1 * rnd(g, d)
        dy32 = torch.randn(T, d, generator=g)
        for dn, dt in DTYPES.items():
            dy = dy32.to(dt).to(DEV)
            for use_dres, use_gamma in itertools.product((False, True), repeat=2):
                dx, dw, db = ops.layernorm_bwd(x, dy, gamma if use_gamma else None, 1e-6, dres if use_dres else None)
                emit(f"layernorm_bwd d{d} T{T} {dn} dres{int(use_dres)} gamma{int(use_gamma)}", dx=dx, dw=dw, db=db)


def gate_ln_bwd(cus):
    for d, T in itertools.product(DS, rows(cus * 16)):
        g = torch.Generator().manual_seed(d * 100019 + T)
        x, g_out = rnd(g, T, d, scale=2.0) + 0.5, rnd(g, T, d)
        ln_w, ln_b, gate_w, gate_b = 1 + 0.1 * rnd(g, d), 0.1 * rnd(g, d), rnd(g, d, scale=d ** -0.5), rnd(g, 1)
        p = torch.rand(T, 1, generator=g)
        hard = (p > 0.5).float()
        masks = {0: None, 1: torch.cat((1 - hard, hard), 1).to(DEV), 2: torch.cat((1 - p, p), 1).to(DEV)}
        gf32 = torch.randn(T, d, generator=g)
        for dn, dt in DTYPES.items():
            g_f = gf32.to(dt).to(DEV)
            for gate_on, use_out in itertools.product((0, 1, 2), (False, True)):
                dx, dlw, dlb, dgw, dgb, dz = ops.gate_ln_bwd(x, g_f, g_out if use_out else None, ln_w, ln_b, 1e-6, gate_w, gate_b,
                                                             masks[gate_on], gate_on=gate_on, want_dz=True)
                emit(f"gate_ln_bwd d{d} T{T} {dn} gate{gate_on} gout{int(use_out)}", dx=dx, dlw=dlw, dlb=dlb, dgw=dgw, dgb=dgb, dz=dz)


def soft_gate(cus):
    for d, T in itertools.product(SOFT_DS, rows(cus * 16)):
        g = torch.Generator().manual_seed(d * 100043 + T)
        x = rnd(g, T, d, scale=2.0) + 0.5
        ln = (1 + 0.1 * rnd(g, d), 0.1 * rnd(g, d), 1e-6)
        gate_w, gate_b = rnd(g, d, scale=d ** -0.5), rnd(g, 1)
        for use_ln, dt, count in itertools.product((False, True), (torch.float16, torch.bfloat16), (False, True)):
            counter = torch.full((1,), 7, dtype=torch.int32, device=DEV) if count else None
            r = ops.soft_gate_ln(x, gate_w, gate_b, ln=ln if use_ln else None, xn16_dtype=dt, want_xn32=True, want_tk32=True,
                                 want_mask=True, skip_count=counter)
            emit(f"soft_gate d{d} T{T} ln{int(use_ln)} {str(dt)[6:]} count{int(count)}", xn16=r["xn16"], xn32=r["xn32"], tk32=r["tk32"],
                 mask=r["mask"], counter=counter)


def switch_ln(cus):
    for d, K, T in itertools.product(DS, (1, 2, 5, 32), rows(cus * 32)):
        g = torch.Generator().manual_seed((d * 64 + K) * 100057 + T)
        cent = rnd(g, K, d, scale=2.0)
        x = (cent[torch.randint(0, K, (T,), generator=g).to(DEV)] + rnd(g, T, d, scale=1.5) + 300.0).contiguous()
        cent = cent + 300.0
        w, b = 1 + 0.1 * rnd(g, K, d), 0.1 * rnd(g, K, d)
        given = torch.randint(0, K, (T,), generator=g).to(DEV)
        given[T // 2] = K          # one row outside the tables: a NaN row
        dy32 = torch.randn(T, d, generator=g)
        tag = f"switch_ln d{d} K{K} T{T}"
        y, picked = ops.switch_ln(x, w, b, cent, 1e-6)
        emit(f"{tag} select", y=y, buckets=picked)
        y, _ = ops.switch_ln(x, None, None, cent, 1e-6)
        emit(f"{tag} select plain", y=y)
        y, bo = ops.switch_ln(x, w, b, cent, 1e-6, buckets=given)
        emit(f"{tag} given", y=y, buckets=bo)
        y, bo = ops.switch_ln(x, w, None, cent, 1e-6, buckets=K - 1)
        emit(f"{tag} all", y=y, buckets=bo)
        for dn, dt in DTYPES.items():
            dy = dy32.to(dt).to(DEV)
            for bn, bk in (("picked", picked), ("given", given)):
                dx, dw, db = ops.switch_ln_bwd(x, dy, w, bk, 1e-6)
                emit(f"{tag} bwd {dn} {bn}", dx=dx, dw=dw, db=db)
            dx, dw, db = ops.switch_ln_bwd(x, dy, None, given, 1e-6, num_buckets=K)
            emit(f"{tag} bwd {dn} plain", dx=dx, dw=dw, db=db)
            dx, _, _ = ops.switch_ln_bwd(x, dy, w, picked, 1e-6, want_param_grads=False)
            emit(f"{tag} bwd {dn} dx only", dx=dx)


def butterfly_only(cus):
    """the kernels whose only change is wave_sum: shapes of their tests (tests/test_gpu_parity.py, test_gpu_offgrid_shapes.py,
    test_gpu_dense.py, test_gpu_optim.py)"""
    for (d, E, k), (dn, dt) in itertools.product(((200, 8, 2), (520, 64, 2), (776, 6, 1), (1032, 12, 4), (2048, 16, 1), (768, 64, 2)),
                                                 DTYPES.items()):
        g = torch.Generator().manual_seed(d * 131 + E)
        x, wg, bg = rnd(g, 333, d, dt=dt), rnd(g, E, d, scale=d ** -0.5), 0.1 * rnd(g, E)
        for kind in (ops.GATE_NAIVE, ops.GATE_SWITCH):
            if kind == ops.GATE_SWITCH and k != 1:
                continue
            idx, score, logits, probs = ops.router_topk(x, wg, bg, k, kind, want_logits=True, want_probs=kind == ops.GATE_SWITCH)
            emit(f"router d{d} E{E} k{k} {dn} kind{kind}", idx=idx, score=score, logits=logits, probs=probs)
            idx, score, _, _ = ops.router_topk(x, wg, bg, k, kind, force_f64=True)
            emit(f"router f64 d{d} E{E} k{k} {dn} kind{kind}", idx=idx, score=score)
    for dn, dt in DTYPES.items():
        g = torch.Generator().manual_seed(17)
        grads = [rnd(g, n, dt=dt) for n in (1, 7, 2048, 2049, 100003)]
        mul, found = torch.full((1,), 0.5, device=DEV), torch.zeros(1, device=DEV)
        for i, part in enumerate(optim._grad_sumsq_partials(grads, mul, found, DEV)):
            emit(f"grad_sumsq {dn} {i}", partials=part, found=found)
    for d in (768, 1024):
        g = torch.Generator().manual_seed(d)
        T = 1000
        x, y = rnd(g, T, d), rnd(g, T, d, dt=torch.float16)
        w, b = 1 + 0.1 * rnd(g, d), 0.1 * rnd(g, d)
        inv, score = torch.randperm(T, generator=g).to(DEV), torch.rand(T, generator=g).to(DEV)
        for odt in (torch.float16, torch.bfloat16):
            out, xn = ops.gather_combine_ln(y, inv, score, T, 1, x, w, b, 1e-6, odt)
            emit(f"gather_combine_ln d{d} {str(odt)[6:]}", out=out, xn=xn)
        for odt in DTYPES.values():
            emit(f"layernorm d{d} {str(odt)[6:]}", y=ops.layernorm(x, w, b, 1e-6, odt))
        emit(f"layernorm_rows d{d}", y=ops.layernorm_rows(x, 5 * d, T // 5, d, w, b, 1e-6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "wave_row4_digest.py needs the GPU"
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    for part in (layernorm_bwd, gate_ln_bwd, soft_gate, switch_ln, butterfly_only):
        part(cus)
        torch.cuda.synchronize()
        print(f"# {part.__name__}: {len(LINES)} lines so far", file=sys.stderr, flush=True)
    text = "\n".join(LINES)
    print(f"# {len(LINES)} lines, library {sm._lib.binary_build_id()}", file=sys.stderr)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
