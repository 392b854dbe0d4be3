#!/usr/bin/env python3
"""One sha256 per output tensor of the optimizer-side entry points (csrc/optim.hip, csrc/lamb.hip: the kernels on csrc/optim_table.h)
over a fixed grid of seeded inputs, driven through the C entry points.  Run it once per build of the library on the same device
(SLIMMOE_LIB selects another build) and compare the two outputs line by line: equal lines = equal bits.  Sizes: the scalar tail alone,
one vector, vector + tail, either side of a 16K block, several blocks with a tail.
usage: optim_digest.py [--out FILE]"""
import argparse
import hashlib
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import _lib, ops, optim  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SIZES = (1, 3, 4, 5, 16383, 16384, 16385, 40003, 100003)
IMAGES = (torch.float16, torch.bfloat16, None)
LINES = []


def emit(name, **tensors):
    for k, t in tensors.items():
        raw = t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()
        LINES.append(f"{name} {k} {hashlib.sha256(raw).hexdigest()}")


def emit_each(name, **lists):
    for k, ts in lists.items():
        emit(name, **{f"{k}{i}": t for i, t in enumerate(ts) if t is not None})


def scalar(v):
    return None if v is None else torch.tensor([float(v)], dtype=torch.float32, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def i64(rows):
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def f32(rows):
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


def state(seed, sizes, gdt):
    """p, g, exp_avg, exp_avg_sq of every size, on the host (cloned to the device per case)"""
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(n, generator=g) * 0.5 for n in sizes], [(torch.randn(n, generator=g) * 1e-2).to(gdt) for n in sizes],
            [torch.randn(n, generator=g) * 1e-2 for n in sizes], [torch.rand(n, generator=g) * 1e-4 for n in sizes])


def upload(ts):
    return [t.clone().to(DEV) for t in ts]


def images(sizes, kinds):
    """per tensor a 16-bit image buffer (or None), and the shadow table (None when no tensor has one)"""
    imgs = [torch.full((n,), 0x7FA5, dtype=torch.int16, device=DEV) if k is not None else None for n, k in zip(sizes, kinds)]
    if not any(k is not None for k in kinds):
        return imgs, None
    return imgs, i64([[ptr(t) or 0 for t in imgs], [ops.dtype_code(k) if k is not None else 0 for k in kinds]])


def grad_sumsq(lib):
    for dn, dt in DTYPES.items():
        gs = upload(state(11, SIZES, dt)[1])
        poisoned = upload(state(11, SIZES, dt)[1])
        poisoned[-1][SIZES[-1] // 2] = float("nan")
        for inv, (tag, grads) in itertools.product((None, 0.37), (("finite", gs), ("nan", poisoned))):
            mul = scalar(inv)
            for n, g in zip(SIZES, grads):
                part, found = torch.zeros(lib.smoe_grad_sumsq_blocks(n), device=DEV), torch.zeros(1, device=DEV)
                _lib.check(lib.smoe_grad_sumsq(g.data_ptr(), ops.dtype_code(dt), n, ptr(mul), part.data_ptr(), found.data_ptr(), None),
                           "smoe_grad_sumsq")
                emit(f"grad_sumsq {dn} n{n} inv{inv} {tag}", partials=part, found=found)
            blk, nb = optim._block_table(list(SIZES), DEV)
            zeros = [0] * len(SIZES)
            tab = i64([zeros, [g.data_ptr() for g in grads], zeros, zeros, list(SIZES)])
            part, found = torch.zeros(sum(nb), device=DEV), torch.zeros(1, device=DEV)
            rc = lib.smoe_grad_sumsq_multi(tab.data_ptr(), len(SIZES), blk.data_ptr(), sum(nb), ops.dtype_code(dt), ptr(mul),
                                           part.data_ptr(), found.data_ptr(), None)
            _lib.check(rc, "smoe_grad_sumsq_multi")
            emit(f"grad_sumsq_multi {dn} inv{inv} {tag}", partials=part, found=found)


def adamw(lib):
    blk, nb = optim._block_table(list(SIZES), DEV)
    cases = list(itertools.product(((0.9, 0.999), (0.0, 0.999)), (1, 1000), (0.0, 0.05), (0, 1), (None, 0.25)))
    for dn, dt in DTYPES.items():
        host = state(23, SIZES, dt)
        for (b1, b2), t, wd, found, gm in cases:
            tag = f"{dn} betas{b1},{b2} t{t} wd{wd} found{found} gm{gm}"
            step, found_inf, mult = scalar(t), scalar(found), scalar(gm)
            ps, gs, ms, vs = (upload(x) for x in host)
            for n, p, g, m, v in zip(SIZES, ps, gs, ms, vs):
                rc = lib.smoe_adamw_step(p.data_ptr(), g.data_ptr(), ops.dtype_code(dt), m.data_ptr(), v.data_ptr(), n, 1e-3, b1, b2,
                                         1e-8, wd, step.data_ptr(), ptr(mult), found_inf.data_ptr(), None)
                _lib.check(rc, "smoe_adamw_step")
            emit_each(f"adamw {tag}", p=ps, m=ms, v=vs)
            for shift in range(3):       # every tensor with an f16 image, a bf16 image and none in turn
                kinds = [IMAGES[(i + shift) % 3] for i in range(len(SIZES))]
                ps, gs, ms, vs = (upload(x) for x in host)
                imgs, shadow = images(SIZES, kinds)
                tab = i64([[x.data_ptr() for x in ts] for ts in (ps, gs, ms, vs)] + [list(SIZES)])
                hyp = f32([[1e-3 if i % 2 else 5e-4 for i in range(len(SIZES))], [wd if i % 3 else 0.0 for i in range(len(SIZES))]])
                rc = lib.smoe_adamw_step_multi(tab.data_ptr(), hyp.data_ptr(), len(SIZES), blk.data_ptr(), sum(nb), ops.dtype_code(dt),
                                               b1, b2, 1e-8, step.data_ptr(), ptr(mult), found_inf.data_ptr(), ptr(shadow), None)
                _lib.check(rc, "smoe_adamw_step_multi")
                emit_each(f"adamw_multi {tag} images{shift}", p=ps, m=ms, v=vs, img=imgs)


def lamb(lib):
    sizes = list(SIZES)
    blk, nb = optim._block_table(sizes, DEV)
    first = optim._first_block_table(sizes, DEV)
    n_t, n_blocks = len(sizes), sum(nb)
    kinds = [IMAGES[i % 3] for i in range(n_t)]
    flags = list(itertools.product((0, 1), (0.0, 0.02), (0, 1), (0, 1), (0, 1), (None, 1.0), (0, 1)))
    for dn, dt in DTYPES.items():
        host = state(37, sizes, dt)
        for adapt, wd, bias, trust_clip, averaging, mgn, found in flags:
            tag = f"lamb {dn} adapt{adapt} wd{wd} bias{bias} tclip{trust_clip} avg{averaging} mgn{mgn} found{found}"
            ps, gs, ms, vs = (upload(x) for x in host)
            imgs, shadow = images(sizes, kinds)
            step, found_inf, mult = scalar(5), scalar(found), scalar(0.5)
            tab = i64([[x.data_ptr() for x in ts] for ts in (ps, gs, ms, vs)] + [sizes])
            # (adapt = 0 leaves every third tensor out of the trust ratio; as in optim.Lamb such a tensor has no weight decay)
            adapts = [bool(adapt or i % 3) for i in range(n_t)]
            hyp = f32([[1e-2 if i % 2 else 5e-3 for i in range(n_t)], [wd if a else 0.0 for a in adapts], [float(a) for a in adapts]])
            zeros = [0] * n_t
            gtab = i64([zeros, [g.data_ptr() for g in gs], zeros, zeros, sizes])
            part = torch.zeros(n_blocks, device=DEV)
            rc = lib.smoe_grad_sumsq_multi(gtab.data_ptr(), n_t, blk.data_ptr(), n_blocks, ops.dtype_code(dt), mult.data_ptr(),
                                           part.data_ptr(), None, None)
            _lib.check(rc, "smoe_grad_sumsq_multi")
            out = f32([1.0, 0.0])
            rc = lib.smoe_lamb_clip(part.data_ptr(), n_blocks, None, None, float(mgn) if mgn is not None else 0.0, found_inf.data_ptr(),
                                    out.data_ptr(), None)
            _lib.check(rc, "smoe_lamb_clip")
            norms, trust = torch.zeros((2, n_blocks), device=DEV), torch.ones(n_t, device=DEV)
            rc = lib.smoe_lamb_stage1_multi(tab.data_ptr(), hyp.data_ptr(), n_t, blk.data_ptr(), n_blocks, ops.dtype_code(dt), 0.9, 0.999,
                                            0.1 if averaging else 1.0, 1e-6, bias, step.data_ptr(), mult.data_ptr(), out.data_ptr(),
                                            found_inf.data_ptr(), norms.data_ptr(), None)
            _lib.check(rc, "smoe_lamb_stage1_multi")
            rc = lib.smoe_lamb_trust_multi(norms.data_ptr(), n_blocks, first.data_ptr(), hyp.data_ptr(), n_t, trust_clip,
                                           found_inf.data_ptr(), trust.data_ptr(), None)
            _lib.check(rc, "smoe_lamb_trust_multi")
            rc = lib.smoe_lamb_stage2_multi(tab.data_ptr(), hyp.data_ptr(), n_t, blk.data_ptr(), n_blocks, 0.9, 0.999, 1e-6, bias,
                                            step.data_ptr(), trust.data_ptr(), found_inf.data_ptr(), ptr(shadow), None)
            _lib.check(rc, "smoe_lamb_stage2_multi")
            # (norms of a tensor that does not adapt are never written nor read: the buffer starts zeroed, so its lines compare too)
            emit_each(tag, p=ps, m=ms, v=vs, img=imgs)
            emit(tag, norms=norms, trust=trust, out=out)


def ema(lib):
    sizes = list(SIZES) + [32768 + 5]
    blk, nb = optim._block_table(sizes, DEV)
    g = torch.Generator().manual_seed(41)
    e0, m0 = [torch.randn(n, generator=g) for n in sizes], [torch.randn(n, generator=g) for n in sizes]
    for decay, skip in itertools.product((0.9999, 0.5), (None, 0, 1)):
        es, ms = upload(e0), upload(m0)
        tab = i64([[t.data_ptr() for t in es], [t.data_ptr() for t in ms], sizes])
        flag = scalar(skip)
        rc = lib.smoe_ema_update_multi(tab.data_ptr(), len(sizes), blk.data_ptr(), sum(nb), decay, 1.0 - decay, ptr(flag), None)
        _lib.check(rc, "smoe_ema_update_multi")
        emit_each(f"ema decay{decay} skip{skip}", e=es)


def scalars(lib):
    for scale, tracker, found, interval in itertools.product((65536.0, 3.0), (0.0, 1.0, 1998.0, 1999.0), (None, 0, 1), (1, 2000)):
        s, t, f = scalar(scale), scalar(tracker), scalar(found)
        _lib.check(lib.smoe_amp_update(s.data_ptr(), t.data_ptr(), ptr(f), 2.0, 0.5, interval, None), "smoe_amp_update")
        emit(f"amp_update scale{scale} tracker{tracker} found{found} interval{interval}", scale=s, tracker=t)
    for step, found in itertools.product((0.0, 1.0, 999.0, 16777216.0), (None, 0, 1)):
        s, f = scalar(step), scalar(found)
        _lib.check(lib.smoe_step_advance(s.data_ptr(), ptr(f), None), "smoe_step_advance")
        emit(f"step_advance step{step} found{found}", step=s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_digest.py needs the GPU"
    lib = _lib.load()
    for part in (grad_sumsq, adamw, lamb, ema, scalars):
        part(lib)
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
