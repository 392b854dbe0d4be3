#!/usr/bin/env python3
"""Mixup / CutMix and the soft-target cross-entropy (mixup.Mixup, loss.SoftTargetCrossEntropy: the timm objects of main.py:505-517,
653-661 and engine.py:46-47, 54) on the GPU, beside timm's torch lines restated here (timm is not a dependency of this package).

(a) smoe_mixup_images at B 128 / 256, 3x224x224 and B 32, 3x384x384, a Mixup and a CutMix draw in batch mode and an elem-mode draw of
    both kinds: us per call and the EFFECTIVE rate at 2 * 4 * B*C*H*W bytes (one read and one write of every value; the batch fits the
    256-MiB Infinity Cache, so this is no share of the HBM rate).
(b) loss forward + backward at [128, 1000] and [256, 1000] f16 logits, own against the torch composition: us per forward + backward,
    launches per forward + backward (torch.profiler kernel rows), and the max error of each against float64 on f32 logits.
    --loss-loop own|torch runs that loop alone (for `rocprofv3 --kernel-trace --stats -- python tools/mixup_bench.py --loss-loop own`).
(c) resmoe_tiny_patch16_224_expert8, batch 128, train_one_epoch steady state, eager and hip_graph=True: integer labels +
    nn.CrossEntropyLoss (today), restated-timm Mixup + torch soft-target loss, own Mixup + own loss.  Steady state as tools/ema_bench.py
    measures it (device events the loader records as it hands out each batch), ROUNDS rounds, configurations interleaved.
usage: mixup_bench.py [--out FILE.md] [--rounds N] [--steps K] [--parts abc] [--loss-loop own|torch]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402

DEV = torch.device("cuda", 0)


# ---- timm's torch lines, restated ------------------------------------------------------------------------------------------------
def timm_one_hot(x, num_classes, on_value=1., off_value=0.):
    x = x.long().view(-1, 1)
    return torch.full((x.size(0), num_classes), off_value, device=x.device).scatter_(1, x, on_value)


def timm_mixup_target(target, num_classes, lam, smoothing):
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    y1 = timm_one_hot(target, num_classes, on_value, off_value)
    y2 = timm_one_hot(target.flip(0), num_classes, on_value, off_value)
    return y1 * lam + y2 * (1. - lam)


def timm_mix_images(x, mode, lam, use_cutmix, boxes):
    """The image lines of timm's Mixup for a given draw (``lam`` float / f32 [B], ``use_cutmix`` bool / bool [B], ``boxes`` [B, 4])."""
    if mode == "batch":
        if use_cutmix:
            yl, yh, xl, xh = (int(v) for v in boxes[0])
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        elif lam != 1.:
            x_flipped = x.flip(0).mul_(1. - lam)
            x.mul_(lam).add_(x_flipped)
        return x
    x_orig = x.clone()
    B = len(x)
    for i in range(B):
        j = B - i - 1
        if lam[i] != 1.:
            if use_cutmix[i]:
                yl, yh, xl, xh = (int(v) for v in boxes[i])
                x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
            else:
                x[i] = x[i] * float(lam[i]) + x_orig[j] * float(np.float32(1) - lam[i])
    return x


class TimmMixup:
    """timm.data.Mixup restated on torch lines: the tensors are timm's, the draws are taken from this package's ``Mixup._draw`` (a private
    method: host numpy in timm's order) so that both configurations mix the same draw -- this configuration therefore pays this package's
    host cost for the draw, not timm's own."""

    def __init__(self, **kw):
        self.draw = sm.Mixup(**kw)
        self.mixup_enabled = True

    def __call__(self, x, target):
        d = self.draw
        d._draw(tuple(x.shape))
        timm_mix_images(x, d.mode, d.lam, d.use_cutmix, d.boxes)
        lam = d.lam if d.mode == "batch" else torch.tensor(d.lam, device=x.device, dtype=x.dtype).unsqueeze(1)
        return x, timm_mixup_target(target, d.num_classes, lam, d.label_smoothing)


class TimmSoftTargetCrossEntropy(torch.nn.Module):
    def forward(self, x, target):
        loss = torch.sum(-target * torch.nn.functional.log_softmax(x, dim=-1), dim=-1)
        return loss.mean()


# ---- timing ----------------------------------------------------------------------------------------------------------------------
def one_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def interleaved_us(fns, rounds, inner, warm=3):
    """{name: [us per call] per round}: ``inner`` back-to-back calls between two device events, the configurations interleaved."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            res[n].append(one_us(lambda: [fn() for _ in range(inner)]) / inner)
    return res


def fmt(v):
    return f"{statistics.median(v):.1f} | {min(v):.1f} - {max(v):.1f}"


def images_part(lines, rounds):
    lines += ["## (a) smoe_mixup_images against timm's torch lines", "",
              f"In place on f32 images; device events around 10 back-to-back calls (the table of factors and boxes is on the device "
              f"already), {rounds} rounds, the two interleaved; effective rate at 2 * 4 * B*C*H*W bytes from the median.  The batch "
              "fits the 256-MiB Infinity Cache: an effective rate, not an HBM share.", "",
              "| shape | draw | own us (median) | range | effective TB/s | torch us (median) | range | effective TB/s | own / torch |",
              "|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for B, S in ((128, 224), (256, 224), (32, 384)):
        g = torch.Generator(device=DEV).manual_seed(B)
        x = torch.randn(B, 3, S, S, device=DEV, generator=g)
        nbytes = 2 * 4 * x.numel()
        for name, kw, seed in (("mixup, batch mode", dict(mixup_alpha=0.8, cutmix_alpha=0.), 1),
                               ("cutmix, batch mode", dict(mixup_alpha=0., cutmix_alpha=1.0), 2),
                               ("mixup + cutmix, elem mode", dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem"), 3)):
            m = sm.Mixup(num_classes=1000, **kw)
            np.random.seed(seed)
            img_lam, img_om, _, _, boxes = m._draw(tuple(x.shape))
            lam_d, om_d = torch.from_numpy(img_lam).to(DEV), torch.from_numpy(img_om).to(DEV)
            box_d = torch.from_numpy(boxes).to(DEV)
            lam, cut, bx = m.lam, m.use_cutmix, m.boxes
            res = interleaved_us({"own": lambda: ops.mixup_images_(x, lam_d, om_d, box_d),
                                  "torch": lambda: timm_mix_images(x, m.mode, lam, cut, bx)}, rounds, 10 if m.mode == "batch" else 2)
            x.normal_(generator=g)        # (repeated in-place mixing shrinks the values: fresh ones for the next draw)
            mo, mt = statistics.median(res["own"]), statistics.median(res["torch"])
            what = name + (f" (lam {lam:.3f}" + (f", box {bx[0].tolist()})" if cut else ")") if m.mode == "batch"
                           else f" ({int(np.sum(cut & (lam != 1)))} cutmix, {int(np.sum(~cut & (lam != 1)))} mixup samples)")
            lines.append(f"| {B}x3x{S}x{S} | {what} | {fmt(res['own'])} | {nbytes / mo / 1e6:.2f} | {fmt(res['torch'])} | "
                         f"{nbytes / mt / 1e6:.2f} | {mo / mt:.2f} |")
            ok &= mo <= mt
        del x
        torch.cuda.empty_cache()
    lines += ["", f"Own kernel no slower than timm's torch lines at every listed shape and draw: **{'yes' if ok else 'NO'}**.", ""]
    return ok


def _loss_inputs(B, C, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    labels = torch.randint(0, C, (B,), generator=g, device=DEV)
    lam = torch.rand(B, 1, generator=g, device=DEV)
    t = timm_mixup_target(labels, C, lam, 0.1)
    x = (torch.randn(B, C, generator=g, device=DEV) * 4).to(dtype)
    return x, t


def _fwd_bwd(crit, x, t, scale):
    xr = x.detach().requires_grad_(True)
    (crit(xr, t) * scale).backward()
    return xr.grad


def _launches(fn):
    from torch.profiler import profile, ProfilerActivity
    for _attempt in range(3):      # (a pass that already completed outside the profiler; repeated only when the trace came back empty)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, e.count) for e in prof.key_averages() if not e.key.startswith("hip") and "Memcpy" not in e.key and "Memset" not in e.key]
        if rows:
            return rows
    return []


def loss_part(lines, rounds):
    lines += ["## (b) loss forward + backward, own kernels against the torch composition", "",
              "f16 logits, dense f32 targets, loss x 65536 before the backward (the loss scaler's multiply is part of both); device "
              f"events around 20 back-to-back forward + backward passes, {rounds} rounds, the two interleaved; launches = kernel rows of "
              "one pass under torch.profiler.", "",
              "| logits | own us (median) | range | own launches | torch us (median) | range | torch launches | own / torch |",
              "|---|---|---|---|---|---|---|---|"]
    ok = ok_host = True
    own_c, torch_c = sm.SoftTargetCrossEntropy(), TimmSoftTargetCrossEntropy()
    scale = torch.tensor(65536.0, device=DEV)
    detail = []
    for B in (128, 256):
        x, t = _loss_inputs(B, 1000, torch.float16)
        res = interleaved_us({"own": lambda: _fwd_bwd(own_c, x, t, scale), "torch": lambda: _fwd_bwd(torch_c, x, t, scale)}, rounds, 20)
        lo, lt = _launches(lambda: _fwd_bwd(own_c, x, t, scale)), _launches(lambda: _fwd_bwd(torch_c, x, t, scale))
        no, nt = sum(c for _, c in lo), sum(c for _, c in lt)
        mo, mt = statistics.median(res["own"]), statistics.median(res["torch"])
        lines.append(f"| [{B}, 1000] f16 | {fmt(res['own'])} | {no} | {fmt(res['torch'])} | {nt} | {mo / mt:.2f} |")
        ok &= no < nt
        ok_host &= mo <= mt
        detail.append((B, lo, lt))
    lines += ["", f"Own loss fewer launches than the torch composition: **{'yes' if ok else 'NO'}**.  No more time in this loop of eager "
              f"back-to-back passes, where the host's cost per pass (Python, autograd, launches) counts as much as the GPU's: "
              f"**{'yes' if ok_host else 'NO'}**.  GPU time per pass: the kernel traces (`--loss-loop own` / `torch` under "
              "`rocprofv3 --kernel-trace --stats`).", ""]
    for B, lo, lt in detail[:1]:
        lines += [f"Kernels of one forward + backward at [{B}, 1000] (name x count):", "",
                  "- own: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in lo),
                  "- torch: " + "; ".join(f"`{n[:70]}` x {c}" for n, c in lt), ""]
    # accuracy against float64 on f32 logits (what tests/test_gpu_mixup_loss.py bounds by 3 x torch's own error)
    lines += ["Max error against float64 on f32 logits [128, 1000] (logit scale 1 / 4 / 12), per-row loss and dlogits of the mean:", "",
              "| logit scale | row loss: own | row loss: torch f32 | dlogits: own | dlogits: torch f32 |", "|---|---|---|---|---|"]
    for s in (1.0, 4.0, 12.0):
        x, t = _loss_inputs(128, 1000, torch.float32, seed=int(s))
        x = x / 4 * s
        x64 = x.double().requires_grad_(True)
        r64 = (-(t.double()) * torch.log_softmax(x64, -1)).sum(-1)
        r64.mean().backward()
        x32 = x.clone().requires_grad_(True)
        r32 = torch.sum(-t * torch.log_softmax(x32, -1), dim=-1)
        r32.mean().backward()
        loss, rows = ops.soft_ce_fwd(x, t)
        dx = ops.soft_ce_bwd(x, rows, torch.ones((), device=DEV), t)
        lines.append(f"| {s:g} | {(rows[0].double() - r64).abs().max().item():.2e} | {(r32.double() - r64).abs().max().item():.2e} | "
                     f"{(dx.double() - x64.grad).abs().max().item():.2e} | {(x32.grad.double() - x64.grad).abs().max().item():.2e} |")
    lines.append("")
    return ok and ok_host


def loss_loop(which, n=200):
    """The loop alone, for a kernel trace of its own."""
    x, t = _loss_inputs(128, 1000, torch.float16)
    crit = sm.SoftTargetCrossEntropy() if which == "own" else TimmSoftTargetCrossEntropy()
    scale = torch.tensor(65536.0, device=DEV)
    for _ in range(n):
        _fwd_bwd(crit, x, t, scale)
    torch.cuda.synchronize()
    print(f"{which}: {n} forward + backward passes at [128, 1000] f16")


# ---- (c) the harness -------------------------------------------------------------------------------------------------------------
class EventLoader:
    """``n`` times the same (images, labels) batch (a fresh copy of the images: Mixup works in place); records an event on the current
    stream as each batch is handed out and one after the last step."""

    def __init__(self, batch, n):
        self.batch, self.n, self.events = batch, n, []
        self.scratch = batch[0].clone()

    def __iter__(self):
        self.events = []
        for _ in range(self.n):
            self.events.append(torch.cuda.Event(enable_timing=True))
            self.events[-1].record()
            self.scratch.copy_(self.batch[0])
            yield self.scratch, self.batch[1]
        self.events.append(torch.cuda.Event(enable_timing=True))
        self.events[-1].record()


MIX_KW = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=1000)


def step_ms(cfg, batch, w, k):
    torch.manual_seed(0)
    np.random.seed(0)
    model = sm.create_model("resmoe_tiny_patch16_224_expert8").to(DEV)
    opt = sm.AdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    scaler = sm.NativeScaler()
    loader = EventLoader(batch, w + k)
    mix, crit = cfg["make"]()
    st = sm.train_one_epoch(model, crit, loader, opt, DEV, 0, scaler, None, None, mix, hip_graph=cfg["graph"])
    torch.cuda.synchronize()
    return loader.events[w].elapsed_time(loader.events[w + k]) / k, st["hip_graph_steps"]


def harness_part(lines, rounds, k):
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(128, 3, 224, 224, device=DEV, generator=g)
    y = torch.randint(0, 1000, (128,), device=DEV, generator=g)
    w = 8       # 3 eager warm steps, the capture, 4 replays
    makers = [("integer labels + nn.CrossEntropyLoss (today)", lambda: (None, torch.nn.CrossEntropyLoss())),
              ("restated-timm Mixup + torch soft-target loss", lambda: (TimmMixup(**MIX_KW), TimmSoftTargetCrossEntropy())),
              ("own Mixup + own SoftTargetCrossEntropy", lambda: (sm.Mixup(**MIX_KW), sm.SoftTargetCrossEntropy()))]
    cfgs = [dict(name=f"{n}, {'hip_graph=True' if gr else 'eager'}", make=mk, graph=gr) for gr in (False, True) for n, mk in makers]
    res = {c["name"]: [] for c in cfgs}
    graphed = {}
    step_ms(cfgs[3], (x, y), 4, 4)                 # first-use costs (code objects, allocator) outside the table
    for _ in range(rounds):
        for c in cfgs:
            ms, gs = step_ms(c, (x, y), w, k)
            res[c["name"]].append(ms)
            graphed[c["name"]] = gs
    lines += ["## (c) train_one_epoch, resmoe_tiny_patch16_224_expert8, batch 128", "",
              "AdamW + NativeScaler, autocast f16, --mixup 0.8 --cutmix 1.0 --smoothing 0.1 in batch mode (the reference's default); the restated-timm configuration takes its draws from this package's `Mixup._draw` "
              "(same draw, same host cost) and runs timm's torch lines on them.  ms per "
              f"step = device events from the start of step {w} to the end of step {w + k - 1} of an epoch of {w + k} steps, over {k}; "
              f"the loader's copy of the batch into a scratch buffer (Mixup works in place) is inside every configuration; {rounds} rounds, "
              "configurations interleaved.", "",
              "| configuration | ms per step (median) | range | every round | graphed steps in the epoch |", "|---|---|---|---|---|"]
    for c in cfgs:
        v = res[c["name"]]
        lines.append(f"| {c['name']} | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} | "
                     f"{', '.join('%.2f' % t for t in v)} | {graphed[c['name']]} |")
    lines.append("")
    med = {n: statistics.median(v) for n, v in res.items()}
    ok = True
    for mode in ("eager", "hip_graph=True"):
        own, timm, today = (med[f"{n}, {mode}"] for n in (makers[2][0], makers[1][0], makers[0][0]))
        spread = max(max(res[f"{n}, {mode}"]) - min(res[f"{n}, {mode}"]) for n in (makers[2][0], makers[1][0]))
        fine = own <= timm + spread
        ok &= fine
        lines.append(f"- {mode}: own {own:.2f} ms, restated timm {timm:.2f} ms ({own - timm:+.2f} ms; spread of repeated runs {spread:.2f} ms): "
                     f"**{'no slower' if fine else 'SLOWER'}**; distance from today's integer-label step {own - today:+.2f} ms")
    lines.append("")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--loss-loop", choices=["own", "torch"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mixup_bench.py needs the GPU"
    if a.loss_loop:
        return loss_loop(a.loss_loop)
    lines = ["# Mixup / CutMix and the soft-target loss on the GPU (tools/mixup_bench.py)", "",
             f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    if "a" in a.parts:
        images_part(lines, a.rounds)
        print("\n".join(lines), flush=True)
    if "b" in a.parts:
        loss_part(lines, a.rounds)
        print("\n".join(lines), flush=True)
    if "c" in a.parts:
        harness_part(lines, a.rounds, a.steps)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
