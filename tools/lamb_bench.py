#!/usr/bin/env python3
"""LAMB (optim.Lamb, the timm.optim.Lamb surface of the DeiT-III recipes' --opt lamb) on the GPU.

(a) The Lamb step over ViT-B/16 E = 8's parameter set (moe_base_patch16_224_expert8_top1) with f16 gradients: device-event time per
    step and the effective rate at the algorithmic traffic per element -- norm pass 2 B (f16 gradient), stage 1 22 B (gradient 2,
    exp_avg and exp_avg_sq read and written 16, parameter read 4), stage 2 16 B (parameter read and written 8, moments read 8; 18 with
    a 16-bit image) -- against 6.3 TB/s, beside timm's Lamb restated in torch ops (what a user gets today).
(b) resmoe_tiny_patch16_224_expert8 (the reference's model), batch 128, train_one_epoch steady-state ms per step by
    tools/ema_bench.py's method: sm.Lamb eager, sm.Lamb hip_graph=True, the restated timm Lamb through the scaler's stock path, and
    sm.AdamW hip_graph=True (what LAMB's second pass costs).  Arms interleaved in one process, median and range.
(c) The errors behind the bars of tests/test_gpu_lamb.py: the case set of tests/_lamb_cases.py through the kernels and through the same
    rule in f32 torch ops on the CPU, both against the float64 restatement.
usage: lamb_bench.py [--out FILE.md] [--rounds N] [--steps K] [--skip-harness]"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slim_switch_moe_vit_amd as sm  # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_TBS = 6.3


class TimmLamb(torch.optim.Optimizer):
    """timm.optim.Lamb (0.4.12 / 0.5), restated in its own torch ops: timm is not a dependency of this package."""

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True,
                 max_grad_norm=1.0, trust_clip=False, always_adapt=False):
        super().__init__(params, dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay,
                                      grad_averaging=grad_averaging, max_grad_norm=max_grad_norm, trust_clip=trust_clip,
                                      always_adapt=always_adapt))

    @torch.no_grad()
    def step(self, closure=None):
        device = self.param_groups[0]["params"][0].device
        one = torch.tensor(1.0, device=device)
        norm = torch.zeros(1, device=device)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    norm.add_(p.grad.float().pow(2).sum())
        norm = torch.sqrt(norm)
        mgn = self.defaults["max_grad_norm"]
        clip = one if mgn is None else torch.where(norm > mgn, norm / mgn, one)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            beta3 = 1 - b1 if group["grad_averaging"] else 1.0
            group["step"] = group.get("step", 0) + 1
            bc1, bc2 = (1 - b1 ** group["step"], 1 - b2 ** group["step"]) if group["bias_correction"] else (1.0, 1.0)
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad.float().div_(clip)
                st = self.state[p]
                if not st:
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.mul_(b1).add_(grad, alpha=beta3)
                v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
                update = (m / bc1).div_((v.sqrt() / math.sqrt(bc2)).add_(group["eps"]))
                wd = group["weight_decay"]
                if wd != 0:
                    update.add_(p, alpha=wd)
                if wd != 0 or group["always_adapt"]:
                    w_norm, g_norm = p.norm(2.0), update.norm(2.0)
                    trust = torch.where(w_norm > 0, torch.where(g_norm > 0, w_norm / g_norm, one), one)
                    if group["trust_clip"]:
                        trust = torch.minimum(trust, one)
                    update.mul_(trust)
                p.add_(update, alpha=-group["lr"])


def events_ms(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _groups(params, wd=0.05):
    """timm's split: no weight decay on biases and norm weights."""
    return [dict(params=[p for p in params if p.ndim > 1], weight_decay=wd), dict(params=[p for p in params if p.ndim <= 1], weight_decay=0.0)]


def kernel_part(lines):
    cpu = sm.create_model("moe_base_patch16_224_expert8_top1")
    shapes = [p.shape for p in cpu.parameters()]
    del cpu
    g = torch.Generator(device=DEV).manual_seed(0)

    def params_with_grads(gdt):
        ps = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=g) * 0.02) for s in shapes]
        for p in ps:
            if gdt != torch.float32:
                p.grad_dtype = gdt
            p.grad = (torch.randn(p.shape, device=DEV, generator=g) * 1e-2).to(gdt)
        return ps

    ps = params_with_grads(torch.float16)
    n = sum(p.numel() for p in ps)
    adapt = sum(p.numel() for p in ps if p.ndim > 1)
    opt = sm.Lamb(_groups(ps), lr=1e-3)
    ms = events_ms(opt.step, 20)
    # stage 1 reads the parameter only where the tensor adapts (weight decay on): 22 B there, 18 B elsewhere
    moved = 2.0 * n + (22.0 * adapt + 18.0 * (n - adapt)) + 16.0 * n
    rate = moved / (ms * 1e-3) / 1e12
    del opt, ps
    torch.cuda.empty_cache()
    ps = params_with_grads(torch.float32)      # (the stock path hands a foreign optimizer unscaled f32 gradients)
    topt = TimmLamb(_groups(ps), lr=1e-3)
    ms_t = events_ms(topt.step, 5, warm=2)
    del topt, ps
    torch.cuda.empty_cache()
    lines += ["## (a) The Lamb step on ViT-B/16 E = 8's parameter set", "",
              f"{len(shapes)} f32 parameter tensors, {n / 1e6:.1f} M values ({adapt / 1e6:.1f} M with weight decay 0.05, the rest 0: "
              f"timm's split), f16 gradients; {moved / 1e9:.2f} GB of algorithmic traffic per step (norm pass 2 B, stage 1 22 B, "
              "stage 2 16 B per element; no 16-bit images here).  Device events around 20 back-to-back steps after 3 warm-up steps; "
              "the step is the norm pass, smoe_lamb_clip, smoe_step_advance, stage 1, trust, stage 2 per batch.", "",
              f"| step | ms per step | effective TB/s | of {PEAK_TBS} TB/s |", "|---|---|---|---|",
              f"| sm.Lamb (HIP kernels) | {ms:.3f} | {rate:.2f} | {100 * rate / PEAK_TBS:.0f} % |",
              f"| timm's Lamb restated in torch ops, f32 gradients (5 steps after 2) | {ms_t:.3f} | "
              f"{moved / (ms_t * 1e-3) / 1e12:.2f} (same byte count) | |", ""]
    return ms, ms_t


class EventLoader:
    """``n`` times the same (images, labels) batch; records an event on the current stream as each batch is handed out (= after
    everything the previous step enqueued) and one after the last step (tools/ema_bench.py)."""

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


def step_ms(cfg, batch, w, k):
    """ms per step over steps w .. w + k - 1 of one epoch of w + k steps."""
    torch.manual_seed(0)
    model = sm.create_model("resmoe_tiny_patch16_224_expert8").to(DEV)
    opt = cfg["opt"](_groups(list(model.parameters())), lr=5e-4)
    scaler = sm.NativeScaler()
    loader = EventLoader(batch, w + k)
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), loader, opt, DEV, 0, scaler, None, hip_graph=cfg["graph"])
    torch.cuda.synchronize()
    return loader.events[w].elapsed_time(loader.events[w + k]) / k, st["hip_graph_steps"]


def harness_part(lines, rounds, k):
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(128, 3, 224, 224, device=DEV, generator=g)
    y = torch.randint(0, 1000, (128,), device=DEV, generator=g)
    w = 8       # 3 eager warm steps, the capture, 4 replays
    cfgs = [dict(name="sm.Lamb, eager", opt=sm.Lamb, graph=False),
            dict(name="sm.Lamb, hip_graph=True", opt=sm.Lamb, graph=True),
            dict(name="timm's Lamb restated, stock scaler path (today)", opt=TimmLamb, graph=False),
            dict(name="sm.AdamW, hip_graph=True (one pass less)", opt=sm.AdamW, graph=True)]
    res = {c["name"]: [] for c in cfgs}
    graphed = {}
    step_ms(cfgs[1], (x, y), 4, 4)                 # first-use costs (code objects, allocator) outside the table
    for _ in range(rounds):
        for c in cfgs:
            ms, gs = step_ms(c, (x, y), w, k)
            res[c["name"]].append(ms)
            graphed[c["name"]] = gs
    lines += ["## (b) train_one_epoch, resmoe_tiny_patch16_224_expert8, batch 128", "",
              f"NativeScaler, autocast f16, lr 5e-4, weight decay 0.05 on the matrices.  ms per step = device events from the start of "
              f"step {w} to the end of step {w + k - 1} of an epoch of {w + k} steps, over {k}; {rounds} rounds, arms interleaved.", "",
              "| arm | ms per step (median) | range | every round | graphed steps in the epoch |", "|---|---|---|---|---|"]
    for c in cfgs:
        v = res[c["name"]]
        lines.append(f"| {c['name']} | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} | "
                     f"{', '.join('%.2f' % t for t in v)} | {graphed[c['name']]} |")
    lines.append("")
    names = [c["name"] for c in cfgs]
    med = {n_: statistics.median(v) for n_, v in res.items()}
    for a, b in ((names[1], names[2]), (names[0], names[2]), (names[1], names[0]), (names[1], names[3])):
        gap = med[a] - med[b]
        spread = max(max(res[a]) - min(res[a]), max(res[b]) - min(res[b]))      # the wider range of the two arms compared
        verdict = "inside the measured spread: no difference shown" if abs(gap) <= spread else (
            "faster, by more than the spread" if gap < 0 else "slower, by more than the spread")
        lines.append(f"- {a} minus {b}: {gap:+.2f} ms (wider range of the two arms {spread:.2f} ms): {verdict}")
    lines.append("")


def error_part(lines):
    import _lamb_cases as cases
    lines += ["## (c) Errors behind the bars of tests/test_gpu_lamb.py", "",
              f"The case set of tests/_lamb_cases.py ({len(cases.SHAPES)} tensors in 2 groups, {cases.STEPS} steps), against the float64 "
              "restatement, relative to max(1, max |reference|); trust ratios, G and clip relative to themselves.  `f32 CPU` = the same "
              "rule in f32 torch ops on the CPU, the floor the kernels are judged against.", "",
              "| setting (max_grad_norm, gradient scale, trust_clip, always_adapt) | gradients | parameters | exp_avg | exp_avg_sq | "
              "trust ratios | G | clip | parameters, f32 CPU | trust ratios, f32 CPU |", "|---|---|---|---|---|---|---|---|---|---|"]
    for s, (mgn, gscale, trust_clip, always_adapt) in enumerate(cases.SETTINGS):
        for gdt in (torch.float32, torch.float16, torch.bfloat16):
            vdt = torch.float16 if gdt == torch.float32 else gdt
            ref = cases.reference(s, vdt)
            f32 = cases.lamb_steps(cases.initial_weights(), cases.gradients(gscale, vdt), cases.GROUP_OF, cases.HYPER, max_grad_norm=mgn,
                                   trust_clip=trust_clip, always_adapt=always_adapt, dtype=torch.float32)
            ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in cases.initial_weights()]
            opt = cases.make_optimizer(sm.Lamb, ps, s)
            for grads in cases.gradients(gscale, vdt):
                for p, gr in zip(ps, grads):
                    if gdt != torch.float32:
                        p.grad_dtype = gdt
                    p.grad = gr.to(gdt).to(DEV)
                opt.step()
            tr = opt.trust_ratios()
            rel = lambda got: max(abs(a - b) / b for a, b in zip(got, ref["trust"][-1]))
            clip, G = opt.last_grad_norm.tolist()
            lines.append(f"| {mgn}, {gscale:g}, {trust_clip}, {always_adapt} | {str(gdt).replace('torch.', '')} | "
                         f"{cases.rel_err(ps, ref['params']):.2e} | {cases.rel_err([opt.state[p]['exp_avg'] for p in ps], ref['exp_avg']):.2e} | "
                         f"{cases.rel_err([opt.state[p]['exp_avg_sq'] for p in ps], ref['exp_avg_sq']):.2e} | {rel([tr[p] for p in ps]):.2e} | "
                         f"{abs(G - ref['G'][-1]) / ref['G'][-1]:.1e} | {abs(clip - ref['clip'][-1]) / ref['clip'][-1]:.1e} | "
                         f"{cases.rel_err(f32['params'], ref['params']):.2e} | {rel(f32['trust'][-1]):.2e} |")
    lo = min(min(t) for s in range(len(cases.SETTINGS)) for t in cases.reference(s)["trust"])
    hi = max(max(t) for s in range(len(cases.SETTINGS)) for t in cases.reference(s)["trust"])
    lines += ["", f"Trust ratios of the reference run from {lo:.4g} to {hi:.4g}.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--skip-harness", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lamb_bench.py needs the GPU"
    lines = ["# LAMB on the GPU (tools/lamb_bench.py)", "", f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}", ""]
    kernel_part(lines)
    print("\n".join(lines), flush=True)
    if not a.skip_harness:
        harness_part(lines, a.rounds, a.steps)
        print("\n".join(lines[-12:]), flush=True)
    error_part(lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
