#!/usr/bin/env python3
"""One sha256 per tensor a MoE forward leaves -- output, every tensor of ``last_plan``, the gate's ``last_routing`` / ``last_noise``, its
loss, and in training the gradients of x, the gate parameters and the four expert tensors -- for every gate at every routing site,
over seeded inputs (``torch.manual_seed`` per case, so device-side draws repeat).  Run it in a fresh process in two trees that share
one build of the library (SLIMMOE_LIB selects it) and compare the two files line by line: equal lines = equal bits.
Gates: naive k = 1 / 2, switch (train / eval mode, with noise + capacity and without), gshard (random routing x capacity), noisy
(k = 1 / 2, eval / training mode); d = 192, h = 384, E = 8 (E = 4 for one row of each gate), T = 129 and 394, f16 compute.
Sites: mod(x), forward_add, forward_norm_add, forward_norm_add_steps with tail= / next_norm=, forward_norm_gate_add (naive), each on a
single rank and with force_ep on a one-rank NCCL group (counted and static exchange); moe_forward_train plain / residual / zero_rows
and force_ep counted / static.
usage: route_digest.py [--out FILE]"""
import argparse
import contextlib
import hashlib
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ep  # noqa: E402
from slim_switch_moe_vit_amd.autograd import moe_forward_train  # noqa: E402

DEV = torch.device("cuda", 0)
D, H = 192, 384
LINES = []

# (name, gate, k, training mode, attributes set on the gate)
GATES = [
    ("naive_k1", "naive", 1, False, {}), ("naive_k2", "naive", 2, False, {}),
    ("switch_train_eps_cap", "switch", 1, True, {}), ("switch_eval_eps_cap", "switch", 1, False, {}),
    ("switch_train_plain", "switch", 1, True, {"switch_eps": 0.0, "capacity_factor": None}),
    ("switch_eval_plain", "switch", 1, False, {"switch_eps": 0.0, "capacity_factor": None}),
    ("gshard_rr_cap", "gshard", 2, False, {}), ("gshard_rr_nocap", "gshard", 2, False, {"capacity_factor": None}),
    ("gshard_norr_cap", "gshard", 2, False, {"random_routing": False}),
    ("gshard_norr_nocap", "gshard", 2, False, {"random_routing": False, "capacity_factor": None}),
    ("noisy_k1_eval", "noisy", 1, False, {}), ("noisy_k2_eval", "noisy", 2, False, {}),
    ("noisy_k1_train", "noisy", 1, True, {}), ("noisy_k2_train", "noisy", 2, True, {}),
]
SMALL_E = ("naive_k1", "switch_train_eps_cap", "gshard_rr_cap", "noisy_k2_train")      # the E = 4 rows


def emit(case, name, t):
    if t is None or not torch.is_tensor(t):
        LINES.append(f"{case} {name} {t}")
        return
    raw = t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()
    LINES.append(f"{case} {name} {hashlib.sha256(raw).hexdigest()}")


def emit_state(case, mod, out, pos_rows=None):
    for i, o in enumerate(out if isinstance(out, tuple) else (out,)):
        emit(case, f"out{i}", o)
    for i, t in enumerate(mod.last_plan):
        # (a plan over a row subset fills the first entries of pos alone: the rest is never written)
        emit(case, f"plan{i}", t[:pos_rows] if i == 4 and pos_rows is not None and t is not None else t)
    for attr in ("last_routing", "last_noise"):
        for i, t in enumerate(getattr(mod.gate, attr, None) or ()):
            emit(case, f"{attr}{i}", t)
    emit(case, "loss", mod.gate.get_loss(clear=False))


def module(gate, k, E, training, attrs):
    torch.manual_seed(1)
    mod = sm.FMoETransformerMLP(E, D, H, top_k=k, gate=gate)
    with torch.no_grad():
        for p in mod.experts.parameters():
            p.copy_(torch.randn_like(p) * 0.05)
        for p in mod.gate.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    for a, v in attrs.items():
        setattr(mod.gate, a, v)
    mod = mod.to(DEV)
    return mod.train() if training else mod.eval()


def exchange(mod, mode):
    """single rank / counted exchange / static exchange (slots that hold every row for a gate without a capacity)"""
    mod.force_ep = mode != "single"
    mod.ep_speculative = float(mod.gate.tot_expert) if mode == "static" else None
    mod.ep_speculative_train = mode == "static"
    return ep.dynamic_only() if mode == "counted" else contextlib.nullcontext()


def nograd_sites(tag, mod, x, ln, ln2, skip_gate):
    T, k = x.shape[0], mod.top_k
    sites = {
        "call": lambda: mod(x),
        "forward_add": lambda: mod.forward_add(x, x),
        "forward_norm_add": lambda: mod.forward_norm_add(x, ln),
        "steps_tail": lambda: ep.drain(mod.forward_norm_add_steps(x.clone(), ln, tail=(197, 1))),
        "steps_next_norm": lambda: ep.drain(mod.forward_norm_add_steps(x, ln, next_norm=ln2)),
    }
    with torch.no_grad():
        gated = type(mod.gate) is sm.NaiveGate and mod.norm_gate_fusable(x, ln)
    emit(tag, "norm_gate_fusable", gated)
    if gated:
        sites["forward_norm_gate_add"] = lambda: mod.forward_norm_gate_add(x.clone().reshape(1, T, D), ln, skip_gate)
    for mode in ("single", "counted", "static"):
        for name, fn in sites.items():
            if name == "forward_norm_gate_add" and mode == "static":
                continue
            case = f"{tag} {mode} {name}"
            torch.manual_seed(7)
            with exchange(mod, mode), torch.no_grad():
                out = fn()
            sub = name == "steps_tail" and mode == "single" and T % 197 == 0 and mod.gate.capacity(T) < 0
            emit_state(case, mod, out, (T // 197) * k if sub else None)
            ep.check_static_overflow(flush=True)


def train_sites(tag, mod, x):
    T = x.shape[0]
    zero_rows = torch.arange(T, device=DEV) % 3 == 0
    xz = x * (~zero_rows).reshape(T, 1)
    sites = [("single", "plain", x, {}), ("single", "residual", x, {"residual": x}),
             ("single", "zero_rows", xz, {"residual": xz, "zero_rows": zero_rows}),
             ("counted", "plain", x, {}), ("static", "plain", x, {})]
    ex = mod.experts
    params = {**{"gate." + n: p for n, p in mod.gate.named_parameters()}, "htoh4.weight": ex.htoh4.weight, "htoh4.bias": ex.htoh4.bias,
              "h4toh.weight": ex.h4toh.weight, "h4toh.bias": ex.h4toh.bias}
    for mode, name, inp, kw in sites:
        case = f"{tag} train {mode} {name}"
        mod.zero_grad(set_to_none=True)
        xg = inp.clone().requires_grad_(True)
        if "residual" in kw:
            kw = dict(kw, residual=kw["residual"].clone())
        torch.manual_seed(7)
        with exchange(mod, mode):
            out = moe_forward_train(mod, xg, **kw)
            emit_state(case, mod, out)
            loss = mod.gate.get_loss(clear=False)
            obj = out.float().square().mean()
            (obj + 0.1 * loss if loss is not None else obj).backward()
        emit(case, "grad_x", xg.grad)
        for n, p in params.items():
            emit(case, "grad_" + n, p.grad)
        ep.check_static_overflow(flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "route_digest.py needs the GPU"
    import torch.distributed as dist
    torch.cuda.set_device(0)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=DEV)
    try:
        torch.manual_seed(3)
        ln, ln2 = torch.nn.LayerNorm(D, eps=1e-6).to(DEV), torch.nn.LayerNorm(D, eps=1e-6).to(DEV)
        with torch.no_grad():
            for m in (ln, ln2):
                m.weight.copy_(1 + 0.1 * torch.randn(D))
                m.bias.copy_(0.1 * torch.randn(D))
        skip_gate = sm.Gate(D, 1.0, target_threshold=0.55).to(DEV).eval()
        for name, gate, k, training, attrs in GATES:
            for E, T in ((8, 129), (8, 394)) + (((4, 129),) if name in SMALL_E else ()):
                x = torch.randn(T, D, generator=torch.Generator().manual_seed(100 + T)).to(DEV)
                tag = f"{name} E{E} T{T}"
                nograd_sites(tag, module(gate, k, E, training, attrs), x, ln, ln2, skip_gate)
                train_sites(tag, module(gate, k, E, training, attrs), x)
                torch.cuda.synchronize()
                print(f"# {tag}: {len(LINES)} lines so far", file=sys.stderr, flush=True)
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    print(f"# {len(LINES)} lines, library {sm._lib.binary_build_id()}", file=sys.stderr)
    text = "\n".join(LINES)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
