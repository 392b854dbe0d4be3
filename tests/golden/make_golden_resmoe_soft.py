"""Fixture from the reference's OWN ``forward_residule_moe`` (models/resMoE.py:126-145) with both ``Gate``s built ``is_hard=False``,
in train mode: the soft relaxation ``skip_tk = 1 - p``, ``tk = p`` (resMoE.py:72-74).  Run HERE (build container), never on the GPU box:

    python tests/golden/make_golden_resmoe_soft.py

The reference's definitions are loaded the way ``make_golden_resmoe.py`` loads them (its ``load_reference_defs`` / ``load_ref_layers``
are imported, nothing of the reference's text is copied).  Block parameters, ``x`` and ``dy`` are those of ``ref_resblock_tiny.npz``,
read from the committed file, so the two fixtures describe the same block.

Written (data only), for the soft training step: ``train_y``, ``train_dx``, every parameter gradient (``g.*``), both masks
``(1 - p, p)`` and both gates' token counters (the reference's ``_skipped_tokens`` is the fractional sum of ``1 - p``).  The inputs
are NOT repeated (read ``p.*``, ``x``, ``dy``, ``num_heads`` from ``ref_resblock_tiny.npz``), and the two large gradients have
files of their own, so that every file stays below 1 MiB:
  soft/ref_resblock_soft_tiny.npz         everything but ...
  soft/ref_resblock_soft_tiny_g_fc1.npz   g.mlp.fc1.weight
  soft/ref_resblock_soft_tiny_g_fc2.npz   g.mlp.fc2.weight
``load()`` below puts the three back together.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_resmoe as base  # noqa: E402

# (a directory of its own: tests/test_oracle.py requires the .npz files directly under tests/golden/ to be exactly what the two older
# scripts write)
OUT = os.environ.get("SLIMMOE_GOLDEN_OUT", os.path.join(HERE, "soft"))


SPLIT = {"_g_fc1": "g.mlp.fc1.weight", "_g_fc2": "g.mlp.fc2.weight"}


def load(directory=None):
    """The fixture's arrays as one dict, from its three files."""
    directory = directory or os.path.join(HERE, "soft")
    out = {}
    for suffix in ("",) + tuple(SPLIT):
        with np.load(os.path.join(directory, f"ref_resblock_soft_tiny{suffix}.npz")) as f:
            out.update({k: f[k] for k in f.files})
    return out


def resblock_soft_fixture(ref, layers, out):
    Gate, fwd = ref["Gate"], ref["forward_residule_moe"]
    hard = np.load(os.path.join(HERE, "ref_resblock_tiny.npz"))
    heads = int(hard["num_heads"])
    x = torch.from_numpy(hard["x"])
    dy = torch.from_numpy(hard["dy"])
    d = x.shape[-1]

    class Holder(torch.nn.Module):
        """What the reference's factory leaves on a Block (models/resMoE.py:163-186), with the gates' ``is_hard`` set to False."""

        def __init__(self):
            super().__init__()
            self.norm1 = torch.nn.LayerNorm(d, eps=1e-6)
            self.attn = layers.Attention(d, num_heads=heads, qkv_bias=True)
            self.drop_path = torch.nn.Identity()
            self.norm2 = torch.nn.LayerNorm(d, eps=1e-6)
            self.mlp = layers.Mlp(d, 4 * d)
            self.dense_gate = Gate(d, 1.0, target_threshold=0.55, starting_threshold=0.6, is_hard=False)
            self.moe_gate = Gate(d, 1.0, target_threshold=0.55, starting_threshold=0.6, is_hard=False)

    blk = Holder()
    blk.load_state_dict({k[2:]: torch.from_numpy(hard[k]) for k in hard.files if k.startswith("p.")})
    blk.forward = fwd.__get__(blk, Holder)            # the reference's own bind idiom (models/resMoE.py:185-186)
    masks = {}
    hooks = [blk.dense_gate.register_forward_hook(lambda m, i, o: masks.__setitem__("dense", o.detach().clone())),
             blk.moe_gate.register_forward_hook(lambda m, i, o: masks.__setitem__("moe", o.detach().clone()))]
    blk.train()
    xg = x.clone().requires_grad_(True)
    y = blk.forward(xg)
    y.backward(dy)
    for h in hooks:
        h.remove()
    out.update(train_y=y.detach().numpy(), train_dx=xg.grad.numpy(), train_dense_mask=masks["dense"].numpy(),
               train_moe_mask=masks["moe"].numpy())
    out.update({"g." + k: p.grad.numpy() for k, p in blk.named_parameters()})
    for name, gate in (("dense", blk.dense_gate), ("moe", blk.moe_gate)):
        out[f"train_{name}_total"] = np.int64(gate._total_tokens)
        out[f"train_{name}_skipped"] = np.float64(gate._skipped_tokens)
    print("soft resblock: mean 1 - p", float(out["train_dense_mask"][..., 0].mean()), float(out["train_moe_mask"][..., 0].mean()),
          "| counters", float(out["train_dense_skipped"]), float(out["train_moe_skipped"]))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    ref = base.load_reference_defs()
    layers = base.load_ref_layers()
    blk = {}
    resblock_soft_fixture(ref, layers, blk)
    os.makedirs(OUT, exist_ok=True)
    for suffix, key in SPLIT.items():
        np.savez_compressed(os.path.join(OUT, f"ref_resblock_soft_tiny{suffix}.npz"), **{key: blk.pop(key)})
    np.savez_compressed(os.path.join(OUT, "ref_resblock_soft_tiny.npz"), **blk)
    print("wrote ref_resblock_soft_tiny.npz and", ", ".join(f"ref_resblock_soft_tiny{s}.npz" for s in SPLIT))


if __name__ == "__main__":
    sys.exit(main())
