"""Fixture from the reference's OWN module: ``SwitchableLayerNorm`` (models/layers.py) run on small stored inputs.

The reference file needs only torch, so it is imported from its path at run time; nothing of it is copied here and only arrays are
stored.  Cases (rows drawn as ``centroids[a] + 0.5 * noise``: the two nearest centroids of every row are far apart relative to any
rounding, so the reference's f32 ``cdist`` and float64 agree on every row):

    sw_192x4      d = 192, K = 4, x [3, 37, 192], buckets selected by the module
    int_192x4     the same rows, ``buckets = 2``
    tensor_192x4  the same rows, a stored bucket tensor [3, 37]
    sw_768x8      d = 768, K = 8, x [2, 50, 768], buckets selected

Per case: the inputs (x, dy, the weights / biases / centroids tables, the given buckets if any), the reference's y and buckets, and
its x.grad / weights.grad / biases.grad for the stored dy.  Three files, each below the size limit for committed fixtures: the d = 192
cases in ``ref_switch_ln_tiny.npz``; the d = 768 case in ``ref_switch_ln_tiny_d768.npz`` with its two [2, 50, 768] gradient-side
arrays (dy, x.grad) apart in ``ref_switch_ln_tiny_d768_g.npz``.

    python tests/golden/switch/make_golden_switch_ln.py          # -> tests/golden/switch/ref_switch_ln_tiny*.npz
"""
import importlib.util
import os

import numpy as np
import torch

REF_LAYERS = os.path.join(os.environ.get("SLIMMOE_REFERENCE", "/root/reference"), "models", "layers.py")
OUT_DIR = os.environ.get("SLIMMOE_GOLDEN_OUT", os.path.dirname(os.path.abspath(__file__)))

# name, d, K, leading shape, buckets mode, output file tag
CASES = [("sw_192x4", 192, 4, (3, 37), "select", ""), ("int_192x4", 192, 4, (3, 37), "int", ""),
         ("tensor_192x4", 192, 4, (3, 37), "tensor", ""), ("sw_768x8", 768, 8, (2, 50), "select", "_d768")]
INT_BUCKET = 2
FILES = {"": "ref_switch_ln_tiny.npz", "_d768": "ref_switch_ln_tiny_d768.npz", "_d768_g": "ref_switch_ln_tiny_d768_g.npz"}
SPLIT_OFF = ("dy", "dx")          # of the d = 768 case: the arrays that go to the "_g" file


def inputs(d, K, lead, seed):
    g = torch.Generator().manual_seed(seed)
    centroids = torch.randn(K, d, generator=g)
    assign = torch.randint(0, K, lead, generator=g)
    x = centroids[assign] + 0.5 * torch.randn(*lead, d, generator=g)
    weights = 1.0 + 0.25 * torch.randn(K, d, generator=g)
    biases = 0.25 * torch.randn(K, d, generator=g)
    dy = torch.randn(*lead, d, generator=g)
    given = torch.randint(0, K, lead, generator=g)
    return x, dy, weights, biases, centroids, given


def run(ref_cls, x, dy, weights, biases, centroids, buckets):
    K, d = weights.shape
    m = ref_cls(d, switchable_buckets=K)
    with torch.no_grad():
        m.weights.copy_(weights)
        m.biases.copy_(biases)
    m.set_centroids(torch.nn.Parameter(centroids.clone(), requires_grad=False))
    xin = x.clone().requires_grad_(True)
    y, b = m(xin, buckets)
    y.backward(dy)
    return (y.detach().numpy(), b.broadcast_to(x.shape[:-1]).contiguous().numpy().astype(np.int64), xin.grad.numpy(),
            m.weights.grad.numpy(), m.biases.grad.numpy())


def main():
    spec = importlib.util.spec_from_file_location("ref_layers", REF_LAYERS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(1)                  # one summation order whatever the machine
    out = {tag: {} for tag in FILES}
    made = {}
    for name, d, K, lead, mode, tag in CASES:
        key = (d, K, lead)
        if key not in made:
            made[key] = inputs(d, K, lead, 1000 + d + K)
        x, dy, weights, biases, centroids, given = made[key]
        buckets = None if mode == "select" else (INT_BUCKET if mode == "int" else given)
        y, b, dx, dw, db = run(mod.SwitchableLayerNorm, x, dy, weights, biases, centroids, buckets)
        arrays = {"x": x.numpy(), "dy": dy.numpy(), "weights": weights.numpy(), "biases": biases.numpy(),
                  "centroids": centroids.numpy(), "y": y, "buckets": b, "dx": dx, "dweights": dw, "dbiases": db}
        if mode == "tensor":
            arrays["given"] = given.numpy().astype(np.int64)
        if mode != "select":                  # the d = 192 cases share their inputs: stored once, under the first case's name
            for k in ("x", "dy", "weights", "biases", "centroids"):
                del arrays[k]
        for k, v in arrays.items():
            out[tag + "_g" if (tag and k in SPLIT_OFF) else tag][f"{name}/{k}"] = v
    for tag, fname in FILES.items():
        path = os.path.join(OUT_DIR, fname)
        np.savez(path, **out[tag])
        print(path, len(out[tag]), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
