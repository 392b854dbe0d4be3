"""Case table, generators and the float64 restatement shared by tests/test_switch_ln_host.py and tests/test_gpu_switch_ln.py.

The restatement is the rule of SwitchableLayerNorm (models/layers.py:105-151) written out in float64 with explicit gradient formulas
(no autograd): the reference every other implementation -- the fixture's f32 numbers, the module's torch composition, the kernels --
is measured against.  The bar of a comparison is ``3 * max(e_ref, ulp)``: ``e_ref`` the error of an f32 evaluation that is accepted
as correct (the reference's own for the fixture, the CPU composition's for a table cell) against float64, ``ulp`` one f32 ulp of the
float64 result's largest magnitude -- nothing is derived from what the code under test returns.
"""
import os

import numpy as np
import torch

EPS = 1e-5
# T: the block edges of a wave (63 / 64 / 65), several workgroups (257), one value each side of the 4 rows a workgroup of the
# forward / dx kernels takes per round (3, 5) and of the 16 rows a slab of the column pass holds at least (15, 17)
TS = (1, 3, 5, 15, 17, 63, 64, 65, 257)
DS = (192, 384, 768, 1024)
KS = (1, 2, 5, 8, 32)
REGIMES = ("separated", "one_bucket", "near_tie", "offset", "given_int", "given_tensor")
SEPARATED_MARGIN = 1e-3
TIE_WINDOW = (1e-7, 1e-5)
# beside the grid: K = 9 .. 16 (the 16-slot instantiation of the forward's argmin), below and above the table size from which the
# forward runs one 16-wave workgroup per CU (K d > 12288)
EXTRA_CELLS = (("separated", 257, 384, 9), ("near_tie", 63, 768, 12), ("near_tie", 17, 1024, 13), ("separated", 65, 1024, 16),
               ("given_tensor", 5, 1024, 16))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "switch")
FIXTURE_FILES = ("ref_switch_ln_tiny.npz", "ref_switch_ln_tiny_d768.npz", "ref_switch_ln_tiny_d768_g.npz")
# (case, the case that stores its inputs, buckets argument: None / an int / "given" = the stored tensor)
FIXTURE_CASES = [("sw_192x4", "sw_192x4", None), ("int_192x4", "sw_192x4", 2), ("tensor_192x4", "sw_192x4", "given"),
                 ("sw_768x8", "sw_768x8", None)]


def load_fixture():
    out = {}
    for f in FIXTURE_FILES:
        z = np.load(os.path.join(GOLDEN, f))
        out.update({k: z[k] for k in z.files})
    return out


def fixture_case(fx, name, src, mode):
    """(inputs as torch tensors, buckets argument, the reference's results) of one fixture case."""
    t = {k: torch.from_numpy(fx[f"{src}/{k}"]) for k in ("x", "dy", "weights", "biases", "centroids")}
    buckets = torch.from_numpy(fx[f"{name}/given"]) if mode == "given" else mode
    ref = {k: torch.from_numpy(fx[f"{name}/{k}"]) for k in ("y", "buckets", "dx", "dweights", "dbiases")}
    return t, buckets, ref


def cells():
    """(regime, T, d, K): every regime meets every (d, K) pair of the grid; the T values rotate so that each meets every regime and every d;
    then EXTRA_CELLS."""
    out = []
    for r, regime in enumerate(REGIMES):
        i = 0
        for di, d in enumerate(DS):
            for ki, K in enumerate(KS):
                if regime == "near_tie" and K == 1:
                    i += 1
                    continue                      # one centroid has no bisector (K = 1 selects bucket 0: covered by "separated")
                T = TS[(i + 2 * r + di) % len(TS)]
                out.append((regime, T, d, K))
                i += 1
    return out + list(EXTRA_CELLS)


def cell_id(c):
    return "%s-T%d-d%d-K%d" % c


def dist64(x, cent):
    """[T, K] float64 squared distances in the direct form."""
    x, cent = x.double(), cent.double()
    return torch.stack([(x - cent[k]).square().sum(-1) for k in range(cent.shape[0])], dim=-1)


def margins(x, cent):
    """Relative gap between the two smallest float64 squared distances of every row ([T]; inf for K = 1)."""
    dd = dist64(x, cent)
    if dd.shape[1] == 1:
        return torch.full((dd.shape[0],), float("inf"), dtype=torch.float64)
    two = dd.topk(2, dim=1, largest=False).values
    return (two[:, 1] - two[:, 0]) / two[:, 0]


def select64(x, cent, reverse=False):
    """torch.argmin's rule on the float64 direct form; ``reverse``: the sums taken over the columns in reversed order."""
    if reverse:
        x, cent = x.flip(-1), cent.flip(-1)
    return dist64(x, cent).argmin(dim=1)


def select32_expanded(x, cent):
    """Upstream's arithmetic for comparison: |x|^2 + |c|^2 - 2 x.c in f32."""
    x, cent = x.float(), cent.float()
    dd = x.square().sum(-1, keepdim=True) + cent.square().sum(-1)[None] - 2.0 * (x @ cent.t())
    return dd.argmin(dim=1)


def restate64(x, dy, weights, biases, cent, buckets=None, eps=EPS):
    """The rule and its gradients in float64.  x [T, d]; buckets None / int / int64 [T].  -> dict y, b, dx, dw, db (float64)."""
    x64 = x.double()
    T, d = x64.shape
    K = weights.shape[0] if weights is not None else cent.shape[0]
    if buckets is None:
        b = select64(x, cent) if K > 1 else torch.zeros(T, dtype=torch.int64)
    elif isinstance(buckets, torch.Tensor):
        b = buckets.to(torch.int64).reshape(T)
    else:
        b = torch.full((T,), int(buckets), dtype=torch.int64)
    mean = x64.mean(-1, keepdim=True)
    var = (x64 - mean).square().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x64 - mean) * rstd
    out = {"b": b}
    w = weights.double()[b] if weights is not None else torch.ones_like(x64)
    out["y"] = xhat * w + (biases.double()[b] if biases is not None else 0.0)
    if dy is not None:
        dy64 = dy.double()
        g = dy64 * w
        out["dx"] = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
        dw = torch.zeros(K, d, dtype=torch.float64)
        db = torch.zeros(K, d, dtype=torch.float64)
        dw.index_add_(0, b, dy64 * xhat)
        db.index_add_(0, b, dy64)
        out["dw"], out["db"] = dw, db
    return out


def ulp32(ref64):
    """One f32 ulp of the largest magnitude of a float64 result."""
    m = float(ref64.abs().max()) if ref64.numel() else 0.0
    return float(np.spacing(np.float32(m))) if np.isfinite(m) else float("inf")


def bar(ref64, accepted32):
    """3 * max(error of an accepted f32 evaluation against float64, one f32 ulp of the float64 result's largest magnitude)."""
    e = float((accepted32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return 3.0 * max(e, ulp32(ref64))


def _near_tie_rows(T, d, K, cent, g):
    """Rows on the bisector of two centroids, pushed towards one of them so that the float64 relative margin of the f32 row lies in
    TIE_WINDOW; drawn by rejection until every row does.  -> (x f32 [T, d], fraction of draws kept)."""
    rows, draws = [], 0
    c64 = cent.double()
    lo, hi = np.log(2e-7), np.log(5e-6)
    while len(rows) < T:
        draws += 1
        assert draws < 50 * T + 200, "near-tie rejection does not converge"
        a, b = torch.randperm(K, generator=g)[:2].tolist()
        u = c64[a] - c64[b]
        n = 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
        n = n - (n @ u) / (u @ u) * u                               # along the bisector plane: the margin comes from the push alone
        target = float(np.exp(lo + (hi - lo) * torch.rand((), generator=g, dtype=torch.float64).item()))
        d1 = float(u @ u) / 4.0 + float(n @ n)
        t = target * d1 / (2.0 * float(u @ u))
        x = ((c64[a] + c64[b]) / 2.0 + n + t * u).float()
        m = float(margins(x[None], cent)[0])
        if TIE_WINDOW[0] <= m <= TIE_WINDOW[1]:
            rows.append(x)
    return torch.stack(rows), T / draws


def make_cell(regime, T, d, K):
    """Deterministic inputs of one cell: dict x, dy, weights, biases, cent (f32 CPU tensors), buckets (None / int / int64 [T]), and
    ``kept`` (near-tie: the fraction of draws the rejection kept)."""
    seed = 7919 * REGIMES.index(regime) + 31 * T + 7 * d + K
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn(K, d, generator=g)
    weights = 1.0 + 0.25 * torch.randn(K, d, generator=g)
    biases = 0.25 * torch.randn(K, d, generator=g)
    dy = torch.randn(T, d, generator=g)
    buckets, kept = None, None
    if regime == "near_tie":
        x, kept = _near_tie_rows(T, d, K, cent, g)
    else:
        assign = torch.randint(0, K, (T,), generator=g)
        if regime == "one_bucket":
            assign = torch.full((T,), K - 1, dtype=torch.int64)
        x = cent[assign] + 0.5 * torch.randn(T, d, generator=g)
        if regime == "offset":
            x = x + 300.0
            cent = cent + 300.0
        if regime == "given_int":
            buckets = K - 1
        if regime == "given_tensor":
            buckets = torch.randint(0, K, (T,), generator=g)
    return {"x": x.contiguous(), "dy": dy, "weights": weights, "biases": biases, "cent": cent, "buckets": buckets, "kept": kept}
