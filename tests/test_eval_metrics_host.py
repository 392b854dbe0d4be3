"""CPU tests of the evaluation metrics: what the library answers for ``smoe_eval_metrics`` without a GPU, the reference rank rule
(``ref_rank``: the contract of the kernel's ``row_rank``, float64 torch on the CPU -- tests/test_gpu_eval_metrics.py imports it) against
``torch.topk`` on tie-free rows, and ``EvalMeter`` on CPU tensors, alone and summed over a two-rank gloo group."""
import ctypes
import math
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _mp import join_or_kill

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slimmoe.h")
INT32_MAX = 2 ** 31 - 1


def ref_rank(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """THE rule, i64 [B]: the number of classes that come before the label's class in a stable descending order of the row, with x_t =
    logits[b, label]: #{c : x_c > x_t} + #{c < label : x_c ~ x_t}, where a > b means (isnan(a) and not isnan(b)) or a > b, and a ~ b
    means both are NaN or a == b -- a NaN is the largest value, ties go to the lower index.  A label outside [0, C): INT32_MAX."""
    x = logits.detach().cpu().double()
    lab = labels.detach().cpu().long()
    B, C = x.shape
    ok = (lab >= 0) & (lab < C)
    safe = lab.clamp(0, C - 1).view(-1, 1)
    xt = x.gather(1, safe)
    xn, tn = x.isnan(), xt.isnan()
    before = (xn & ~tn) | (x > xt)
    tie = (xn & tn) | (x == xt)
    lower = torch.arange(C).view(1, -1) < safe
    rank = (before | (tie & lower)).sum(1)
    return torch.where(ok, rank, torch.full_like(rank, INT32_MAX))


def ulp32(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def timm_accuracy(output, target, topk=(1,)):
    """timm.utils.accuracy, restated."""
    maxk = min(max(topk), output.shape[1])
    _, pred = output.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[: min(k, maxk)].reshape(-1).float().sum(0) * 100.0 / target.shape[0] for k in topk]


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_point_is_declared_prototyped_and_exported_and_the_abi_stays_29():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    s = "smoe_eval_metrics"
    assert re.search(r"\bint\s+%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
    assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), s), f"libslimmoe_hip.so does not export {s}"
    n_args = len([a for a in re.search(r"%s\s*\((.*?)\)" % s, text, re.S).group(1).split(",") if a.strip()])
    assert n_args == len(_lib.SIGNATURES[s][1]) == 12
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    assert _lib.binary_build_id() == _lib.source_build_id()


def test_argument_checks_come_before_any_launch():
    lib = _lib.load()
    fake = 4096          # never dereferenced
    ks = (ctypes.c_int * 5)(1, 5, 2, 3, 4)
    zero = (ctypes.c_int * 2)(1, 0)

    def call(logits=fake, dtype=0, labels=fake, B=4, C=10, k=ks, nk=2, row_loss=fake, row_rank=fake, batch=fake):
        return lib.smoe_eval_metrics(logits, dtype, labels, B, C, k, nk, row_loss, row_rank, batch, None, None)

    assert call(B=0) == 0                                  # B == 0 returns at once
    for name in ("logits", "labels", "row_loss", "row_rank", "batch"):
        assert call(**{name: None}) != 0, name
        assert b"smoe_eval_metrics" in lib.smoe_last_error() and b"null" in lib.smoe_last_error(), name
    for nk in (0, 5):
        assert call(nk=nk) != 0
        assert b"nk" in lib.smoe_last_error()
    assert call(k=zero) != 0
    assert b"k must be >= 1" in lib.smoe_last_error()
    assert call(k=None) != 0
    for C in (0, 2 ** 30 + 1):
        assert call(C=C) != 0
        assert b"C <= 2^30" in lib.smoe_last_error()
    assert call(C=2 ** 30, B=-1) != 0
    assert call(dtype=7) != 0
    assert b"dtype" in lib.smoe_last_error()
    assert call(B=-1) != 0
    assert b"B" in lib.smoe_last_error()
    assert call(B=2 ** 31) != 0


# ------------------------------------------------------------------------------------------------------- the rule against torch
def tie_free_rows(B, C, seed, nan_every=0):
    """f32 [B, C]: every row a permutation of C distinct values (exact in f32); ``nan_every``: one NaN in every such row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([(torch.randperm(C, generator=g).float() - C / 2) / 64 for _ in range(B)])
    if nan_every:
        for b in range(0, B, nan_every):
            x[b, int(torch.randint(0, C, (1,), generator=g))] = float("nan")
    return x, torch.randint(0, C, (B,), generator=g)


@pytest.mark.parametrize("C", [1, 3, 5, 8, 100, 1000, 1001])
def test_reference_rank_agrees_with_topk_on_tie_free_rows(C):
    B = 70
    x, labels = tie_free_rows(B, C, 3 + C, nan_every=7)
    labels[0] = int(x[0].isnan().nonzero()[0])             # (a NaN AT the label too: it is the largest value, rank 0)
    rank = ref_rank(x, labels)
    assert rank[0].item() == 0 and 0 <= rank.min().item() and rank.max().item() <= C - 1
    for k in (1, 5):
        _, pred = x.topk(min(k, C), 1, True, True)
        hit = pred.eq(labels.view(-1, 1)).any(1)
        assert torch.equal(rank < k, hit), (C, k, int(((rank < k) != hit).sum()))
    # a NaN row elsewhere: the NaN comes before every other class
    b = 7
    nan_at = int(x[b].isnan().nonzero()[0])
    other = (nan_at + 1) % C
    if C > 1:
        assert ref_rank(x[b:b + 1], torch.tensor([other])).item() == 1 + int((x[b] > x[b, other]).sum())


def test_reference_rank_ties_and_bad_labels():
    x = torch.tensor([[1., 2., 2., 0., 2.], [3., 3., 3., 3., 3.]])
    assert ref_rank(x, torch.tensor([2, 3])).tolist() == [1, 3]
    assert ref_rank(x, torch.tensor([0, 0])).tolist() == [3, 0]
    assert ref_rank(x, torch.tensor([-1, 5])).tolist() == [INT32_MAX, INT32_MAX]
    nan = float("nan")
    assert ref_rank(torch.tensor([[nan, 1., nan, nan]]), torch.tensor([2])).tolist() == [1]
    assert ref_rank(torch.tensor([[nan, 1., nan, nan]]), torch.tensor([1])).tolist() == [3]


# ---------------------------------------------------------------------------------------------------------- EvalMeter on the CPU
def _batches(sizes, C, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for bs in sizes:
        x = torch.randn(bs, C, generator=g) * 3
        labels = torch.randint(0, C, (bs,), generator=g)
        for b in range(0, bs, 2):                          # half of the rows are made correct at rank 0 or 3
            r = (b // 2) % 2 * 3
            labels[b] = x[b].topk(r + 1).indices[r]
        out.append((x, labels))
    return out


def _reference_lines(batches):
    """engine.py:99-113 of the reference: per-batch CrossEntropyLoss and accuracy, weighted by the batch size, read with .item()."""
    crit = torch.nn.CrossEntropyLoss()
    n, loss, a1, a5 = 0, 0.0, 0.0, 0.0
    for x, labels in batches:
        acc1, acc5 = timm_accuracy(x, labels, (1, 5))
        bs = x.shape[0]
        n += bs
        loss += crit(x, labels).item() * bs
        a1 += acc1.item() * bs
        a5 += acc5.item() * bs
    return loss / n, a1 / n, a5 / n, n


def test_eval_meter_on_cpu_tensors_against_the_reference_lines():
    C = 100
    batches = _batches((6, 6, 3), C, 21)
    meter = sm.EvalMeter("cpu", topk=(1, 5))
    assert sm.EvalMeter is sm.engine.EvalMeter and meter.acc.dtype == torch.float64 and meter.acc.shape == (4,)
    for x, labels in batches:
        meter.update(x, labels)
    res = meter.result()
    bits = meter.acc.clone()
    assert set(res) == {"loss", "acc1", "acc5", "n"}
    xs, ls = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    assert not (xs == xs.gather(1, ls.view(-1, 1))).sum(1).gt(1).any(), "a label's logit ties another: the comparison below is void"
    rank = ref_rank(xs, ls)
    c1, c5 = int((rank < 1).sum()), int((rank < 5).sum())
    assert 0 < c1 < c5 < 15
    assert res["n"] == 15 and meter.acc[1:].tolist() == [15.0, float(c1), float(c5)]          # counts exact
    assert res["acc1"] == 100.0 * c1 / 15 and res["acc5"] == 100.0 * c5 / 15
    l_ref, a1_ref, a5_ref, n_ref = _reference_lines(batches)
    assert n_ref == 15 and abs(res["acc1"] - a1_ref) <= 1e-5 and abs(res["acc5"] - a5_ref) <= 1e-5
    l64 = torch.nn.functional.cross_entropy(xs.double(), ls).item()
    e_ref = abs(l_ref - l64)
    bar = max(3 * e_ref, ulp32(l64))
    print(f"EvalMeter (CPU) loss {res['loss']!r}: error {abs(res['loss'] - l64):.3e} against float64, the reference lines' {e_ref:.3e}, bar {bar:.3e}")
    assert abs(res["loss"] - l64) <= bar
    meter.reset()
    assert meter.acc.tolist() == [0.0] * 4 and meter.result()["n"] == 0
    for x, labels in batches:
        meter.update(x, labels)
    assert torch.equal(meter.acc, bits) and meter.result() == res
    other = sm.EvalMeter("cpu", topk=(1, 2, 3))
    other.update(xs, ls)
    assert set(other.result()) == {"loss", "acc1", "acc2", "acc3", "n"}
    with pytest.raises(ValueError):
        sm.EvalMeter("cpu", metrics="host")


def test_evaluate_on_cpu_keeps_its_keys_under_both_metrics():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 4 * 4, 10))
    g = torch.Generator().manual_seed(1)
    data = [(torch.randn(bs, 3, 4, 4, generator=g), torch.randint(0, 10, (bs,), generator=g)) for bs in (6, 6, 3)]
    dev_res = sm.evaluate(data, model, "cpu", autocast=False, metrics="device")
    ref_res = sm.evaluate(data, model, "cpu", autocast=False, metrics="torch")
    keys = {"loss", "acc1", "acc5", "images_per_sec", "ep_repeated_steps", "hip_graph"}
    assert set(dev_res) == keys and set(ref_res) == keys
    assert abs(dev_res["acc1"] - ref_res["acc1"]) <= 1e-5 and abs(dev_res["acc5"] - ref_res["acc5"]) <= 1e-5
    assert abs(dev_res["loss"] - ref_res["loss"]) <= 1e-5 * ref_res["loss"]
    with pytest.raises(ValueError):
        sm.evaluate(data, model, "cpu", autocast=False, metrics="host")


# ------------------------------------------------------------------------------------------------------------- two gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_batches(rank):
    return _batches((6, 3) if rank == 0 else (5, 6, 2), 100, 40 + rank)


def _meter_worker(rank, W, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    try:
        meter = sm.EvalMeter("cpu", topk=(1, 5))
        for x, labels in _rank_batches(rank):
            meter.update(x, labels)
        alone = meter.acc.tolist()
        meter.synchronize_between_processes()
        q.put((rank, alone, meter.acc.tolist(), meter.result()))
    finally:
        dist.destroy_process_group()


def test_synchronize_between_processes_sums_the_meter_over_a_two_rank_gloo_group():
    W = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_meter_worker, args=(r, W, port, q)) for r in range(W)]
    for p in procs:
        p.start()
    join_or_kill(procs, 120)
    got = sorted(q.get(timeout=5) for _ in range(W))
    assert [g[0] for g in got] == [0, 1]
    one = sm.EvalMeter("cpu", topk=(1, 5))
    for r in range(W):
        for x, labels in _rank_batches(r):
            one.update(x, labels)
    want = one.acc.tolist()
    assert want[1] == 22.0
    for rank, alone, summed, res in got:
        assert alone[1] == (9.0 if rank == 0 else 13.0)
        assert summed[1:] == want[1:], (rank, summed, want)                        # n and the counts: exact
        assert abs(summed[0] - want[0]) <= 1e-12 * abs(want[0]), (summed[0], want[0])   # f64 sums in another order
        assert res["n"] == 22 and res["acc1"] == 100.0 * want[2] / 22
    # without a process group the call is a no-op
    before = one.acc.clone()
    one.synchronize_between_processes()
    assert torch.equal(one.acc, before)
