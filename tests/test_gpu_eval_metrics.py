"""GPU tests of the evaluation metrics on the library's kernel: smoe_eval_metrics' ranks against the rule (ref_rank, float64 on the
CPU) on rows that are tie-free by construction, its accuracies bit-equal to timm's lines on the device, its losses bit-equal to
smoe_soft_ce_fwd and within the bar taken from torch's own f32 composition, ties, the non-finite / bad-label contract (INTEGRATION.md
section B), the f64 accumulator, graph capture, and engine.evaluate / engine.accuracy / EvalMeter on top of it."""
import math

import pytest
import torch

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import ops

from test_eval_metrics_host import INT32_MAX, ref_rank, timm_accuracy, ulp32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows_with_ranks(B, C, dtype, seed, offset=False):
    """(x [B, C] on the device, labels i64 [B], the ranks the labels were placed at).  Rows are tie-free by construction: a permutation
    of (0..C-1 - C/2) / 64, exact in f32 for every C used here, in f16 for C <= 4096 and in bf16 for C <= 500.  The target ranks cycle
    through 0, k-1, k for k in (1, 5), C-1 and a random one, where they exist.  ``offset``: the base pointer is one element off."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(B, C, generator=g).argsort(1)
    x = ((perm.float() - C / 2) / 64).to(dtype)
    assert (x.double().sort(1).values.diff(dim=1) > 0).all(), "rows are not tie-free in this dtype"
    cycle = [r for r in (0, 1, 4, 5, C - 1) if r < C]
    want = torch.tensor([cycle[b % (len(cycle) + 1)] if b % (len(cycle) + 1) < len(cycle) else int(torch.randint(0, C, (1,), generator=g))
                         for b in range(B)])
    labels = x.double().argsort(1, descending=True).gather(1, want.view(-1, 1)).squeeze(1)
    if offset:
        flat = torch.empty(B * C + 1, dtype=dtype, device=DEV)
        xd = flat[1:].view(B, C)
        xd.copy_(x)
        assert xd.data_ptr() % 16 != 0 and xd.is_contiguous()
    else:
        xd = x.to(DEV)
    return xd, labels.to(DEV), want


GRID = ([(torch.float32, C) for C in (1, 3, 5, 8, 100, 1000, 1001, 2056, 4104)]
        + [(torch.float16, C) for C in (5, 8, 1000, 1001, 2056, 4096)]
        + [(torch.bfloat16, C) for C in (5, 8, 250, 500)])


def _check_ranks(x, labels, want, topks):
    B = x.shape[0]
    for topk in topks:
        batch, row_loss, row_rank = ops.eval_metrics(x, labels, None, topk)
        assert batch.dtype == torch.float32 and batch.shape == (1 + len(topk),)
        assert row_loss.dtype == torch.float32 and row_rank.dtype == torch.int32 and row_loss.shape == row_rank.shape == (B,)
        assert torch.equal(row_rank.cpu().long(), want), (row_rank.tolist(), want.tolist())
        assert torch.equal(ref_rank(x, labels), want)
        timm = torch.stack(timm_accuracy(x, labels, topk))           # timm's lines, on the device
        assert timm.is_cuda and timm.dtype == torch.float32
        assert torch.equal(batch[1:], timm), (topk, batch[1:].tolist(), timm.tolist())
        for i, k in enumerate(topk):
            assert batch[1 + i].item() == pytest.approx(100.0 * int((want < k).sum()) / B, rel=1e-6)


@pytest.mark.parametrize("dtype,C", GRID, ids=[f"{str(d).split('.')[1]}-{C}" for d, C in GRID])
def test_ranks_are_exact_and_accuracies_are_timms_bits(dtype, C):
    """2056 and 4104: more than one 2048-logit step per workgroup; 1001 and 100 (f16: 1001): the element-wise path."""
    for B in (1, 3, 257):
        x, labels, want = _rows_with_ranks(B, C, dtype, 1000 * B + C)
        _check_ranks(x, labels, want, [(1,), (1, 5), (1, 2, 3, 5)] if B == 257 else [(1, 5)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_ranks_with_a_base_pointer_one_element_off(dtype):
    x, labels, want = _rows_with_ranks(257, 1000, dtype, 77, offset=True)
    _check_ranks(x, labels, want, [(1, 5)])


# ---------------------------------------------------------------------------------------------------------------------- loss
def _bars(x, labels):
    """tests/test_gpu_mixup_loss.py::_bars for the cross-entropy: (float64 rows, bar, torch's own error) -- 3 x the max error of torch's
    f32 composition against float64 on these inputs, and at least one f32 ulp of the largest reference value."""
    r64 = -torch.log_softmax(x.double(), -1).gather(-1, labels.view(-1, 1)).squeeze(1)
    r32 = -torch.log_softmax(x.float(), -1).gather(-1, labels.view(-1, 1)).squeeze(1)
    e_row = (r32.double() - r64).abs().max().item()
    return r64, max(3 * e_row, ulp32(r64.abs().max().item())), e_row


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,C", [(64, 1000), (3, 1001), (257, 2056), (2, 4099)])
def test_loss_is_soft_ce_fwds_bits_and_within_torchs_own_error(B, C, dtype, scale):
    """(257, 2056): more rows than the mean kernels' 256 threads and more than one 2048-logit step on the 8-per-lane path; (2, 4099):
    more than one step on the element path."""
    g = torch.Generator(device=DEV).manual_seed(B + C)
    x = (torch.randn(B, C, generator=g, device=DEV) * scale).to(dtype)
    labels = torch.randint(0, C, (B,), generator=g, device=DEV)
    batch, row_loss, _ = ops.eval_metrics(x, labels)
    loss, rows = ops.soft_ce_fwd(x, labels=labels, smoothing=0.0)
    r64, bar, e_row = _bars(x, labels)
    o_row = (row_loss.double() - r64).abs().max().item()
    o_mean = abs(batch[0].double().item() - r64.mean().item())
    print(f"eval_metrics {str(dtype).split('.')[1]} [{B}, {C}] scale {scale}: row loss max error own {o_row:.3e} / torch {e_row:.3e} "
          f"(bar {bar:.3e}); mean own {o_mean:.3e}")
    assert torch.equal(row_loss.view(torch.int32), rows[0].view(torch.int32)), "row_loss differs from smoe_soft_ce_fwd's"
    assert torch.equal(batch[0].view(torch.int32), loss.view(torch.int32)), "batch[0] differs from smoe_soft_ce_fwd's loss"
    assert o_row <= bar, (o_row, e_row)
    assert o_mean <= bar, (o_mean, bar)


# ---------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("dtype,C", [(torch.float32, 1000), (torch.float16, 1001), (torch.float32, 2056)])
def test_ties_go_to_the_lower_index(dtype, C):
    g = torch.Generator().manual_seed(C)
    B = 9
    x = torch.randn(B, C, generator=g).to(dtype)
    labels = torch.randint(20, C - 20, (B,), generator=g)
    for b in range(B - 1):                                 # copies of the label's value before AND after the label
        L = int(labels[b])
        v = x[b, L].item()
        x[b, [L - 7, L - 1, 0]] = v
        x[b, [L + 1, L + 9, C - 1]] = v
        x[b, 3] = v + 1                                      # ... and one value above it for sure
    x[B - 1] = 0.25                                          # an all-equal row: the rank is the label
    want = ref_rank(x, labels)
    assert want[B - 1].item() == int(labels[B - 1]) and (want[:-1] >= 4).all()
    _, _, row_rank = ops.eval_metrics(x.to(DEV), labels.to(DEV))
    assert torch.equal(row_rank.cpu().long(), want), (row_rank.tolist(), want.tolist())


# --------------------------------------------------------------------------------------------------------------- containment
@pytest.mark.parametrize("dtype,C", [(torch.float32, 1000), (torch.float16, 1001)])
def test_non_finite_logits_and_bad_labels_stay_in_their_row(dtype, C):
    g = torch.Generator().manual_seed(5 + C)
    B = 14
    x0 = torch.randn(B, C, generator=g).to(dtype)
    l0 = torch.randint(20, C - 20, (B,), generator=g)
    nan, inf = float("nan"), float("inf")
    x, labels = x0.clone(), l0.clone()
    x[1, int(l0[1]) + 3] = nan                               # a NaN at a non-label class
    L = int(l0[3])
    x[3, [L - 11, L - 2, L, L + 4, L + 15]] = nan            # a NaN at the label, further NaNs before and after it
    x[5, int(l0[5]) - 5] = inf                               # a +inf
    x[7] = -inf                                              # a row of -inf
    labels[9], labels[10], labels[11], labels[12] = -1, C, -100, 2 ** 40
    bad = [1, 3, 5, 7, 9, 10, 11, 12]
    good = [b for b in range(B) if b not in bad]
    want = ref_rank(x, labels)
    was_before = bool(x0[1, int(l0[1]) + 3] > x0[1, int(l0[1])])       # the NaN comes before the label whatever stood there
    assert want[1].item() == ref_rank(x0, l0)[1].item() + (0 if was_before else 1)
    assert want[3].item() == 2 and want[7].item() == int(l0[7])
    assert want[[9, 10, 11, 12]].tolist() == [INT32_MAX] * 4
    _, loss0, rank0 = ops.eval_metrics(x0.to(DEV), l0.to(DEV))
    acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    batch, loss, rank = ops.eval_metrics(x.to(DEV), labels.to(DEV), acc)
    torch.cuda.synchronize()
    assert torch.equal(rank.cpu().long(), want), (rank.tolist(), want.tolist())
    assert loss[bad].isnan().all(), loss[bad].tolist()
    assert loss0.isfinite().all()
    assert torch.equal(loss[good].view(torch.int32), loss0[good].view(torch.int32)) and torch.equal(rank[good], rank0[good])
    a = acc.tolist()
    assert math.isnan(a[0]) and math.isnan(batch[0].item())
    assert a[1:] == [float(B), float((want < 1).sum()), float((want < 5).sum())]
    assert batch[1].item() == pytest.approx(100.0 * a[2] / B, rel=1e-6)


# --------------------------------------------------------------------------------------------------------------- accumulator
def _logit_batches(sizes, C, seed, dtype=torch.float32):
    """Batches with a visible share of correct rows: every other row's label is its rank-0 or rank-3 class."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for bs in sizes:
        x = (torch.randn(bs, C, generator=g) * 3).to(dtype)
        labels = torch.randint(0, C, (bs,), generator=g)
        order = x.double().argsort(1, descending=True)
        for b in range(0, bs, 2):
            labels[b] = order[b, (b // 2) % 2 * 3]
        out.append((x.to(DEV), labels.to(DEV)))
    return out


@pytest.mark.parametrize("sizes,C", [((6, 6, 3), 100), ((192, 192, 77), 1000)])
def test_accumulator_counts_exactly_and_sums_in_double(sizes, C):
    batches = _logit_batches(sizes, C, 9 + C, torch.float16 if C == 1000 else torch.float32)
    runs = []
    for _ in range(2):
        acc = torch.zeros(4, dtype=torch.float64, device=DEV)
        rows = []
        for x, labels in batches:
            rows.append(ops.eval_metrics(x, labels, acc, (1, 5))[1])
        runs.append((acc.clone(), torch.cat(rows)))
    acc, rows = runs[0]
    ranks = torch.cat([ref_rank(x, labels) for x, labels in batches])
    a = acc.tolist()
    assert a[1:] == [float(sum(sizes)), float((ranks < 1).sum()), float((ranks < 5).sum())] and 0 < a[2] < a[3] < a[1]
    want = math.fsum(rows.double().tolist())
    assert abs(a[0] - want) <= 1e-12 * abs(want), (a[0], want)
    assert torch.equal(runs[1][0], acc) and torch.equal(runs[1][1], rows)                 # the same bits run to run
    x, labels = batches[0]
    b0, r0, k0 = ops.eval_metrics(x, labels)                                               # acc=None works
    b1, r1, k1 = ops.eval_metrics(x, labels, torch.zeros(4, dtype=torch.float64, device=DEV))
    assert torch.equal(b0, b1) and torch.equal(r0, r1) and torch.equal(k0, k1)
    with pytest.raises(RuntimeError):
        ops.eval_metrics(x, labels, torch.zeros(3, dtype=torch.float64, device=DEV))       # [2 + nk] expected
    with pytest.raises(RuntimeError):
        ops.eval_metrics(x, labels, None, (1, 2, 3, 4, 5))
    with pytest.raises(RuntimeError):
        ops.eval_metrics(x, labels, None, (0,))


# -------------------------------------------------------------------------------------------------------------------- capture
def test_the_call_captures_into_a_graph_and_replays_bit_exact():
    B, C = 48, 1000
    data = _logit_batches((B, B, B), C, 31, torch.float16)
    eager_acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    eager = []
    for x, labels in data:
        eager.append([t.clone() for t in ops.eval_metrics(x, labels, eager_acc, (1, 5))] + [eager_acc.clone()])
    xs, ls = torch.zeros_like(data[0][0]), torch.zeros_like(data[0][1])
    acc = torch.zeros(4, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # one linear chain on one stream
        outs = ops.eval_metrics(xs, ls, acc, (1, 5))
    acc.zero_()
    for (x, labels), want in zip(data, eager):
        xs.copy_(x)
        ls.copy_(labels)
        graph.replay()
        for got, w in zip(list(outs) + [acc], want):
            assert torch.equal(got, w)
    assert acc[1].item() == 3 * B


# -------------------------------------------------------------------------------------------------------------------- harness
def _model_and_loader(sizes, seed=0):
    torch.manual_seed(seed)
    model = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=100, depth=3).to(DEV).eval()
    g = torch.Generator().manual_seed(seed + 1)
    return model, [torch.randn(bs, 3, 224, 224, generator=g) for bs in sizes]


def _untied(row, candidates):
    """The first of the candidate classes whose logit no other class of the row shares (f16 logits of 100 classes do tie now and then)."""
    return next(int(c) for c in candidates if int((row == row[c]).sum()) == 1)


@pytest.mark.parametrize("autocast", [False, True])
def test_evaluate_device_metrics_against_the_torch_lines(autocast):
    model, images = _model_and_loader((6, 6, 3))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        logits = [model(im.to(DEV)) for im in images]
    loader = []
    for im, out in zip(images, logits):                  # labels at rank 0 / rank 3 of the model's own logits, the rest anywhere
        out = out.double().cpu()
        order = out.argsort(1, descending=True)
        labels = torch.tensor([_untied(out[b], order[b, (b // 2) % 2 * 3:]) if b % 2 == 0
                               else _untied(out[b], [(17 * b + 5 + i) % 100 for i in range(100)]) for b in range(len(im))])
        loader.append((im, labels))
    xs = torch.cat(logits)
    ls = torch.cat([lab for _, lab in loader]).to(DEV)
    assert xs.dtype == (torch.float16 if autocast else torch.float32)
    assert not (xs == xs.gather(1, ls.view(-1, 1))).sum(1).gt(1).any(), "a label's logit ties another logit: the comparison is void"
    l64 = torch.nn.functional.cross_entropy(xs.double(), ls).item()
    for hip_graph in (False, True):
        dev = sm.evaluate(loader, model, DEV, autocast=autocast, hip_graph=hip_graph, metrics="device")
        ref = sm.evaluate(loader, model, DEV, autocast=autocast, hip_graph=hip_graph, metrics="torch")
        again = sm.evaluate(loader, model, DEV, autocast=autocast, hip_graph=hip_graph, metrics="device")
        assert set(dev) == set(ref) == {"loss", "acc1", "acc5", "images_per_sec", "ep_repeated_steps", "hip_graph"}
        assert dev["hip_graph"] is hip_graph and ref["hip_graph"] is hip_graph
        ranks = ref_rank(xs, ls)
        assert dev["acc1"] == 100.0 * int((ranks < 1).sum()) / 15 and dev["acc5"] == 100.0 * int((ranks < 5).sum()) / 15
        assert 0 < dev["acc1"] < dev["acc5"] < 100
        assert abs(dev["acc1"] - ref["acc1"]) <= 1e-5 and abs(dev["acc5"] - ref["acc5"]) <= 1e-5   # (the torch lines weight f32 percentages)
        e_ref = abs(ref["loss"] - l64)
        bar = max(3 * e_ref, ulp32(l64))
        print(f"evaluate autocast {autocast} hip_graph {hip_graph}: loss device {dev['loss']!r} torch {ref['loss']!r} float64 {l64!r}: "
              f"error {abs(dev['loss'] - l64):.3e} / {e_ref:.3e} (bar {bar:.3e})")
        assert abs(dev["loss"] - l64) <= bar
        assert (dev["loss"], dev["acc1"], dev["acc5"]) == (again["loss"], again["acc1"], again["acc5"])


def test_evaluate_device_metrics_read_the_host_once_whatever_the_batch_count(monkeypatch):
    model, images = _model_and_loader((4,) * 5)
    labels = torch.arange(4)
    reads = [0]
    for name in ("item", "cpu", "tolist", "numpy"):
        def probe(self, *a, _orig=getattr(torch.Tensor, name), **kw):
            reads[0] += int(self.is_cuda)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, probe)

    def count(n, metrics):
        reads[0] = 0
        sm.evaluate([(im, labels) for im in images[:n]], model, DEV, hip_graph=False, metrics=metrics)
        return reads[0]

    count(2, "device")                                   # (first use: caches fill)
    d2, d5, t2, t5 = count(2, "device"), count(5, "device"), count(2, "torch"), count(5, "torch")
    print(f"host reads of CUDA tensors during evaluate(): device {d2} (2 batches) / {d5} (5); torch {t2} / {t5}")
    assert d2 == d5 and d2 >= 1
    assert t5 - t2 == 3 * 3 and t2 > d2                  # the probe sees the three .item() per batch of the torch lines


def test_eval_meter_on_the_device_and_its_torch_path(monkeypatch):
    batches = _logit_batches((6, 6, 3), 100, 3)
    calls = [0]
    orig = ops.eval_metrics
    monkeypatch.setattr(ops, "eval_metrics", lambda *a, **kw: (calls.__setitem__(0, calls[0] + 1), orig(*a, **kw))[1])
    dev, tor = sm.EvalMeter(DEV, (1, 5), "device"), sm.EvalMeter(DEV, (1, 5), "torch")
    for x, labels in batches:
        dev.update(x, labels)
        tor.update(x, labels)
        dev.update(x.double(), labels)                   # a dtype the kernel does not take: the torch path, same tensor
    assert calls[0] == 3
    a, b = dev.result(), tor.result()
    assert a["n"] == 30 and b["n"] == 15 and a["acc1"] == b["acc1"] and a["acc5"] == b["acc5"] and 0 < a["acc1"] < a["acc5"]
    assert abs(a["loss"] - b["loss"]) <= 3 * ulp32(b["loss"])


# ------------------------------------------------------------------------------------------------------------ engine.accuracy
def test_accuracy_on_cuda_takes_the_kernel_and_falls_back_for_other_layouts(monkeypatch):
    calls = [0]
    orig = ops.eval_metrics
    monkeypatch.setattr(ops, "eval_metrics", lambda *a, **kw: (calls.__setitem__(0, calls[0] + 1), orig(*a, **kw))[1])
    for dtype, C in [(torch.float32, 1000), (torch.float16, 1001), (torch.bfloat16, 250)]:
        x, labels, _ = _rows_with_ranks(257, C, dtype, 11 + C)
        for topk in [(1,), (1, 5)]:
            n = calls[0]
            got = sm.accuracy(x, labels, topk)
            assert calls[0] == n + 1
            want = timm_accuracy(x, labels, topk)
            assert len(got) == len(topk) and all(t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda for t in got)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (got, want)
        n = calls[0]
        assert torch.equal(sm.accuracy(x, labels.int(), (1,))[0], timm_accuracy(x, labels, (1,))[0]) and calls[0] == n + 1
        wide = torch.zeros(257, 2 * C, dtype=dtype, device=DEV)
        wide[:, ::2] = x
        view = wide[:, ::2]                               # not contiguous: timm's lines
        n = calls[0]
        got = sm.accuracy(view, labels, (1, 5))
        assert calls[0] == n and all(torch.equal(a, b) for a, b in zip(got, timm_accuracy(x, labels, (1, 5))))
    n = calls[0]
    sm.accuracy(x.cpu().float(), labels.cpu(), (1, 5))
    assert calls[0] == n
