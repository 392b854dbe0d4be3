"""The last block of an eval forward runs its expert FFN for the rows the classifier reads only (VisionTransformer.tail_rows_only):
the dispatch plan over a periodic subset of the tokens (smoe_dispatch_plan_subset) against a host plan, the model with and without
it bit for bit (logits and every block's routing record), the other rows of the operator's result, the paths that must keep the
full dispatch, and the premise that makes the bits equal at the benchmark's size -- a row of the persistent grouped GEMM does not
depend on the tile height the launcher picks (320 rows for the whole batch, 256 for the few head rows)."""
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _mp import join_or_kill as _join_or_kill  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import ops  # noqa: E402
from slim_switch_moe_vit_amd.ep import drain  # noqa: E402
from slim_switch_moe_vit_amd.resmoe import patch_blocks_with_moe  # noqa: E402
from test_gpu_model import _init  # noqa: E402

DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------- the plan over a subset
def _host_plan(idx: np.ndarray, E: int, period: int, prefix: int):
    """Stable order by expert, then by flat index, over the entries of the tokens t with t % period < prefix (period 0: all)."""
    T, k = idx.shape
    flat = idx.reshape(-1)
    n = flat.size
    keep = [i for i in range(n) if 0 <= flat[i] < E and (period == 0 or (i // k) % period < prefix)]
    order = sorted(keep, key=lambda i: (flat[i], i))
    counts = np.array([sum(1 for i in keep if flat[i] == e) for e in range(E)], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pos = np.full(n, -1, dtype=np.int64)
    pos[:len(order)] = order
    inv_pos = np.full(n, -1, dtype=np.int64)
    inv_pos[order] = np.arange(len(order))
    return counts, offsets, pos, inv_pos


def _plan_case(case: str, T: int, k: int, E: int, period: int, prefix: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, E, size=(T, k)).astype(np.int64)
    head = (np.arange(T) % period) < prefix
    if case == "empty_expert":         # expert 2 holds no dispatched entry (the tokens left out still name it)
        idx[head] = np.where(idx[head] == 2, 3, idx[head])
        idx[~head] = 2
    elif case == "one_expert":         # every dispatched entry on expert 1
        idx[head] = 1
    elif case == "some_dropped":       # idx = -1 among the dispatched and among the other tokens
        idx[rng.random((T, k)) < 0.3] = -1
        idx[0, 0] = -1
    return idx


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("prefix", [1, 2])
@pytest.mark.parametrize("case", ["random", "empty_expert", "one_expert", "some_dropped"])
def test_plan_subset_equals_the_host_plan(case, prefix, k):
    T, period, E = 7 * 5, 5, 4
    idx = _plan_case(case, T, k, E, period, prefix, seed=11 + 7 * prefix + k)
    want = _host_plan(idx, E, period, prefix)
    if case == "empty_expert":
        assert want[0][2] == 0
    if case == "one_expert":
        assert want[0][1] == 7 * prefix * k and want[0].sum() == want[0][1]
    counts, offsets, pos, inv_pos, pruned = ops.dispatch_plan(torch.from_numpy(idx).to(DEV), E, subset=(period, prefix))
    assert pruned is None
    for name, got, ref in zip(("counts", "offsets", "pos", "inv_pos"), (counts, offsets, pos, inv_pos), want):
        assert np.array_equal(got.cpu().numpy(), ref), (name, got.cpu().numpy(), ref)
    kept = int(want[1][-1])
    rows = pos.cpu().numpy()[:kept] // k                 # what GEMM-1 gathers / GEMM-2 writes: rows of the FULL [T, d] tensors
    assert ((rows % period) < prefix).all() and (pos.cpu().numpy()[kept:] == -1).all()


def test_plan_subset_over_several_chunks_equals_the_host_plan():
    """More than one workgroup of the counting / assign kernels (1024 flat entries each), the period the model uses."""
    T, period, prefix, E, k = 15 * 197, 197, 2, 8, 2
    idx = np.random.default_rng(5).integers(0, E, size=(T, k)).astype(np.int64)
    want = _host_plan(idx, E, period, prefix)
    got = ops.dispatch_plan(torch.from_numpy(idx).to(DEV), E, subset=(period, prefix))
    for name, g, ref in zip(("counts", "offsets", "pos", "inv_pos"), got, want):
        assert np.array_equal(g.cpu().numpy(), ref), name


@pytest.mark.parametrize("k", [1, 2])
def test_plan_subset_period_zero_is_the_plan_of_today(k):
    idx = torch.from_numpy(_plan_case("some_dropped", 35, k, 4, 5, 1, seed=3)).to(DEV)
    full = ops.dispatch_plan(idx, 4)
    sub = ops.dispatch_plan(idx, 4, subset=(0, 0))
    for a, b in zip(full[:4], sub[:4]):
        assert torch.equal(a, b)
    want = _host_plan(idx.cpu().numpy(), 4, 0, 0)
    for g, ref in zip(sub[:4], want):
        assert np.array_equal(g.cpu().numpy(), ref)


def test_plan_subset_refuses_a_capacity_and_a_bad_prefix():
    idx = torch.zeros((10, 1), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        ops.dispatch_plan(idx, 4, capacity=3, subset=(5, 1))
    with pytest.raises(RuntimeError):
        ops.dispatch_plan(idx, 4, subset=(5, 6))


# ---------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("k,E", [(1, 4), (2, 8)])
@pytest.mark.parametrize("prefix", [1, 2])
def test_operator_tail_rows_equal_the_full_result_and_the_other_rows_are_the_residual(k, E, prefix):
    d, N, B = 192, 197, 3
    torch.manual_seed(20 + k)
    mod = sm.CustomizedMoEMLP(d, 4 * d, E, k, 0.0).eval().to(DEV)
    norm = torch.nn.LayerNorm(d, eps=1e-6).to(DEV)
    with torch.no_grad():
        for p in mod.experts.parameters():
            p.copy_(torch.randn_like(p) * 0.05)
        x = torch.randn(B, N, d, device=DEV)
        ops.profile_begin(only=["grouped_gemm"])
        full = drain(mod.forward_norm_add_steps(x.clone(), norm))
        plan_full = [t.clone() for t in mod.last_plan[:2]]
        got = drain(mod.forward_norm_add_steps(x.clone(), norm, tail=(N, prefix)))
        torch.cuda.synchronize()
        rec = ops.profile_end()
    rows = [int(round(m["flops"] / (2.0 * m["K"] * m["N"]))) for _, m, _ in rec]
    assert rows == [B * N * k] * 2 + [B * prefix * k] * 2, rows
    assert torch.equal(got[:, :prefix], full[:, :prefix])
    assert torch.equal(got[:, prefix:], x[:, prefix:])                  # defined values: the MoE half's input
    assert not torch.equal(full[:, prefix:], x[:, prefix:])
    for a, b in zip(plan_full, mod.last_plan[:2]):                      # idx, score: all B * N rows
        assert a.shape[0] == B * N and torch.equal(a, b)
    counts = mod.last_plan[2].cpu()
    assert int(counts.sum()) == B * prefix * k, counts


# ---------------------------------------------------------------------------------------------- the model
def _model(kind: str):
    torch.manual_seed(0)
    if kind == "top1":
        m = sm.create_model("moe_tiny_patch16_224_expert4_top1", num_classes=100, depth=2)
    elif kind == "top2":
        m = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=100, depth=2)
    elif kind == "capacity":
        m = sm.create_model("moe_tiny_patch16_224_expert4_top1", num_classes=100, depth=2, gate="switch", capacity_factor=1.0)
    else:
        m = patch_blocks_with_moe(sm.create_model("deit_tiny_distilled_patch16_224", num_classes=100, depth=2), 4, 1, False)
        with torch.no_grad():
            m.head_dist.weight.copy_(torch.randn(m.head_dist.weight.shape, generator=torch.Generator().manual_seed(9)) * 0.02)
    return _init(m, 31).eval().to(DEV)


def _images(B: int):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(40 + B)).to(DEV)


def _forward(model, images, grad=False):
    """-> (logits, [(idx, score) per block], rows of every `grouped_gemm` launch in order)."""
    ops.profile_begin(only=["grouped_gemm"])
    with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=torch.float16):
        out = model(images)
    torch.cuda.synchronize()
    rows = [int(round(m["flops"] / (2.0 * m["K"] * m["N"]))) for _, m, _ in ops.profile_end()]
    out = out[0] if isinstance(out, tuple) else out
    return out.detach().float(), [tuple(t.clone() for t in blk.mlp.last_plan[:2]) for blk in model.blocks], rows


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("kind", ["top1", "distilled", "top2"])
def test_model_with_and_without_tail_rows_bit_for_bit(kind, B):
    model, images = _model(kind), _images(B)
    N, k, prefix = model.pos_embed.shape[1], model.blocks[0].mlp.top_k, model.num_tokens
    assert sm.VisionTransformer.tail_rows_only is True
    model.tail_rows_only = False
    ref, plans_ref, rows_ref = _forward(model, images)
    model.tail_rows_only = True
    got, plans, rows = _forward(model, images)
    assert rows_ref[-2:] == [B * N * k] * 2 and rows[-2:] == [B * prefix * k] * 2, (rows_ref, rows)   # the path under test ran
    assert rows[:-2] == rows_ref[:-2]                                 # ... in the last block, and only there
    assert torch.equal(got, ref)
    for (i0, s0), (i1, s1) in zip(plans_ref, plans):
        assert i0.shape == (B * N, k) and s1.shape == (B * N, k)
        assert torch.equal(i0, i1) and torch.equal(s0, s1)
    counts = model.blocks[-1].mlp.last_plan[2].cpu()
    print(kind, B, "head rows per expert:", counts.tolist())
    assert int(counts.sum()) == B * prefix * k


@pytest.mark.parametrize("case", ["capacity_gate", "compute_streams", "grad_enabled", "train_mode", "block_called_directly"])
def test_paths_that_keep_the_full_dispatch(case):
    B = 4
    model, images = _model("capacity" if case == "capacity_gate" else "top1"), _images(B)
    N = model.pos_embed.shape[1]
    want = B * N
    if case == "block_called_directly":
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            x = model._embed(images)
            x = model.blocks[0](x)
            ops.profile_begin(only=["grouped_gemm"])
            model.blocks[-1](x)
            torch.cuda.synchronize()
        rows = [int(round(m["flops"] / (2.0 * m["K"] * m["N"]))) for _, m, _ in ops.profile_end()]
    else:
        if case == "compute_streams":
            model.compute_streams, want = 2, (B // 2) * N             # each half of the batch on its own stream
        if case == "train_mode":
            model.train()
        _, _, rows = _forward(model, images, grad=case == "grad_enabled")
    assert len(rows) >= 2 and rows[-2:] == [want] * 2, (case, rows)


def _port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _force_ep_worker(q):
    import torch.distributed as dist
    from slim_switch_moe_vit_amd import ep
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_port()}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        model, images = _model("top1"), _images(4)
        for blk in model.blocks:
            blk.mlp.force_ep = True
        model.ep_micro_batches = 1
        ep.set_speculative(model, None)
        _, _, rows = _forward(model, images)
        q.put({"rows": rows, "full": 4 * model.pos_embed.shape[1]})
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_forced_expert_parallel_path_keeps_the_full_dispatch():
    """(the expert-parallel code path needs a process group: a one-rank group in a child process, as the other EP tests)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_force_ep_worker, args=(q,))
    p.start()
    _join_or_kill([p], 120)
    res = q.get(timeout=10)
    # every token's row reaches the experts (the exchange buffers may hold more rows than tokens; the head rows alone would be 4)
    assert len(res["rows"]) >= 2 and min(res["rows"][-2:]) >= res["full"], res


# ---------------------------------------------------------------------------------------------- the launches
# rows per group of the pruned GEMMs' kind: 1, 31, 32, 33 and 129, with empty groups between and at the end
_GROUP_ROWS = [1, 0, 31, 32, 0, 33, 129, 0]


@pytest.fixture(scope="module")
def pruned_gemm_operands():
    g = torch.Generator().manual_seed(77)
    E, d, h, T = len(_GROUP_ROWS), 768, 3072, 1000
    M = sum(_GROUP_ROWS)
    return dict(
        E=E, d=d, h=h, T=T, M=M,
        xn16=(torch.randn(T, d, generator=g)).half().to(DEV),
        w1=(torch.randn(E, h, d, generator=g) * 0.03).half().to(DEV), b1=(torch.randn(E, h, generator=g) * 0.1).to(DEV),
        w2=(torch.randn(E, d, h, generator=g) * 0.03).half().to(DEV), b2=(torch.randn(E, d, generator=g) * 0.1).to(DEV),
        resid=torch.randn(T, d, generator=g).to(DEV), score=(torch.rand(T, generator=g) * 0.5 + 0.5).to(DEV),
        pos=torch.randperm(T, generator=g)[:M].to(torch.int64).to(DEV),
        offsets=torch.tensor(np.concatenate([[0], np.cumsum(_GROUP_ROWS)]), dtype=torch.int32, device=DEV))


def test_pruned_gemm_rows_do_not_depend_on_the_tile_height(pruned_gemm_operands):
    """The whole batch's launches run 320-row tiles, the head rows' launches 256-row tiles (the tile rule, rows = 256, 8 groups):
    both, and the rule's own choice (variant 9), give the same bits -- gathered GELU GEMM-1 (K 768), and GEMM-2 (K 3072) with
    bias, combine scale, row map and residual in its epilogue.  So does the 128 x 128 one-workgroup-per-tile kernel (variant 1) that
    the head rows' GEMM-2 runs on."""
    o = pruned_gemm_operands
    lib = sm._lib.load()
    assert lib.smoe_grouped_gemm_plan(256, o["E"], o["d"], o["h"]) == 11      # GEMM-1 of 256 head rows: 256-row tiles
    assert lib.smoe_grouped_gemm_plan(256, o["E"], o["h"], o["d"]) == 12      # GEMM-2: 256-row tiles, deep
    assert lib.smoe_grouped_gemm_plan(50432, o["E"], o["d"], o["h"]) == 10    # the whole batch: 320-row tiles
    assert lib.smoe_grouped_gemm_plan(50432, o["E"], o["h"], o["d"]) == 13
    hs = [ops.grouped_gemm(o["xn16"], o["w1"], o["b1"], o["offsets"], ops.EPI_GELU, torch.float16, variant=v, a_gather=o["pos"])
          for v in (9, 10, 11)]
    assert hs[0].shape == (o["M"], o["h"]) and torch.equal(hs[0], hs[1]) and torch.equal(hs[0], hs[2])
    ref = torch.nn.functional.gelu(o["xn16"][o["pos"][:1]].float() @ o["w1"][0].float().t() + o["b1"][0])
    assert float((hs[0][:1].float() - ref).abs().max()) <= 2e-2 * max(1.0, float(ref.abs().max()))   # (not all zeros: group 0's row)
    outs = []
    for v in (9, 12, 13, 1):
        out = o["resid"].clone()
        ops.grouped_gemm(hs[0], o["w2"], o["b2"], o["offsets"], ops.EPI_NONE, torch.float32, row_map=o["pos"], row_scale=o["score"],
                         out=out, variant=v, residual=out)            # in place over the residual image, as the model does
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.equal(outs[0], outs[3])
    untouched = torch.ones(o["T"], dtype=torch.bool, device=DEV)
    untouched[o["pos"]] = False
    assert torch.equal(outs[0][untouched], o["resid"][untouched]) and not torch.equal(outs[0][~untouched], o["resid"][~untouched])
