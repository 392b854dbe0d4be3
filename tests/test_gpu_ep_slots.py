"""Kernel-level tests of the static expert exchange's device-side protocol (run with -m gpu): the slot plan
(smoe_dispatch_plan_slots), the in-band headers (smoe_ep_pack_headers / smoe_ep_unpack_headers), the row-range pieces of the
training path (smoe_split_offsets, ops.split_ranges, ops.grouped_wgrad_rows_split) and the whole data path replayed on simulated
ranks, each against the plain loops of oracle/moe_oracle.py.

Bars: every integer output bit for bit; buffers byte for byte.  Outputs are handed to the C ABI pre-filled with a sentinel, so
an entry the kernel never wrote cannot pass by luck.  Float outputs: the bars of the tests this file is the twin of
(test_expert_parallel_data_path_simulated_ranks: 1e-3; test_grouped_wgrad_rows_matches_per_expert_matmul: 2e-3 / 1.5e-2)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import moe_oracle as mo  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import _lib, ops  # noqa: E402
from _mp import float_bar as _float_bar  # noqa: E402
from test_gpu_parity import _gen, _load_module, _mk  # noqa: E402

DEV = "cuda:0"
SENT = -7          # what every output holds before the call
GUARD = 8          # sentinel entries in front of and behind pos_slots: the plan writes inside [0, slot_base[E]) only


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sent(n, dtype):
    return torch.full((int(n),), SENT, dtype=dtype, device=DEV)


def _i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int32), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------ slot plan
def _plan_slots(idx, E, base, hdr_rows, capacity):
    """smoe_dispatch_plan_slots through the C ABI on sentinel-filled outputs -> numpy arrays named like mo.SlotPlan's fields."""
    lib = _lib.load()
    idx = np.array(idx, dtype=np.int64)                      # (a writable copy: the cached routings are read-only)
    n, n_slots = idx.size, int(base[-1])
    idx_d, base_d = torch.from_numpy(idx).to(DEV), _i32(base)
    ws_bytes = lib.smoe_dispatch_plan_workspace_bytes(n, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    counts, offsets, gend, raw = _sent(E, torch.int32), _sent(E + 1, torch.int32), _sent(E, torch.int32), _sent(E, torch.int32)
    inv, pruned = _sent(n, torch.int64), _sent(n, torch.int64)
    guarded = _sent(n_slots + 2 * GUARD, torch.int64)
    pos = guarded[GUARD:GUARD + n_slots]
    rc = lib.smoe_dispatch_plan_slots(_ptr(idx_d), n, E, int(capacity), _ptr(base_d), int(hdr_rows), _ptr(counts), _ptr(offsets),
                                      _ptr(gend), pos.data_ptr(), _ptr(inv), _ptr(pruned), _ptr(raw), _ptr(ws), ws_bytes, None)
    _lib.check(rc, "smoe_dispatch_plan_slots")
    torch.cuda.synchronize()
    g = guarded.cpu().numpy()
    assert np.all(g[:GUARD] == SENT) and np.all(g[GUARD + n_slots:] == SENT), "the plan wrote outside pos_slots"
    return dict(counts=counts.cpu().numpy(), offsets=offsets.cpu().numpy(), group_end=gend.cpu().numpy(),
                pos_slots=g[GUARD:GUARD + n_slots], inv_pos=inv.cpu().numpy(), idx_pruned=pruned.cpu().numpy(),
                raw_counts=raw.cpu().numpy())


def _assert_plan(got, want):
    for name in ("raw_counts", "counts", "offsets", "group_end", "idx_pruned", "inv_pos", "pos_slots"):
        g, w = got[name], getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, int((g != w).sum()), np.nonzero(g != w)[0][:8].tolist())


@functools.lru_cache(maxsize=None)
def _routing(n, E):
    """-1 entries, one overloaded expert (as test_dispatch_plan_bit_exact builds it) -> (idx, raw counts)."""
    rng = np.random.default_rng(n + E)
    idx = rng.integers(-1, E, size=n).astype(np.int64)
    idx[rng.random(n) < 0.3] = 0
    idx.setflags(write=False)
    raw = np.bincount(idx[idx >= 0], minlength=E).astype(np.int64)
    raw.setflags(write=False)
    return idx, raw


def _caps(pattern, raw, n):
    E = raw.size
    if pattern == "roomy":
        return raw + 5
    if pattern == "exact":                       # no drops, and no unused payload slot where raw >= 1
        return np.maximum(raw, 1)
    if pattern == "one_short":                   # every second expert drops exactly its last entry (if it has two or more)
        return np.where(np.arange(E) % 2 == 1, np.maximum(raw - 1, 1), np.maximum(raw, 1))
    assert pattern == "uneven"                   # what _SlotState.fitted_caps installs, e.g. [12, 7, 7, ...], scaled to n
    unit = max(1, n // (8 * E))
    return np.array([12 * unit] + [7 * unit] * (E - 1), dtype=np.int64)


PLAN_SHAPES = [(1, 4), (63, 6), (1024, 8), (1025, 12), (4097, 27), (3000, 64), (9000, 20), (50432, 8)]


@pytest.mark.parametrize("with_capacity", [False, True])
@pytest.mark.parametrize("hdr_rows", [0, 1])
@pytest.mark.parametrize("pattern", ["roomy", "exact", "one_short", "uneven"])
@pytest.mark.parametrize("n,E", PLAN_SHAPES)
def test_slot_plan_bit_exact(n, E, pattern, hdr_rows, with_capacity):
    """One chunk and many, a partial last chunk, E that divides the 256 threads (private sums) and E that does not (LDS atomics);
    regions of caps + hdr_rows rows; optionally a gate capacity below the largest cap on top of the slots."""
    idx, raw = _routing(n, E)
    caps = _caps(pattern, raw, n)
    base = np.concatenate([[0], np.cumsum(caps + hdr_rows)])
    capacity = int(caps.max()) // 2 if with_capacity else -1
    want = mo.dispatch_plan_slots(idx, E, base, hdr_rows, capacity)
    if not with_capacity:                         # the patterns are what their names say (a check of this test's own inputs)
        dropped = int(want.raw_counts.sum() - want.counts.sum())
        if pattern in ("roomy", "exact"):
            assert dropped == 0
        if pattern == "exact":
            payload = np.concatenate([want.pos_slots[base[e]:base[e] + caps[e]] for e in range(E) if raw[e] >= 1])
            assert np.all(payload >= 0)
        if pattern == "one_short":
            assert dropped == int(((np.arange(E) % 2 == 1) & (raw >= 2)).sum())
    _assert_plan(_plan_slots(idx, E, base, hdr_rows, capacity), want)


@pytest.mark.parametrize("bad", [12, 17, 1 << 40, -2, -100, -(1 << 40)])
@pytest.mark.parametrize("n,E", [(1025, 12), (3000, 64)])
def test_slot_plan_drops_ids_outside_the_experts_uncounted(n, E, bad):
    idx, _ = _routing(n, E)
    idx = idx.copy()
    idx[np.random.default_rng(7).random(n) < 0.05] = bad if bad < 0 or bad >= E else E + bad
    idx[0] = idx[n - 1] = idx[1023] = bad if bad < 0 or bad >= E else E + bad
    raw = np.bincount(idx[(idx >= 0) & (idx < E)], minlength=E)
    for hdr_rows in (0, 1):
        base = np.concatenate([[0], np.cumsum(_caps("one_short", raw, n) + hdr_rows)])
        want = mo.dispatch_plan_slots(idx, E, base, hdr_rows)
        assert np.array_equal(want.raw_counts, raw)
        _assert_plan(_plan_slots(idx, E, base, hdr_rows, -1), want)


@pytest.mark.parametrize("hdr_rows,base", [(0, [0, 5, 5, 9, 20]),        # expert 1: an empty region
                                           (1, [0, 6, 7, 12, 23]),       # expert 1: a header row and nothing else
                                           (1, [0, 6, 6, 12, 23]),       # not even that
                                           (0, [0, 0, 4, 4, 9])])        # first and third empty
def test_slot_plan_region_without_payload_keeps_nothing(hdr_rows, base):
    E = 4
    idx = np.array([1, 0, 1, 2, 3, 1, 0, 2, 3, 3, 1, 0, -1, 2, 0, 0, 3, 2, 1, 0, 3, 3, 3], dtype=np.int64)
    base = np.array(base)
    want = mo.dispatch_plan_slots(idx, E, base, hdr_rows)
    got = _plan_slots(idx, E, base, hdr_rows, -1)
    for e in range(E):
        if base[e + 1] - base[e] - hdr_rows <= 0:
            assert got["counts"][e] == 0 and got["group_end"][e] == base[e] and np.all(got["idx_pruned"][idx == e] == -1)
            assert got["raw_counts"][e] == (idx == e).sum() > 0
    _assert_plan(got, want)


# ------------------------------------------------------------------------------------------ fused-table boundary
def _boundary_idx(n, E=64):
    rng = np.random.default_rng(n)
    idx = rng.integers(-1, E, size=n).astype(np.int64)
    idx[rng.random(n) < 0.1] = 0
    return idx


@pytest.mark.parametrize("n", [131072, 131073])
def test_compact_plan_on_both_sides_of_the_fused_table_limit(n):
    """E = 64: 128 chunks x 64 = 8192 table entries is the last size of the fused assign kernel, n = 131073 the first that takes
    the count / scan / assign / tail launches.  Both equal the oracle."""
    E = 64
    idx = _boundary_idx(n)
    for cap in (-1, 1500):
        counts, offsets, pos, inv_pos, pruned = ops.dispatch_plan(torch.from_numpy(idx).to(DEV), E, cap, want_pruned=True)
        p = mo.dispatch_plan(idx, E, cap)
        assert np.array_equal(counts.cpu().numpy(), p.counts) and np.array_equal(offsets.cpu().numpy(), p.offsets)
        assert np.array_equal(pos.cpu().numpy(), p.pos)
        assert np.array_equal(inv_pos.cpu().numpy(), p.inv_pos)
        assert np.array_equal(pruned.cpu().numpy(), p.idx_pruned)


def _padded_want(idx, E, cap, slot):
    p = mo.dispatch_plan(idx, E, cap)
    want_pos = np.full(E * slot, -1, dtype=np.int64)
    want_inv = np.full(idx.size, -1, dtype=np.int64)
    for e in range(E):
        seg = p.pos[p.offsets[e]:p.offsets[e + 1]]
        want_pos[e * slot:e * slot + len(seg)] = seg
        want_inv[seg] = e * slot + np.arange(len(seg))
    return p, want_pos, want_inv


def test_slot_and_padded_plans_at_the_last_fused_size_and_refused_beyond_it():
    E, n = 64, 131072
    idx = _boundary_idx(n)
    raw = np.bincount(idx[idx >= 0], minlength=E)
    base = np.concatenate([[0], np.cumsum(_caps("one_short", raw, n) + 1)])
    _assert_plan(_plan_slots(idx, E, base, 1, -1), mo.dispatch_plan_slots(idx, E, base, 1))
    cap, slot = 1500, 1503
    counts, offsets, gend, pos_pad, inv_pos, pruned, raw_d = ops.dispatch_plan_padded(torch.from_numpy(idx).to(DEV), E, cap, slot,
                                                                                      want_raw=True)
    p, want_pos, want_inv = _padded_want(idx, E, cap, slot)
    assert np.array_equal(counts.cpu().numpy(), p.counts) and np.array_equal(raw_d.cpu().numpy(), raw)
    assert np.array_equal(gend.cpu().numpy(), np.arange(E) * slot + p.counts)
    assert np.array_equal(pos_pad.cpu().numpy(), want_pos) and np.array_equal(inv_pos.cpu().numpy(), want_inv)
    assert np.array_equal(pruned.cpu().numpy(), p.idx_pruned)
    # one entry more, or one expert more, and the padded layouts are refused (before any launch), naming the limit
    for n_bad, E_bad in ((131073, 64), (1000, 65)):
        idx_bad = torch.from_numpy(_boundary_idx(n_bad, E_bad)).to(DEV)
        base_bad = _i32(np.arange(E_bad + 1) * 4000)
        with pytest.raises(_lib.SlimMoEError, match=r"E <= 64 and ceil\(n / 1024\) \* E <= 8192"):
            ops.dispatch_plan_slots(idx_bad, E_bad, base_bad, E_bad * 4000)
        with pytest.raises(_lib.SlimMoEError, match=r"E <= 64 and ceil\(n / 1024\) \* E <= 8192"):
            ops.dispatch_plan_padded(idx_bad, E_bad, 100, 100)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,E,cap", [(50432, 8, 6304), (3000, 8, 100), (777, 4, 1000), (4097, 27, 90), (5000, 16, 1)])
def test_padded_plan_raw_counts_are_the_unclamped_histogram(n, E, cap):
    """smoe_dispatch_plan_padded's raw_counts (what the capacity gate's overflow watch reads): np.bincount of the valid ids,
    whatever the clamp keeps; the layout beside it as test_dispatch_plan_padded_layout_bit_exact states it."""
    lib = _lib.load()
    slot = cap + (n % 3) * 5
    idx, raw = _routing(n, E)
    idx_d = torch.from_numpy(idx.copy()).to(DEV)
    ws_bytes = lib.smoe_dispatch_plan_workspace_bytes(n, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    counts, offsets, gend, raw_d = _sent(E, torch.int32), _sent(E + 1, torch.int32), _sent(E, torch.int32), _sent(E, torch.int32)
    pos, inv, pruned = _sent(E * slot, torch.int64), _sent(n, torch.int64), _sent(n, torch.int64)
    rc = lib.smoe_dispatch_plan_padded(_ptr(idx_d), n, E, cap, slot, _ptr(counts), _ptr(offsets), _ptr(gend), _ptr(pos), _ptr(inv),
                                       _ptr(pruned), _ptr(raw_d), _ptr(ws), ws_bytes, None)
    _lib.check(rc, "smoe_dispatch_plan_padded")
    p, want_pos, want_inv = _padded_want(idx, E, cap, slot)
    assert np.array_equal(raw_d.cpu().numpy(), raw.astype(np.int32))
    assert np.array_equal(counts.cpu().numpy(), np.minimum(raw, cap)) and np.array_equal(counts.cpu().numpy(), p.counts)
    assert np.array_equal(offsets.cpu().numpy(), p.offsets)
    assert np.array_equal(gend.cpu().numpy(), np.arange(E) * slot + p.counts)
    assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(inv.cpu().numpy(), want_inv)
    assert np.array_equal(pruned.cpu().numpy(), p.idx_pruned)


# ------------------------------------------------------------------------------------------ headers
def _uneven_caps(G, seed=0):
    return [1 + (5 * g + 3 * seed) % 7 + (11 if g == 0 else 0) for g in range(G)]      # [12, 6, 4, 2, 7, ...]


def _pattern_bytes(rows, row_bytes):
    return ((np.arange(rows * row_bytes, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8).reshape(rows, row_bytes)


def _pack(buf_np, counts, raw, base, t_rows):
    """smoe_ep_pack_headers through the C ABI on a uint8 buffer [rows, row_bytes] -> the buffer afterwards."""
    buf = torch.from_numpy(buf_np.copy()).to(DEV)
    c = None if counts is None else _i32(counts)
    r = None if raw is None else _i32(raw)
    base_d = _i32(base)
    rc = _lib.load().smoe_ep_pack_headers(_ptr(c), _ptr(r), _ptr(base_d), len(base) - 1, buf_np.shape[1], int(t_rows), _ptr(buf), None)
    _lib.check(rc, "smoe_ep_pack_headers")
    return buf.cpu().numpy()


@pytest.mark.parametrize("form", ["counts_and_raw", "raw_none", "no_rows"])
@pytest.mark.parametrize("G", [1, 4, 8, 32, 64])
def test_pack_headers_writes_its_words_and_nothing_else(G, form):
    """The wire format {kept, raw, T, G, raw[0 .. G)}: 4 + G int32 words at the start of each region's last row.  Rows exactly
    as wide as a header (16 + 4 G bytes) and rows of d = 192 elements in f16, bf16 and f32; the WHOLE buffer is compared."""
    caps = _uneven_caps(G)
    base = np.concatenate([[0], np.cumsum(np.array(caps) + 1)])
    rng = np.random.default_rng(G)
    raw = rng.integers(0, 40, size=G).astype(np.int32)
    raw[G // 2] = 0
    counts = np.minimum(raw, np.array(caps)).astype(np.int32)
    c, r, t_rows = {"counts_and_raw": (counts, raw, 1234), "raw_none": (counts, None, 77), "no_rows": (None, None, 0)}[form]
    buf = _pattern_bytes(int(base[-1]), 16 + 4 * G)
    assert np.array_equal(_pack(buf, c, r, base, t_rows), mo.pack_headers_ref(buf, c, r, base, t_rows))
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        row_bytes = 192 * torch.empty(0, dtype=dtype).element_size()
        buf = _pattern_bytes(int(base[-1]), row_bytes)
        send = torch.from_numpy(buf.copy()).to(DEV).view(dtype)
        assert tuple(send.shape) == (int(base[-1]), 192)
        ops.ep_pack_headers(send, None if c is None else _i32(c), None if r is None else _i32(r), _i32(base), t_rows)
        want = mo.pack_headers_ref(buf, c, r, base, t_rows)
        assert np.array_equal(send.view(torch.uint8).cpu().numpy(), want)
        hdr = want[base[1:] - 1]
        assert np.array_equal(hdr[:, 4 * (4 + G):], buf[base[1:] - 1][:, 4 * (4 + G):])        # (the reference itself: 4 + G words)


def _recv_buffer(W, lb, E_total, row_bytes, kinds_at, seed):
    """A received buffer in numpy: source w's block holds the regions of ``lb``; every header {count, raw, T_w, E_total, raw_w};
    the counts cycle through 0, the full region, a negative value and a value above the region, starting at ``kinds_at``."""
    rng = np.random.default_rng(seed)
    E_local, block = len(lb) - 1, int(lb[-1])
    buf = rng.integers(0, 256, size=(W * block, row_bytes), dtype=np.uint8)
    T = rng.integers(0, 5000, size=W).astype(np.int32)
    raw = rng.integers(0, 900, size=(W, E_total)).astype(np.int32)
    for w in range(W):
        for e in range(E_local):
            room = int(lb[e + 1] - lb[e]) - 1
            count = [0, room, -1 - (w + e) * 1000, room + 1 + (w + e) * 100000][(kinds_at + w * E_local + e) % 4]
            words = np.concatenate([[count, raw[w, e % E_total], T[w], E_total], raw[w]]).astype("<i4")
            buf[w * block + int(lb[e + 1]) - 1, :4 * words.size] = words.view(np.uint8)
    return buf, T, raw


def _unpack(buf_np, W, lb, E_total, with_stats=True):
    """smoe_ep_unpack_headers through the C ABI on sentinel-filled outputs."""
    G = W * (len(lb) - 1)
    recv = torch.from_numpy(buf_np).to(DEV)
    starts, ends = _sent(G, torch.int32), _sent(G, torch.int32)
    stats = _sent(W * (1 + E_total), torch.int32) if with_stats else None
    lb_d = _i32(lb)
    rc = _lib.load().smoe_ep_unpack_headers(_ptr(recv), W, len(lb) - 1, _ptr(lb_d), buf_np.shape[1], E_total, _ptr(starts), _ptr(ends),
                                            _ptr(stats), None)
    _lib.check(rc, "smoe_ep_unpack_headers")
    return starts.cpu().numpy(), ends.cpu().numpy(), None if stats is None else stats.cpu().numpy().reshape(W, 1 + E_total)


@pytest.mark.parametrize("E_local", [1, 2, 4])
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_unpack_headers_ranges_clamp_and_stats(W, E_local):
    """starts / ends of every (source, local expert) group and the [W, 1 + E] stats matrix; a count outside its region (negative,
    or above the payload rows) is clamped to [0, region - 1] -- the kernel's own defence against a corrupt header."""
    E_total = W * E_local
    lb = np.concatenate([[0], np.cumsum(np.array(_uneven_caps(E_local, seed=W)) + 1)])
    for row_bytes in (16 + 4 * E_total, 384):
        for kinds_at in range(4):
            buf, T, raw = _recv_buffer(W, lb, E_total, row_bytes, kinds_at, seed=W * 10 + E_local)
            want_s, want_e, want_stats = mo.unpack_headers_ref(buf, W, lb, E_total)
            assert np.array_equal(want_stats, np.concatenate([T[:, None], raw], axis=1))      # (the reference itself)
            assert np.all(want_e >= want_s) and np.all(want_e - want_s <= np.tile(np.diff(lb) - 1, W))
            starts, ends, stats = _unpack(buf, W, lb, E_total)
            assert np.array_equal(starts, want_s) and np.array_equal(ends, want_e), (row_bytes, kinds_at)
            assert np.array_equal(stats, want_stats), (row_bytes, kinds_at)


def test_unpack_headers_foreign_expert_count_and_null_stats():
    """A header written for another expert count (word 3 != E_total) gives no routing histogram (-1) but still its row count;
    stats = NULL is accepted and changes nothing else."""
    W, E_local, E_total = 4, 2, 8
    lb = np.array([0, 5, 14])
    buf, T, raw = _recv_buffer(W, lb, E_total, 64, 1, seed=3)
    for w in (1, 3):
        buf[w * 14 + 4].view("<i4")[3] = E_total + (1 if w == 1 else -1)
    want_s, want_e, want_stats = mo.unpack_headers_ref(buf, W, lb, E_total)
    assert np.all(want_stats[[1, 3], 1:] == -1) and np.array_equal(want_stats[:, 0], T) and np.array_equal(want_stats[[0, 2], 1:], raw[[0, 2]])
    starts, ends, stats = _unpack(buf, W, lb, E_total)
    assert np.array_equal(stats, want_stats)
    assert np.array_equal(starts, want_s) and np.array_equal(ends, want_e)
    starts, ends, none = _unpack(buf, W, lb, E_total, with_stats=False)
    assert none is None and np.array_equal(starts, want_s) and np.array_equal(ends, want_e)


def _exchange(bufs, tables, forward=True):
    """The all-to-all by hand: bufs[src] is split by the table's in_splits (forward; out_splits backward), destination dst gets
    the pieces in source order."""
    W = len(bufs)
    out = []
    for dst in range(W):
        pieces = []
        for src in range(W):
            splits = tables[src].in_splits if forward else tables[src].out_splits
            lo = sum(splits[:dst])
            pieces.append(bufs[src][lo:lo + splits[dst]])
            assert splits[dst] == (tables[dst].out_splits if forward else tables[dst].in_splits)[src]
        out.append(torch.cat(pieces, 0))
    return out


@pytest.mark.parametrize("W,E_local", [(1, 4), (2, 3), (4, 2), (8, 1), (8, 4)])
def test_headers_round_trip_over_simulated_ranks(W, E_local):
    """Every rank plans its own routing into its _SlotTable send buffer and packs the headers; after the exchange every
    destination finds the expected row ranges, and the SAME stats matrix [T_w, raw_w] as every other destination."""
    from slim_switch_moe_vit_amd import ep
    E = W * E_local
    caps = _uneven_caps(E, seed=W)
    n_r = [300, 0, 1, 77, 512, 64, 5, 129][:W]
    tables = [ep._SlotTable(caps, r, E_local, DEV) for r in range(W)]
    base = np.concatenate([[0], np.cumsum(np.array(caps) + 1)])
    sends, plans = [], []
    for r in range(W):
        tab = tables[r]
        assert tab.base_dev.cpu().tolist() == base.tolist()
        send = torch.from_numpy(_pattern_bytes(tab.rows, 384)).to(DEV).view(torch.float16)
        idx = np.random.default_rng(100 * W + r).integers(-1, E, size=n_r[r]).astype(np.int64)
        idx[: n_r[r] // 3] = r % E                              # a group larger than its slot: kept < raw
        want = mo.dispatch_plan_slots(idx, E, base, 1)
        plans.append(want)
        if n_r[r] > 0:
            counts, _, _, _, _, _, raw = ops.dispatch_plan_slots(torch.from_numpy(idx).to(DEV), E, tab.base_dev, tab.rows)
            assert np.array_equal(counts.cpu().numpy(), want.counts) and np.array_equal(raw.cpu().numpy(), want.raw_counts)
        else:
            counts = raw = None                                 # a rank without rows: the counts = NULL header form
        ops.ep_pack_headers(send, counts, raw, tab.base_dev, n_r[r])
        sends.append(send)
    assert any((p.counts < p.raw_counts).any() for p in plans)
    want_stats = np.stack([np.concatenate([[n_r[r]], plans[r].raw_counts]) for r in range(W)])
    recvs = _exchange(sends, tables)
    for dst in range(W):
        tab = tables[dst]
        assert recvs[dst].shape[0] == tab.recv_rows
        starts, ends, stats = ops.ep_unpack_headers(recvs[dst], W, tab.lbase_dev, E)
        lb = np.array(tab.lbase_dev.cpu().tolist())
        want_s = np.concatenate([w * lb[-1] + lb[:-1] for w in range(W)])
        kept = np.concatenate([plans[w].counts[dst * E_local:(dst + 1) * E_local] for w in range(W)])
        assert np.array_equal(starts.cpu().numpy(), want_s)
        assert np.array_equal(ends.cpu().numpy(), want_s + kept)
        assert np.array_equal(stats.cpu().numpy(), want_stats)


# ------------------------------------------------------------------------------------------ data path on simulated ranks
@pytest.mark.parametrize("slots", ["roomy", "tight"])
@pytest.mark.parametrize("W_ranks,E_local,k,d,h,T_r", [(2, 4, 1, 192, 768, [700, 0]),
                                                       (4, 2, 2, 192, 768, [333, 0, 1, 512]),
                                                       (8, 1, 1, 192, 768, [700, 333, 1, 512, 0, 900, 257, 128]),
                                                       (2, 3, 2, 192, 768, [1, 640])])
def test_static_exchange_data_path_simulated_ranks(W_ranks, E_local, k, d, h, T_r, slots):
    """The static twin of test_expert_parallel_data_path_simulated_ranks: every rank's side of ep._ep_forward_static replayed
    on one GPU.  HIP router -> slot plan -> scatter into a send buffer pre-filled with NaN (unused slots are poison) -> headers
    -> exchange by hand -> unpack -> expert FFN on the received row ranges -> exchange back -> gather + combine.  Roomy slots:
    the oracle's single-rank forward of every shard.  Tight uniform slots c: the oracle's forward with capacity c (a rank
    keeps at most c of its rows per global expert), with entries dropped and slots left partly empty in the same run."""
    from slim_switch_moe_vit_amd import ep
    E = W_ranks * E_local
    cd = torch.float16
    _, wg, bg, w1, b1, w2, b2 = _mk(1, d, h, E, seed=700 + W_ranks + k)
    xs = [torch.randn(t, d, generator=_gen(800 + r)) for r, t in enumerate(T_r)]
    raws = [np.bincount(mo.naive_gate(x, wg, bg, k)[0].reshape(-1).numpy(), minlength=E) if x.shape[0] else np.zeros(E, dtype=np.int64)
            for x in xs]
    if slots == "roomy":
        caps, capacity = (np.max(raws, axis=0) + 5).tolist(), -1
    else:
        big = raws[int(np.argmax(T_r))]
        c = max(1, (int(big.min()) + int(big.max())) // 2)
        assert big.max() > c > big.min(), "the largest shard must overflow one slot and leave another partly empty"
        caps, capacity = [c] * E, c
    mods = []
    for r in range(W_ranks):   # rank r holds the gate for all E experts and the weights of its E_local experts
        m = sm.FMoETransformerMLP(E_local, d, h, torch.nn.GELU(), top_k=k, world_size=W_ranks, compute_dtype=cd)
        sl = slice(r * E_local, (r + 1) * E_local)
        mods.append(_load_module(m, wg, bg, w1[sl], b1[sl], w2[sl], b2[sl]))
    tables = [ep._SlotTable(caps, r, E_local, DEV) for r in range(W_ranks)]
    # sender side
    sends, invs, scores = [], [], []
    dropped = partly_empty = 0
    for r in range(W_ranks):
        tab, T = tables[r], T_r[r]
        send = torch.full((tab.rows, d), float("nan"), dtype=cd, device=DEV)
        if T > 0:
            x = xs[r].to(DEV)
            idx, score, _, _ = ops.router_topk(x, wg.to(DEV), bg.to(DEV), k, ops.GATE_NAIVE)
            counts, _, _, pos, inv_pos, _, raw = ops.dispatch_plan_slots(idx, E, tab.base_dev, tab.rows)
            assert np.array_equal(raw.cpu().numpy(), raws[r]), "routing must be the oracle's"
            ops.scatter_rows(x, pos, k, cd, out=send)
            dropped += int((raw - counts).sum())
            partly_empty += int((counts.cpu() < torch.tensor(tab.caps)).sum())
        else:
            counts = raw = inv_pos = score = None
        ops.ep_pack_headers(send, counts, raw, tab.base_dev, T)
        sends.append(send)
        invs.append(inv_pos)
        scores.append(score)
    if slots == "tight":
        assert dropped > 0 and partly_empty > 0
    else:
        assert dropped == 0
    # the exchange, the experts, the exchange back
    recvs = _exchange(sends, tables)
    ys, all_stats = [], []
    for dst in range(W_ranks):
        tab = tables[dst]
        starts, ends, stats = ops.ep_unpack_headers(recvs[dst], W_ranks, tab.lbase_dev, E)
        all_stats.append(stats.cpu())
        gexp = ep._group_expert_ids(W_ranks, E_local, torch.device(DEV))
        ys.append(mods[dst]._experts_fwd(recvs[dst], starts, cd, out_dtype=cd, group_expert=gexp, group_end=ends))
    for s in all_stats:
        assert torch.equal(s, all_stats[0]) and s[:, 0].tolist() == T_r and np.array_equal(s[:, 1:].numpy(), np.stack(raws))
    backs = _exchange(ys, tables, forward=False)
    for r in range(W_ranks):
        T = T_r[r]
        assert backs[r].shape[0] == tables[r].rows
        if T == 0:
            continue
        got = ops.gather_combine(backs[r], invs[r], scores[r], T, k, torch.float32).cpu()
        assert torch.isfinite(got).all(), "a poisoned (unused) slot reached the output"
        ref = mo.moe_forward(xs[r], wg, bg, w1, b1, w2, b2, k, capacity=capacity).out
        _float_bar(got, ref, 1e-3)


# ------------------------------------------------------------------------------------------ row ranges of the training path
SPLIT_COUNTS = [0, 1, 63, 64, 65, 128, 700, 513]


def _split_rule(counts, S):
    """The documented rule, per group: ceil(count / 64) whole 64-row chunks dealt to S pieces, ceil(chunks / S) each, the last
    pieces taking what is left (possibly nothing) -> piece boundaries relative to the group's start, [G, S + 1]."""
    cuts = np.zeros((len(counts), S + 1), dtype=np.int64)
    for g, cnt in enumerate(counts):
        chunks = -(-cnt // 64)
        per = -(-chunks // S)
        for s in range(S + 1):
            cuts[g, s] = min(s * per * 64, cnt)
    return cuts


@pytest.mark.parametrize("S", [1, 2, 3, 7, 16])
def test_split_offsets_and_split_ranges_follow_the_chunk_rule(S):
    counts = SPLIT_COUNTS
    G = len(counts)
    cuts = _split_rule(counts, S)
    assert np.all(cuts[:, 0] == 0) and np.array_equal(cuts[:, -1], counts) and np.all(np.diff(cuts, axis=1) >= 0)   # a partition
    inner = cuts[:, 1:-1]
    assert np.all((inner % 64 == 0) | (inner == np.array(counts)[:, None]))
    # contiguous groups
    offsets = np.concatenate([[0], np.cumsum(counts)])
    out = _sent(G * S + 1, torch.int32)
    offsets_d = _i32(offsets)
    rc = _lib.load().smoe_split_offsets(_ptr(offsets_d), G, S, _ptr(out), None)
    _lib.check(rc, "smoe_split_offsets")
    want = np.concatenate([(offsets[:-1, None] + cuts[:, :-1]).reshape(-1), [offsets[-1]]])
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(ops.split_offsets(_i32(offsets), S).cpu().numpy(), want)
    # the same cut points on ranges with gaps (the static exchange's slots)
    starts = np.concatenate([[3], 3 + np.cumsum(np.array(counts[:-1]) + np.arange(1, G) * 5)])
    ends = starts + np.array(counts)
    s0, e0 = ops.split_ranges(_i32(starts), _i32(ends), S)
    assert s0.dtype == torch.int32 and e0.dtype == torch.int32
    assert np.array_equal(s0.cpu().numpy(), (starts[:, None] + cuts[:, :-1]).reshape(-1))
    assert np.array_equal(e0.cpu().numpy(), (starts[:, None] + cuts[:, 1:]).reshape(-1))


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.5e-2)])
@pytest.mark.parametrize("S", [2, 5])
def test_grouped_wgrad_rows_split_matches_per_group_matmul(S, dtype, tol):
    """Both forms of the split weight gradient against the per-group fp64 P^T Q: contiguous groups (split_offsets), and separate
    row ranges inside a padded buffer (group_end) whose rows outside the ranges hold NaN.  Bars: those of
    test_grouped_wgrad_rows_matches_per_expert_matmul."""
    counts, R1, R2 = [700, 0, 513, 64, 1, 320], 128, 256
    G, n = len(counts), sum(counts)
    g = _gen(n + S)
    P = (torch.randn(n, R1, generator=g) * 0.5).to(dtype)
    Q = (torch.randn(n, R2, generator=g) * 0.5).to(dtype)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    refs = [P[offsets[e]:offsets[e + 1]].double().t() @ Q[offsets[e]:offsets[e + 1]].double() for e in range(G)]

    def check(got, what):
        assert tuple(got.shape) == (G, R1, R2) and got.dtype == torch.float32
        for e in range(G):
            err = (got[e].double() - refs[e]).abs().max().item()
            assert err <= tol * max(1.0, refs[e].abs().max().item()), (what, e, err)     # (NaN fails the comparison)

    check(ops.grouped_wgrad_rows_split(P.to(DEV), Q.to(DEV), _i32(offsets), S).cpu(), "contiguous")
    # the same groups spread over a padded buffer: group e at rows [starts[e], starts[e] + counts[e]), NaN everywhere else
    gaps = [3, 70, 1, 64, 129, 5]
    starts = np.cumsum([gaps[0]] + [counts[e] + gaps[e + 1] for e in range(G - 1)])
    rows = int(starts[-1] + counts[-1] + 67)
    Pp = torch.full((rows, R1), float("nan"), dtype=dtype)
    Qp = torch.full((rows, R2), float("nan"), dtype=dtype)
    for e in range(G):
        Pp[starts[e]:starts[e] + counts[e]] = P[offsets[e]:offsets[e + 1]]
        Qp[starts[e]:starts[e] + counts[e]] = Q[offsets[e]:offsets[e + 1]]
    check(ops.grouped_wgrad_rows_split(Pp.to(DEV), Qp.to(DEV), _i32(starts), S, group_end=_i32(starts + np.array(counts))).cpu(),
          "row ranges")
