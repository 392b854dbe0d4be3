"""Host-side checks of the attention length sweep (tests/_attn_sweep_cases.py): the sweep covers every N in 1 .. 640 and every
N mod 16 in every instantiation, the library agrees on the range, and the float64 references the GPU sweep is judged by are right."""
import torch

import slim_switch_moe_vit_amd as sm  # noqa: F401
from slim_switch_moe_vit_amd import _lib

import _attn_sweep_cases as ac
import _skip_attn_cases as sc


def test_the_chunks_partition_1_to_640_exactly():
    assert len(ac.CHUNKS) == 10 and all(len(c) == 64 for c in ac.CHUNKS)
    flat = [N for c in ac.CHUNKS for N in c]
    assert flat == list(range(1, 641)) == list(ac.FULL_NS)
    assert list(ac.VARLEN_LENS) == list(range(1, 257))


def test_every_residue_occurs_in_every_bucket_wide_enough_to_hold_it():
    for waves in (8, 4):
        table = ac.buckets(waves)
        assert sorted(N for ns in table.values() for N in ns) == list(range(1, 641)), "every length has exactly one bucket"
        for b, ns in table.items():
            assert ns == list(range(ns[0], ns[-1] + 1)), (b, "a bucket is one run of consecutive lengths")
            if len(ns) >= 16:
                assert {N % 16 for N in ns} == set(range(16)), b
                for r in ac.RESIDUES_GUARDED:
                    assert any(N % 16 == r for N in ns), (b, r)
    table = ac.buckets()
    fwd = {b.fwd for b in table}
    assert fwd == {f"attn_fwd<{t},{k}>" for t in (4, 8, 13, 16) for k in ("exact", "masked")} | \
        {f"attn_fwd_long<{t}>" for t in (20, 30, 37, 40)}, "the twelve forward instantiations"
    for t in (4, 8, 13, 16):            # the exact kernels' buckets are 16 wide: the lengths with ceil(N / 16) == t
        ns = [N for b, n in table.items() if b.fwd == f"attn_fwd<{t},exact>" for N in n]
        assert ns == list(range(16 * t - 15, 16 * t + 1)), t
        assert {N % 16 for N in ns} == set(range(16)), t
    assert {b.bwd for b in table} == {"attn_bwd<4,4>", "attn_bwd<8,8>", "attn_bwd<13,8>", "attn_bwd<16,8>", "attn_bwd_dq+dkv"}
    assert {b.bwd for b in ac.buckets(4)} == {"attn_bwd<4,4>", "attn_bwd<8,4>", "attn_bwd<13,4>", "attn_bwd<16,4>", "attn_bwd_dq+dkv"}
    # the lengths whose backward branches on the wave count: 49 .. 256 (N <= 48 takes <4,4> either way, and so does N = 49 .. 64)
    differ = [N for N in ac.FULL_NS if ac.bucket(N, 4) != ac.bucket(N, 8)]
    assert differ == list(range(65, 257))
    # the spots the dispatch functions switch at
    for N, f, bw in ((48, "attn_fwd<4,masked>", "attn_bwd<4,4>"), (49, "attn_fwd<4,exact>", "attn_bwd<4,4>"),
                     (64, "attn_fwd<4,exact>", "attn_bwd<4,4>"), (65, "attn_fwd<8,masked>", "attn_bwd<8,8>"),
                     (192, "attn_fwd<13,masked>", "attn_bwd<13,8>"), (208, "attn_fwd<13,exact>", "attn_bwd<13,8>"),
                     (209, "attn_fwd<16,masked>", "attn_bwd<16,8>"), (241, "attn_fwd<16,exact>", "attn_bwd<16,8>"),
                     (256, "attn_fwd<16,exact>", "attn_bwd<16,8>"), (257, "attn_fwd_long<20>", "attn_bwd_dq+dkv"),
                     (320, "attn_fwd_long<20>", "attn_bwd_dq+dkv"), (321, "attn_fwd_long<30>", "attn_bwd_dq+dkv"),
                     (577, "attn_fwd_long<37>", "attn_bwd_dq+dkv"), (593, "attn_fwd_long<40>", "attn_bwd_dq+dkv")):
        assert ac.bucket(N) == (f, bw), N


def test_the_library_agrees_on_the_range():
    lib = _lib.load()
    for N, want in ((0, 0), (641, 0), (1, 1), (640, 1)):
        assert lib.smoe_attention_supported(N, 64) == want, N
        assert lib.smoe_attention_bwd_supported(N, 64) == want, N
    for N in ac.FULL_NS:
        assert lib.smoe_attention_supported(N, 64) == 1 and lib.smoe_attention_bwd_supported(N, 64) == 1, N


def test_inputs_have_one_seed_per_length_and_dtype():
    seeds = {ac.seed(N, dt) for N in ac.FULL_NS for dt in ac.DTYPES}
    assert len(seeds) == 2 * 640
    qkv, do = ac.inputs(37, torch.bfloat16)
    assert qkv.shape == (3, 37, 3, 2, 64) and do.shape == (3, 37, 128) and qkv.dtype == do.dtype == torch.bfloat16
    again, _ = ac.inputs(37, torch.bfloat16)
    assert torch.equal(qkv, again)
    other, _ = ac.inputs(38, torch.bfloat16)
    assert not torch.equal(qkv[:, :37], other[:, :37])
    # the NaN payloads are NaNs of their formats
    for dt in ac.DTYPES:
        assert torch.isnan(torch.tensor([ac.NAN16[dt]], dtype=torch.int16).view(dt)).all()
    assert torch.isnan(torch.tensor([ac.NAN32], dtype=torch.int32).view(torch.float32)).all()


def test_float64_reference_against_torch_sdpa_and_autograd():
    for N in (1, 2, 15, 16, 17, 50, 255, 257, 640):
        for dt in ac.DTYPES:
            qkv, do = ac.inputs(N, dt)
            ref = ac.reference(qkv, do)
            q, k, v = qkv.double().permute(2, 0, 3, 1, 4).unbind(0)
            sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=ac.SCALE).transpose(1, 2).reshape(3, N, 128)
            assert ref["out"].dtype == torch.float64 and (ref["out"] - sdpa).abs().max().item() <= 1e-12, N
            lse = torch.logsumexp(q @ k.transpose(-2, -1) * ac.SCALE, -1) / torch.log(torch.tensor(2.0, dtype=torch.float64))
            assert ref["lse"].shape == (3, 2, N) and (ref["lse"] - lse).abs().max().item() <= 1e-12, N
            grad = ac.reference_autograd(qkv, do)
            assert ref["dqkv"].shape == grad.shape == qkv.shape
            assert (ref["dqkv"] - grad).abs().max().item() <= 1e-12 * max(1.0, grad.abs().max().item()), N


def test_varlen_reference_against_the_full_reference_on_the_expanded_rows():
    """The last key physically repeated ``mult`` times, through the full-sequence reference above."""
    for L, m in ((1, 0), (1, 1), (1, 255), (2, 254), (16, 1), (17, 239), (65, 0), (200, 56), (256, 0)):
        img = torch.randn(L, 3, ac.H, 64, generator=torch.Generator().manual_seed(L + m)).half()
        got = ac.varlen_reference(img, m)
        assert got.shape == (L, ac.H, 64) and got.dtype == torch.float64
        rows = sc.expand_rows(L - 1, m) if m > 0 else list(range(L))
        exp = img[rows].unsqueeze(0)                                           # [1, Nx, 3, H, 64]
        full = ac.reference(exp, torch.zeros(1, len(rows), ac.H * 64), scale=0.125)["out"].reshape(len(rows), ac.H, 64)
        assert (full - got[rows]).abs().max().item() <= 1e-12, (L, m)


def test_varlen_sweep_covers_every_length_with_every_multiplicity():
    cases = ac.varlen_cases()
    assert sorted(cases) == sorted((L, m) for L in range(1, 257) for m in (0, 1, 256 - L)) and len(cases) == 768
    batches = ac.varlen_batches()
    assert len(batches) == 12
    seen = []
    for lens, mults, rs, rows in batches:
        assert len(lens) == 64 and max(lens) <= 256
        owned = torch.zeros(rows, dtype=torch.bool)
        for L, r in zip(lens, rs):
            assert not owned[r:r + L].any() and r + L <= rows
            assert r == 0 or not owned[r - 1], "an unowned row in front of every image"
            owned[r:r + L] = True
        assert not owned[0] and not owned[-1] and int((~owned).sum()) >= 64
        assert len({L <= 64 for L in lens}) == 2, "short and long images share a launch"
        seen += list(zip(lens, mults))
    assert seen == cases
