"""CPU tests of the skip-aware attention half: the identity it rests on (float64), the host plan against a brute-force loop, and the
C-ABI surface (three additive entry points under ABI 29, the model's flag off by default)."""
import os
import re

import numpy as np
import pytest
import torch

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib, ops, resmoe, vit

import _skip_attn_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("smoe_skip_plan", "smoe_attention_fwd_varlen", "smoe_skip_expand")


@pytest.mark.parametrize("N", [1, 16, 17, 65, 197])
@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_weighted_key_attention_is_attention_over_the_expanded_rows(N, pattern):
    """Plain float64 attention over all N rows -- zero operand rows for the bypassed tokens, a qkv bias -- against the compact form:
    n entering rows plus one representative whose key counts m times, the representative's output copied to every bypassed row.
    Includes m = 0 (pattern none) and n = 0 (pattern all)."""
    H, hd = 2, 8
    d = H * hd
    g = torch.Generator().manual_seed(N * 131 + len(pattern))
    byp = torch.from_numpy(sc.bypass_pattern(pattern, 1, N, seed=3)[0])
    x = torch.randn(N, d, generator=g, dtype=torch.float64)
    x[byp] = 0.0
    w = torch.randn(3 * d, d, generator=g, dtype=torch.float64) * 0.3
    bias = torch.randn(3 * d, generator=g, dtype=torch.float64)
    scale = hd ** -0.5
    qkv = (x @ w.T + bias).reshape(N, 3, H, hd)
    plan = sc.host_plan(byp.numpy()[None])
    L, m = int(plan["len"][0]), int(plan["mult"][0])
    rows = torch.from_numpy(plan["gather"][:L])
    cq = (x[rows] @ w.T + bias).reshape(L, 3, H, hd)
    for h in range(H):
        full = sc.attention_f64(qkv[:, 0, h], qkv[:, 1, h], qkv[:, 2, h], scale)
        comp = sc.weighted_attention_f64(cq[:, 0, h], cq[:, 1, h], cq[:, 2, h], scale, m)
        got = torch.empty_like(full)
        got[rows[:L - (m > 0)]] = comp[:L - (m > 0)]
        if m:
            got[byp] = comp[L - 1]
        assert (got - full).abs().max().item() <= 1e-12


@pytest.mark.parametrize("B", sc.PLAN_B)
@pytest.mark.parametrize("N", sc.PLAN_N)
def test_host_plan_matches_the_brute_force_loop(B, N):
    names = sc.PATTERNS + (("all_next_to_none",) if B > 1 else ())
    for name in names:
        byp = sc.bypass_pattern(name, B, N, seed=1)
        a, b = sc.host_plan(byp), sc.brute_plan(byp)
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k)
        R = int(a["offsets"][1])
        assert 1 <= R <= B * N and (a["len"] >= 1).all() and (a["len"] <= N).all()
        assert sorted(a["row_map"][:R].tolist()) == sorted(set(a["row_map"][:R].tolist()))    # every output row written once


def test_three_entry_points_are_declared_exported_and_bound_under_abi_29():
    text = open(os.path.join(ROOT, "include", "slimmoe.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
        assert s in _lib.SIGNATURES and _lib.has_symbol(s), s
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[s][1]), s
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    assert "attention_skip.hip" in _lib._HASHED and _lib.source_build_id() == _lib.binary_build_id()
    for f in ("skip_plan", "attention_varlen", "skip_expand"):
        assert callable(getattr(ops, f))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake = 4096                                           # never dereferenced: the argument checks come first
    assert lib.smoe_skip_plan(fake, 2, 0, fake, fake, fake, fake, fake, fake, fake, None, 0, None) != 0
    assert lib.smoe_skip_plan(None, 2, 4, fake, fake, fake, fake, fake, fake, fake, None, 0, None) != 0 and b"null" in lib.smoe_last_error()
    assert lib.smoe_attention_fwd_varlen(fake, fake, 1, fake, fake, fake, 2, 257, 8, 1, 64, 0.125, 0, None) != 0
    assert b"max_len" in lib.smoe_last_error()
    assert lib.smoe_attention_fwd_varlen(fake, fake, 1, fake, fake, fake, 2, 197, 8, 1, 32, 0.125, 0, None) != 0
    assert lib.smoe_attention_fwd_varlen(fake, fake, 0, fake, fake, fake, 2, 197, 8, 1, 64, 0.125, 0, None) != 0
    assert lib.smoe_attention_fwd_varlen(fake, fake, 1, fake, fake, fake, 2, 197, 8, 1, 64, 0.125, 4, None) != 0
    assert lib.smoe_skip_expand(fake, fake, fake, 8, 6, 8, None) != 0
    assert lib.smoe_skip_expand(fake, fake, fake, 8, 8, 4, None) != 0 and b"out_rows" in lib.smoe_last_error()


def test_flag_exists_and_is_off_by_default():
    assert vit.VisionTransformer.skip_aware_attention is False
    assert vit.Block.skip_aware_attention is False
    m = sm.create_model("resmoe_tiny_patch16_224_expert8", depth=1, num_classes=10)
    assert m.skip_aware_attention is False and all(b.skip_aware_attention is False for b in m.blocks)
    assert "skip_aware_attention" not in m.state_dict()
    assert not resmoe._skip_attention_ok(m.blocks[0], torch.zeros(1, 197, 192))
    assert ops.skip_attention_supported(197, 64) and ops.skip_attention_supported(256, 64)
    assert not ops.skip_attention_supported(257, 64) and not ops.skip_attention_supported(197, 32)
