"""CPU tests of the counter-based dropout: the mask rule's numpy restatement (tests/_dropout_cases.py) against the Random123
known-answer vectors and its own statistics, the host-side parameters, the C entry points' refusals (no launch, no GPU), and the
modules' behaviour on CPU tensors."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _dropout_cases as dc
from slim_switch_moe_vit_amd import _lib, ops, vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,want", dc.KAT)
def test_philox_known_answer_vectors(ctr, key, want):
    got = dc.philox4x32_10(*ctr, *key)
    assert tuple(int(g) for g in got) == want, [hex(int(g)) for g in got]
    # ... and on arrays: every lane the same answer
    got = dc.philox4x32_10(*(np.full(5, c, dtype=np.uint64) for c in ctr), *key)
    assert all((g == np.uint64(w)).all() for g, w in zip(got, want))


@pytest.mark.parametrize("p,thr16,scale", dc.PARAM_CASES)
def test_dropout_params(p, thr16, scale):
    """thr16 = round(keep * 65536), ties to even (keep = 2^-17 keeps nothing); scale = f32(65536 / thr16) formed in double, 0 -- not a
    division by zero -- when nothing is kept.  The package and the restatement agree."""
    want = (thr16, float(np.float32(scale)))
    got = ops.dropout_params(p)
    assert got == want and isinstance(got[0], int), (got, want)
    ref = dc.params(p)
    assert (ref[0], float(ref[1])) == want
    assert math.isfinite(got[1])
    if thr16:
        assert abs(got[1] * thr16 / 65536.0 - 1.0) < 2.0 ** -23        # the inverse of the keep probability really applied


def test_dropout_params_refuses_probabilities_outside_the_unit_interval():
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.dropout_params(p)


@pytest.mark.parametrize("first_block", dc.FIRST_BLOCKS)
@pytest.mark.parametrize("p", dc.STAT_PS)
@pytest.mark.parametrize("key", dc.STAT_KEYS)
def test_mask_statistics(key, p, first_block):
    """2^20 elements: the kept count lies within 4 standard deviations of n q (q = thr16 / 65536, the probability really applied), and so
    does the number of neighbours that agree (rate q^2 + (1 - q)^2 for independent draws)."""
    n = 1 << 20
    m = dc.mask(key, n, p, first_block)
    q = dc.params(p)[0] / 65536.0
    kept = int(m.sum())
    assert abs(kept - n * q) <= 4.0 * math.sqrt(n * q * (1.0 - q)), (kept, n * q)
    r = q * q + (1.0 - q) * (1.0 - q)
    agree = int((m[1:] == m[:-1]).sum())
    assert abs(agree - (n - 1) * r) <= 4.0 * math.sqrt((n - 1) * r * (1.0 - r)), (agree, (n - 1) * r)


@pytest.mark.parametrize("first_block", dc.FIRST_BLOCKS)
def test_mask_of_row_pieces_is_the_mask_of_the_whole(first_block):
    """What the backward and a piecewise run rest on: the mask depends on (key, first_block, element index) alone, so the mask of
    [rows, cols] is the concatenation of the masks of its row pieces, each run with the number of blocks in front of it."""
    key, p, rows, cols = (-7, 2 ** 63 - 1), 0.3, 37, 24
    whole = dc.mask(key, rows * cols, p, first_block)
    parts, at = [], 0
    for r in (1, 5, 0, 30, 1):
        parts.append(dc.mask(key, r * cols, p, first_block + at * cols // 8))
        at += r
    assert at == rows and np.array_equal(np.concatenate(parts), whole)
    assert not np.array_equal(dc.mask(key, rows * cols, p, first_block + 1), whole)
    assert not np.array_equal(dc.mask((key[0], key[1] - 1), rows * cols, p, first_block), whole)
    assert not np.array_equal(dc.mask((key[0] + 1, key[1]), rows * cols, p, first_block), whole)
    # p moves the threshold over the SAME draws: a mask at a larger keep probability contains the smaller one
    assert (dc.mask(key, rows * cols, 0.5, first_block) <= dc.mask(key, rows * cols, 0.1, first_block)).all()
    assert dc.mask(key, 64, 0.0).all() and not dc.mask(key, 64, 1.0).any()


def test_emulated_arithmetic_selects_zero_and_rounds_once():
    key, p = (3, 4), 0.5
    x = torch.tensor([[float("nan"), float("inf"), -float("inf"), 1.0, -2.0, 65504.0, 3.0e-8, -0.0]] * 4, dtype=torch.float32)
    m = torch.from_numpy(dc.mask(key, 32, p)).reshape(4, 8)
    assert m.any() and not m.all()
    y = dc.dropout(x, key, p, torch.float16)
    assert (y[~m].view(torch.int16) == 0).all(), "a dropped element is +0.0 whatever it held"
    assert torch.isnan(y[:, 0][m[:, 0]]).all() and torch.isinf(y[:, 1][m[:, 1]]).all()
    assert torch.isinf(y[:, 5][m[:, 5]]).all(), "2 x 65504 overflows f16: round to nearest gives inf"
    rs = torch.tensor([1.0, 0.0, 2.0, 0.5])
    res = torch.full((4, 8), 10.0)
    z = dc.dropout_add(x[:, 3:5].repeat(1, 4), res, key, p, row_scale=rs)
    assert z.dtype == torch.float32 and torch.equal(z[1], res[1])      # row factor 0 (a dropped sample): the residual
    kept = torch.from_numpy(dc.mask(key, 32, p)).reshape(4, 8)
    assert torch.equal(z[0][~kept[0]], res[0][~kept[0]])


def _declared():
    text = open(os.path.join(ROOT, "include", "slimmoe.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_dropout_entry_points_are_declared_exported_and_prototyped():
    text = _declared()
    lib = _lib.load()
    for name, n_args in (("smoe_dropout", 12), ("smoe_dropout_add", 12)):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert proto, f"{name} is not declared in include/slimmoe.h"
        assert len(proto.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "const int64_t* key" in text and "uint64_t first_block" in text, "the key travels by address, first_block as uint64"
    assert _lib.ABI_VERSION == 30 and lib.smoe_abi_version() == 30, "the change only adds entry points"
    assert "dropout.hip" in _lib._HASHED
    assert re.search(r"^SRCS\s*=.*\bdropout\.hip\b", open(os.path.join(ROOT, "slim-switch-moe-vit_amd", "csrc", "Makefile")).read(), re.M)
    for f in ("dropout_key", "dropout", "dropout_add", "dropout_params"):
        assert callable(getattr(ops, f))
    from slim_switch_moe_vit_amd import dense
    assert issubclass(dense.DropoutFn, torch.autograd.Function) and issubclass(dense.DropoutAddFn, torch.autograd.Function)


def test_dropout_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal comes back as a message, with pointers that are never dereferenced (safe without a GPU)."""
    lib = _lib.load()
    ok, odd = 4096, 4096 + 4                                   # a 16-byte aligned "address" and a misaligned one

    def drop(x=ok, y=8192, rs=None, key=ok, fb=0, rows=4, cols=64, thr=32768, scale=2.0, di=ops.F16, do=ops.F16):
        return lib.smoe_dropout(x, y, rs, key, fb, rows, cols, thr, scale, di, do, None)

    def add(h=ok, res=8192, rs=None, out=8192, key=ok, fb=0, rows=4, cols=64, thr=32768, scale=2.0, dh=ops.F16):
        return lib.smoe_dropout_add(h, res, rs, out, key, fb, rows, cols, thr, scale, dh, None)

    def refused(rc, word):
        msg = lib.smoe_last_error()
        assert rc != 0 and word in msg, (rc, msg)

    for fn, name in ((drop, b"smoe_dropout:"), (add, b"smoe_dropout_add:")):
        refused(fn(key=None), b"null")
        refused(fn(cols=60), b"multiple of 8")
        refused(fn(cols=0), b"multiple of 8")
        refused(fn(rows=-1), b"rows=-1")
        refused(fn(thr=65537), b"thr16=65537")
        refused(fn(rows=1 << 40, cols=1 << 24), b"overflows")
        refused(fn(rows=(1 << 61) // 64 + 1, cols=64), b"overflows")
        refused(fn(key=ok + 4), b"misaligned key")
        refused(fn(rs=ok + 2), b"row_scale")
        assert name in lib.smoe_last_error()
    refused(drop(x=None), b"null")
    refused(drop(y=None), b"null")
    refused(drop(di=3), b"unknown dtype")
    refused(drop(do=-1), b"unknown dtype")
    refused(drop(x=odd), b"16-byte aligned")
    refused(drop(y=odd), b"16-byte aligned")
    refused(drop(x=ok, y=ok, di=ops.F32, do=ops.F16), b"dtypes are equal")
    refused(add(h=None), b"null")
    refused(add(res=None), b"null")
    refused(add(out=None), b"null")
    refused(add(dh=7), b"unknown dtype")
    refused(add(h=odd), b"16-byte aligned")
    refused(add(res=odd), b"16-byte aligned")
    refused(add(out=odd), b"16-byte aligned")
    refused(add(h=ok, out=ok), b"never h")
    with pytest.raises(_lib.SlimMoEError, match="multiple of 8"):
        _lib.check(drop(cols=12), "smoe_dropout")
    # nothing to do is not an error -- and still no launch
    assert drop(rows=0) == 0 and add(rows=0) == 0
    assert drop(thr=65536, rows=0) == 0 and drop(thr=0, rows=0) == 0


def test_python_face_refuses_cpu_tensors_and_bad_shapes():
    key = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dropout(torch.zeros(2, 8), key, 0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dropout_add(torch.zeros(2, 8), torch.zeros(2, 8), key, 0.1)


def test_modules_on_cpu_tensors_take_torchs_line():
    """No kernel of the library runs for a CPU tensor: the block's dropouts are nn.Dropout calls there -- training draws torch's masks,
    eval is the identity -- and no fallback warning is raised (they speak about GPU runs)."""
    import warnings
    torch.manual_seed(0)
    blk = vit.Block(64, 2, drop=0.5, drop_path=0.0)
    x = torch.randn(2, 5, 64)
    with warnings.catch_warnings():
        warnings.simplefilter("error", vit.SlimMoEFallbackWarning)
        blk.train()
        xg = x.clone().requires_grad_(True)
        y1, y2 = blk(xg), blk(xg)
        y1.sum().backward()
        assert torch.isfinite(y1).all() and xg.grad is not None and not torch.equal(y1, y2)      # two draws, two masks
        blk.eval()
        assert torch.equal(blk(x), blk(x))
