"""The counter-based dropout on the GPU: smoe_dropout / smoe_dropout_add bit for bit against the numpy restatement of the mask rule
(tests/_dropout_cases.py), the autograd Functions dense.DropoutFn / dense.DropoutAddFn, and a captured key draw + dropout."""
import numpy as np
import pytest
import torch

import _dropout_cases as dc
from slim_switch_moe_vit_amd import dense, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                       # elements of NaN-payload guard band on either side of every output
_PAYLOAD = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.float16: (torch.int16, 0x7E5A), torch.bfloat16: (torch.int16, 0x7FDA)}


def _gen(s):
    return torch.Generator().manual_seed(s)


def _key(s):
    return torch.randint(-(1 << 63), (1 << 63) - 1, (2,), dtype=torch.int64, generator=_gen(s))


def _banded(shape, dtype):
    """(buffer, view of `shape` in its middle): the bands hold a NaN with a payload no kernel produces."""
    n = int(np.prod(shape))
    it, word = _PAYLOAD[dtype]
    buf = torch.full((n + 2 * GUARD,), word, dtype=it, device=DEV).view(dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _bands_intact(buf, dtype):
    it, word = _PAYLOAD[dtype]
    b = buf.view(it)
    return bool((b[:GUARD] == word).all()) and bool((b[-GUARD:] == word).all())


def _input(shape, dtype, seed):
    return (torch.randn(shape, generator=_gen(seed)) * 3).to(dtype)


@pytest.mark.parametrize("rows,cols", dc.SHAPES)
def test_dropout_kernel_is_the_rule_bit_for_bit(rows, cols):
    """Every in / out dtype pairing at every shape; p, the row scale, first_block and in-place running cycle through the pairings so that
    each value meets each shape's neighbours.  Outputs between guard bands."""
    for j, (din, dout) in enumerate(dc.PAIRS):
        i = dc.SHAPES.index((rows, cols))
        p = dc.PS[(i + j) % 3]
        fb = dc.FIRST_BLOCKS[(i + j // 3) % 2]
        rs = torch.rand(rows, generator=_gen(j)) * 2 if (i + j) % 2 else None
        key = _key(100 * i + j)
        x = _input((rows, cols), din, 7 * i + j)
        want = dc.dropout(x, dc.key_of(key), p, dout, rs, fb)
        buf, y = _banded((rows, cols), dout)
        got = ops.dropout(x.to(DEV), key.to(DEV), p, row_scale=rs.to(DEV) if rs is not None else None, out=y, first_block=fb)
        assert got.data_ptr() == y.data_ptr()
        assert dc.same_bits(y, want), (din, dout, p, fb, rs is not None)
        assert _bands_intact(buf, dout)
        if din == dout:                                   # in place: the input buffer between its own bands
            buf, xi = _banded((rows, cols), din)
            xi.copy_(x)
            ops.dropout(xi, key.to(DEV), p, row_scale=rs.to(DEV) if rs is not None else None, out=xi, first_block=fb)
            assert dc.same_bits(xi, want) and _bands_intact(buf, din), (din, p, fb)
        if p == 1.0:
            assert not want.view(torch.int16 if dout != torch.float32 else torch.int32).any(), "p = 1: every element +0.0"


@pytest.mark.parametrize("rows,cols", dc.SHAPES)
def test_dropout_add_kernel_is_the_rule_bit_for_bit(rows, cols):
    i = dc.SHAPES.index((rows, cols))
    for j, dh in enumerate(dc.DTYPES):
        for alias in (False, True):
            p = dc.PS[(i + j + alias) % 3]
            rs = torch.rand(rows, generator=_gen(j)) * 2 if (i + j + alias) % 2 == 0 else None
            key = _key(900 + 10 * i + j)
            h = _input((rows, cols), dh, 3 * i + j)
            res = torch.randn(rows, cols, generator=_gen(50 + i))
            want = dc.dropout_add(h, res, dc.key_of(key), p, rs)
            buf, out = _banded((rows, cols), torch.float32)
            rs_d = rs.to(DEV) if rs is not None else None
            if alias:
                out.copy_(res)
                ops.dropout_add(h.to(DEV), out, key.to(DEV), p, row_scale=rs_d, out=out)
            else:
                ops.dropout_add(h.to(DEV), res.to(DEV), key.to(DEV), p, row_scale=rs_d, out=out)
            assert dc.same_bits(out, want), (dh, alias, p, rs is not None)
            assert _bands_intact(buf, torch.float32)


@pytest.mark.parametrize("blocks", dc.CAP_BLOCKS)
def test_dropout_on_both_sides_of_its_grid_cap(blocks):
    """One 8-element block below the cap of 4096 workgroups x 256 lanes, just past it, and past twice it (a third trip exists): f16 in
    place with a row scale over [blocks, 8] (the row of a block by the 32-bit division), and the residual form."""
    key = _key(blocks)
    x = _input((blocks, 8), torch.float16, 1)
    rs = torch.rand(blocks, generator=_gen(2)) + 0.5
    want = dc.dropout(x, dc.key_of(key), 0.1, row_scale=rs)
    buf, xi = _banded((blocks, 8), torch.float16)
    xi.copy_(x)
    ops.dropout(xi, key.to(DEV), 0.1, row_scale=rs.to(DEV), out=xi)
    assert dc.same_bits(xi, want) and _bands_intact(buf, torch.float16)
    res = torch.randn(blocks, 8, generator=_gen(3))
    want = dc.dropout_add(x, res, dc.key_of(key), 0.5)
    buf, out = _banded((blocks, 8), torch.float32)
    out.copy_(res)
    ops.dropout_add(x.to(DEV), out, key.to(DEV), 0.5, out=out)
    assert dc.same_bits(out, want) and _bands_intact(buf, torch.float32)


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_dropped_non_finite_values_read_zero_and_kept_ones_propagate(dtype):
    rows, cols, p = 16, 64, 0.5
    key = _key(5)
    x = _input((rows, cols), dtype, 9)
    flat = x.view(-1)
    flat[0::7] = float("nan")
    flat[1::7] = float("inf")
    flat[2::7] = -float("inf")
    m = torch.from_numpy(dc.mask(dc.key_of(key), rows * cols, p))
    y = ops.dropout(x.to(DEV), key.to(DEV), p).cpu().view(-1)
    bits = y.view(torch.int32 if dtype == torch.float32 else torch.int16)
    assert (bits[~m] == 0).all(), "dropped positions read +0.0 exactly"
    assert torch.isnan(y[0::7][m[0::7]]).all() and m[0::7].any() and (~m[0::7]).any()
    assert (y[1::7][m[1::7]] == float("inf")).all() and (y[2::7][m[2::7]] == -float("inf")).all()
    res = torch.ones(rows, cols)
    z = ops.dropout_add(x.to(DEV), res.to(DEV), key.to(DEV), p).cpu().view(-1)
    assert (z[~m] == 1.0).all() and torch.isnan(z[0::7][m[0::7]]).all() and (z[1::7][m[1::7]] == float("inf")).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_backward_regenerates_the_forwards_mask(dtype):
    rows, cols, p = 33, 200, 0.3
    key = _key(11).to(DEV)
    k = dc.key_of(key)
    rs = (torch.rand(rows, generator=_gen(1)) + 0.5).to(DEV)
    x = _input((rows, cols), dtype, 2).to(DEV).requires_grad_(True)
    dy = _input((rows, cols), dtype, 3).to(DEV)
    y = dense.DropoutFn.apply(x, p, key, rs)
    saved = y.grad_fn.saved_tensors
    assert sorted(t.numel() for t in saved) == [2, rows], "the key and row_scale, nothing else"
    y.backward(dy)
    assert dc.same_bits(y, dc.dropout(x, k, p, row_scale=rs)) and dc.same_bits(x.grad, dc.dropout(dy, k, p, row_scale=rs))
    y2 = dense.DropoutFn.apply(x, p, key, rs)
    assert dc.same_bits(y2, y), "two runs with one key"
    y3 = dense.DropoutFn.apply(x, p, _key(12).to(DEV), rs)
    assert not torch.equal(y3 == 0, y == 0), "two keys, two masks"
    # the residual form: h 16- or 32-bit, residual and output f32; d residual IS dout
    res = torch.randn(rows, cols, generator=_gen(4)).to(DEV).requires_grad_(True)
    x.grad = None
    out = dense.DropoutAddFn.apply(x, res, p, key, rs)
    assert sorted(t.numel() for t in out.grad_fn.saved_tensors) == [2, rows]
    dout = torch.randn(rows, cols, generator=_gen(5)).to(DEV)
    out.backward(dout)
    assert dc.same_bits(out, dc.dropout_add(x, res, k, p, rs))
    assert dc.same_bits(x.grad, dc.dropout(dout, k, p, out_dtype=dtype, row_scale=rs))
    assert torch.equal(res.grad, dout)
    # a key nobody passed is drawn from torch's generator: the seed reproduces it
    torch.manual_seed(77)
    a = dense.DropoutFn.apply(x, p)
    torch.manual_seed(77)
    drawn = ops.dropout_key(DEV)
    assert dc.same_bits(a, dc.dropout(x, dc.key_of(drawn), p))
    # in place on a fresh tensor
    z = x.detach() + 1.0
    z.requires_grad_(True)
    w = z * 1.0
    v = dense.DropoutFn.apply(w, p, key, None, True)
    assert v.data_ptr() == w.data_ptr()
    v.backward(dy)
    assert dc.same_bits(z.grad, dc.dropout(dy, k, p))


def test_captured_dropout_reads_a_fresh_key_on_every_replay():
    x = torch.ones(64, 256, device=DEV)
    torch.manual_seed(3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                       # warm-up outside the capture (library load, launch attributes)
        ops.dropout(x, ops.dropout_key(DEV), 0.5)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        key = ops.dropout_key(DEV)
        y = ops.dropout(x, key, 0.5)
    masks = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        k = dc.key_of(key)
        assert dc.same_bits(y, dc.dropout(x, k, 0.5)), "the kernel read the key this replay drew"
        masks.append((y != 0).cpu())
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) and not torch.equal(masks[0], masks[2])
