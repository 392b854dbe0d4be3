"""CPU tests of the soft token-skip gate (Gate(is_hard=False) in training; smoe_soft_gate_ln_fwd and gate_on = 2 of the two gate
backward entry points): the formulas against float64 autograd of the reference's expressions, an f32 emulation of the forward
kernel's arithmetic against float64 on Gaussian, ill-conditioned and saturated rows (the figures the GPU bars of
tests/test_gpu_soft_gate.py are checked against), the reference Gate's own train-soft outputs, the refusals of the C entry points
and the reference fixture's regeneration."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _soft_gate_cases as sg
from test_value_regimes_host import DIMS, LN_CLASSES, gate_params, ln_params, ln_rows

from slim_switch_moe_vit_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOFT_CLASSES = tuple(c for c in LN_CLASSES if c != "const")     # (a constant row is beta exactly: nothing to measure)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


# ------------------------------------------------------------------------------------------------------------------- the formulas
@pytest.mark.parametrize("with_out", [True, False])
def test_soft_gradient_formulas_are_float64_autograd_of_the_reference_expressions(with_out):
    """dL/dp = <g_f, xn> (the residual's two terms cancel), dz = +<g_f, xn> p (1 - p) -- the OPPOSITE sign of the straight-through
    path --, dxn = g_f p + g_out + dz w, dW = dz^T xn, db = sum dz."""
    T, d = 37, 192
    g = torch.Generator().manual_seed(11)
    xn = torch.randn(T, d, generator=g)
    w, b = torch.randn(d, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1
    g_f, g_out = torch.randn(T, d, generator=g) * 0.3, (torch.randn(T, d, generator=g) * 0.2 if with_out else None)
    ref = sg.soft_bwd_f64(xn, None, None, w, b, g_f, g_out, ln=False)
    p = ref["p"]
    dot = (g_f.double() * xn.double()).sum(-1)
    dz = dot * p * (1 - p)
    assert _rel(dz, ref["dz"]) <= 1e-13
    dxn = g_f.double() * p[:, None] + (g_out.double() if with_out else 0.0) + dz[:, None] * w.double()
    assert _rel(dxn, ref["dxn"]) <= 1e-13
    assert _rel(dz @ xn.double(), ref["dgate_w"]) <= 1e-13 and abs(float(dz.sum()) - float(ref["dgate_b"])) <= 1e-12
    # the sign: the straight-through path's dz (tests/test_value_regimes_host.py gate_dz_f64) is the negative of this one
    from test_value_regimes_host import gate_dz_f64
    assert _rel(-gate_dz_f64(xn, g_f, w, b), ref["dz"]) <= 1e-13
    # the cancellation: a loss on the residual alone leaves the gate no gradient at all
    only_out = sg.soft_bwd_f64(xn, None, None, w, b, torch.zeros(T, d), torch.randn(T, d, generator=g), ln=False)
    assert float(only_out["dz"].abs().max()) <= 1e-14 * float(xn.abs().max()) * d
    assert float(only_out["dgate_w"].abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------- the kernel's arithmetic, emulated
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cls", SOFT_CLASSES)
def test_forward_emulation_is_inside_a_third_of_the_bars(cls, d):
    """Gaussian rows and the ill-conditioned rows of tests/test_value_regimes_host.py (common offset, outlier channel, variance near
    eps) through LayerNorm, logit, the e-forms of p and 1 - p and the products, in the kernel's order, against float64."""
    x, (gamma, beta), (w, b) = ln_rows(cls, d), ln_params(d), gate_params(d)
    ref = sg.soft_f64(x, gamma, beta, w, b)
    emu = sg.soft_emulate(x, gamma, beta, w, b)
    r = sg.soft_ratios(emu, ref, w)
    r16 = sg.soft_ratios({"xn16": emu["tk32"].half()}, ref, w, torch.float16)
    print(f"soft forward emulation {cls} d {d}: error / bar {({k: round(v, 3) for k, v in {**r, **r16}.items()})}")
    # xn / tk: the LayerNorm bar is the suite's own (LN_C), met here with the 4-per-lane summation order of the backward kernel: 0.336 of
    # it at worst (off3000, d = 192) -- a GPU bar of 1 is at most 3 x what this emulation shows.  p and 1 - p stay below a fifth.
    assert max(r.values()) <= 0.35 and max(r["p"], r["1-p"]) <= 0.2 and r16["tk16"] <= 1.0
    s = emu["mask"].sum(-1)
    assert float((s - 1).abs().max()) <= 2.0 ** -23


@pytest.mark.parametrize("d", DIMS)
def test_saturated_logits_keep_both_masks_and_the_subtracting_form_misses(d):
    """|z| out to 30 (no LayerNorm, rows along gate_w): p and 1 - p both keep their RELATIVE bars; 1 - p taken from the rounded p
    misses its bar by orders of magnitude once the gate saturates, and is 0 from z = 17 on where 1 - p is 4e-8."""
    w, b = gate_params(d)
    zs = torch.linspace(-30, 30, 61)
    x = sg.saturating_rows(w, b, zs)
    ref = sg.soft_f64(x, None, None, w, b, ln=False)
    assert float((ref["z"] - zs.double()).abs().max()) <= 1e-4
    r = sg.soft_ratios(sg.soft_emulate(x, None, None, w, b, ln=False), ref, w)
    sub = sg.soft_emulate(x, None, None, w, b, ln=False, subtract=True)
    r_sub = sg.soft_ratios(sub, ref, w)
    print(f"saturated d {d}: e-forms {({k: round(v, 3) for k, v in r.items()})}; 1 - p from the rounded p: {r_sub['1-p']:.3g} bars")
    assert max(r.values()) <= 1 / 3
    assert r_sub["1-p"] > 100
    assert float(sub["mask"][zs >= 17, 0].abs().max()) == 0.0 and float(ref["om"][zs >= 17].min()) > 0.0
    m = sg.soft_emulate(x, None, None, w, b, ln=False)["mask"]
    assert bool(((m >= 0) & (m <= 1)).all()) and bool(torch.isfinite(m).all())


# -------------------------------------------------------------------------------------------- the reference Gate's train-soft outputs
def test_reference_gate_fixture_train_soft_entries_follow_from_the_formulas():
    """ref_gate_tiny.npz train_soft_* (the reference Gate.forward, is_hard=False, train mode; f32 torch): mask = (1 - p, p), and with
    L = <dret, mask>: dz = (dret[..., 1] - dret[..., 0]) p (1 - p), dx = dz w, dw = dz^T x, db = sum dz; the counters."""
    g = {k: v for k, v in np.load(os.path.join(GOLDEN, "ref_gate_tiny.npz")).items()}
    x = torch.from_numpy(g["x"]).double()
    B, N, d = x.shape
    w, b = torch.from_numpy(g["w"]).double().reshape(-1), torch.from_numpy(g["b"]).double()
    z = x @ w + b
    p, om = torch.sigmoid(z), torch.sigmoid(-z)
    mask = torch.stack((om, p), dim=-1)
    # f32 torch: the logit is a d = 192 dot product (a few 1e-7 relative to sum |x w|), the sigmoid an ulp or two: 1e-6 absolute
    assert float((mask - torch.from_numpy(g["train_soft_mask"]).double()).abs().max()) <= 1e-6
    dret = torch.from_numpy(g["dret"]).double()
    dz = (dret[..., 1] - dret[..., 0]) * p * om
    assert _rel(torch.from_numpy(g["train_soft_dx"]), dz[..., None] * w) <= 1e-5
    assert _rel(torch.from_numpy(g["train_soft_dw"]).reshape(-1), (dz[..., None] * x).sum((0, 1))) <= 1e-5
    assert abs(float(g["train_soft_db"].reshape(-1)[0]) - float(dz.sum())) <= 1e-5 * max(1.0, abs(float(dz.sum())))
    assert int(g["train_soft_total"]) == B * N
    assert abs(float(g["train_soft_skipped"]) - float(om.sum())) <= 1e-4


# ----------------------------------------------------------------------------------------------------------------------- refusals
def test_backward_entry_points_refuse_an_unknown_gate_mode():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    for bad in (3, -1, 7):
        rc = lib.smoe_gate_ln_bwd(ptr, ptr, 0, None, None, None, 1e-6, ptr, None, ptr, bad, 4, 192, ptr, None, ptr, ptr, 1 << 30, None)
        assert rc != 0 and b"gate_on" in lib.smoe_last_error(), lib.smoe_last_error()
        rc = lib.smoe_skip_gate_bwd(ptr, ptr, 0, None, ptr, None, ptr, bad, 4, 192, ptr, None, None)
        assert rc != 0 and b"gate_on" in lib.smoe_last_error(), lib.smoe_last_error()
    assert [ops._gate_mode(v) for v in (False, True, 0, 1, 2)] == [0, 1, 0, 1, 2]
    for bad in (3, -1, 2.0, "soft", None):
        with pytest.raises(ValueError):
            ops._gate_mode(bad)
    t = torch.zeros(4, 192)
    with pytest.raises(ValueError):          # refused before anything else is looked at
        ops.gate_ln_bwd(t, t, None, None, None, 1e-6, t[0], None, None, gate_on=3)
    with pytest.raises(ValueError):
        ops.skip_gate_bwd(t, t, None, t[0], None, None, gate_on=3)


def test_forward_entry_point_refuses_what_it_does_not_take():
    lib = _lib.load()
    assert [lib.smoe_soft_gate_ln_fwd_supported(d) for d in (192, 384, 768, 1024, 0, 64, 256, 512, 1000, 2048)] == [1, 1, 1, 1] + [0] * 6
    assert lib.smoe_soft_gate_ln_fwd_workspace_bytes(0) == 0 and lib.smoe_soft_gate_ln_fwd_workspace_bytes(-5) == 0
    assert lib.smoe_soft_gate_ln_fwd_workspace_bytes(1) == 8 and lib.smoe_soft_gate_ln_fwd_workspace_bytes(9) == 24
    assert lib.smoe_soft_gate_ln_fwd_workspace_bytes(1 << 30) % 8 == 0
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)

    def call(x=ptr, x_dtype=0, w=ptr, T=4, d=192, tk16_dtype=1, count=None, ws=None, ws_bytes=0):
        return lib.smoe_soft_gate_ln_fwd(x, x_dtype, 1, None, None, 1e-6, w, None, None, None, tk16_dtype, None, None, count, T, d, ws,
                                         ws_bytes, None)
    assert call(T=0) == 0                                      # an empty call returns at once
    for kw, word in ((dict(d=256), b"unsupported d"), (dict(d=100), b"unsupported d"), (dict(x=None), b"null"), (dict(w=None), b"null"),
                     (dict(x_dtype=1), b"f32"), (dict(T=-1), b"bad T"), (dict(T=1 << 31), b"bad T"), (dict(tk16_dtype=0), b"f16 or bf16"),
                     (dict(count=ptr), b"workspace"), (dict(count=ptr, ws=ptr, ws_bytes=4), b"workspace")):
        assert call(**kw) != 0 and word in lib.smoe_last_error(), (kw, lib.smoe_last_error())


# ------------------------------------------------------------------------------------------------------------------- the fixture
def test_soft_block_fixture_is_data_of_the_hard_fixtures_block():
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_resmoe_soft as gen
    finally:
        sys.path.remove(GOLDEN)
    f = gen.load()
    hard = np.load(os.path.join(GOLDEN, "ref_resblock_tiny.npz"))
    assert {"g." + k[2:] for k in hard.files if k.startswith("p.") and "threshold" not in k} == {k for k in f if k.startswith("g.")}
    assert f["train_y"].shape == hard["x"].shape == f["train_dx"].shape
    for name in ("dense", "moe"):
        m = f[f"train_{name}_mask"].astype(np.float64)
        assert m.shape == hard["x"].shape[:2] + (2,) and np.all((m >= 0) & (m <= 1)) and np.abs(m.sum(-1) - 1).max() <= 2.0 ** -23
        assert int(f[f"train_{name}_total"]) == m.shape[0] * m.shape[1]
        assert abs(float(f[f"train_{name}_skipped"]) - m[..., 0].sum()) <= 1e-4      # the reference's counter is the fractional sum
    for fn in os.listdir(os.path.join(GOLDEN, "soft")):
        assert os.path.getsize(os.path.join(GOLDEN, "soft", fn)) < (1 << 20), fn


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree only exists in the build container")
def test_soft_block_fixture_regenerates_bit_identically(tmp_path):
    env = dict(os.environ, SLIMMOE_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_resmoe_soft.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    made = sorted(os.listdir(tmp_path))
    assert made == sorted(os.listdir(os.path.join(GOLDEN, "soft"))), made
    for fn in made:
        new, old = np.load(os.path.join(tmp_path, fn)), np.load(os.path.join(GOLDEN, "soft", fn))
        assert sorted(new.files) == sorted(old.files), fn
        for key in old.files:
            a, b = old[key], new[key]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (fn, key)
