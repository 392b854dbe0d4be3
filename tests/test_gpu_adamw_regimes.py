"""The optimizer kernels held to per-element bars on the update they apply (tests/_adamw_cases.py has the cells, the float64
references, the measure and the bars; tests/test_adamw_host.py shows on the CPU that the bars separate f32 from double scalar factors).

    smoe_adamw_step, _multi     one step from a given state over the table: p, exp_avg, exp_avg_sq each within 3 x C_ref units of its
                                forward-error scale, per element; single-tensor == multi-tensor bit for bit
    ... 16-bit images           the multi form's shadows: the round-to-nearest cast of the new p on every element, between guard bands
    sm.AdamW over 12 steps      from zero moments against the float64 twin, cumulative per-element bar
    sm.Lamb, one step           from a given state at t = 1, 2, 1000, the same standard (float64 tests/_lamb_cases.lamb_steps)
    smoe_amp_update, smoe_step_advance   bit for bit a few lines of Python f32 restating GradScaler.update

Every group of cells prints `REGIME <entry> <group>: worst error / bar <r> at <cell> <output>[<element>]`;
profiles/r23_adamw_regimes.md holds the tables."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _adamw_cases as ac  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd import _lib, ops, optim  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
GUARD = 64                 # elements of payload on either side of a 16-bit image
NAN16 = 0x7FA5             # a NaN in f16 and in bf16


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _upload(c):
    """[p, m, v, g] of the cell on the device (fresh copies)."""
    return [x.to(DEV) for x in ac.state(c)]


def _scalars(c):
    """(step counter at t - 1 advanced once by smoe_step_advance, grad_mult or None)"""
    step = torch.tensor([float(c.t - 1)], dtype=F32, device=DEV)
    _lib.check(_lib.load().smoe_step_advance(step.data_ptr(), None, None), "smoe_step_advance")
    gm = ac.grad_mult(c)
    return step, (torch.tensor([gm], dtype=F32, device=DEV) if gm is not None else None)


def _single(c):
    lib, h = _lib.load(), ac.hyper(c)
    p, m, v, g = _upload(c)
    step, gm = _scalars(c)
    rc = lib.smoe_adamw_step(p.data_ptr(), g.data_ptr(), ops.dtype_code(c.gdt), m.data_ptr(), v.data_ptr(), p.numel(), h["lr"],
                             h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], step.data_ptr(), _ptr(gm), None, None)
    _lib.check(rc, "smoe_adamw_step")
    return p, m, v


def _multi(cells, shadows=None):
    """One smoe_adamw_step_multi launch over cells that share betas, t, eps, gradient dtype and grad_mult; lr / weight decay per
    tensor.  shadows: per cell a (pointer, dtype) or None."""
    c0 = cells[0]
    assert all((c.betas, c.t, c.gdt, ac.grad_mult(c)) == (c0.betas, c0.t, c0.gdt, ac.grad_mult(c0)) for c in cells)
    lib, dev = _lib.load(), torch.device(DEV)
    st = [_upload(c) for c in cells]
    numels = [s[0].numel() for s in st]
    blk, nb = optim._block_table(numels, dev)
    tab = torch.tensor([[s[k].data_ptr() for s in st] for k in (0, 3, 1, 2)] + [numels], dtype=torch.int64, device=DEV)
    hyp = torch.tensor([[ac.hyper(c)["lr"] for c in cells], [ac.hyper(c)["weight_decay"] for c in cells]], dtype=F32, device=DEV)
    sh = None
    if shadows is not None:
        sh = torch.tensor([[s[0] if s else 0 for s in shadows], [ops.dtype_code(s[1]) if s else 0 for s in shadows]],
                          dtype=torch.int64, device=DEV)
    step, gm = _scalars(c0)
    rc = lib.smoe_adamw_step_multi(tab.data_ptr(), hyp.data_ptr(), len(st), blk.data_ptr(), sum(nb), ops.dtype_code(c0.gdt),
                                   c0.betas[0], c0.betas[1], ac.EPS, step.data_ptr(), _ptr(gm), None, _ptr(sh), None)
    _lib.check(rc, "smoe_adamw_step_multi")
    torch.cuda.synchronize()
    return [tuple(s[:3]) for s in st]


def _hold(entry, group, cells, launches):
    """Single-tensor launches of every cell, the multi-tensor `launches` (lists of cells) over the same cells: bit-equal, and within
    the bars.  Prints the group's line, returns (worst ratio, cells whose two forms differ)."""
    got = {c: _single(c) for c in cells}
    differ = []
    for batch in launches:
        for c, out in zip(batch, _multi(batch)):
            if not all(torch.equal(a, b) for a, b in zip(out, got[c])):
                differ.append(ac.cell_id(c))
    worst = (0.0, "-", "-")
    for c in cells:
        r, where = ac.worst(c, *(x.cpu() for x in got[c]))
        worst = max(worst, (r, ac.cell_id(c), where))
    print(f"REGIME {entry} {group}: worst error / bar {worst[0]:.3f} at {worst[1]} {worst[2]}")
    return worst[0], differ


@pytest.mark.parametrize("betas", ac.BETAS, ids=str)
def test_adamw_kernels_over_betas_steps_and_regimes(betas):
    """Every (t, regime) at 4096 + 3 elements, f32 gradients.  The multi-tensor launch carries the six regimes without grad_mult: two
    parameter groups (lr 1e-3 / wd 0.05, lr 5e-4 / wd 0); the scaled-gradient cell has a launch of its own."""
    failed, differ = [], []
    for t in ac.STEPS:
        cells = [c for c in ac.main_cells() if c.betas == betas and c.t == t]
        plain = [c for c in cells if ac.grad_mult(c) is None]
        r, d = _hold("adamw", f"betas {betas} t {t}", cells, [plain, [c for c in cells if ac.grad_mult(c) is not None]])
        differ += d
        if not r <= 1.0:
            failed.append((t, round(r, 2)))
    assert not differ, f"single-tensor and multi-tensor results differ: {differ}"
    assert not failed, f"betas {betas}: (t, worst error / bar) {failed}"


@pytest.mark.parametrize("gdt", ac.DTYPES, ids=["f32", "f16", "bf16"])
def test_adamw_kernels_over_shapes_and_gradient_types(gdt):
    """Every block-walk shape, the expert-shaped tensors and the 3- / 5-element tails at betas (0.9, 0.999), t = 2 and 1000, one
    multi-tensor launch per t with the two parameter groups alternating."""
    failed, differ = [], []
    for t in (2, 1000):
        cells = [c for c in ac.shape_cells() if c.gdt == gdt and c.t == t]
        r, d = _hold("adamw/shapes", f"{str(gdt)[6:]} t {t}", cells, [cells])
        differ += d
        if not r <= 1.0:
            failed.append((t, round(r, 2)))
    assert not differ, f"single-tensor and multi-tensor results differ: {differ}"
    assert not failed, f"{gdt}: (t, worst error / bar) {failed}"


def test_adamw_16_bit_images_are_the_cast_of_the_new_weights_inside_their_guard_bands():
    """f16 and bf16 images on some tensors of one launch, none (pointer 0) on tensors in between."""
    cells = [c for c in ac.shape_cells() if c.gdt == torch.float16 and c.t == 2]
    kinds = [torch.float16, None, torch.bfloat16, None, torch.float16, torch.bfloat16, None]
    bufs, shadows = [], []
    for i, c in enumerate(cells):
        n, dt = int(np.prod(c.shape)), kinds[i % len(kinds)]
        buf = torch.full((n + 2 * GUARD,), NAN16, dtype=torch.int16, device=DEV)
        bufs.append(buf)
        shadows.append((buf.data_ptr() + 2 * GUARD, dt) if dt is not None else None)
    assert {s[1] for s in shadows if s} == {torch.float16, torch.bfloat16} and None in shadows
    out = _multi(cells, shadows)
    bad = []
    for c, (p, _, _), buf, s in zip(cells, out, bufs, shadows):
        n = p.numel()
        if s is None:
            if not bool((buf == NAN16).all()):
                bad.append((ac.cell_id(c), "a tensor without an image was given one"))
            continue
        if not (bool((buf[:GUARD] == NAN16).all()) and bool((buf[GUARD + n:] == NAN16).all())):
            bad.append((ac.cell_id(c), "guard band written"))
        wrong = int((buf[GUARD:GUARD + n] != p.to(s[1]).view(torch.int16)).sum())
        if wrong:
            bad.append((ac.cell_id(c), f"{wrong} of {n} image elements are not the cast of p"))
    assert not bad, bad
    # the images change nothing else: the same launch without them gives the same bits
    for a, b in zip(out, _multi(cells)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.9999)], ids=str)
def test_adamw_twelve_steps_from_zero_moments_within_the_cumulative_bar(betas):
    """sm.AdamW as a user drives it, 12 steps, against the float64 twin: |p - ref| <= sum over the steps of 3 C_ref u s_p, per element."""
    init, grads = ac.run_inputs()
    ref, bars = ac.run_reference(betas)
    params = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = sm.AdamW(params, betas=betas, **ac.RUN_HYPER)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.to(DEV)
        opt.step()
    assert float(opt._step_counter(torch.device(DEV))) == float(ac.RUN_STEPS)
    worst = (0.0, None, None)
    for j, (p, q, bar) in enumerate(zip(params, ref, bars)):
        r = (p.detach().cpu().double().reshape(-1) - q).abs() / bar
        i = int(r.argmax())
        worst = max(worst, (float(r[i]), ac.SHAPES[j], i))
    print(f"REGIME adamw/run {ac.RUN_STEPS} steps betas {betas}: worst error / cumulative bar {worst[0]:.3f} at shape {worst[1]} p[{worst[2]}]")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("betas", ac.LAMB_BETAS, ids=str)
def test_lamb_one_step_from_a_given_state(betas):
    """sm.Lamb (four launches, csrc/lamb.hip) over every shape at t = 1, 2, 1000, the global clip engaged."""
    failed = []
    for t in ac.LAMB_STEPS:
        ps, ms, vs, gs = ac.lamb_state(t, betas)
        ref = ac.lamb_reference(t, betas)
        params = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
        opt = sm.Lamb(params, betas=betas, max_grad_norm=ac.LAMB_MAX_GRAD_NORM, **ac.LAMB_HYPER)
        for p, m, v, g in zip(params, ms, vs, gs):
            opt.state[p] = dict(exp_avg=m.clone().to(DEV), exp_avg_sq=v.clone().to(DEV))
            p.grad_dtype = torch.float16
            p.grad = g.half().to(DEV)
        opt.param_groups[0]["step"] = t - 1
        opt.step()
        assert float(opt._step_counter(torch.device(DEV))) == float(t)
        worst = (0.0, None, None)
        for j, p in enumerate(params):
            r = ac.ratio(p, ref["p"][j].reshape(-1), ref["scale"][j].reshape(-1)) / (3.0 * ref["C"])
            i = int(r.argmax())
            worst = max(worst, (float(r[i]), ac.SHAPES[j], i))
        print(f"REGIME lamb betas {betas} t {t}: worst error / bar {worst[0]:.3f} at shape {worst[1]} p[{worst[2]}]")
        if not worst[0] <= 1.0:
            failed.append((t,) + worst)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ the loss scale and the step counter
def _scaler_update(scale, tracker, found, growth, backoff, interval):
    """GradScaler.update() in f32 (torch's amp_update_scale_): (scale, growth tracker) after the step."""
    f = np.float32
    if found:
        return f(scale) * f(backoff), 0.0
    if tracker + 1 == interval:
        return f(scale) * f(growth), 0.0
    return f(scale), tracker + 1.0


def test_amp_update_and_step_advance_tables():
    lib = _lib.load()
    rows = []
    for interval, (growth, backoff) in itertools.product((1, 3, 2000), ((2.0, 0.5), (1.7, 0.3))):
        for tracker in sorted({0, max(interval - 2, 0), interval - 1}):
            for scale in (2.0 ** -10, 1.0, 1536.5, 65536.0, 2.0 ** 24):
                for found in (0.0, 1.0, None):
                    rows.append((scale, float(tracker), found, growth, backoff, interval))
    state = torch.tensor([[r[0], r[1]] for r in rows], dtype=F32, device=DEV)
    flags = torch.tensor([r[2] or 0.0 for r in rows], dtype=F32, device=DEV)
    for i, (_, _, found, growth, backoff, interval) in enumerate(rows):
        rc = lib.smoe_amp_update(state.data_ptr() + 8 * i, state.data_ptr() + 8 * i + 4,
                                 flags.data_ptr() + 4 * i if found is not None else None, growth, backoff, interval, None)
        _lib.check(rc, "smoe_amp_update")
    want = torch.tensor([_scaler_update(r[0], r[1], bool(r[2]), *r[3:]) for r in rows], dtype=F32)
    got = state.cpu()
    bad = [(rows[i], got[i].tolist(), want[i].tolist()) for i in range(len(rows)) if not torch.equal(got[i], want[i])]
    assert not bad, bad[:5]
    assert torch.equal(flags.cpu(), torch.tensor([r[2] or 0.0 for r in rows])), "found_inf is read only"

    # the step counter advances on clean steps only, up to 2^24, where an f32 counter still counts
    starts = [0.0, 5.0, 2.0 ** 24 - 2]
    cases = [(s, found) for s in starts for found in (0.0, 1.0, None)]
    steps = torch.tensor([s for s, _ in cases], dtype=F32, device=DEV)
    found_t = torch.tensor([f or 0.0 for _, f in cases], dtype=F32, device=DEV)
    for _ in range(2):
        for i, (_, found) in enumerate(cases):
            rc = lib.smoe_step_advance(steps.data_ptr() + 4 * i, found_t.data_ptr() + 4 * i if found is not None else None, None)
            _lib.check(rc, "smoe_step_advance")
    assert steps.cpu().tolist() == [s if found else s + 2.0 for s, found in cases]
