"""CPU side of tests/_adamw_cases.py: the bars of tests/test_gpu_adamw_regimes.py separate the two forms of the AdamW step's scalar
factors, and nothing in them is degenerate.

`emulate` is an EMULATION of csrc/optim.hip's adamw_range in numpy f32 (an FMA where the compiler contracts one; written from the
source, not run on a device; numpy's power stands in for the device's powf):
    "abi29"        the arithmetic up to ABI 29: 1 - powf(b, t), 1.0f - b1, 1.0f - b2 from f32 betas
    "double"       1 - b^t, 1 - b1, 1 - b2 taken in double from double betas and rounded once (csrc/smoe_common.h)
    "double+lerp"  ... and exp_avg by torch's lerp: m + w (g - m) for w = 1 - b1 < 0.5, g - b1 (g - m) otherwise
The first fails the bars on the (0.9, 0.999) and (0.9, 0.9999) cells at 2 <= t <= 1000 (the tests print by how many bars); at t = 1
its two errors cancel in p, but the second moment it stores, (1.0f - b2) g^2, is out there too.  The second passes every cell with
beta1 = 0.9 and fails with beta1 = 0: m + 1 (g - m) is not g where |m| >> |g| (the rounding of g - m is half an ulp of m), while
torch's lerp returns g exactly.  The third, what csrc/optim.hip does from ABI 30 on, passes every cell."""
import numpy as np
import torch

import _adamw_cases as ac
import slim_switch_moe_vit_amd as sm

f32 = np.float32


def _fma(a, b, c):
    """f32 fma(a, b, c): the product of two f32 is exact in float64 (the sum is then rounded twice: a half-ulp tie apart, the same)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def emulate(c, form: str):
    """(p, m, v) of the cell after adamw_range, as f32 torch tensors."""
    p, m, v, g = (x.float().numpy().copy() for x in ac.state(c))
    h = ac.hyper(c)
    b1d, b2d = h["betas"]
    lr, eps, wd, b1, b2, t = f32(h["lr"]), f32(h["eps"]), f32(h["weight_decay"]), f32(b1d), f32(b2d), f32(c.t)
    gm = f32(ac.grad_mult(c) if ac.grad_mult(c) is not None else 1.0)
    if form != "abi29":
        bc1, bc2_sqrt = f32(1.0 - b1d ** c.t), f32(np.sqrt(1.0 - b2d ** c.t))
        omb1, omb2 = f32(1.0 - b1d), f32(1.0 - b2d)
    else:
        bc1, bc2_sqrt = f32(1) - np.power(b1, t, dtype=f32), np.sqrt(f32(1) - np.power(b2, t, dtype=f32), dtype=f32)
        omb1, omb2 = f32(1) - b1, f32(1) - b2
    step_size = lr / bc1
    decay = f32(np.float64(1.0) - np.float64(lr) * np.float64(wd))     # fma(-lr, wd, 1)
    gq = g * gm
    p = p * decay
    if form == "double+lerp" and not omb1 < f32(0.5):
        m = _fma(gq - m, -b1, gq)                                      # g - b1 (g - m)
    else:
        m = _fma(gq - m, omb1, m)                                      # m + (1 - b1) (g - m)
    v = _fma(v, b2, (omb2 * gq) * gq)
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = _fma(m / denom, -step_size, p)
    assert p.dtype == m.dtype == v.dtype == denom.dtype == f32
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


def _defect_cell(c) -> bool:
    return c.betas in ((0.9, 0.999), (0.9, 0.9999)) and 2 <= c.t <= 1000


def test_c_ref_stays_under_the_cap_on_every_cell():
    """A condition on the inputs: no cell inflates its own bar."""
    worst = {}
    for c in ac.all_cells():
        C = ac.reference(c)["C"]
        key = (c.betas, c.regime) if c.shape == (ac.MAIN_N,) else ("shapes", str(c.gdt)[6:])
        lo, hi = worst.get(key, (C, C))
        worst[key] = (min(lo, C), max(hi, C))
        assert ac.C_REF_FLOOR <= C < ac.C_REF_CAP, (ac.cell_id(c), C)
    for key, (lo, hi) in worst.items():
        print(f"REGIME adamw C_ref {key}: {lo:.2f} .. {hi:.2f}")


def test_c_ref_of_the_lamb_cells_and_of_the_twelve_step_run():
    for betas in ac.LAMB_BETAS:
        for t in ac.LAMB_STEPS:
            r = ac.lamb_reference(t, betas)
            assert r["clip"] > 1.0, "the global clip must engage"
            print(f"REGIME lamb C_ref betas {betas} t {t}: {r['C']:.2f} (clip {r['clip']:.2f})")
            # (the cap of the AdamW cells does not apply: the f32 restatement's sums put 10 to 20 units into the large tensors' updates;
            # a bar of 60 units is still 3 x below what an f32 `1 - beta2` does to an update)
            assert ac.C_REF_FLOOR <= r["C"] < 4 * ac.C_REF_CAP, (betas, t, r["C"])
    for betas in ac.BETAS[:1] + ac.BETAS[2:3]:
        ps, bars = ac.run_reference(betas)
        units = max(float((b / (ac.U * p.abs().clamp_min(1e-30))).median()) for p, b in zip(ps, bars))
        print(f"REGIME adamw run of {ac.RUN_STEPS} steps betas {betas}: the cumulative bar's median is {units:.1f} u |p| at most")
        assert all(bool((b > 0).all()) for b in bars)


def test_the_f32_factor_emulation_fails_the_bars_where_predicted():
    cells = ac.main_cells()
    by = {}
    at_one = {}
    for c in cells:
        out = ac.worst_by_output(c, *emulate(c, "abi29"))
        if _defect_cell(c) and c.regime != "g1e-10":   # (there the update is m / eps: p does not see sqrt(1 - b2^t) at all)
            assert out["p"][0] > 1.0, ("the bars must catch the f32 factors in the update here", ac.cell_id(c), out)
            by.setdefault((c.betas, c.t), []).append(out["p"][0])
        elif c.t == 1:
            assert out["p"][0] <= 1.0, ("at t = 1 the two errors cancel in the update", ac.cell_id(c), out)
            at_one.setdefault(c.betas, []).append(out["exp_avg_sq"][0])
    for (betas, t), rs in by.items():
        print(f"REGIME adamw emulation/f32-factors betas {betas} t {t}: p fails by {min(rs):.1f} .. {max(rs):.1f} bars over the regimes")
    for betas, rs in at_one.items():   # p passes at t = 1, the stored second moment (1.0f - b2) g^2 does not
        print(f"REGIME adamw emulation/f32-factors betas {betas} t 1: p passes; exp_avg_sq error / bar {min(rs):.1f} .. {max(rs):.1f}")
        assert (max(rs) > 1.0) == (betas[1] in (0.999, 0.9999)), (betas, rs)


def test_the_double_factor_emulations_pass():
    """Double factors alone: every cell but beta1 = 0 (exp_avg is not g there); with torch's lerp: every cell."""
    worst = {"double": (0.0, None, None), "double+lerp": (0.0, None, None)}
    failed_b1_zero = 0
    for c in ac.all_cells():
        for form in worst:
            r, where = ac.worst(c, *emulate(c, form))
            if form == "double" and c.betas[0] == 0.0:
                failed_b1_zero += r > 1.0
                continue
            assert r <= 1.0, (form, ac.cell_id(c), r, where)
            worst[form] = max(worst[form], (r, ac.cell_id(c), where))
    for form, w in worst.items():
        print(f"REGIME adamw emulation/{form}: worst error / bar {w[0]:.3f} at {w[1]} {w[2]}")
    print(f"REGIME adamw emulation/double: {failed_b1_zero} of the beta1 = 0 cells fail without torch's lerp")
    assert failed_b1_zero > 0, "the bars see m + 1 (g - m) != g"


def test_the_torch_branch_of_adamw_passes_every_cell():
    """sm.AdamW.step on CPU tensors (the torch composition, Python-double factors) through the same table and bars."""
    for c in ac.all_cells():
        p, m, v, g = ac.state(c)
        q = torch.nn.Parameter(p.clone())
        opt = sm.AdamW([q], **ac.hyper(c))
        opt.state[q] = dict(step=c.t - 1, exp_avg=m.clone(), exp_avg_sq=v.clone())
        q.grad = g.float()
        gm = ac.grad_mult(c)
        opt.step(grad_mult=torch.tensor([gm], dtype=torch.float32) if gm is not None else None)
        st = opt.state[q]
        assert st["step"] == c.t
        r, where = ac.worst(c, q, st["exp_avg"], st["exp_avg_sq"])
        assert r <= 1.0, (ac.cell_id(c), r, where)
