"""Shared by tests/test_adamw_host.py and tests/test_gpu_adamw_regimes.py: ONE AdamW step from a given state, its float64 reference,
the per-element measure and the bar.  Nothing here needs a GPU or the library, and no bar is taken from the code under test.

A cell is (betas, t, regime, gradient dtype, shape).  The kernels are pure functions of (p, m, v, g, t, hyper-parameters, grad_mult),
so a cell is a single step:
    m, v   the f32 roundings of a float64 AdamW trajectory of min(t - 1, 3000) seeded steps (zeros at t = 1)
    g      exactly representable in the cell's gradient dtype
    t      the device step counter is set to t - 1 before the call

REFERENCE  the same step by torch.optim.AdamW(..., foreach=False) on float64 CPU tensors with state[p] = {step: tensor(t - 1.),
           exp_avg, exp_avg_sq}, the hyper-parameters as the Python floats a user passes (not their f32 roundings) and, where
           grad_mult is not 1, the gradient times the f32 value of grad_mult, in float64.

MEASURE    per element, in float64, u = 2^-24, decay = 1 - lr wd, v1 = b2 v + (1 - b2) g^2, den = sqrt(v1) / sqrt(1 - b2^t) + eps:
    p            |got - ref| / (u s_p),  s_p = |decay p| + lr / (1 - b1^t) (b1 |m| + (1 - b1) |g|) / den
    exp_avg      |got - ref| / (u (b1 |m| + (1 - b1) |g|))
    exp_avg_sq   |got - ref| / (u v1)
           The second term of s_p is a forward-error scale: it does not shrink where the new m cancels.  An element whose scale is 0
           is compared for equality (ratio 0 or inf).

BAR        3 x C_ref per cell, for each of the three outputs.  C_ref = the worst value of the measure, over the three outputs and every
           element, of torch.optim.AdamW(foreach=False) on f32 CPU tensors from the same state against the float64 run: the reference's
           own f32 error with the project's usual factor 3.  ONE figure per cell: with betas (0.0, 0.999) torch's lerp returns
           exp_avg = g exactly, and a bar per output would be 0 there.  C_ref is computed here, cached per process, never written down as
           a constant; tests/test_adamw_host.py holds it inside [C_REF_FLOOR, C_REF_CAP) on every cell, conditions on the INPUTS (a
           degenerate cell must not inflate its own bar, nor a lucky one ask for less than roundings take).

REGIMES (lr 1e-3 but where stated, eps 1e-8):
    p0        p = 0, wd 0.05, g ~ N(0, 1): the update alone
    pn        p ~ N(0, 1), wd 0.05
    pn_wd0    p ~ N(0, 1), wd 0, lr 5e-4 (the second parameter group of the multi-tensor launches)
    g1e-3     pn with gradients of scale 1e-3
    g1e-10    pn with gradients of scale 1e-10: sqrt(v) << eps, the update is m / eps
    scaled    pn with f16 values x 65536 as gradients and grad_mult = f32(2^-16 x 0.37): NativeScaler with clipping engaged
    const     pn with the SAME gradient at every step of the trajectory and at the cell's: g - m cancels in the lerp

TABLE      every (betas, t, regime) at 4096 + 3 elements with f32 gradients (`main_cells`), and every (shape, dtype) at betas
           (0.9, 0.999), t = 2 and t = 1000, regimes pn / pn_wd0 alternating (`shape_cells`)."""
import collections
import functools
import math

import numpy as np
import torch

import _lamb_cases as lc

U = 2.0 ** -24
EPS = 1e-8
C_REF_CAP = 8.0
TRAJECTORY_CAP = 3000
BETAS = [(0.9, 0.999), (0.9, 0.95), (0.9, 0.9999), (0.0, 0.999)]
STEPS = [1, 2, 3, 10, 100, 1000, 10000, 375000]     # 375000 = 300 DeiT epochs: beta^t has long underflowed in f32
GRAD_MULT = float(np.float32(2.0 ** -16 * 0.37))
#            p ~ N(0,1)?  wd    lr    gradient kind
REGIMES = {"p0": (False, 0.05, 1e-3, "n"),
           "pn": (True, 0.05, 1e-3, "n"),
           "pn_wd0": (True, 0.0, 5e-4, "n"),
           "g1e-3": (True, 0.05, 1e-3, "1e-3"),
           "g1e-10": (True, 0.05, 1e-3, "1e-10"),
           "scaled": (True, 0.05, 1e-3, "scaled"),
           "const": (True, 0.05, 1e-3, "const")}
MAIN_N = 4096 + 3
SHAPES = list(lc.SHAPES) + [(3,), (5,)]              # the block walk, and the scalar tail before / after one vector
DTYPES = [torch.float32, torch.float16, torch.bfloat16]

Cell = collections.namedtuple("Cell", "betas t regime gdt shape")


def main_cells():
    return [Cell(b, t, r, torch.float32, (MAIN_N,)) for b in BETAS for t in STEPS for r in REGIMES]


def shape_cells():
    return [Cell(BETAS[0], t, ("pn", "pn_wd0")[i % 2], dt, s) for t in (2, 1000) for dt in DTYPES for i, s in enumerate(SHAPES)]


def all_cells():
    return main_cells() + shape_cells()


def cell_id(c) -> str:
    return f"betas {c.betas} t {c.t} {c.regime} {str(c.gdt)[6:]} {'x'.join(map(str, c.shape))}"


def hyper(c):
    """dict(lr, betas, eps, weight_decay) of the cell: Python floats."""
    _, wd, lr, _ = REGIMES[c.regime]
    return dict(lr=lr, betas=c.betas, eps=EPS, weight_decay=wd)


def grad_mult(c):
    """The f32 value of the cell's grad_mult as a Python float, or None (= 1)."""
    return GRAD_MULT if c.regime == "scaled" else None


def _numel(shape) -> int:
    return int(np.prod(shape))


def _kind_grads(kind: str, z):
    """float64 gradients of one trajectory step from N(0,1) draws z."""
    if kind == "n":
        return z
    if kind == "1e-3":
        return z * 1e-3
    if kind == "1e-10":
        return z * 1e-10
    if kind == "scaled":
        return z.astype(np.float16).astype(np.float64) * 65536.0 * GRAD_MULT
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _trajectory(kind: str, n: int, betas_set: tuple, snapshots: tuple):
    """{steps: (m, v)}, float64 [len(betas_set), n]: exp_avg / exp_avg_sq after `steps` AdamW steps from zeros.  Step k reads the window
    [k, k + n) of ONE seeded pool of N(0,1) draws (every element sees an i.i.d. sequence; the kernels are element-wise); `const` reads
    window 0 at every step."""
    pool = np.random.default_rng(77 + n).standard_normal(n + TRAJECTORY_CAP)
    b1 = np.array([b[0] for b in betas_set])[:, None]
    b2 = np.array([b[1] for b in betas_set])[:, None]
    m = np.zeros((len(betas_set), n))
    v = np.zeros((len(betas_set), n))
    out = {0: (m.copy(), v.copy())}
    const = _const_grad(n).double().numpy() if kind == "const" else None
    for k in range(max(snapshots)):
        g = const if kind == "const" else _kind_grads(kind, pool[k:k + n])
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * (g * g)
        if k + 1 in snapshots:
            out[k + 1] = (m, v)
    return out


def _const_grad(n: int):
    return torch.from_numpy(np.random.default_rng(991 + n).standard_normal(n)).float()


_MAIN_SNAPSHOTS = tuple(sorted({min(t - 1, TRAJECTORY_CAP) for t in STEPS}))


@functools.lru_cache(maxsize=None)
def state(c):
    """(p, m, v, g): f32 p / m / v and the gradient in the cell's dtype, flat CPU tensors (treat as read-only).  The scaled regime's
    gradient is f16 values x 65536 held in the cell's dtype (f32)."""
    n = _numel(c.shape)
    p_on, _, _, kind = REGIMES[c.regime]
    steps = min(c.t - 1, TRAJECTORY_CAP)
    if c.shape == (MAIN_N,):
        tr = _trajectory(kind, n, tuple(BETAS), _MAIN_SNAPSHOTS)[steps]
        row = BETAS.index(c.betas)
    else:
        tr = _trajectory(kind, n, (c.betas,), (1, 999))[steps]
        row = 0
    m = torch.from_numpy(tr[0][row]).float()
    v = torch.from_numpy(tr[1][row]).float()
    gen = torch.Generator().manual_seed(4242 + n)
    p = torch.randn(n, generator=gen) if p_on else torch.zeros(n)
    z = torch.randn(n, generator=gen)
    if kind == "const":
        g = _const_grad(n)
    elif kind == "scaled":
        g = z.half().float() * 65536.0
    else:
        g = (z * {"n": 1.0, "1e-3": 1e-3, "1e-10": 1e-10}[kind]).to(c.gdt)
    return p, m, v, g.to(c.gdt)


def torch_step(p, m, v, g, t, hyp, dtype):
    """One torch.optim.AdamW(foreach=False) step in `dtype` on CPU copies; g already carries grad_mult.  Returns new (p, m, v)."""
    q = torch.nn.Parameter(p.detach().to(dtype).clone())
    opt = torch.optim.AdamW([q], foreach=False, **hyp)
    opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.detach().to(dtype).clone(), exp_avg_sq=v.detach().to(dtype).clone())
    q.grad = g.detach().to(dtype).clone()
    opt.step()
    st = opt.state[q]
    assert float(st["step"]) == float(t)
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def scales(p, m, v, g, t, hyp):
    """(s_p, s_m, s_v): the measure's float64 scales (without u) from float64 p, m, v and the effective gradient g."""
    b1, b2 = hyp["betas"]
    lr, wd, eps = hyp["lr"], hyp["weight_decay"], hyp["eps"]
    v1 = b2 * v + (1 - b2) * g * g
    den = v1.sqrt() / math.sqrt(1 - b2 ** t) + eps
    s_m = b1 * m.abs() + (1 - b1) * g.abs()
    s_p = ((1 - lr * wd) * p).abs() + lr / (1 - b1 ** t) * s_m / den
    return s_p, s_m, v1


def ratio(got, ref, scale):
    """|got - ref| / (u scale) per element in float64; where the scale is 0: 0 if equal, inf if not."""
    err = (got.detach().double().cpu().reshape(-1) - ref).abs()
    return torch.where(scale > 0, err / (U * scale).clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf).double())


def step_reference(p, m, v, g_eff, t, hyp):
    """The float64 step from f32-representable state and the float64 effective gradient: dict(p, m, v: float64 results; s: the three
    scales; C: torch's own f32 step's worst measure = C_ref).  The f32 run reads the effective gradient rounded to f32."""
    p, m, v, g_eff = p.double(), m.double(), v.double(), g_eff.double()
    ref = torch_step(p, m, v, g_eff, t, hyp, torch.float64)
    f32 = torch_step(p, m, v, g_eff.float(), t, hyp, torch.float32)
    s = scales(p, m, v, g_eff, t, hyp)
    C = max(float(ratio(a, b, sc).max()) for a, b, sc in zip(f32, ref, s))
    return dict(p=ref[0], m=ref[1], v=ref[2], s=s, C=C)


def effective_grad(c, g):
    gm = grad_mult(c)
    return g.double() * gm if gm is not None else g.double()


@functools.lru_cache(maxsize=None)
def reference(c):
    """`step_reference` of the cell (computed once per process; treat as read-only)."""
    p, m, v, g = state(c)
    return step_reference(p, m, v, effective_grad(c, g), c.t, hyper(c))


# ---------------------------------------------------------------------------------------------- 12 steps from zeros: the cumulative bar
RUN_STEPS = 12
RUN_HYPER = dict(lr=1e-3, eps=EPS, weight_decay=0.05)


@functools.lru_cache(maxsize=None)
def run_inputs():
    """(initial f32 parameters, RUN_STEPS lists of f32 gradients) over SHAPES, N(0,1), seeded (treat as read-only)."""
    gen = torch.Generator().manual_seed(31337)
    return ([torch.randn(s, generator=gen) for s in SHAPES],
            [[torch.randn(s, generator=gen) for s in SHAPES] for _ in range(RUN_STEPS)])


@functools.lru_cache(maxsize=None)
def run_reference(betas):
    """The float64 twin of RUN_STEPS AdamW steps from zero moments: (final float64 parameters, per-element bars), lists over SHAPES.
    bar = sum over the steps of 3 C_ref u s_p of that step, C_ref and s_p from the twin's state rounded to f32 (`step_reference`)."""
    hyp = dict(betas=betas, **RUN_HYPER)
    init, grads = run_inputs()
    ps, bars = [], []
    for j, p0 in enumerate(init):
        p, m, v = p0.double().reshape(-1), torch.zeros(p0.numel(), dtype=torch.float64), torch.zeros(p0.numel(), dtype=torch.float64)
        bar = torch.zeros_like(p)
        for k in range(RUN_STEPS):
            g = grads[k][j].double().reshape(-1)
            r = step_reference(p.float(), m.float(), v.float(), g, k + 1, hyp)
            bar += 3.0 * r["C"] * U * r["s"][0]
            p, m, v = torch_step(p, m, v, g, k + 1, hyp, torch.float64)
        ps.append(p)
        bars.append(bar)
    return ps, bars


# ---------------------------------------------------------------------------------------------- LAMB: one step from a given state
LAMB_STEPS = [1, 2, 1000]
LAMB_BETAS = [(0.9, 0.999), (0.9, 0.9999)]
LAMB_HYPER = dict(lr=3e-3, weight_decay=0.05, eps=1e-6)
LAMB_MAX_GRAD_NORM = 1.0        # engaged: the gradients below have G ~ 4.5
LAMB_WEIGHT_SCALES = [0.02, 5.0, 1.0]
LAMB_SEED = 2718
C_REF_FLOOR = 0.5               # a chain of three correctly rounded operations may take 1.5 units: a cell whose reference happens to land
                                # closer than that (C_ref < 0.5, bar < 1.5 units) measures luck; a condition on the inputs, like the cap


@functools.lru_cache(maxsize=None)
def lamb_state(t: int, betas):
    """(params, exp_avg, exp_avg_sq, grads): f32 lists over SHAPES; the gradients are f16 values.  The moments are those of the AdamW
    trajectory of N(0,1) gradients scaled to the size of the clipped gradients (1e-2 / 4.5)."""
    gen = torch.Generator().manual_seed(LAMB_SEED + t)
    ps, ms, vs, gs = [], [], [], []
    for j, s in enumerate(SHAPES):
        n = _numel(s)
        tr = _trajectory("n", n, (betas,), (1, 999))[min(t - 1, 999)]
        ps.append(torch.randn(n, generator=gen) * LAMB_WEIGHT_SCALES[j % 3])
        ms.append(torch.from_numpy(tr[0][0] * 2e-3).float())
        vs.append(torch.from_numpy(tr[1][0] * 4e-6).float())
        gs.append((torch.randn(n, generator=gen) * 1e-2).half().float())
    return ps, ms, vs, gs


@functools.lru_cache(maxsize=None)
def lamb_reference(t: int, betas):
    """dict(p: float64 results, scale: the measure's float64 scales, C: C_ref) of one LAMB step at step count t.
    Measure: |got - ref| / (u (|p| + lr r (|m| / bc1 / den + wd |p|))), r the tensor's trust ratio, den from the new exp_avg_sq, all
    float64, and |m| the FORWARD-error scale of the new exp_avg, b1 |exp_avg| + (1 - b1) |g / clip|, as in s_p above: it does not shrink
    where the new exp_avg cancels.  (With |new exp_avg| itself the measure reads the cancellation, not the arithmetic: the f32
    restatement's C_ref doubles at t = 2, 20 against 9-10 at t = 1 / 1000, and on the MI355X the kernels, at 0.38-0.49 of the bar at
    t = 1000, stood at 1.21 / 1.45 of it at t = 2 on the one element of the (8, 96, 64) tensor whose new exp_avg is 3.1e-6 out of
    -1.39e-4 + 1.36e-4 and whose p is -4.5e-7.)
    C_ref from the same restatement in f32 torch ops: ONE figure per step, the worst over every tensor.  The global norm makes the step
    the unit, and a figure per tensor is luck on the 1- to 21-element tensors: over 60 seeds it ranged from 0.00 to 121."""
    ps, ms, vs, gs = lamb_state(t, betas)
    hyp = [dict(betas=betas, **LAMB_HYPER)]
    kw = dict(max_grad_norm=LAMB_MAX_GRAD_NORM, exp_avg=ms, exp_avg_sq=vs, first_step=t)
    ref = lc.lamb_steps(ps, [gs], [0] * len(ps), hyp, **kw)
    f32 = lc.lamb_steps(ps, [gs], [0] * len(ps), hyp, dtype=torch.float32, **kw)
    lr, wd, eps = LAMB_HYPER["lr"], LAMB_HYPER["weight_decay"], LAMB_HYPER["eps"]
    bc1, bc2 = 1 - betas[0] ** t, 1 - betas[1] ** t
    scale, C = [], []
    for j, p in enumerate(ps):
        den = ref["exp_avg_sq"][j].sqrt() / math.sqrt(bc2) + eps
        m_scale = betas[0] * ms[j].double().abs() + (1 - betas[0]) * (gs[j].double() / ref["clip"][0]).abs()
        sc = p.double().abs() + lr * ref["trust"][0][j] * (m_scale / bc1 / den + wd * p.double().abs())
        scale.append(sc)
        C.append(float(ratio(f32["params"][j], ref["params"][j], sc).max()))
    return dict(p=ref["params"], scale=scale, C=max(C), clip=ref["clip"][0])


def worst_by_output(c, got_p, got_m, got_v):
    """{"p" / "exp_avg" / "exp_avg_sq": (worst error / bar, element)}: bar = 3 C_ref u scale."""
    r = reference(c)
    out = {}
    for name, got, ref, sc in zip(("p", "exp_avg", "exp_avg_sq"), (got_p, got_m, got_v), (r["p"], r["m"], r["v"]), r["s"]):
        q = ratio(got, ref, sc) / (3.0 * r["C"])
        i = int(q.argmax())
        out[name] = (float(q[i]), i)
    return out


def worst(c, got_p, got_m, got_v):
    """(worst error / bar over the three outputs, description of where)."""
    by = worst_by_output(c, got_p, got_m, got_v)
    name = max(by, key=lambda k: by[k][0])
    return by[name][0], f"{name}[{by[name][1]}]"
