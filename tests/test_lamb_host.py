"""CPU tests of optim.Lamb (timm.optim.Lamb restated; csrc/lamb.hip on the GPU): the float64 restatement of the rule the GPU tests
compare against (tests/_lamb_cases.py), the torch composition sm.Lamb takes for CPU tensors, checkpoints, and the argument checks
of the four entry points (no launch without a GPU)."""
import copy
import io

import pytest
import torch

import _lamb_cases as cases
import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

# f32 torch ops against the float64 restatement over the case set, 12 steps, relative to max(1, max |ref|): measured 2.0e-7 .. 2.6e-7
# for the parameters and up to 5.6e-7 (relative) for the trust ratios; the bars are 3 x the largest measured figure, rounded down
F32_PARAM_BAR = 7.5e-7
F32_MOMENT_BAR = 7e-7        # exp_avg / exp_avg_sq: measured up to 2.09e-7 / 2.45e-7 (max_grad_norm=None; below 1e-9 elsewhere)
F32_TRUST_BAR = 1.6e-6


def _run(opt_cls, setting, steps=cases.STEPS, first=0, params=None, opt=None, **step_kw):
    mgn, gscale, _, _ = cases.SETTINGS[setting]
    if params is None:
        params = [torch.nn.Parameter(t.clone()) for t in cases.initial_weights()]
    if opt is None:
        opt = cases.make_optimizer(opt_cls, params, setting)
    for grads in cases.gradients(gscale)[first:first + steps]:
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step(**step_kw)
    return params, opt


def test_restatement_fixed_points():
    """Zero gradient with wd = 0 leaves p unchanged (u = 0 / eps = 0), and a tensor of zeros has r = 1 (w = 0)."""
    p = [torch.randn(5, 3, generator=torch.Generator().manual_seed(0)), torch.zeros(7)]
    hyper = [dict(lr=1e-2, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-6)]
    out = cases.lamb_steps(p, [[torch.zeros(5, 3), torch.zeros(7)]] * 3, [0, 0], hyper, always_adapt=True)
    assert torch.equal(out["params"][0], p[0].double()) and torch.equal(out["params"][1], p[1].double())
    assert out["G"] == [0.0] * 3 and out["clip"] == [1.0] * 3
    g = [[torch.ones(5, 3), torch.ones(7)]]
    out = cases.lamb_steps(p, g, [0, 0], hyper, always_adapt=True, max_grad_norm=None)
    assert out["trust"][0][1] == 1.0 and out["trust"][0][0] != 1.0
    # w = 0, r = 1: the first step's update is m / bc1 / (sqrt(v) / sqrt(bc2) + eps) = 1 / (1 + eps)
    assert torch.allclose(out["params"][1], torch.full((7,), -1e-2 / (1 + 1e-6), dtype=torch.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize("setting", range(len(cases.SETTINGS)))
def test_f32_restatement_against_float64(setting):
    """The floor the GPU bars are judged against: the same rule in f32 torch ops (profiles/r17_lamb.md holds the figures)."""
    mgn, gscale, trust_clip, always_adapt = cases.SETTINGS[setting]
    ref = cases.reference(setting)
    f32 = cases.lamb_steps(cases.initial_weights(), cases.gradients(gscale), cases.GROUP_OF, cases.HYPER, max_grad_norm=mgn,
                           trust_clip=trust_clip, always_adapt=always_adapt, dtype=torch.float32)
    err = cases.rel_err(f32["params"], ref["params"])
    terr = max(abs(a - b) / b for a, b in zip(f32["trust"][-1], ref["trust"][-1]))
    lo, hi = min(min(t) for t in ref["trust"]), max(max(t) for t in ref["trust"])
    print(f"setting {setting}: f32 vs f64 parameters {err:.3e}, trust ratios {terr:.3e} (ratios {lo:.4g} .. {hi:.4g}), G {ref['G'][-1]:.6g}")
    assert err <= F32_PARAM_BAR and terr <= F32_TRUST_BAR
    assert (ref["clip"][-1] > 1.0) == (mgn is not None and gscale == 1.0), "the settings engage / do not engage the global clip"


@pytest.mark.parametrize("setting", range(len(cases.SETTINGS)))
def test_lamb_cpu_composition_matches_the_restatement(setting):
    ref = cases.reference(setting)
    params, opt = _run(sm.Lamb, setting)
    err = cases.rel_err(params, ref["params"])
    print(f"setting {setting}: sm.Lamb (CPU composition) vs f64 {err:.3e}")
    assert err <= F32_PARAM_BAR
    assert cases.rel_err([opt.state[p]["exp_avg"] for p in params], ref["exp_avg"]) <= F32_MOMENT_BAR
    assert cases.rel_err([opt.state[p]["exp_avg_sq"] for p in params], ref["exp_avg_sq"]) <= F32_MOMENT_BAR
    tr = opt.trust_ratios()
    assert max(abs(tr[p] - b) / b for p, b in zip(params, ref["trust"][-1])) <= F32_TRUST_BAR
    clip, G = opt.last_grad_norm.tolist()
    assert abs(G - ref["G"][-1]) <= 1e-6 * ref["G"][-1] and abs(clip - ref["clip"][-1]) <= 1e-6 * ref["clip"][-1]
    assert [g["step"] for g in opt.param_groups] == [cases.STEPS] * 2


def test_lamb_constructor_refusals():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-1.0), dict(eps=-1e-6), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1),
               dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            sm.Lamb(p, **kw)
    opt = sm.Lamb(p)     # timm's defaults
    assert opt.defaults == dict(lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True,
                                max_grad_norm=1.0, trust_clip=False, always_adapt=False)
    assert sm.Lamb.supports_device_scalars and sm.Lamb._slimmoe_refreshes_images and sm.Lamb.wants_grad_sumsq
    q = torch.nn.Parameter(torch.zeros(4, 4))
    q.grad = torch.zeros(4, 4).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        sm.Lamb([q]).step()


def test_lamb_state_dict_has_timms_layout_and_a_resume_equals_the_uninterrupted_run():
    setting = 0
    full, _ = _run(sm.Lamb, setting)
    params, opt = _run(sm.Lamb, setting, steps=5)
    sd = opt.state_dict()
    assert all(set(st) == {"exp_avg", "exp_avg_sq"} for st in sd["state"].values()) and len(sd["state"]) == len(cases.SHAPES)
    assert [g["step"] for g in sd["param_groups"]] == [5, 5]
    assert set(sd["param_groups"][0]) == {"lr", "bias_correction", "betas", "eps", "weight_decay", "grad_averaging", "max_grad_norm",
                                          "trust_clip", "always_adapt", "step", "params"}
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    resumed = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = cases.make_optimizer(sm.Lamb, resumed, setting)
    opt2.load_state_dict(torch.load(buf, weights_only=False))
    _run(sm.Lamb, setting, steps=cases.STEPS - 5, first=5, params=resumed, opt=opt2)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(resumed, full))
    assert [g["step"] for g in opt2.state_dict()["param_groups"]] == [cases.STEPS] * 2


def test_lamb_composition_honours_found_inf_and_grad_mult():
    setting = 1
    _, gscale, _, _ = cases.SETTINGS[setting]
    init = cases.initial_weights()
    # found_inf = 1: parameters, moments and the count are untouched
    params, opt = _run(sm.Lamb, setting, steps=2)
    before = [p.detach().clone() for p in params]
    moments = [opt.state[p]["exp_avg"].clone() for p in params]
    _run(sm.Lamb, setting, steps=1, first=2, params=params, opt=opt, found_inf=torch.ones(1))
    assert all(torch.equal(a.detach(), b) for a, b in zip(params, before))
    assert all(torch.equal(opt.state[p]["exp_avg"], m) for p, m in zip(params, moments))
    assert [g["step"] for g in opt.param_groups] == [2, 2]
    # grad_mult = 1/8 over gradients stored times 8 (a power of two: exact) == the plain run, found_inf = 0 steps
    a = [torch.nn.Parameter(t.clone()) for t in init]
    oa = cases.make_optimizer(sm.Lamb, a, setting)
    for grads in cases.gradients(gscale)[:3]:
        for p, g in zip(a, grads):
            p.grad = g * 8.0
        oa.step(grad_mult=torch.full((1,), 0.125), found_inf=torch.zeros(1))
    b, _ = _run(sm.Lamb, setting, steps=3)
    assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))


def test_lamb_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    fake = 4096                                            # never dereferenced: the argument checks come first

    def refused(rc, word):
        return rc != 0 and word in lib.smoe_last_error()

    assert refused(lib.smoe_lamb_clip(fake, 4, None, None, 1.0, None, None, None), b"null")
    assert refused(lib.smoe_lamb_clip(None, 4, None, None, 1.0, None, fake, None), b"null")
    assert refused(lib.smoe_lamb_clip(fake, -1, None, None, 1.0, None, fake, None), b"bad arguments")
    s1 = lambda tab=fake, hyp=fake, n_t=2, blk=fake, nb=3, dt=1, b1=0.9, b2=0.999, eps=1e-6, step=fake, norms=fake: \
        lib.smoe_lamb_stage1_multi(tab, hyp, n_t, blk, nb, dt, b1, b2, 0.1, eps, 1, step, None, None, None, norms, None)
    for kw in (dict(tab=None), dict(hyp=None), dict(blk=None), dict(step=None), dict(norms=None)):
        assert refused(s1(**kw), b"null"), kw
    for kw in (dict(n_t=-1), dict(nb=-1), dict(nb=1 << 31), dict(dt=77), dict(b1=1.0), dict(b2=-0.5), dict(eps=-1.0)):
        assert refused(s1(**kw), b"bad arguments"), kw
    tr = lambda norms=fake, nb=3, first=fake, hyp=fake, n_t=2, out=fake: \
        lib.smoe_lamb_trust_multi(norms, nb, first, hyp, n_t, 0, None, out, None)
    for kw in (dict(norms=None), dict(first=None), dict(hyp=None), dict(out=None)):
        assert refused(tr(**kw), b"null"), kw
    for kw in (dict(n_t=-1), dict(nb=-1), dict(nb=1 << 31)):
        assert refused(tr(**kw), b"bad arguments"), kw
    s2 = lambda tab=fake, hyp=fake, n_t=2, blk=fake, nb=3, b1=0.9, b2=0.999, eps=1e-6, step=fake, trust=fake: \
        lib.smoe_lamb_stage2_multi(tab, hyp, n_t, blk, nb, b1, b2, eps, 1, step, trust, None, None, None)
    for kw in (dict(tab=None), dict(hyp=None), dict(blk=None), dict(step=None), dict(trust=None)):
        assert refused(s2(**kw), b"null"), kw
    for kw in (dict(n_t=-1), dict(nb=-1), dict(nb=1 << 31), dict(b1=1.5), dict(b2=1.0), dict(eps=-1.0)):
        assert refused(s2(**kw), b"bad arguments"), kw
    # nothing to do is not an error (and launches nothing)
    assert s1(nb=0) == 0 and s2(nb=0) == 0 and tr(n_t=0) == 0


def test_graphed_step_hyper_changes_with_the_values_lamb_bakes_in():
    """engine.GraphedTrainStep._hyper(): trust_clip (and max_grad_norm, always_adapt, bias_correction, grad_averaging) are baked into
    the captured launches, so changing one must re-capture; optimizers without the optional method keep the old comparison."""
    from slim_switch_moe_vit_amd.engine import GraphedTrainStep
    model = torch.nn.Linear(4, 3)
    opt = sm.Lamb(model.parameters(), lr=1e-3)
    step = GraphedTrainStep(model, torch.nn.CrossEntropyLoss(), opt, sm.NativeScaler(), 1.0, False, 0.0, True)
    h0 = step._hyper()
    assert step._hyper() == h0
    for key, value in (("trust_clip", True), ("always_adapt", True), ("bias_correction", False), ("grad_averaging", False)):
        opt.param_groups[0][key] = value
        h1 = step._hyper()
        assert h1 != h0, key
        h0 = h1
    opt.defaults["max_grad_norm"] = None
    assert step._hyper() != h0
    adam = sm.AdamW(model.parameters(), lr=1e-3)
    s2 = GraphedTrainStep(model, torch.nn.CrossEntropyLoss(), adam, sm.NativeScaler(), 1.0, False, 0.0, True)
    a0 = s2._hyper()
    adam.param_groups[0]["lr"] = 2e-3
    assert s2._hyper() != a0


def test_restatement_matches_timm_where_timm_is_installed():
    timm_optim = pytest.importorskip("timm.optim")
    if not hasattr(timm_optim, "Lamb"):
        pytest.skip("this timm has no Lamb")
    for setting in range(len(cases.SETTINGS)):
        mgn, gscale, _, _ = cases.SETTINGS[setting]
        params = [torch.nn.Parameter(t.clone().double()) for t in cases.initial_weights()]
        opt = cases.make_optimizer(timm_optim.Lamb, params, setting)
        for grads in cases.gradients(gscale):
            for p, g in zip(params, grads):
                p.grad = g.double()
            opt.step()
        assert cases.rel_err(params, cases.reference(setting)["params"]) <= 1e-12
