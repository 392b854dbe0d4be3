"""GPU tests of optim.Lamb on its HIP kernels (csrc/lamb.hip: smoe_lamb_clip / _stage1_multi / _trust_multi / _stage2_multi) against
the float64 restatement of timm.optim.Lamb in tests/_lamb_cases.py, through optim.NativeScaler and through the graphed training step.

Bars (profiles/r17_lamb.md holds the measurements): errors are relative to max(1, max |reference|).  The same rule in f32 torch ops on
the CPU measures 2.0e-7 .. 2.6e-7 for the parameters on these inputs (tests/test_lamb_host.py); the kernels measured, on the MI355X,
parameters 2.04e-7 .. 2.98e-7 (the largest with bf16 gradients), moments <= 1.8e-7, trust ratios <= 2.03e-7 (relative), G and the
clip factor <= 3.9e-8 (relative) -- the f32 floor, no more.  Every bar is at most 3 x the largest figure measured for it."""
import copy
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

import _lamb_cases as cases  # noqa: E402
import slim_switch_moe_vit_amd as sm  # noqa: E402
from slim_switch_moe_vit_amd._cache import shadow_of  # noqa: E402

DEV = "cuda:0"
PARAM_BAR = 7.5e-7       # parameters after 12 steps (measured <= 2.98e-7)
MOMENT_BAR = 5.4e-7      # exp_avg / exp_avg_sq after 12 steps (measured <= 1.80e-7)
RESUME_BAR = 7e-7        # parameters after 5 float64 + 7 kernel steps from a timm-layout checkpoint (measured 2.38e-7)
TRUST_BAR = 6e-7         # trust ratios of the last step, relative (measured <= 2.03e-7)
NORM_BAR = 1.2e-7        # G and the clip factor, relative (measured <= 3.9e-8: one f32 rounding of a double sum of f32 block partials)
SCALER_BAR = 2.5e-7      # the MLP through NativeScaler against the float64 twin, absolute (measured 8.3e-8)
SCALER_NORM_BAR = 2.2e-7 # ... and its G, relative (measured 7.4e-8: an f32 forward and backward against float64)


def _device_params(values):
    return [torch.nn.Parameter(t.clone().to(DEV)) for t in values]


def _set_grads(params, grads, gdt, scale=1.0):
    for p, g in zip(params, grads):
        if gdt != torch.float32:
            p.grad_dtype = gdt          # torch >= 2.10: a gradient dtype other than the parameter's must be declared
        p.grad = (g * scale).to(gdt).to(DEV)


def _run(setting, gdt, steps=cases.STEPS, first=0, params=None, opt=None, scale=1.0, **step_kw):
    _, gscale, _, _ = cases.SETTINGS[setting]
    if params is None:
        params = _device_params(cases.initial_weights())
    if opt is None:
        opt = cases.make_optimizer(sm.Lamb, params, setting)
    for grads in cases.gradients(gscale, torch.float16 if gdt == torch.float32 else gdt)[first:first + steps]:
        _set_grads(params, grads, gdt, scale)
        opt.step(**step_kw)
    return params, opt


def _moments(opt, params):
    return [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params]


@pytest.mark.parametrize("gdt", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("setting", range(len(cases.SETTINGS)))
def test_lamb_kernels_match_the_float64_restatement(setting, gdt):
    """Two parameter groups, nine tensors, 12 steps: parameters, moments, the last step's trust ratios, G and the clip factor."""
    ref = cases.reference(setting, torch.float16 if gdt == torch.float32 else gdt)
    params, opt = _run(setting, gdt)
    m, v = _moments(opt, params)
    err = cases.rel_err(params, ref["params"])
    merr, verr = cases.rel_err(m, ref["exp_avg"]), cases.rel_err(v, ref["exp_avg_sq"])
    tr = opt.trust_ratios()
    terr = max(abs(tr[p] - b) / b for p, b in zip(params, ref["trust"][-1]))
    clip, G = opt.last_grad_norm.tolist()
    gerr, cerr = abs(G - ref["G"][-1]) / ref["G"][-1], abs(clip - ref["clip"][-1]) / ref["clip"][-1]
    print(f"LAMB setting {setting} {gdt}: parameters {err:.3e} exp_avg {merr:.3e} exp_avg_sq {verr:.3e} trust {terr:.3e} "
          f"G {gerr:.3e} clip {cerr:.3e}")
    assert err <= PARAM_BAR and merr <= MOMENT_BAR and verr <= MOMENT_BAR
    assert terr <= TRUST_BAR and gerr <= NORM_BAR and cerr <= NORM_BAR
    assert float(opt._step_counter(torch.device(DEV))) == float(cases.STEPS)
    assert [g["step"] for g in opt.state_dict()["param_groups"]] == [cases.STEPS] * 2


def test_a_tensor_stepped_alone_equals_the_same_tensor_in_the_nine_tensor_launch_bitwise():
    """With max_grad_norm=None nothing couples the tensors: every sum a tensor's update depends on has an order that depends on that
    tensor alone.  And two runs of the same steps are bit-equal."""
    setting, gdt, steps = 2, torch.float16, 3           # (None, 1.0, trust_clip, always_adapt)
    multi, om = _run(setting, gdt, steps=steps)
    again, oa = _run(setting, gdt, steps=steps)
    init = cases.initial_weights()
    _, gscale, trust_clip, always_adapt = cases.SETTINGS[setting]
    for j, t in enumerate(init):
        p = _device_params([t])[0]
        o = sm.Lamb([p], max_grad_norm=None, trust_clip=trust_clip, always_adapt=always_adapt, **cases.HYPER[cases.GROUP_OF[j]])
        for grads in cases.gradients(gscale, gdt)[:steps]:
            _set_grads([p], [grads[j]], gdt)
            o.step()
        assert torch.equal(p.detach(), multi[j].detach()), cases.SHAPES[j]
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(o.state[p][key], om.state[multi[j]][key]), (cases.SHAPES[j], key)
    for a, b in zip(multi, again):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(om.state[a]["exp_avg"], oa.state[b]["exp_avg"])
        assert torch.equal(om.state[a]["exp_avg_sq"], oa.state[b]["exp_avg_sq"])


def test_found_inf_leaves_everything_alone_and_grad_mult_equals_premultiplied_gradients():
    setting, gdt = 0, torch.float16
    params, opt = _run(setting, gdt, steps=2)
    before = [p.detach().clone() for p in params]
    m0, v0 = ([t.clone() for t in ts] for ts in _moments(opt, params))
    _run(setting, gdt, steps=1, first=2, params=params, opt=opt, found_inf=torch.ones(1, device=DEV))
    m1, v1 = _moments(opt, params)
    assert all(torch.equal(a.detach(), b) for a, b in zip(params, before))
    assert all(torch.equal(a, b) for a, b in zip(m0, m1)) and all(torch.equal(a, b) for a, b in zip(v0, v1))
    assert float(opt._step_counter(torch.device(DEV))) == 2.0, "a skipped step does not count"
    # every gradient times a device scalar == the same gradients multiplied beforehand (f32), within the bar of the kernels
    mult = torch.full((1,), 1.0 / 3.0, device=DEV)
    a, oa = _run(setting, gdt, steps=4, grad_mult=mult, found_inf=torch.zeros(1, device=DEV))
    b = _device_params(cases.initial_weights())
    ob = cases.make_optimizer(sm.Lamb, b, setting)
    for grads in cases.gradients(cases.SETTINGS[setting][1], gdt)[:4]:
        for p, g in zip(b, grads):
            p.grad = g.to(DEV) * mult
        ob.step()
    err = cases.rel_err(a, b)
    ga, gb = float(oa.last_grad_norm[1]), float(ob.last_grad_norm[1])
    print(f"LAMB grad_mult vs pre-multiplied gradients: parameters {err:.3e}, G {ga:.8g} vs {gb:.8g}")
    assert err <= PARAM_BAR and abs(ga - gb) <= NORM_BAR * gb


def test_found_inf_leaves_the_16_bit_images_alone_and_steps_keep_them_current():
    """The images the forward reads are written by stage 2: after steps an eval forward equals a freshly loaded copy's bit for bit; a
    step skipped on the device leaves images and weights as they were."""
    name, kw = "resmoe_tiny_patch16_224_expert8", dict(num_classes=10, depth=2)
    torch.manual_seed(0)
    model = sm.create_model(name, **kw).to(DEV)
    opt = sm.Lamb(model.parameters(), lr=2e-3, weight_decay=0.05)
    scaler = sm.NativeScaler(init_scale=1024.0)
    g = torch.Generator().manual_seed(11)
    batches = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(3)]
    w0 = model.head.weight.detach().clone()
    sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), batches, opt, DEV, 0, scaler, 1.0)
    assert float((model.head.weight.detach() - w0).abs().max()) > 0
    images = batches[0][0].to(DEV)

    def infer(m):
        m.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return m(images).float()

    def fresh_copy():
        m = sm.create_model(name, **kw)
        m.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        return m.to(DEV)

    assert torch.equal(infer(model), infer(fresh_copy())), "the 16-bit images are current after the steps"
    for blk in model.blocks:
        lin = blk.mlp.experts.htoh4
        assert torch.equal(lin.weight_as(torch.float16), lin.weight.detach().half())
    # a step with found_inf = 1: weights, images and the count stay
    model.train()
    with torch.autocast("cuda", dtype=torch.float16):
        loss = torch.nn.functional.cross_entropy(model(images).float(), batches[0][1].to(DEV))
    opt.zero_grad()
    loss.backward()
    held = [(p, shadow_of(p)) for p in model.parameters() if p.grad is not None]
    held = [(p, sh[2], sh[2].clone(), p.detach().clone()) for p, sh in held if sh is not None]
    assert held, "the forward left 16-bit images of its weights behind"
    count = float(opt._step_counter(torch.device(DEV)))
    opt.step(found_inf=torch.ones(1, device=DEV))
    for p, img, img0, p0 in held:
        assert torch.equal(img, img0) and torch.equal(p.detach(), p0)
    assert float(opt._step_counter(torch.device(DEV))) == count
    # ... and an applied one writes them: every image equals the cast of its parameter
    opt.step()
    assert any(not torch.equal(p.detach(), p0) for p, _, _, p0 in held)
    for p, img, _, _ in held:
        assert torch.equal(img, p.detach().to(img.dtype))
    assert torch.equal(infer(model), infer(fresh_copy()))


def test_lamb_through_native_scaler_matches_the_stock_sequence_on_a_float64_twin():
    """scale -> backward -> (unscale, clip_grad_norm_, Lamb.step, update) with the scaler's norm-pass partials handed to the optimizer
    == the stock sequence around the restated rule on a float64 twin: clip_grad engages, Lamb's own max_grad_norm engages on the
    clipped gradients, a poisoned step is skipped and not counted, the scale grows and backs off."""
    torch.manual_seed(0)
    lin = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.GELU(), torch.nn.Linear(128, 10)).to(DEV)
    twin = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.GELU(), torch.nn.Linear(128, 10)).double()
    twin.load_state_dict({k: v.double().cpu() for k, v in lin.state_dict().items()})
    hyper = dict(lr=1e-2, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-6)
    lamb_norm = 0.25
    opt = sm.Lamb(lin.parameters(), max_grad_norm=lamb_norm, **hyper)
    sc = sm.NativeScaler(init_scale=1024.0, growth_interval=3)
    max_norm = 0.5
    tp = list(twin.parameters())
    m = v = None
    applied = 0
    g = torch.Generator().manual_seed(1)
    scales, worst_g = [], 0.0
    for it in range(7):
        x = torch.randn(32, 64, generator=g)
        y = torch.randint(0, 10, (32,), generator=g)
        poison = (it == 4)
        loss = torch.nn.functional.cross_entropy(lin(x.to(DEV)), y.to(DEV))
        if poison:
            loss = loss + float("inf") * lin[0].weight.sum() * 0   # nan gradients on one tensor
        opt.zero_grad()
        before = [p.detach().clone() for p in lin.parameters()]
        sc(loss, opt, clip_grad=max_norm, parameters=lin.parameters())
        scales.append(sc.get_scale())
        if poison:
            for p, q in zip(lin.parameters(), before):
                assert torch.equal(p.detach(), q), "a non-finite step must leave the parameters alone"
            continue
        rl = torch.nn.functional.cross_entropy(twin(x.double()), y)
        twin.zero_grad()
        rl.backward()
        norm = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        assert float(norm) > max_norm, "the test must exercise clipping"
        out = cases.lamb_steps([p.detach() for p in tp], [[p.grad for p in tp]], [0] * len(tp), [hyper], max_grad_norm=lamb_norm,
                               exp_avg=m, exp_avg_sq=v, first_step=applied + 1)
        applied += 1
        m, v = out["exp_avg"], out["exp_avg_sq"]
        with torch.no_grad():
            for p, q in zip(tp, out["params"]):
                p.copy_(q)
        assert out["clip"][0] > 1.0, "Lamb's own clip engages on the clipped gradients"
        G = float(opt.last_grad_norm[1])
        worst_g = max(worst_g, abs(G - out["G"][0]) / out["G"][0])
        assert abs(float(sc.last_grad_norm) - float(norm)) <= 1e-4 * float(norm)
    err = max(float((p.detach().cpu().double() - q.detach()).abs().max()) for p, q in zip(lin.parameters(), tp))
    print(f"LAMB through NativeScaler vs the float64 twin: parameters {err:.3e} (absolute), G {worst_g:.3e} (relative)")
    assert err <= SCALER_BAR
    assert worst_g <= SCALER_NORM_BAR, "G is the norm of the unscaled, clipped gradients"
    assert float(opt._step_counter(torch.device(DEV))) == 6.0, "the skipped step does not count"
    assert scales == [1024.0, 1024.0, 2048.0, 2048.0, 1024.0, 1024.0, 1024.0], scales
    assert [gr["step"] for gr in opt.state_dict()["param_groups"]] == [6]


def test_training_harness_with_lamb_on_one_hip_graph_reproduces_the_eager_harness():
    """engine.train_one_epoch(hip_graph=True) with sm.Lamb: the model and the 9 batches of
    test_training_harness_on_one_hip_graph_reproduces_the_eager_harness; parameters, moments, scaler state and mean loss bit for bit."""
    name, kw = "resmoe_tiny_patch16_224_expert8", dict(num_classes=10, depth=2, starting_threshold=0.55, target_threshold=0.5)
    g = torch.Generator().manual_seed(70)
    batches = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(9)]

    def run(graph):
        torch.manual_seed(0)
        model = sm.create_model(name, **kw)
        with torch.no_grad():
            for n_, p in model.named_parameters():
                if "_gate.head.1.weight" in n_:
                    p.normal_(0, 0.3, generator=torch.Generator().manual_seed(5))
        model = model.to(DEV)
        opt = sm.Lamb(model.parameters(), lr=1e-3, weight_decay=0.05)
        scaler = sm.NativeScaler()
        stats = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), batches, opt, DEV, 0, scaler, 1.0, hip_graph=graph)
        moments = [opt.state[p][k].clone() for p in model.parameters() if p in opt.state for k in ("exp_avg", "exp_avg_sq")]
        steps = [gr["step"] for gr in opt.state_dict()["param_groups"]]
        return stats, [p.detach().clone() for p in model.parameters()], moments, scaler.state_dict(), steps

    s_e, p_e, m_e, sc_e, n_e = run(False)
    s_g, p_g, m_g, sc_g, n_g = run(True)
    assert s_g["hip_graph_steps"] == 6 and s_e["hip_graph_steps"] == 0
    assert s_g["loss"] == s_e["loss"], (s_g, s_e)
    assert all(torch.equal(a, b) for a, b in zip(p_e, p_g)), "parameters after 9 steps"
    assert m_e and all(torch.equal(a, b) for a, b in zip(m_e, m_g)), "Lamb moments after 9 steps"
    assert sc_e == sc_g and n_e == n_g, (sc_e, sc_g, n_e, n_g)


def test_lamb_checkpoint_round_trip_in_timms_layout():
    """A timm-layout dict (state = {exp_avg, exp_avg_sq}, 'step' in the groups) taken from the float64 run after 5 steps loads; the 7
    steps after it land on the uninterrupted run; state_dict() gives the layout back with the device-side count."""
    setting, gdt, cut = 0, torch.float16, 5
    mgn, gscale, trust_clip, always_adapt = cases.SETTINGS[setting]
    half = cases.lamb_steps(cases.initial_weights(), cases.gradients(gscale)[:cut], cases.GROUP_OF, cases.HYPER, max_grad_norm=mgn,
                            trust_clip=trust_clip, always_adapt=always_adapt)
    groups, at = [], 0
    for grp, h in zip(cases.GROUPS, cases.HYPER):
        n = len(grp["shapes"])
        groups.append(dict(h, bias_correction=True, grad_averaging=True, max_grad_norm=mgn, trust_clip=trust_clip,
                           always_adapt=always_adapt, step=cut, params=list(range(at, at + n))))
        at += n
    timm_sd = {"state": {j: {"exp_avg": half["exp_avg"][j].float(), "exp_avg_sq": half["exp_avg_sq"][j].float()}
                         for j in range(len(cases.SHAPES))}, "param_groups": groups}
    buf = io.BytesIO()
    torch.save(timm_sd, buf)
    buf.seek(0)
    params = _device_params([t.float() for t in half["params"]])
    opt = cases.make_optimizer(sm.Lamb, params, setting)
    opt.load_state_dict(torch.load(buf, weights_only=False))
    _run(setting, gdt, steps=cases.STEPS - cut, first=cut, params=params, opt=opt)
    err = cases.rel_err(params, cases.reference(setting)["params"])
    print(f"LAMB resumed from a timm-layout checkpoint: parameters {err:.3e}")
    assert err <= RESUME_BAR
    assert float(opt._step_counter(torch.device(DEV))) == float(cases.STEPS)
    sd = opt.state_dict()
    assert [gr["step"] for gr in sd["param_groups"]] == [cases.STEPS] * 2
    assert all(set(st) == {"exp_avg", "exp_avg_sq"} for st in sd["state"].values()) and len(sd["state"]) == len(cases.SHAPES)
    assert all(st["exp_avg"].is_cuda and st["exp_avg"].dtype == torch.float32 for st in sd["state"].values())
    # ... and out again: a second instance resumed from it takes the same next step, bit for bit
    again = _device_params([p.detach().cpu() for p in params])
    opt2 = cases.make_optimizer(sm.Lamb, again, setting)
    opt2.load_state_dict(copy.deepcopy(sd))      # (load_state_dict keeps tensors that already match: not the first instance's own)
    for ps, o in ((params, opt), (again, opt2)):
        _set_grads(ps, cases.gradients(gscale)[0], gdt)
        o.step()
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(params, again))
    assert float(opt2._step_counter(torch.device(DEV))) == float(cases.STEPS + 1)


IMAGE_NUMELS = [3, 5, 16385]      # the scalar tail alone; one 16-byte vector and a tail; a second block
NAN16 = 0x7FA5                    # a NaN in f16 and in bf16: what an image holds before a step writes it


def _image_step(kind, img_dt, found):
    """One fused step of `kind` ("adamw": smoe_adamw_step_multi; "lamb": stage 1, trust ratios, stage 2) over three tensors from the
    same seeded state, every tensor with a 16-bit image of `img_dt`, found_inf = `found`: (p before, p after, images)."""
    from slim_switch_moe_vit_amd import _lib, ops, optim
    lib, dev = _lib.load(), torch.device(DEV)
    gen = torch.Generator().manual_seed(7)
    p0 = [torch.randn(n, generator=gen) * 0.5 for n in IMAGE_NUMELS]
    ps = [t.clone().to(DEV) for t in p0]
    gs = [(torch.randn(n, generator=gen) * 1e-2).half().to(DEV) for n in IMAGE_NUMELS]
    ms = [(torch.randn(n, generator=gen) * 1e-2).to(DEV) for n in IMAGE_NUMELS]
    vs = [(torch.rand(n, generator=gen) * 1e-4).to(DEV) for n in IMAGE_NUMELS]
    imgs = [torch.full((n,), NAN16, dtype=torch.int16, device=DEV) for n in IMAGE_NUMELS]
    n_t = len(ps)
    blk, nb = optim._block_table(IMAGE_NUMELS, dev)
    tab = torch.tensor([[t.data_ptr() for t in ts] for ts in (ps, gs, ms, vs)] + [IMAGE_NUMELS], dtype=torch.int64, device=DEV)
    shadow = torch.tensor([[t.data_ptr() for t in imgs], [ops.dtype_code(img_dt)] * n_t], dtype=torch.int64, device=DEV)
    step = torch.tensor([3.0], device=DEV)
    found_inf = torch.full((1,), float(found), device=DEV)
    f16 = ops.dtype_code(torch.float16)
    if kind == "adamw":
        hyp = torch.tensor([[1e-2] * n_t, [0.05] * n_t], dtype=torch.float32, device=DEV)
        rc = lib.smoe_adamw_step_multi(tab.data_ptr(), hyp.data_ptr(), n_t, blk.data_ptr(), sum(nb), f16, 0.9, 0.999, 1e-8,
                                       step.data_ptr(), None, found_inf.data_ptr(), shadow.data_ptr(), None)
        _lib.check(rc, "smoe_adamw_step_multi")
    else:
        hyp = torch.tensor([[1e-2] * n_t, [0.05] * n_t, [1.0] * n_t], dtype=torch.float32, device=DEV)
        first = optim._first_block_table(IMAGE_NUMELS, dev)
        norms = torch.zeros((2, sum(nb)), device=DEV)
        trust = torch.ones(n_t, device=DEV)
        rc = lib.smoe_lamb_stage1_multi(tab.data_ptr(), hyp.data_ptr(), n_t, blk.data_ptr(), sum(nb), f16, 0.9, 0.999, 0.1, 1e-6, 1,
                                        step.data_ptr(), None, None, found_inf.data_ptr(), norms.data_ptr(), None)
        _lib.check(rc, "smoe_lamb_stage1_multi")
        rc = lib.smoe_lamb_trust_multi(norms.data_ptr(), sum(nb), first.data_ptr(), hyp.data_ptr(), n_t, 0, found_inf.data_ptr(),
                                       trust.data_ptr(), None)
        _lib.check(rc, "smoe_lamb_trust_multi")
        rc = lib.smoe_lamb_stage2_multi(tab.data_ptr(), hyp.data_ptr(), n_t, blk.data_ptr(), sum(nb), 0.9, 0.999, 1e-6, 1,
                                        step.data_ptr(), trust.data_ptr(), found_inf.data_ptr(), shadow.data_ptr(), None)
        _lib.check(rc, "smoe_lamb_stage2_multi")
    torch.cuda.synchronize()
    return p0, ps, imgs


@pytest.mark.parametrize("img_dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_the_16_bit_image_a_fused_step_writes_is_the_cast_of_the_new_weights_bitwise(kind, img_dt):
    """AdamW's launch and LAMB's stage 2 write the image of every tensor through one store (csrc/optim_table.h): every element, in the
    scalar tail, the vector body and a second block, is the round-to-nearest-even cast of the new f32 weight (finite values: torch's
    `.to()` is that cast); a step skipped by found_inf leaves image and weights as they were."""
    p0, ps, imgs = _image_step(kind, img_dt, 0)
    for a, p, img in zip(p0, ps, imgs):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.cpu(), a), "the step moved the weights"
        assert torch.equal(img, p.to(img_dt).view(torch.int16)), (kind, img_dt, p.numel())
    p0, ps, imgs = _image_step(kind, img_dt, 1)
    for a, p, img in zip(p0, ps, imgs):
        assert torch.equal(p.cpu(), a) and bool((img == NAN16).all()), (kind, img_dt, p.numel())
