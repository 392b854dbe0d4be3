"""GPU tests of the weight EMA (timm.utils.ModelEma surface, main.py:599-606 / engine.py:77-78): the kernel
smoe_ema_update_multi against torch's `ema * decay + (1. - decay) * model`, optim.ModelEma on a model trained by optim.AdamW, the
EMA inside the graphed training step, the overflow / non-finite-loss paths of train_one_epoch, and evaluate() on the EMA model."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import slim_switch_moe_vit_amd as sm  # noqa: E402

DEV = "cuda:0"
SIZES = [(8, 96, 64), (3, 7), (1,), (40001,), (0,)]


def _timm_line(ema_sd, model_sd, decay):
    for k, ema_v in ema_sd.items():
        ema_v.copy_(ema_v * decay + (1. - decay) * model_sd[k].detach())


def _pairs(seed):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(s, generator=g).to(DEV) for s in SIZES], [torch.randn(s, generator=g).to(DEV) for s in SIZES])


@pytest.mark.parametrize("decay", [0.99996, 0.9])
def test_kernel_is_bit_equal_to_torch(decay):
    emas, models = _pairs(0)
    want = [e * decay + (1. - decay) * m for e, m in zip(emas, models)]
    one = [e.clone() for e in emas]
    sm.optim.ema_update_(one, models, decay)                      # every tensor in one launch
    each = [e.clone() for e in emas]
    for e, m in zip(each, models):                                # one launch per tensor
        sm.optim.ema_update_([e], [m], decay)
    torch.cuda.synchronize()
    for a, b, c in zip(one, each, want):
        assert torch.equal(a, c) and torch.equal(b, c)
    # f32(1 - decay) with the difference in double, as torch takes it: NOT 1.0f - f32(decay) (for 0.99996 they differ)
    if decay == 0.99996:
        f = torch.tensor(decay, dtype=torch.float32)
        assert float(torch.tensor(1. - decay, dtype=torch.float32)) != float(1 - f)
    skip = torch.ones(1, dtype=torch.float32, device=DEV)
    kept = [e.clone() for e in one]
    sm.optim.ema_update_(one, models, decay, skip=skip)
    assert all(torch.equal(a, b) for a, b in zip(one, kept)), "a set skip flag writes nothing"
    skip.zero_()
    sm.optim.ema_update_(one, models, decay, skip=skip)
    assert all(torch.equal(a, b * decay + (1. - decay) * m) for a, b, m in zip(one, kept, models))


def _images(n=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 224, 224, generator=g), torch.randint(0, 10, (n,), generator=g)


def test_model_ema_follows_adamw_steps_and_its_images_are_current():
    torch.manual_seed(0)
    name, kw = "moe_tiny_patch16_224_expert8", dict(num_classes=10, depth=2)
    model = sm.create_model(name, **kw).to(DEV)
    x, y = _images()
    x, y = x.to(DEV), y.to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        model.eval()(x)                           # the original's caches are filled before the copy
    model.train()
    ema = sm.ModelEma(model, 0.99996)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ema.ema(x)                                # ... and the EMA's own image cache
    twin = {k: v.clone() for k, v in ema.state_dict().items()}
    opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    for _ in range(5):
        with torch.autocast("cuda", dtype=torch.float16):
            loss = torch.nn.functional.cross_entropy(model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        ema.update(model)
        _timm_line(twin, model.state_dict(), 0.99996)
    sd = ema.state_dict()
    assert list(sd) == list(twin)
    assert all(torch.equal(sd[k], twin[k]) for k in twin), [k for k in twin if not torch.equal(sd[k], twin[k])][:5]
    assert not all(torch.equal(sd[k], v) for k, v in model.state_dict().items())
    fresh = sm.create_model(name, **kw)
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()})
    fresh = fresh.to(DEV).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(ema.ema(x).float(), fresh(x).float()), "the EMA model's 16-bit images follow its updates"


RES, RES_KW = "resmoe_tiny_patch16_224_expert8", dict(num_classes=10, depth=2, starting_threshold=0.55, target_threshold=0.5)


def _resmoe():
    torch.manual_seed(0)
    model = sm.create_model(RES, **RES_KW)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if "_gate.head.1.weight" in n_:
                p.normal_(0, 0.3, generator=torch.Generator().manual_seed(5))
    return model.to(DEV)


def test_graphed_training_step_with_model_ema_reproduces_the_eager_harness():
    g = torch.Generator().manual_seed(70)
    batches = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(9)]

    def run(graph):
        model = _resmoe()
        opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
        scaler = sm.NativeScaler()
        ema = sm.ModelEma(model, 0.99996)
        start = {k: v.clone() for k, v in ema.state_dict().items()}
        snaps = []
        ce = torch.nn.CrossEntropyLoss()

        def crit(out, y):
            if not graph:                   # the weights this step starts from (= those the previous step left)
                snaps.append({k: v.detach().clone() for k, v in model.state_dict().items()})
            return ce(out, y)
        stats = sm.train_one_epoch(model, crit, batches, opt, DEV, 0, scaler, 1.0, ema, hip_graph=graph)
        moments = [opt.state[p]["exp_avg"].clone() for p in model.parameters() if p in opt.state]
        moments += [opt.state[p]["exp_avg_sq"].clone() for p in model.parameters() if p in opt.state]
        final = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return stats, final, moments, scaler.state_dict(), {k: v.clone() for k, v in ema.state_dict().items()}, start, snaps

    s_e, p_e, m_e, sc_e, ema_e, start, snaps = run(False)
    s_g, p_g, m_g, sc_g, ema_g, _, _ = run(True)
    assert s_g["hip_graph_steps"] == 6 and s_e["hip_graph_steps"] == 0
    assert s_g["loss"] == s_e["loss"], (s_g, s_e)
    assert all(torch.equal(p_e[k], p_g[k]) for k in p_e), "parameters after 9 steps"
    assert all(torch.equal(a, b) for a, b in zip(m_e, m_g)), "AdamW moments after 9 steps"
    assert sc_e == sc_g
    assert all(torch.equal(ema_e[k], ema_g[k]) for k in ema_e), "EMA after 9 steps"
    assert len(snaps) == 9
    twin = start
    for w in snaps[1:] + [p_e]:
        _timm_line(twin, w, 0.99996)
    assert all(torch.equal(ema_e[k], twin[k]) for k in twin), "the eager harness' EMA is timm's line after every step"


def test_overflowing_step_moves_the_ema_and_a_nan_loss_moves_nothing():
    x, y = _images(8, 11)
    model = _resmoe()
    opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    ema = sm.ModelEma(model, 0.9)
    w0 = {k: v.clone() for k, v in model.state_dict().items()}
    twin = {k: v.clone() for k, v in ema.state_dict().items()}
    # gradients overflow (loss x 2^40 in the f16 backward), the loss itself is finite: AdamW skips, the EMA still moves
    scaler = sm.NativeScaler(init_scale=2.0 ** 40)
    sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), [(x, y)], opt, DEV, 0, scaler, None, ema)
    assert scaler.get_scale() < 2.0 ** 40, "the step overflowed"
    assert all(torch.equal(model.state_dict()[k], v) for k, v in w0.items()), "an overflowed step leaves the weights"
    _timm_line(twin, w0, 0.9)
    assert all(torch.equal(ema.state_dict()[k], twin[k]) for k in twin)
    assert not all(torch.equal(twin[k], w0[k]) for k in twin if twin[k].is_floating_point())

    def nan_crit(out, t):
        return torch.nn.functional.cross_entropy(out, t) * float("nan")
    kept = {k: v.clone() for k, v in ema.state_dict().items()}
    with pytest.raises(SystemExit):
        sm.train_one_epoch(model, nan_crit, [(x, y)], opt, DEV, 1, sm.NativeScaler(), None, ema)
    assert all(torch.equal(model.state_dict()[k], v) for k, v in w0.items()), "a NaN loss leaves the weights"
    assert all(torch.equal(ema.state_dict()[k], v) for k, v in kept.items()), "a NaN loss leaves the EMA"


def test_evaluate_on_the_ema_model_replays_like_any_model():
    model = _resmoe()
    ema = sm.ModelEma(model, 0.9)
    opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    data = [_images(8, s) for s in (21, 22)]
    sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), data, opt, DEV, 0, sm.NativeScaler(), None, ema)
    loader = [_images(8, s) for s in (31, 32, 33)]
    got = sm.evaluate(loader, ema.ema, DEV)
    assert got["hip_graph"]
    fresh = sm.create_model(RES, **RES_KW)
    fresh.load_state_dict({k: v.cpu() for k, v in ema.state_dict().items()})
    want = sm.evaluate(loader, fresh.to(DEV), DEV)
    assert (got["loss"], got["acc1"], got["acc5"]) == (want["loss"], want["acc1"], want["acc5"])


@pytest.mark.parametrize("device", ["cuda", torch.device("cuda")])
def test_graphed_step_with_model_ema_for_the_reference_device_value(device):
    """main.py passes ``torch.device(args.device)``, default "cuda" (no index): the step with a ModelEma is still captured."""
    g = torch.Generator().manual_seed(71)
    batches = [(torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(5)]
    model = _resmoe()
    opt = sm.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    ema = sm.ModelEma(model, 0.99996)
    st = sm.train_one_epoch(model, torch.nn.CrossEntropyLoss(), batches, opt, device, 0, sm.NativeScaler(), 1.0, ema, hip_graph=True)
    assert st["hip_graph_steps"] == 2


def test_tied_weights_on_the_gpu_are_timms_line_once_per_key():
    """A storage under two state-dict keys is updated twice, in order, as timm does -- not by two racing workgroups of one launch."""
    import copy
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.Linear(256, 10))
    model[2].weight = model[0].weight
    model = model.to(DEV)
    ema = sm.ModelEma(model, 0.9)
    twin = copy.deepcopy(model)
    for i in range(3):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(i)).to(DEV))
        ema.update(model)
        _timm_line(twin.state_dict(), model.state_dict(), 0.9)
    assert all(torch.equal(ema.state_dict()[k], v) for k, v in twin.state_dict().items())
