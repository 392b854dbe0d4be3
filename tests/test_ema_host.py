"""CPU tests of optim.ModelEma, the timm.utils.ModelEma surface (main.py:599-606, engine.py:77-78, utils.py:214-221): the
constructor, timm's update line on CPU tensors, DataParallel keys, checkpoints, the independent copy's caches, and the refusal of
expert-parallel models."""
import copy
import inspect
import io

import pytest
import torch
import torch.nn as nn

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _cache, vit


def _net(seed=0, bn=True):
    torch.manual_seed(seed)
    if not bn:
        return nn.Sequential(nn.Flatten(), nn.Linear(12, 7), nn.ReLU(), nn.Linear(7, 5))
    return nn.Sequential(nn.Flatten(), nn.Linear(12, 7), nn.BatchNorm1d(7), nn.ReLU(), nn.Linear(7, 5))


def _timm_update(ema_sd, model_sd, decay):
    """timm.utils.ModelEma.update's line, applied by hand."""
    for k, ema_v in ema_sd.items():
        ema_v.copy_(ema_v * decay + (1. - decay) * model_sd[k].detach())


def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.1)


def test_constructor_matches_timm():
    params = list(inspect.signature(sm.ModelEma.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("model", inspect.Parameter.empty), ("decay", 0.9999), ("device", ""),
                                                     ("resume", "")]
    model = _net().train()
    ema = sm.ModelEma(model, 0.99996)
    assert ema.decay == 0.99996 and ema.device == "" and ema.ema_has_module is False
    assert ema.ema is not model and not ema.ema.training and model.training
    assert all(not p.requires_grad for p in ema.ema.parameters()) and all(p.requires_grad for p in model.parameters())
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(ema.ema.parameters(), model.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(ema.ema.state_dict().values(), model.state_dict().values()))
    assert sm.ModelEma is sm.optim.ModelEma


@pytest.mark.parametrize("decay", [0.99996, 0.9])
def test_three_updates_on_cpu_are_timms_line(decay):
    model = _net()
    ema = sm.ModelEma(model, decay)
    twin = {k: v.clone() for k, v in model.state_dict().items()}
    for i in range(3):
        _perturb(model, i)
        model.train()(torch.randn(4, 3, 2, 2))          # moves the BatchNorm buffers too (timm walks the buffers)
        ema.update(model)
        _timm_update(twin, model.state_dict(), decay)
    sd = ema.state_dict()
    assert list(sd) == list(twin)
    assert all(torch.equal(sd[k], twin[k]) for k in twin), [k for k in twin if not torch.equal(sd[k], twin[k])]
    assert sd["2.num_batches_tracked"].dtype == torch.int64       # an integer entry: timm's line, truncated back by copy_


def test_update_from_a_data_parallel_wrapped_model_reads_module_keys():
    model = _net()
    ema = sm.ModelEma(model, 0.9)
    twin = {k: v.clone() for k, v in model.state_dict().items()}
    _perturb(model, 3)
    wrapped = nn.DataParallel(model)
    assert all(k.startswith("module.") for k in wrapped.state_dict())
    ema.update(wrapped)
    _timm_update(twin, model.state_dict(), 0.9)
    assert all(torch.equal(ema.state_dict()[k], twin[k]) for k in twin)


def test_skip_flag_on_the_torch_path():
    model = _net()
    ema = sm.ModelEma(model, 0.9)
    before = {k: v.clone() for k, v in ema.state_dict().items()}
    _perturb(model, 1)
    ema.update(model, skip=torch.ones((), dtype=torch.float32))
    assert all(torch.equal(ema.state_dict()[k], before[k]) for k in before)
    ema.update(model, skip=torch.zeros((), dtype=torch.float32))
    _timm_update(before, model.state_dict(), 0.9)
    assert all(torch.equal(ema.state_dict()[k], before[k]) for k in before)


@pytest.mark.parametrize("prefixed", [False, True])
def test_load_checkpoint_from_a_path_and_from_bytes(tmp_path, prefixed):
    src = _net(1)
    sd = src.state_dict()
    if prefixed:
        sd = {"module." + k: v for k, v in sd.items()}
    # a plain EMA (timm keeps the saved keys as they are: an unwrapped EMA loads unprefixed ones)
    ema = sm.ModelEma(_net(2), 0.9)
    wrapped_ema = sm.ModelEma(nn.DataParallel(_net(2)), 0.9)
    assert wrapped_ema.ema_has_module
    path = tmp_path / "ckpt.pth"
    torch.save({"state_dict_ema": sd, "model": {}}, path)
    if not prefixed:
        ema._load_checkpoint(str(path))
        assert all(torch.equal(ema.state_dict()[k], v) for k, v in src.state_dict().items())
    wrapped_ema._load_checkpoint(str(path))           # timm's rule: "module." added where missing
    assert all(torch.equal(wrapped_ema.state_dict()[k], v) for k, v in src.state_dict().items())
    # utils._load_checkpoint_for_ema: torch.save({"state_dict_ema": checkpoint}) into a BytesIO
    buf = io.BytesIO()
    torch.save({"state_dict_ema": sd}, buf)
    buf.seek(0)
    other = sm.ModelEma(nn.DataParallel(_net(3)), 0.9)
    other._load_checkpoint(buf)
    assert all(torch.equal(other.state_dict()[k], v) for k, v in src.state_dict().items())
    # resume= at construction
    r = sm.ModelEma(nn.DataParallel(_net(4)), 0.9, resume=str(path))
    assert all(torch.equal(r.state_dict()[k], v) for k, v in src.state_dict().items())
    assert all(not p.requires_grad for p in r.ema.parameters())


def test_state_dict_is_unwrapped_and_there_is_no_module_attribute():
    ema = sm.ModelEma(nn.DataParallel(_net()), 0.9)
    assert not hasattr(ema, "module")      # timm.utils.unwrap_model falls through to .state_dict() for this class
    sd = ema.state_dict()
    assert sd and not any(k.startswith("module.") for k in sd)
    new = {k: v + 1 if v.is_floating_point() else v for k, v in sd.items()}
    ema.load_state_dict(new)
    assert all(torch.equal(ema.state_dict()[k], new[k]) for k in new)
    # what timm.utils.get_state_dict(model_ema) does for a class that is not timm's and has no .module
    unwrap = ema.module if hasattr(ema, "module") else ema
    assert list(unwrap.state_dict()) == list(_net().state_dict())


def test_the_copy_has_its_own_empty_weight_image_caches():
    """A deepcopy would share nothing but carry COPIES of the original's caches that _cache._ALL does not know; the EMA's caches are
    fresh objects of the same class, empty, reachable by invalidate_weight_images(), and still invalidated by load_state_dict."""
    model = sm.create_model("moe_tiny_patch16_224_expert8", num_classes=10, depth=2)
    lin = model.blocks[0].mlp.experts.htoh4
    lin._shadow._c[("probe", None)] = (0, torch.zeros(1), None, None)
    attn = model.blocks[0].attn
    hc = vit._half_cache(attn)
    hc._c[("probe", None)] = (0, torch.zeros(1), None, None)
    model.__dict__["_side_streams"] = [object()]                           # per-process plumbing is not copied at all
    ema = sm.ModelEma(model, 0.99996)
    assert "_side_streams" not in ema.ema.__dict__ and "_side_streams" in model.__dict__
    e_lin, e_attn = ema.ema.blocks[0].mlp.experts.htoh4, ema.ema.blocks[0].attn
    assert e_lin._shadow is not lin._shadow and type(e_lin._shadow) is type(lin._shadow) and not e_lin._shadow._c
    e_hc = e_attn.__dict__["_half"]
    assert e_hc is not hc and type(e_hc) is type(hc) and not e_hc._c
    assert e_lin._shadow in _cache._ALL and e_hc in _cache._ALL
    assert ("probe", None) in lin._shadow._c and ("probe", None) in hc._c      # the original's caches are untouched
    e_hc._c[("probe", None)] = (0, torch.zeros(1), None, None)
    e_lin._shadow._c[("probe", None)] = (0, torch.zeros(1), None, None)
    ema.load_state_dict(ema.state_dict())                                   # the copied post-hooks reach the EMA's own caches
    assert not e_hc._c and not e_lin._shadow._c
    e_hc._c[("probe", None)] = (0, torch.zeros(1), None, None)
    sm.invalidate_weight_images()
    assert not e_hc._c
    assert list(ema.state_dict()) == list(model.state_dict())
    assert any("threshold" in k for k in sm.ModelEma(sm.create_model("resmoe_tiny_patch16_224_expert8", num_classes=10,
                                                                       depth=2), 0.9).state_dict())


def test_expert_parallel_models_are_refused():
    m = sm.create_model("moe_tiny_patch16_224_expert4_top1", num_classes=5, depth=2, world_size=2)
    with pytest.raises(ValueError, match="expert-parallel"):
        sm.ModelEma(m, 0.9)
    single = sm.create_model("moe_tiny_patch16_224_expert4_top1", num_classes=5, depth=2)
    single.blocks[1].mlp.force_ep = True
    assert single.blocks[1].mlp.ep_active()
    with pytest.raises(ValueError, match="expert-parallel"):
        sm.ModelEma(single, 0.9)
    single.blocks[1].mlp.force_ep = False
    sm.ModelEma(single, 0.9)


def test_train_one_epoch_with_model_ema_and_an_enabled_scaler_skips_a_non_finite_step():
    """optim.ModelEma + an enabled optim.NativeScaler: no per-step read; a NaN loss leaves weights and EMA unchanged (the scaler
    skips the step, the EMA is skipped by the flag) and the abort comes at the end of the epoch; finite steps move the EMA by timm's
    line."""
    model = _net(bn=False)     # (a BatchNorm would move its buffers in the forward, after the criterion's snapshot)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    ema = sm.ModelEma(model, 0.9)
    data = [(torch.randn(4, 3, 2, 2), torch.randint(0, 5, (4,))) for _ in range(2)]
    seen = []

    def crit(out, y):
        seen.append({k: v.clone() for k, v in model.state_dict().items()})
        return nn.functional.cross_entropy(out, y)

    twin = {k: v.clone() for k, v in ema.state_dict().items()}
    st = sm.train_one_epoch(model, crit, data, opt, "cpu", 0, sm.NativeScaler(), None, ema)
    assert st["steps"] == 2
    weights = seen[1:] + [model.state_dict()]
    for w in weights:
        _timm_update(twin, w, 0.9)
    assert all(torch.equal(ema.state_dict()[k], twin[k]) for k in twin)

    def nan_crit(out, y):
        return nn.functional.cross_entropy(out, y) * float("nan")

    before = copy.deepcopy(model.state_dict())
    before_ema = copy.deepcopy(ema.state_dict())
    with pytest.raises(SystemExit):
        sm.train_one_epoch(model, nan_crit, data[:1], opt, "cpu", 1, sm.NativeScaler(), None, ema)
    assert all(torch.equal(model.state_dict()[k], v) for k, v in before.items())
    assert all(torch.equal(ema.state_dict()[k], v) for k, v in before_ema.items())


class _Dev:
    def __init__(self, dev):
        self.device = torch.device(dev)


class _ModelOnGpu(nn.Module):
    """A model whose parameters report cuda:0 (what any GPU tensor reports: its device always carries an index)."""

    def parameters(self, recurse=True):
        return iter([_Dev("cuda:0")])


class _EmaOn(sm.ModelEma):
    def __init__(self, dev):     # (no copy: only what GraphedTrainStep.supported() looks at)
        self.decay, self._dev = 0.9, dev

    def tensors(self):
        return [_Dev(self._dev)]


@pytest.mark.parametrize("device", ["cuda", torch.device("cuda"), "cuda:0", torch.device("cuda", 0)])
def test_graphed_step_accepts_a_model_ema_for_a_device_without_an_index(device):
    """The reference passes ``torch.device(args.device)`` with the default "cuda" (main.py:377, 831): an EMA on the model's device must
    be accepted for it exactly as for "cuda:0"; an EMA elsewhere, or one that is not this package's, keeps the step eager."""
    opt = sm.AdamW([nn.Parameter(torch.zeros(2))])
    scaler = sm.NativeScaler()
    supported = sm.GraphedTrainStep.supported
    assert supported(_ModelOnGpu(), opt, scaler, device, None)
    assert supported(_ModelOnGpu(), opt, scaler, device, _EmaOn("cuda:0"))
    assert not supported(_ModelOnGpu(), opt, scaler, device, _EmaOn("cpu"))
    assert not supported(_ModelOnGpu(), opt, scaler, device, _EmaOn("cuda:1"))

    class Foreign:
        decay = 0.9

        def update(self, m):
            pass
    assert not supported(_ModelOnGpu(), opt, scaler, device, Foreign())


def _tied_net(seed=0):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(6, 6), nn.ReLU(), nn.Linear(6, 6), nn.ReLU(), nn.Linear(6, 3))
    net[2].weight = net[0].weight            # one storage under two keys
    return net


def test_tied_weights_get_timms_line_once_per_key_in_order():
    """timm applies its line to a tied weight once per state-dict key, one after the other; the copy keeps the tie."""
    model = _tied_net()
    ema = sm.ModelEma(model, 0.9)
    assert ema.ema[2].weight is ema.ema[0].weight
    twin = copy.deepcopy(model)
    for i in range(2):
        _perturb(model, 10 + i)
        ema.update(model)
        _timm_update(twin.state_dict(), model.state_dict(), 0.9)
    assert all(torch.equal(ema.state_dict()[k], v) for k, v in twin.state_dict().items())
