"""CPU tests of DeiT distillation: the ``DistillationLoss`` fixture made by the reference's own class and the class on its torch lines,
what the library answers for the three new entry points without a GPU, and ``DistilledVisionTransformer`` (keys, shapes, outputs,
factories, MoE patching)."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "slimmoe.h")
GOLDEN = os.path.join(HERE, "golden", "distill")
NEW = ["smoe_embed_ln2", "smoe_distill_fwd", "smoe_distill_bwd"]
CASES = [(kind, tau, alpha, B, C) for kind, tau in (("soft", 1.0), ("soft", 3.0), ("hard", 1.0)) for alpha in (0.5, 0.1)
         for B, C in ((5, 37), (3, 1000))]


REFERENCE_HERE = os.path.exists(os.path.join(os.environ.get("SLIMMOE_REFERENCE", "/root/reference"), "losses.py"))


def _name(kind, tau, alpha, B, C):
    return f"{kind}_tau{tau:g}_alpha{alpha:g}_{B}x{C}"


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "ref_distill_loss.npz"))


# ------------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.skipif(not REFERENCE_HERE, reason="the reference's losses.py is not on this machine")
def test_fixture_regenerates_bit_for_bit(tmp_path, fixture):
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_distill.py")], env=dict(os.environ, SLIMMOE_GOLDEN_OUT=str(tmp_path)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    new = np.load(os.path.join(tmp_path, "ref_distill_loss.npz"))
    assert sorted(new.files) == sorted(fixture.files) and len(new.files) == 10 * len(CASES)
    for key in fixture.files:
        a, b = fixture[key], new[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


def test_fixture_holds_every_case_and_the_hard_rows_are_tied(fixture):
    for case in CASES:
        n = _name(*case)
        kind, _, _, B, C = case
        assert fixture[n + "/kd"].shape == (B, C) and fixture[n + "/kd"].dtype == np.float32
        assert fixture[n + "/dkd_f64"].dtype == np.float64 and fixture[n + "/labels"].dtype == np.int64
        if kind == "hard":
            t = fixture[n + "/teacher"]
            for row in (0, 1):
                assert int((t[row] == t[row].max()).sum()) == 2, "two exact ties at the maximum"


@pytest.mark.parametrize("case", CASES, ids=lambda c: _name(*c))
def test_distillation_loss_on_cpu_equals_the_references_results(fixture, case):
    kind, tau, alpha, B, C = case
    n = _name(*case)
    torch.set_num_threads(1)
    labels = torch.from_numpy(fixture[n + "/labels"])
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        cls = torch.from_numpy(fixture[n + "/cls"]).to(dt).requires_grad_(True)
        kd = torch.from_numpy(fixture[n + "/kd"]).to(dt).requires_grad_(True)
        teacher = torch.from_numpy(fixture[n + "/teacher"]).to(dt)
        seen = []

        def teacher_model(inp):
            seen.append((inp, torch.is_grad_enabled()))
            return teacher
        crit = sm.DistillationLoss(F.cross_entropy, teacher_model, kind, alpha, tau)
        inputs = torch.zeros(1)
        loss = crit(inputs, (cls, kd), labels)
        loss.backward()
        assert seen[0][0] is inputs and seen[0][1] is False, "the teacher sees the inputs, under no_grad"
        want = [torch.from_numpy(fixture[f"{n}/{k}_{tag}"]) for k in ("loss", "dcls", "dkd")]
        if tag == "f32":
            same = [torch.equal(loss.detach(), want[0]), torch.equal(cls.grad, want[1]), torch.equal(kd.grad, want[2])]
            if REFERENCE_HERE:
                # where the fixture regenerates bit for bit (the test above), the class's torch lines give the stored bits
                assert all(same), same
            else:
                # another CPU's exp / log may round differently from the one that made the fixture: there the stored f32 results hold
                # up to the fixture's own f32 error against its float64 results, three times over (at least one f32 ulp of the largest value)
                for got, w32, key in ((loss.detach(), want[0], "loss"), (cls.grad, want[1], "dcls"), (kd.grad, want[2], "dkd")):
                    w64 = torch.from_numpy(fixture[f"{n}/{key}_f64"])
                    top = float(w64.abs().max())
                    bar = max(3 * float((w32.double() - w64).abs().max()), 2.0 ** (np.floor(np.log2(top)) - 23))
                    assert float((got.double() - w64).abs().max()) <= bar, (key, bar)
        else:
            assert abs(loss.item() - want[0].item()) <= 1e-12
            assert (cls.grad - want[1]).abs().max().item() <= 1e-12 and (kd.grad - want[2]).abs().max().item() <= 1e-12


def test_constructor_assert_none_type_and_the_tuple_error():
    with pytest.raises(AssertionError):
        sm.DistillationLoss(F.cross_entropy, None, "medium", 0.5, 1.0)
    x, labels = torch.randn(4, 10), torch.randint(0, 10, (4,))
    called = []
    crit = sm.DistillationLoss(F.cross_entropy, lambda inp: called.append(1), "none", 0.5, 1.0)
    assert torch.equal(crit(None, x, labels), F.cross_entropy(x, labels))
    assert torch.equal(crit(None, (x, torch.randn(4, 10)), labels), F.cross_entropy(x, labels)) and not called
    for kind in ("soft", "hard"):
        crit = sm.DistillationLoss(F.cross_entropy, lambda inp: torch.randn(4, 10), kind, 0.5, 1.0)
        with pytest.raises(ValueError, match="Tuple\\[Tensor, Tensor\\]"):
            crit(None, x, labels)
    crit = sm.DistillationLoss(F.cross_entropy, torch.nn.Identity(), "soft", 0.25, 2.0)
    assert isinstance(crit, torch.nn.Module) and sm.DistillationLoss is sm.loss.DistillationLoss
    assert (crit.base_criterion, crit.distillation_type, crit.alpha, crit.tau) == (F.cross_entropy, "soft", 0.25, 2.0)
    assert isinstance(crit.teacher_model, torch.nn.Identity)
    assert sm.engine._criterion_takes_inputs(crit), "train_one_epoch calls it as criterion(samples, outputs, targets)"
    # a base criterion that returns shape [1] keeps the reference's result shape and gets its gradient
    kd = torch.randn(4, 10, requires_grad=True)
    xs = x.clone().requires_grad_(True)
    out = sm.DistillationLoss(lambda o, l: F.cross_entropy(o, l).reshape(1), lambda inp: torch.randn(4, 10), "soft", 0.5, 1.0)(None, (xs, kd), labels)
    assert out.shape == (1,)
    out.sum().backward()
    assert xs.grad is not None and kd.grad is not None


# ----------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_are_declared_prototyped_and_exported_and_the_abi_stays_29():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
        assert hasattr(lib, s), f"libslimmoe_hip.so does not export {s}"
        n_args = len([a for a in re.search(r"%s\s*\((.*?)\)" % s, text, re.S).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[s][1]), s
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    assert _lib.binary_build_id() == _lib.source_build_id()


def test_argument_checks_come_before_any_launch():
    lib = _lib.load()
    fake = 4096          # never dereferenced

    def fwd(student=fake, sd=0, teacher=fake, td=0, mode=0, tau=1.0, B=4, C=10, base=fake, loss=fake):
        return lib.smoe_distill_fwd(student, sd, teacher, td, mode, tau, 0.5, base, B, C, fake, fake, fake, fake, loss, None)

    def bwd(student=fake, sd=0, teacher=fake, td=0, mode=0, tau=1.0, B=4, C=10, g=fake, out=fake):
        return lib.smoe_distill_bwd(student, sd, teacher, td, mode, tau, 0.5, B, C, fake, fake, g, out, None)

    for f in (fwd, bwd):
        assert f(B=0) == 0                                       # B == 0 returns at once
        assert f(student=None) != 0 and b"null" in lib.smoe_last_error()
        assert f(teacher=None) != 0 and b"null" in lib.smoe_last_error()
        assert f(sd=7) != 0 and b"dtype" in lib.smoe_last_error()
        assert f(td=3) != 0 and b"dtype" in lib.smoe_last_error()
        assert f(mode=2) != 0 and b"mode" in lib.smoe_last_error()
        assert f(mode=-1) != 0
        assert f(C=0) != 0 and b"C" in lib.smoe_last_error()
        assert f(tau=0.0) != 0 and b"tau" in lib.smoe_last_error()
        assert f(tau=-1.0) != 0
        assert f(B=-1) != 0
    assert fwd(base=None) != 0 and b"null" in lib.smoe_last_error()
    assert fwd(loss=None) != 0
    assert bwd(g=None) != 0 and b"null" in lib.smoe_last_error()
    assert bwd(out=None) != 0
    assert bwd(B=65536) != 0 and b"65535" in lib.smoe_last_error()

    def embed(tokens=fake, dt=1, cls=fake, dist=fake, pos=fake, B=2, P=4, d=192, x32=fake, xn=None, xdt=1):
        return lib.smoe_embed_ln2(tokens, dt, cls, dist, pos, None, None, 1e-6, B, P, d, x32, xn, xdt, None)
    assert embed(B=0) == 0
    for d in (0, 64, 200, 512, 2048):
        assert embed(d=d) != 0 and b"smoe_embed_ln2" in lib.smoe_last_error()
    assert embed(P=0) != 0
    assert embed(tokens=None) != 0 and b"null" in lib.smoe_last_error()
    assert embed(cls=None) != 0 and embed(pos=None) != 0 and embed(x32=None) != 0
    assert embed(dt=0) != 0 and b"f16 or bf16" in lib.smoe_last_error()
    assert embed(xn=fake, xdt=0) != 0 and b"xn" in lib.smoe_last_error()


# ------------------------------------------------------------------------------------------------ DistilledVisionTransformer
def _tiny(**kw):
    torch.manual_seed(0)
    return sm.create_model("deit_tiny_distilled_patch16_224", depth=2, num_classes=10, img_size=64, **kw)


EXPECTED_KEYS = {
    "cls_token": (1, 1, 192), "dist_token": (1, 1, 192), "pos_embed": (1, 18, 192),
    "patch_embed.proj.weight": (192, 3, 16, 16), "patch_embed.proj.bias": (192,),
    "norm.weight": (192,), "norm.bias": (192,), "head.weight": (10, 192), "head.bias": (10,),
    "head_dist.weight": (10, 192), "head_dist.bias": (10,),
}
for _i in range(2):
    EXPECTED_KEYS.update({
        f"blocks.{_i}.norm1.weight": (192,), f"blocks.{_i}.norm1.bias": (192,),
        f"blocks.{_i}.attn.qkv.weight": (576, 192), f"blocks.{_i}.attn.qkv.bias": (576,),
        f"blocks.{_i}.attn.proj.weight": (192, 192), f"blocks.{_i}.attn.proj.bias": (192,),
        f"blocks.{_i}.norm2.weight": (192,), f"blocks.{_i}.norm2.bias": (192,),
        f"blocks.{_i}.mlp.fc1.weight": (768, 192), f"blocks.{_i}.mlp.fc1.bias": (768,),
        f"blocks.{_i}.mlp.fc2.weight": (192, 768), f"blocks.{_i}.mlp.fc2.bias": (192,),
    })


def test_distilled_state_dict_keys_and_shapes_and_a_strict_round_trip():
    model = _tiny()
    sd = model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == EXPECTED_KEYS
    assert isinstance(model, sm.VisionTransformer) and model.num_tokens == 2
    assert float(model.dist_token.abs().max()) > 0 and float(model.pos_embed[0, 1].abs().max()) > 0, "trunc_normal_ initialised"
    assert float(model.head_dist.bias.abs().max()) == 0 and 0 < float(model.head_dist.weight.std()) < 0.05
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    other = sm.create_model("deit_tiny_distilled_patch16_224", depth=2, num_classes=10, img_size=64)
    res = other.load_state_dict(torch.load(buf), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    x = torch.randn(2, 3, 64, 64)
    assert torch.equal(other.eval()(x), model.eval()(x))
    assert {"dist_token", "cls_token", "pos_embed"} <= set(model.no_weight_decay())


def test_train_mode_returns_the_pair_and_eval_their_mean():
    model = _tiny()
    x = torch.randn(3, 3, 64, 64)
    out = model.train()(x)
    assert isinstance(out, tuple) and len(out) == 2 and out[0].shape == out[1].shape == (3, 10)
    assert not torch.equal(out[0], out[1])
    a, b = model.forward_features(x)
    assert a.shape == b.shape == (3, 192)
    mean = model.eval()(x)
    assert isinstance(mean, torch.Tensor) and torch.equal(mean, (out[0] + out[1]) / 2)
    # the reference's lines, written out: cat(cls, dist, patches) + pos_embed, the blocks, the norm, rows 0 and 1
    with torch.no_grad():
        t = model.patch_embed(x)
        t = torch.cat((model.cls_token.expand(3, -1, -1), model.dist_token.expand(3, -1, -1), t), dim=1) + model.pos_embed
        t = model.norm(model.blocks(t))
        want = (model.head(t[:, 0]) + model.head_dist(t[:, 1])) / 2
    assert torch.allclose(mean, want, rtol=0, atol=1e-6)
    loss = sm.DistillationLoss(F.cross_entropy, lambda inp: torch.randn(3, 10), "soft", 0.5, 1.0)(x, model.train()(x), torch.tensor([1, 2, 3]))
    loss.backward()
    for name in ("dist_token", "pos_embed", "head_dist.weight", "head_dist.bias", "cls_token", "head.weight"):
        g = dict(model.named_parameters())[name].grad
        assert g is not None and float(g.abs().max()) > 0, name


def test_the_four_distilled_factories_are_registered_with_the_references_dims():
    dims = {"deit_tiny_distilled_patch16_224": (192, 3, 224), "deit_small_distilled_patch16_224": (384, 6, 224),
            "deit_base_distilled_patch16_224": (768, 12, 224), "deit_base_distilled_patch16_384": (768, 12, 384)}
    for name, (d, heads, img) in dims.items():
        assert name in sm.list_models() and getattr(sm, name) is sm.vit._MODEL_REGISTRY[name]
        m = sm.create_model(name, depth=1)
        assert isinstance(m, sm.DistilledVisionTransformer) and m.embed_dim == d and m.blocks[0].attn.num_heads == heads
        P = (img // 16) ** 2
        assert m.pos_embed.shape == (1, P + 2, d) and m.head_dist.weight.shape == (1000, d) and m.patch_embed.img_size == (img, img)
        assert m.blocks[0].norm1.eps == 1e-6 and m.blocks[0].attn.qkv.bias is not None and m.blocks[0].mlp.fc1.out_features == 4 * d
    assert len(sm.create_model("deit_tiny_distilled_patch16_224").blocks) == 12
    with pytest.raises(RuntimeError):
        sm.create_model("deit_tiny_distilled_patch16_224", pretrained=True)


def test_the_plain_vision_transformer_is_unchanged():
    torch.manual_seed(0)
    m = sm.create_model("deit_tiny_patch16_224", depth=1, num_classes=10, img_size=64)
    keys = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {k: v for k, v in EXPECTED_KEYS.items() if not k.startswith("blocks.1") and k not in
            ("dist_token", "head_dist.weight", "head_dist.bias")}
    want["pos_embed"] = (1, 17, 192)
    assert keys == want
    assert m.dist_token is None and m.head_dist is None and m.num_tokens == 1
    x = torch.randn(2, 3, 64, 64)
    out = m.train()(x)
    assert isinstance(out, torch.Tensor) and out.shape == (2, 10) and torch.equal(m.eval()(x), out)
    with torch.no_grad():
        t = torch.cat((m.cls_token.expand(2, -1, -1), m.patch_embed(x)), dim=1) + m.pos_embed
        assert torch.equal(out, m.head(m.norm(m.blocks(t))[:, 0]))


@pytest.mark.parametrize("residual", [True, False])
def test_patch_blocks_with_moe_on_a_distilled_model_keeps_the_surface(residual):
    """The MoE operator itself has no CPU path (that is the library's contract): what can be checked without a GPU is that patching
    leaves the distilled surface alone -- token count, keys of the shell, the two heads -- and that every block got its MoE."""
    model = sm.resmoe.patch_blocks_with_moe(_tiny(), 8, 2, residual)
    assert isinstance(model, sm.DistilledVisionTransformer) and model.num_tokens == 2
    keys = set(model.state_dict())
    assert {"dist_token", "head_dist.weight", "head_dist.bias", "pos_embed"} <= keys
    assert all(isinstance(b.mlp, sm.CustomizedMoEMLP) for b in model.blocks)
    assert model.pos_embed.shape == (1, 18, 192)
    x = torch.randn(2, 3, 64, 64)
    emb = model._embed(x)
    assert emb.shape == (2, 18, 192)
    assert torch.equal(emb[:, 1], (model.dist_token + model.pos_embed[:, 1:2]).expand(2, -1, -1)[:, 0])
    f = model._final_norm_cls(emb)
    assert f.shape == (2, 2, 192) and torch.equal(f, model.norm(emb)[:, :2])
    with pytest.raises(RuntimeError, match="no CPU path"):      # (the whole forward runs in tests/test_gpu_distill.py)
        model(x)
