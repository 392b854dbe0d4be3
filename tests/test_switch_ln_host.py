"""CPU tests of SwitchableLayerNorm / SwitchableVisionTransformer: the C ABI's new entry points, the model registry and the model's
surface, the fixture made by the reference's own module, the module's torch composition against it, and the case table the GPU
file walks (margins, the teeth of the near-tie regime, the stability of the float64 restatement)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import slim_switch_moe_vit_amd as sm
from slim_switch_moe_vit_amd import _lib

import _switch_ln_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "slimmoe.h")
GOLDEN, FILES = sc.GOLDEN, sc.FIXTURE_FILES
NEW = ["smoe_switch_ln_supported", "smoe_switch_ln_fwd", "smoe_switch_ln_bwd_workspace_bytes", "smoe_switch_ln_bwd"]
ALL_MODELS = ["deit_tiny_patch16_224", "deit_small_patch16_224", "deit_base_patch16_224", "deit_tiny_distilled_patch16_224",
              "deit_small_distilled_patch16_224", "deit_base_distilled_patch16_224", "deit_base_patch16_384",
              "deit_base_distilled_patch16_384", "deit_sw_tiny_patch16_224"]          # models/model.py __all__
FIXTURE_CASES, load_fixture, fixture_case = sc.FIXTURE_CASES, sc.load_fixture, sc.fixture_case
REFERENCE_HERE = os.path.exists(os.path.join(os.environ.get("SLIMMOE_REFERENCE", "/root/reference"), "models", "layers.py"))


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


# ----------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_are_declared_prototyped_and_exported_and_the_abi_stays_29():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % s, text), f"include/slimmoe.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
        assert hasattr(lib, s), f"libslimmoe_hip.so does not export {s}"
        n_args = len([a for a in re.search(r"%s\s*\((.*?)\)" % s, text, re.S).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[s][1]), s
    assert "models/layers.py:31-157" in open(HEADER).read()
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    assert _lib.binary_build_id() == _lib.source_build_id()


def test_reach_and_argument_checks_come_before_any_launch():
    lib = _lib.load()
    for d in sm.ops.LN_DIMS + (4, 196, 1020):
        for K in (1, 2, 32):
            assert lib.smoe_switch_ln_supported(d, K) == 1 and sm.ops.switch_ln_supported(d, K)
    for d, K in ((0, 1), (194, 1), (1028, 1), (192, 0), (192, 33)):
        assert lib.smoe_switch_ln_supported(d, K) == 0
    fake = 4096          # never dereferenced
    assert lib.smoe_switch_ln_fwd(None, None, None, None, None, -1, 1e-5, 0, 192, 4, None, None, None) != 0   # K > 1 selects: centroids
    assert lib.smoe_switch_ln_fwd(None, None, None, fake, None, -1, 1e-5, 0, 192, 4, None, None, None) == 0   # T == 0: a no-op
    assert lib.smoe_switch_ln_fwd(None, None, None, None, None, -1, 1e-5, 0, 192, 1, None, None, None) == 0   # K == 1: no centroids
    assert lib.smoe_switch_ln_fwd(fake, fake, fake, fake, None, -1, 1e-5, 8, 194, 4, fake, fake, None) != 0
    assert lib.smoe_switch_ln_fwd(fake, fake, fake, fake, None, -1, 1e-5, 8, 192, 33, fake, fake, None) != 0
    assert lib.smoe_switch_ln_fwd(fake, fake, fake, fake, fake, 1, 1e-5, 8, 192, 4, fake, fake, None) != 0    # both kinds of given bucket
    assert lib.smoe_switch_ln_fwd(fake, None, fake, fake, None, 0, 1e-5, 8, 192, 4, fake, fake, None) != 0    # biases without weights
    assert lib.smoe_switch_ln_fwd(fake + 4, fake, fake, fake, None, 0, 1e-5, 8, 192, 4, fake, fake, None) != 0  # alignment
    assert lib.smoe_switch_ln_bwd_workspace_bytes(8, 192, 33) == 0 and lib.smoe_switch_ln_bwd_workspace_bytes(8, 192, 4) > 0
    assert lib.smoe_switch_ln_bwd(fake, fake, 0, fake, fake, 1e-5, 8, 192, 4, fake, fake, fake, fake, 16, None) != 0   # workspace size
    assert lib.smoe_switch_ln_bwd(fake, fake, 7, fake, fake, 1e-5, 8, 192, 4, fake, fake, fake, fake, 1 << 30, None) != 0
    assert b"smoe_switch_ln_bwd" in lib.smoe_last_error()


# -------------------------------------------------------------------------------------------------------------- registry and model
def test_every_reference_model_name_resolves():
    for name in ALL_MODELS:
        m = sm.create_model(name, depth=1, num_classes=3)
        assert isinstance(m, torch.nn.Module), name
    assert isinstance(sm.create_model("deit_sw_tiny_patch16_224", depth=1), sm.SwitchableVisionTransformer)
    assert sm.create_model("deit_small_patch16_224", depth=1).embed_dim == 384
    m = sm.create_model("deit_base_patch16_384", depth=1)
    assert m.embed_dim == 768 and m.pos_embed.shape == (1, 577, 768)


def _block_keys(prefix):
    leaf = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
            "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]
    return {f"{prefix}.{k}" for k in leaf}


def test_switchable_model_keys_counts_and_modes():
    m = sm.create_model("deit_sw_tiny_patch16_224", buckets=3)
    want = {"cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight", "norm.bias", "head.weight",
            "head.bias", "router.weights", "router.biases", "router.centroids"}
    for i in range(11):
        want |= _block_keys(f"mid_blocks.{i}")
    want |= _block_keys("post_blocks.0")
    sd = m.state_dict()
    assert set(sd) == want
    assert sd["router.weights"].shape == (3, 192) and sd["router.centroids"].shape == (3, 192)
    assert not m.router.centroids.requires_grad and float(m.router.centroids.abs().sum()) == 0.0
    assert (len(m.pre_blocks), len(m.mid_blocks), len(m.post_blocks)) == (0, 11, 1) and len(m.blocks) == 12
    assert (m.router_start, m.router_end, m.routing) == (0, -1, False)
    # stochastic-depth indices: upstream's formulas -- mid i takes dpr[i], the post block dpr[(-1) % depth]
    md = sm.create_model("deit_sw_tiny_patch16_224", drop_path_rate=0.11)
    rates = [getattr(b.drop_path, "drop_prob", 0.0) for b in md.blocks]
    assert np.allclose(rates, np.linspace(0, 0.11, 12), atol=1e-7)
    assert m.no_weight_decay() == {"pos_embed", "cls_token", "dist_token"} and m.get_classifier() is m.head
    m.reset_classifier(7)
    assert m.head.out_features == 7
    m.router.eval()
    m.train(False)
    m.train(True)
    assert m.training and m.mid_blocks.training and m.router.training is False          # train() never touches the router
    m.router.train()
    m.train(False)
    assert not m.training and m.router.training is True
    with pytest.raises(NotImplementedError):
        sm.SwitchableVisionTransformer(img_size=32, depth=2, embed_dim=192, num_heads=3, weight_init="jax")


def test_switchable_model_forward_surface_on_cpu():
    torch.manual_seed(0)
    img = torch.randn(2, 3, 32, 32)
    m = sm.create_model("deit_sw_tiny_patch16_224", buckets=3, depth=2, img_size=32, num_classes=5, collect_embeddings=True).eval()
    m.router.set_centroids(torch.randn(3, 192))
    with torch.no_grad():
        logits, emb = m(img)
        assert logits.shape == (2, 5) and emb.shape == (2, 5, 192)
        assert torch.equal(emb, m._embed(img))                               # the pre-router stream, unmodified
        assert torch.equal(m(img, bucket=1)[0], m(img, bucket=torch.ones(2, 5, dtype=torch.int64))[0])
    m.route(True)
    with pytest.raises(NotImplementedError):
        m(img)
    m.route(False)
    d = sm.create_model("deit_sw_tiny_patch16_224", buckets=2, depth=2, img_size=32, num_classes=5, distilled=True)
    assert d.pos_embed.shape == (1, 6, 192) and "dist_token" in d.state_dict() and "head_dist.weight" in d.state_dict()
    out = d(img)
    assert isinstance(out, tuple) and out[0].shape == (2, 5) and out[1].shape == (2, 5)
    assert d.eval()(img).shape == (2, 5)
    r = sm.create_model("deit_sw_tiny_patch16_224", depth=1, img_size=32, num_classes=5, representation_size=16)
    assert r.head.in_features == 16 and "pre_logits.fc.weight" in r.state_dict() and r(img).shape == (2, 5)
    p = sm.patch_blocks_with_moe(sm.create_model("deit_sw_tiny_patch16_224", depth=2, img_size=32), 4, 1, True)
    assert all(hasattr(b, "dense_gate") for b in p.blocks) and "mid_blocks.0.mlp.gate.gate.weight" in p.state_dict()


def test_module_surface():
    m = sm.SwitchableLayerNorm(8, switchable_buckets=3)
    assert set(m.state_dict()) == {"weights", "biases", "centroids"}
    assert torch.equal(m.weights, torch.ones(3, 8)) and torch.equal(m.biases, torch.zeros(3, 8)) and torch.equal(m.centroids, torch.zeros(3, 8))
    m.set_centroids(torch.arange(24.0).reshape(3, 8))                         # a plain tensor is accepted
    assert m.centroids.requires_grad is False and float(m.centroids[2, 7]) == 23.0
    with pytest.raises(ValueError):
        m.set_centroids(torch.zeros(3, 7))
    x = torch.randn(4, 5, 8)
    keep = x.clone()
    y, b = m(x)
    assert y.shape == x.shape and b.shape == (4, 5) and b.dtype == torch.int64 and torch.equal(x, keep)
    for bad in (3, -1):
        with pytest.raises(ValueError):
            m(x, bad)
    with pytest.raises(ValueError):
        m(x, torch.full((4, 5), 3))
    with pytest.raises(TypeError):
        m(x, torch.zeros(4, 5))
    assert torch.equal(m(x, 1)[1], torch.ones(4, 5, dtype=torch.int64))
    assert torch.equal(m(x, torch.tensor([[0], [1], [2], [0]]))[1], torch.tensor([0, 1, 2, 0])[:, None].expand(4, 5))
    n = sm.SwitchableLayerNorm((5, 8), elementwise_affine=False, switchable_buckets=2)      # tuple-valued shape: the composition
    assert n.weights is None and n.centroids.shape == (2, 40)
    y2, b2 = n(x)
    assert b2.shape == (4,) and torch.allclose(y2, torch.nn.functional.layer_norm(x, (5, 8)), atol=1e-5)
    one = sm.SwitchableLayerNorm(8)                                            # K = 1: a plain LayerNorm, whatever the centroids hold
    one.set_centroids(torch.full((1, 8), float("nan")))
    y1, b1 = one(x)
    assert int(b1.abs().sum()) == 0 and torch.allclose(y1, torch.nn.functional.layer_norm(x, (8,)), atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.skipif(not REFERENCE_HERE, reason="the reference's models/layers.py is not on this machine")
def test_fixture_regenerates_bit_for_bit(tmp_path, fixture):
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_switch_ln.py")],
                       env=dict(os.environ, SLIMMOE_GOLDEN_OUT=str(tmp_path)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    new = {}
    for f in FILES:
        z = np.load(os.path.join(tmp_path, f))
        new.update({k: z[k] for k in z.files})
    assert sorted(new) == sorted(fixture)
    for key in fixture:
        a, b = fixture[key], new[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


def test_fixture_files_hold_arrays_only_and_stay_small(fixture):
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= 1 << 20, f
    assert all(v.dtype in (np.float32, np.int64) for v in fixture.values())
    assert fixture["sw_192x4/x"].shape == (3, 37, 192) and fixture["sw_768x8/x"].shape == (2, 50, 768)
    assert fixture["sw_192x4/centroids"].shape == (4, 192) and fixture["sw_768x8/centroids"].shape == (8, 768)
    assert (fixture["int_192x4/buckets"] == 2).all() and (fixture["tensor_192x4/buckets"] == fixture["tensor_192x4/given"]).all()
    for name in ("sw_192x4", "sw_768x8"):                     # well separated: the reference's f32 cdist and float64 agree on every row
        x = torch.from_numpy(fixture[name + "/x"]).flatten(0, 1)
        c = torch.from_numpy(fixture[name + "/centroids"])
        assert float(sc.margins(x, c).min()) > 0.5
        assert torch.equal(sc.select64(x, c), torch.from_numpy(fixture[name + "/buckets"]).flatten())


@pytest.mark.parametrize("name,src,mode", FIXTURE_CASES, ids=[c[0] for c in FIXTURE_CASES])
def test_composition_against_the_fixture(fixture, name, src, mode):
    t, buckets, ref = fixture_case(fixture, name, src, mode)
    K, d = t["weights"].shape
    mod = sm.SwitchableLayerNorm(d, switchable_buckets=K)
    with torch.no_grad():
        mod.weights.copy_(t["weights"])
        mod.biases.copy_(t["biases"])
    mod.set_centroids(t["centroids"])
    x = t["x"].clone().requires_grad_(True)
    y, b = mod(x, buckets)
    y.backward(t["dy"])
    assert torch.equal(b, ref["buckets"])
    assert mod.centroids.grad is None and torch.equal(x.detach(), t["x"])
    r64 = sc.restate64(t["x"].flatten(0, 1), t["dy"].flatten(0, 1), t["weights"], t["biases"], t["centroids"],
                       buckets.flatten() if isinstance(buckets, torch.Tensor) else buckets)
    assert torch.equal(r64["b"], ref["buckets"].flatten())
    for got, key, rk in ((y.detach(), "y", "y"), (x.grad, "dx", "dx"), (mod.weights.grad, "dw", "dweights"), (mod.biases.grad, "db", "dbiases")):
        want = r64[key].reshape(got.shape)
        bound = sc.bar(want, ref[rk])
        err = float((got.double() - want).abs().max())
        print(f"{name} {key}: err {err:.3e} bar {bound:.3e}")
        assert err <= bound, (name, key, err, bound)


# ------------------------------------------------------------------------------------------------------------------ case table
CELLS = sc.cells()


def test_table_covers_every_size_and_regime():
    assert {c[0] for c in CELLS} == set(sc.REGIMES)
    grid = [c for c in CELLS if c not in sc.EXTRA_CELLS]
    for regime in sc.REGIMES:
        mine = [c for c in grid if c[0] == regime]
        assert {c[2] for c in mine} == set(sc.DS) and {c[1] for c in mine} == set(sc.TS), regime
        assert {(c[2], c[3]) for c in mine} >= {(d, K) for d in sc.DS for K in sc.KS if not (regime == "near_tie" and K == 1)}
    assert {c[3] for c in grid} == set(sc.KS)
    extra = {c[3] for c in sc.EXTRA_CELLS}
    assert extra & set(range(9, 13)) and 16 in extra and all(9 <= k <= 16 for k in extra)          # the 16-slot argmin
    assert any(c[2] * c[3] > 12288 for c in sc.EXTRA_CELLS if c[3] <= 16) and any(c[2] * c[3] <= 12288 for c in sc.EXTRA_CELLS)


def test_margins_of_every_cell_and_the_teeth_of_the_near_tie_regime():
    wrong32, tie_rows, kept = 0, 0, []
    for cell in CELLS:
        regime, T, d, K = cell
        c = sc.make_cell(*cell)
        assert c["x"].shape == (T, d) and c["x"].dtype == torch.float32
        m = sc.margins(c["x"], c["cent"])
        b64 = sc.select64(c["x"], c["cent"])
        # the float64 restatement does not depend on the order of its sums
        assert torch.equal(b64, sc.select64(c["x"], c["cent"], reverse=True)), cell
        if regime == "near_tie":
            assert float(m.min()) >= sc.TIE_WINDOW[0] and float(m.max()) <= sc.TIE_WINDOW[1], (cell, float(m.min()), float(m.max()))
            wrong32 += int((sc.select32_expanded(c["x"], c["cent"]) != b64).sum())
            tie_rows += T
            kept.append(c["kept"])
        elif K > 1:
            assert float(m.min()) >= sc.SEPARATED_MARGIN, (cell, float(m.min()))
        if regime == "one_bucket":
            assert (b64 == K - 1).all()
    print(f"near-tie: the f32 expanded form misassigns {wrong32} of {tie_rows} rows; rejection kept {min(kept):.2f}-{max(kept):.2f} of the draws")
    assert wrong32 >= 1


def test_composition_follows_the_restatement_on_near_ties_and_nan_rules():
    for cell in [c for c in CELLS if c[0] == "near_tie"][:6]:
        c = sc.make_cell(*cell)
        _, b = sm.switch_ln_compose(c["x"], sc.EPS, c["weights"], c["biases"], c["cent"], None, cell[3])
        assert torch.equal(b, sc.select64(c["x"], c["cent"])), cell
    c = sc.make_cell("separated", 17, 192, 5)
    x = c["x"].clone()
    x[3, 7] = float("nan")
    y, b = sm.switch_ln_compose(x, sc.EPS, c["weights"], c["biases"], c["cent"], None, 5)
    y0, b0 = sm.switch_ln_compose(c["x"], sc.EPS, c["weights"], c["biases"], c["cent"], None, 5)
    keep = torch.arange(17) != 3
    assert int(b[3]) == 0 and torch.equal(b[keep], b0[keep]) and torch.equal(y[keep], y0[keep]) and bool(y[3].isnan().all())
    cent = c["cent"].clone()
    cent[2, 0] = float("nan")
    assert (sm.switch_ln_compose(c["x"], sc.EPS, c["weights"], c["biases"], cent, None, 5)[1] == 2).all()
