"""LoRA on any linear layer of a DINOv2 block (Lora_config.target_modules: qkv, attn.proj, fc1, fc2) - what needs no GPU: the containers
every subset builds, the state_dict key scheme against the reference's (tests/golden/lora_sites.npz), what trains, the order the engine
hands the factors to autograd, optimiser groups and DP buckets, the refusals, and the pretrained-checkpoint rename."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import lora_sites_helpers as H
from vfmseg_amd import parallel, presets
from vfmseg_amd.optim import param_options, production_order
from vfmseg_amd.registry import MODELS
import vfmseg_amd.backbones  # noqa: F401
import vfmseg_amd.segmentors  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lora_sites.npz")
SUBSETS = [list(c) for n in range(1, 5) for c in itertools.combinations(H.ALL, n)]


def _build(targets, **kw):
    return MODELS.build(H.lora_backbone_cfg(targets, **kw))


@pytest.mark.parametrize("targets", SUBSETS, ids=lambda t: "+".join(t))
def test_every_subset_builds_and_trains_only_its_factors(targets):
    m = _build(targets).train()
    eng = m.vit.engine()
    assert eng.sites() == tuple(k for k, t in zip(("qkv", "proj", "fc1", "fc2"), H.ALL) if t in targets)
    assert sorted(m.state_dict()) == sorted(H.lora_state_dict(targets))
    train = [n for n, p in m.named_parameters() if p.requires_grad]
    assert train and all("lora_" in n for n in train) and len(train) == 2 * len(targets) * H.DEPTH
    assert len(eng.trainable()) == len(train) and all(p.requires_grad for p in eng.trainable())
    # the patch embedding is a Conv2d named `proj`: no target may ever wrap it
    assert isinstance(m.vit.patch_embed.proj, torch.nn.Conv2d)


def test_state_dict_names_equal_the_references():
    names = [str(n) for n in np.load(GOLD)["param_names"]]
    m = _build(H.ALL)
    assert sorted(m.state_dict()) == names
    assert sorted(n for n, p in m.train().named_parameters() if p.requires_grad) == [str(n) for n in np.load(GOLD)["trainable_names"]]


def test_trainable_order_is_block_then_qkv_proj_fc1_fc2():
    m = _build(["fc2", "qkv", "fc1", "attn.proj"])     # the order of the list does not matter
    by_id = {id(p): n for n, p in m.vit.named_parameters()}
    got = [by_id[id(p)] for p in m.vit.engine().trainable()]
    want = [f"blocks.{i}.{mod}.{ab}.default.weight" for i in range(H.DEPTH) for mod in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")
            for ab in ("lora_A", "lora_B")]
    assert got == want
    m2 = _build(["fc1"])
    by_id = {id(p): n for n, p in m2.vit.named_parameters()}
    assert [by_id[id(p)] for p in m2.vit.engine().trainable()] == \
        [f"blocks.{i}.mlp.fc1.{ab}.default.weight" for i in range(H.DEPTH) for ab in ("lora_A", "lora_B")]


def test_train_plan_is_for_the_qkv_only_model():
    """_train_plan answers None before it looks at anything on the GPU unless the adapted set is exactly {qkv}"""
    for targets in (["qkv", "fc1"], ["attn.proj"], H.ALL):
        eng = _build(targets, dropout=0.1).vit.engine()
        assert eng._train_plan(dict(cd=torch.bfloat16), 2, 42, True, None) is None


def test_optimiser_groups_and_buckets():
    cfg = presets.dinov2_linear(depth=H.DEPTH)
    cfg["backbone"]["backbone"]["out_indices"] = list(H.OUT)
    cfg["backbone"]["Lora_config"] = presets.lora_cfg(target_modules=presets.ALL_LINEAR)
    m = MODELS.build(cfg).train()
    oc = presets.optim_cfg()["optim_wrapper"]
    opts = param_options(m, oc["optimizer"]["lr"], oc["optimizer"]["weight_decay"], oc["paramwise_cfg"])
    named = {n: p for n, p in m.named_parameters() if p.requires_grad}
    assert set(opts) == set(named)
    bb = [n for n in named if n.startswith("backbone.")]
    assert len(bb) == 2 * 4 * H.DEPTH and all("lora_" in n for n in bb)
    for mod in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
        assert opts[f"backbone.model.base_model.model.blocks.1.{mod}.lora_B.default.weight"] == opts[
            "backbone.model.base_model.model.blocks.0.attn.qkv.lora_A.default.weight"]
    names = production_order(list(named))
    blocks = [int(n.split("blocks.")[1].split(".")[0]) for n in names if "lora_" in n]
    assert blocks == sorted(blocks, reverse=True)        # the LoRA run of the flat buffer: layers L-1 .. 0, whatever the sites
    offs = [0]
    for n in names:
        offs.append(offs[-1] + named[n].numel())
    b = parallel.make_buckets(names, offs)
    lora_b = [x for x in b if x[0].startswith("lora")]
    assert lora_b and lora_b[0][1] == offs[names.index(next(n for n in names if "lora_" in n))] and lora_b[-1][2] == offs[-1]
    for x, y in zip(b[:-1], b[1:]):
        assert x[2] == y[1]


def test_refusals_name_the_option():
    with pytest.raises(NotImplementedError, match=r"target_modules.*attn\.proj"):
        _build(["qkv", "proj"])
    with pytest.raises(NotImplementedError, match=r"Lora_config\.r=65"):
        _build(["qkv"], r=65)
    with pytest.raises(NotImplementedError, match=r"target_modules.*'norm1'"):
        _build(["qkv", "norm1"])
    with pytest.raises(NotImplementedError, match=r"target_modules.*'mlp'"):
        _build(["mlp"])
    with pytest.raises(ValueError, match="target_modules"):
        _build([])
    assert _build(["qkv"], r=64).vit.blocks[0].attn.qkv.r == 64


def test_base_checkpoint_loads_patch_embed_and_wrapped_modules():
    base = H.base_state_dict()
    cfg = H.lora_backbone_cfg(["attn.proj", "fc2"])
    cfg["checkpoint"] = base
    m = MODELS.build(cfg)
    sd = m.vit.state_dict()
    assert torch.equal(sd["patch_embed.proj.weight"], base["patch_embed.proj.weight"])
    assert torch.equal(sd["patch_embed.proj.bias"], base["patch_embed.proj.bias"])
    assert torch.equal(sd["blocks.1.attn.proj.base_layer.weight"], base["blocks.1.attn.proj.weight"])
    assert torch.equal(sd["blocks.0.mlp.fc2.base_layer.bias"], base["blocks.0.mlp.fc2.bias"])
    assert torch.equal(sd["blocks.0.attn.qkv.weight"], base["blocks.0.attn.qkv.weight"])       # not a target: stays a plain linear
    assert torch.equal(sd["blocks.1.mlp.fc1.weight"], base["blocks.1.mlp.fc1.weight"])
    # the qkv-only load is what it was: the substring rename and the module rename agree
    cfg = H.lora_backbone_cfg(["qkv"])
    cfg["checkpoint"] = base
    sd = MODELS.build(cfg).vit.state_dict()
    for k, v in base.items():
        assert torch.equal(sd[k.replace("attn.qkv.", "attn.qkv.base_layer.")], v), k


def test_presets_and_config():
    assert presets.lora_cfg()["target_modules"] == ["qkv"]
    assert presets.lora_cfg(target_modules=presets.ALL_LINEAR)["target_modules"] == H.ALL
    from vfmseg_amd.config import Config, parse_cfg_options
    opt = parse_cfg_options(["model.backbone.Lora_config.target_modules=['qkv','attn.proj','fc1','fc2']"])     # the README's turn-on line
    assert opt == {"model.backbone.Lora_config.target_modules": H.ALL}
    cfg = Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "dg_lora_dinov2_linearhead_all_linear.py"))
    assert cfg["model"]["backbone"]["Lora_config"]["target_modules"] == H.ALL and cfg["model"]["type"] == "EncoderDecoder"
    ref = presets.dinov2_linear()
    for k in ("decode_head", "test_cfg", "data_preprocessor"):
        assert cfg["model"][k] == ref[k]
