"""Full fine-tuning of the DINOv2 backbone, the parts that need no GPU: trainable sets, gradient-production order and buckets, the
config and its parameter groups, the refused options, init_cfg."""
import importlib.util
import os

import pytest
import torch

import vfmseg_amd  # noqa: F401
from tests.fullft_helpers import DEPTH, build_small, inert_backbone_keys, small_cfg, small_state_dict, trained_backbone_keys
from vfmseg_amd import presets
from vfmseg_amd.optim import grad_group, param_options, production_order
from vfmseg_amd.parallel import make_buckets
from vfmseg_amd.registry import MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainable(model):
    return {n for n, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("head", ["linear", "segformer"])
def test_trainable_set_of_the_full_model(head):
    """train(): every backbone tensor that enters the graph trains; norm.* and mask_token are frozen and stay in the checkpoint."""
    model = build_small(head).train()
    sd = model.state_dict()
    tr = _trainable(model)
    assert set(trained_backbone_keys(sd)) <= tr
    assert len(trained_backbone_keys(sd)) == 4 + 14 * DEPTH
    for k in inert_backbone_keys(sd):
        assert k not in tr and k in sd
    assert len(inert_backbone_keys(sd)) == 3
    assert model.backbone.full_training()
    model.eval()
    assert not model.backbone.full_training()


def test_trainable_sets_of_the_other_models_are_unchanged():
    """LoRA: names with 'lora' (and the heads); Rein: names with 'reins' minus the inert link layers; frozen: no backbone name."""
    lora = MODELS.build(presets.dinov2_linear(depth=2)).train()
    bb = {n for n in _trainable(lora) if n.startswith("backbone.")}
    assert bb and all("lora_" in n for n in bb) and len(bb) == 2 * 2
    rein = MODELS.build(presets.rein_dinov2_linear(depth=2)).train()
    bb = {n for n in _trainable(rein) if n.startswith("backbone.")}
    assert bb and all(".reins." in n for n in bb) and not any("transform" in n or "merge" in n for n in bb)
    assert not rein.backbone.full_training()
    frozen = build_small(kind="frozen").train()
    assert not any(n.startswith("backbone.") for n in _trainable(frozen))
    assert not frozen.backbone.full_training()
    # a LoRA-wrapped ViT is never "bare"
    assert not lora.backbone.vit.full_training()


def test_production_order_and_buckets_of_a_full_model():
    model = build_small().train()
    names = production_order(sorted(_trainable(model)))
    groups = [grad_group(n) for n in names]
    first_bb = groups.index("backbone")
    assert set(groups[:first_bb]) == {"decode_head"} and set(groups[first_bb:]) == {"backbone"}    # heads first
    blks = [int(n.split("blocks.")[1].split(".")[0]) if ".blocks." in n else -1 for n in names[first_bb:]]
    assert blks == sorted(blks, reverse=True) and blks[0] == DEPTH - 1 and blks[-1] == -1              # blocks descending, embeddings last
    assert {n for n, b in zip(names[first_bb:], blks) if b == -1} == {"backbone.patch_embed.proj.weight", "backbone.patch_embed.proj.bias",
                                                                      "backbone.cls_token", "backbone.pos_embed"}
    sizes = dict((n, p.numel()) for n, p in model.named_parameters())
    offsets = [0]
    for n in names:
        offsets.append((offsets[-1] + sizes[n] + 15) // 16 * 16)
    buckets = make_buckets(names, offsets)
    assert [b[0] for b in buckets] == ["decode_head", "backbone0", "backbone1"]
    assert buckets[0][1] == 0 and buckets[-1][2] == offsets[-1]
    for (_, _, e0), (_, s1, _) in zip(buckets, buckets[1:]):
        assert e0 == s1
    # boundaries fall on block boundaries: each backbone bucket holds whole blocks, the last one the embeddings too
    for name, a, b in buckets[1:]:
        inside = [n for n, o in zip(names, offsets[:-1]) if a <= o < b]
        per_block = {}
        for n in inside:
            if ".blocks." in n:
                per_block.setdefault(int(n.split("blocks.")[1].split(".")[0]), []).append(n)
        assert all(len(v) == 14 for v in per_block.values()), (name, {k: len(v) for k, v in per_block.items()})
    assert any("pos_embed" in n for n, o in zip(names, offsets[:-1]) if buckets[-1][1] <= o < buckets[-1][2])
    # a deep model is cut into MAX_BACKBONE_BUCKETS slices of whole blocks, last blocks first
    deep = ["decode_head.conv_seg.weight"] + [f"backbone.blocks.{i}.{leaf}" for i in range(23, -1, -1) for leaf in ("attn.qkv.weight", "norm1.bias")] \
        + ["backbone.cls_token"]
    assert production_order(list(reversed(deep))) == production_order(deep)
    offs = list(range(0, 16 * (len(deep) + 1), 16))
    bk = make_buckets(production_order(deep), offs)
    assert [b[0] for b in bk] == ["decode_head", "backbone0", "backbone1", "backbone2", "backbone3"]
    assert [(b[2] - b[1]) // 32 for b in bk[1:4]] == [6, 6, 6]


def test_orders_of_lora_and_rein_names_are_unchanged():
    names = ["backbone.model.base_model.model.blocks.1.attn.qkv.lora_A.default.weight", "decode_head.conv_seg.weight",
             "backbone.reins.scale", "aux_decoder.fuse_conv.0.weight", "backbone.model.base_model.model.blocks.0.attn.qkv.lora_B.default.weight"]
    assert [grad_group(n) for n in names] == ["lora", "decode_head", "reins", "aux_decoder", "lora"]
    assert production_order(names) == [names[3], names[1], names[0], names[4], names[2]]


def _load_config(name):
    spec = importlib.util.spec_from_file_location("cfg_" + name.replace(".", "_"), os.path.join(ROOT, "configs", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_config_builds_equals_its_preset_and_groups_the_backbone():
    cfg = _load_config("dg_full_dinov2_segformer.py")
    assert cfg.model == presets.full_dinov2_segformer()
    oc = presets.optim_cfg(backbone_lr_mult=0.1)
    assert cfg.optim_wrapper == oc["optim_wrapper"] and cfg.param_scheduler == oc["param_scheduler"]
    ck = cfg.optim_wrapper["paramwise_cfg"]["custom_keys"]
    assert ck["backbone"] == dict(lr_mult=0.1) and ck["norm"] == dict(decay_mult=0.0)
    assert presets.optim_cfg() == presets.optim_cfg(backbone_lr_mult=None) and "backbone" not in presets.optim_cfg()["optim_wrapper"]["paramwise_cfg"]["custom_keys"]
    m = dict(cfg.model)
    m["backbone"] = dict(m["backbone"], depth=2, embed_dim=256, num_heads=4, img_size=64)
    m["decode_head"] = dict(m["decode_head"], in_channels=[256] * 4)
    model = MODELS.build(m).train()
    assert type(model).__name__ == "EncoderDecoder" and type(model.backbone).__name__ == "DinoVisionTransformer"
    o = cfg.optim_wrapper["optimizer"]
    opts = param_options(model, o["lr"], o["weight_decay"], cfg.optim_wrapper["paramwise_cfg"])
    assert set(opts) == {n for n, p in model.named_parameters() if p.requires_grad}
    for n, (lr_mult, wd) in opts.items():
        if n.startswith("backbone."):
            assert lr_mult == 0.1, n
            assert wd == (0.0 if ".norm" in n else o["weight_decay"]), n
        else:
            assert lr_mult == 1.0, n
            if "norm" in n or ".gn." in n or ".ln" in n:
                assert wd == 0.0, n


def test_refused_options_are_named():
    from vfmseg_amd.precision import set_compute_dtype
    cfg = small_cfg()["backbone"]
    vit = MODELS.build(dict(cfg, drop_path_rate=0.1)).train()
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        vit.engine().check_full_training(4, 4)
    vit = MODELS.build(cfg).train()
    vit.engine().check_full_training(4, 4)
    with pytest.raises(NotImplementedError, match="img_size"):
        vit.engine().check_full_training(8, 8)
    set_compute_dtype("bf16x3")
    try:
        with pytest.raises(NotImplementedError, match="bf16x3"):
            vit.engine().check_full_training(4, 4)
    finally:
        set_compute_dtype("bf16")


def test_init_cfg_of_the_bare_backbone(tmp_path):
    sd = small_state_dict()
    bare = {k[len("backbone."):]: v + 0.5 for k, v in sd.items() if k.startswith("backbone.")}
    good = tmp_path / "dinov2.pth"
    torch.save(bare, good)
    cfg = small_cfg()
    cfg["backbone"]["init_cfg"] = dict(type="Pretrained", checkpoint=str(good))
    model = MODELS.build(cfg)
    got = model.backbone.state_dict()
    assert all(torch.equal(got[k], v) for k, v in bare.items())
    assert model.backbone.pretrained == str(good)
    bad = tmp_path / "prefixed.pth"
    torch.save({"backbone." + k: v for k, v in bare.items()}, bad)
    cfg["backbone"]["init_cfg"] = dict(type="Pretrained", checkpoint=str(bad))
    with pytest.raises(RuntimeError, match="(Missing|Unexpected) key"):
        MODELS.build(cfg)
    cfg["backbone"]["init_cfg"] = dict(type="Kaiming", checkpoint=str(good))
    with pytest.raises(NotImplementedError, match="init_cfg"):
        MODELS.build(cfg)


@pytest.mark.parametrize("make", [lambda bb: dict(presets.dinov2_ms_masked(depth=2, embed_dim=256, num_heads=4), backbone=bb),
                                  lambda bb: dict(presets.dinov2_hrda(depth=2, embed_dim=256, num_heads=4), backbone=bb),
                                  lambda bb: dict(presets.uda_rein_dinov2_segformer(depth=2, embed_dim=256, num_heads=4), backbone=bb)],
                         ids=["MsVFMEncoderDecoder", "HRDAEncoderDecoder", "DACS"])
def test_multi_pass_segmentors_refuse_the_bare_backbone_by_name(make, request):
    """MsVFMEncoderDecoder / HRDAEncoderDecoder / DACS over a bare DINOv2 in train() mode: a NotImplementedError that names the combination
    (raised where the backbone would be called: the tokens never reach a kernel, so no GPU is needed)."""
    cfg = make(small_cfg()["backbone"])
    model = MODELS.build(cfg).train()
    with pytest.raises(NotImplementedError, match=request.node.callspec.id + ".*bare DinoVisionTransformer"):
        model._tokens([(torch.zeros(1, 3, 64, 64), None)])
    model.eval()
    assert not model.backbone.full_training()
