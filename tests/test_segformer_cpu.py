"""SegFormer-head baselines, CPU side: the reference's three config files load and build unchanged, the presets equal them, the head's
state-dict keys are mmcv's, the optimiser options are what the configs ask for, and the float64 restatement the GPU tests compare with
(tests/segformer_helpers.py) reproduces the reference-made fixture.  The config checks are skipped where the reference tree is absent."""
import os

import numpy as np
import pytest
import torch

import vfmseg_amd  # noqa: F401
from tests import segformer_helpers as S
from tests.helpers import sl, stats
from tests.test_reference_configs_cpu import ALLOWED, SHRINK, _diff, _plain
from vfmseg_amd import presets
from vfmseg_amd.config import Config
from vfmseg_amd.registry import MODELS
from vfmseg_amd.synth import synth_label

REF = "/root/reference/configs/dg/gta2citys"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segformer.npz")

CASES = [("dg_lora_dinov2_SegFormer.py", presets.dinov2_segformer, "LoraBackboneEncoderDecoder"),
         ("dg_rein_dinov2_Segformer_512x512_bs1x4.py", presets.rein_dinov2_segformer, "EncoderDecoder"),
         ("dg_fzn_dinov2_Segformer_512x512_bs1x4.py", presets.frozen_dinov2_segformer, "FrozenBackboneEncoderDecoder")]


def _shrunk(fname):
    cfg = Config.fromfile(os.path.join(REF, fname))
    m = cfg.model
    m["backbone"].update(SHRINK["DinoVisionTransformer"])
    if "reins_config" in m["backbone"]:
        m["backbone"]["reins_config"]["num_layers"] = 2
    if "checkpoint" in m:
        m["checkpoint"] = None
    if "init_cfg" in m["backbone"]:
        m["backbone"]["init_cfg"]["checkpoint"] = None
    return cfg, m


@needs_ref
@pytest.mark.parametrize("fname,preset,typ", CASES)
def test_reference_config_equals_preset(fname, preset, typ):
    cfg = Config.fromfile(os.path.join(REF, fname))
    ref_model, ours = _plain(cfg.model), _plain(preset())
    bad = [d for d in _diff(ref_model, ours) if not any(a in d[0] for a in ALLOWED)]
    assert not bad, bad[:8]
    assert ours["type"] == typ and ours["decode_head"] == _plain(presets.segformer_head())


@needs_ref
@pytest.mark.parametrize("fname,preset,typ", CASES)
def test_reference_config_builds_unchanged_and_param_options(fname, preset, typ):
    from vfmseg_amd.optim import param_options
    cfg, m = _shrunk(fname)
    model = MODELS.build(m)
    assert type(model).__name__ == typ == m["type"] and type(model.decode_head).__name__ == "SegformerHead"
    ow = cfg.optim_wrapper
    lr, wd = ow["optimizer"]["lr"], ow["optimizer"]["weight_decay"]
    opts = param_options(model.train(), lr, wd, ow.get("paramwise_cfg"))
    names = {n for n, p in model.named_parameters() if p.requires_grad}
    assert set(opts) == names
    gn = [n for n in opts if ".gn." in n]
    assert len(gn) == 10 and all(opts[n][1] == 0.0 for n in gn)            # norm_decay_mult=0: no weight decay on GroupNorm
    assert all(opts[n][1] == wd for n in opts if n.endswith("conv.weight") or n.endswith("conv_seg.weight"))
    if typ == "FrozenBackboneEncoderDecoder":
        assert opts and all(n.startswith("decode_head.") for n in opts)
        assert not model.backbone.training and not any(p.requires_grad for p in model.backbone.parameters())
        assert any(k.startswith("backbone.blocks.0.") for k in model.state_dict())     # the checkpoint holds the whole model
    elif typ == "EncoderDecoder":
        assert any(n.startswith("backbone.reins.") for n in opts) and opts["backbone.reins.scale"][1] == 0.0
    else:
        assert any("lora_A" in n for n in opts) and not any(n.startswith("backbone.") and "lora_" not in n for n in opts)


def test_head_state_dict_keys_and_refusals():
    head = MODELS.build(presets.segformer_head())
    assert sorted(head.state_dict()) == sorted(S.HEAD_KEYS)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {k: tuple(v) for k, v in S.head_shapes(prefix="").items()}
    assert head.convs[0].conv.bias is None and head.fusion_conv.conv.bias is None
    for bad in (dict(norm_cfg=dict(type="BN", requires_grad=True)), dict(norm_cfg=None), dict(interpolate_mode="nearest"),
                dict(in_channels=[1024, 1024, 512, 1024])):
        with pytest.raises(NotImplementedError):
            MODELS.build(dict(presets.segformer_head(), **bad))
    with pytest.raises(NotImplementedError, match="differing size"):
        head._pack([torch.zeros(1, 1024, 8, 8)] * 3 + [torch.zeros(1, 1024, 4, 4)])


def test_configs_are_thin_pass_throughs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for fname, preset in (("dg_lora_dinov2_segformer.py", presets.dinov2_segformer), ("dg_rein_dinov2_segformer.py", presets.rein_dinov2_segformer),
                          ("dg_fzn_dinov2_segformer.py", presets.frozen_dinov2_segformer)):
        cfg = Config.fromfile(os.path.join(root, "configs", fname))
        assert _plain(cfg.model) == _plain(preset())
        assert _plain(cfg.optim_wrapper) == _plain(presets.optim_cfg()["optim_wrapper"])


def test_frozen_segmentor_freezes_the_backbone_for_good():
    cfg = S.model_config("frozen", depth=2)
    model = MODELS.build(cfg)
    for mode in (True, False, True):
        model.train(mode)
        assert not model.backbone.training and model.decode_head.training == mode
        assert not any(p.requires_grad for p in model.backbone.parameters()) and all(p.requires_grad for p in model.decode_head.parameters())


def test_float64_restatement_reproduces_the_fixture():
    """tests/segformer_helpers.head_forward / head_loss (what the GPU tests call float64 truth) against the head the generator restated on
    the reference shim's own ConvModule / resize / accuracy / CrossEntropyLoss: outputs to 1e-6 of their range."""
    g = np.load(GOLD)
    assert list(g["seeds_depth"]) == [S.HEAD_SEED, S.TRAIN_SEED, S.EVAL_SEED, S.DEPTH]
    assert list(g["head_param_names"]) == sorted(S.HEAD_KEYS)
    sd = S.head_state_dict(prefix="")
    logits, loss, acc, grads, tap_grads = S.head_ref_grads(sd, S.head_feats(), synth_label(2, 512, seed=S.HEAD_SEED))

    def close(a, b, tol=1e-6):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert a.shape == b.shape and np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30), (np.abs(a - b).max(), np.abs(b).max())
    close(sl(logits), g["head::logits_slice"])
    close(logits[:, :, 3::8, 5::8].numpy(), g["head::logits_grid"])
    close(stats(logits), g["head::logits_stats"])
    close([loss.item(), acc.item()], g["head::loss_acc"])
    for k in S.HEAD_KEYS:
        gr = grads[k]
        close(sl(gr.reshape(gr.shape[0], -1) if gr.dim() > 1 else gr), g[f"head::grad_slice::{k}"])
        close([gr.norm().item()], g[f"head::grad_norm::{k}"])
    for i, t in enumerate(tap_grads):
        close([t.norm().item()], g[f"head::tap_grad_norm::{i}"])
        close(sl(t[:, :, 8:, 8:]), g[f"head::tap_grad_slice::{i}"])
    close(sl(S.head_forward(sd, S.head_feats())), g["head::eval_logits_slice"])
    assert g["head::sensitivity"].min() >= 0.1     # the fixture sees every branch, the ReLU and the fusion norm


def test_frozen_segmentor_loads_the_backbone_named_by_init_cfg(tmp_path):
    """dinov2_SegFormer_frozen.py hands the frozen weights over through the backbone's init_cfg: a bare state dict on disk arrives in the
    backbone (and nowhere else), a file whose keys do not match is an error and not an untrained frozen base, and an init_cfg type
    other than Pretrained is refused."""
    from tests.rein_helpers import bare_dinov2_state_dict
    depth = 2
    sd = bare_dinov2_state_dict(depth)
    good, bad = tmp_path / "base.pth", tmp_path / "prefixed.pth"
    torch.save(sd, good)
    torch.save({"backbone." + k: v for k, v in sd.items()}, bad)

    def cfg(ck, typ="Pretrained"):
        c = presets.frozen_dinov2_segformer(depth=depth, checkpoint=str(ck))
        c["backbone"]["out_indices"] = [0, 1, 1, 1]
        c["backbone"]["init_cfg"]["type"] = typ
        return c
    model = MODELS.build(cfg(good))
    got = model.backbone.state_dict()
    assert sorted(got) == sorted(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    fresh = MODELS.build(dict(cfg(good), backbone=dict(cfg(good)["backbone"], init_cfg=None)))
    assert not torch.equal(fresh.backbone.state_dict()["blocks.0.attn.qkv.weight"], sd["blocks.0.attn.qkv.weight"])   # the load is what put them there
    assert not any(p.requires_grad for p in model.backbone.parameters()) and not model.backbone.training
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        MODELS.build(cfg(bad))
    with pytest.raises(NotImplementedError, match="init_cfg type"):
        MODELS.build(cfg(good, typ="Kaiming"))
    # {"state_dict": ...} files, as checkpoints are written, load too
    torch.save({"state_dict": sd}, good)
    assert torch.equal(MODELS.build(cfg(good)).backbone.state_dict()["pos_embed"], sd["pos_embed"])
