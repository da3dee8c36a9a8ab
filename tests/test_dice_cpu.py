"""DiceLoss and multi-loss loss_decode lists without a GPU:

- the float64 restatement of mmseg 1.2.2 DiceLoss (tests/dice_helpers.py): its autograd gradient against the closed form
  (alpha, beta, gamma) the HIP kernels use, in all four forms,
- the registry / config surface: the list and DiceLoss build from a config dict and from --cfg-options, every refusal names its option,
  loss_options_named sees lists, and a dict loss_decode still builds the single module it built before.
"""
import os

import pytest
import torch

import vfmseg_amd  # noqa: F401
from tests import dice_helpers as DH
from vfmseg_amd import presets
from vfmseg_amd.registry import MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE_DICE = "[dict(type='CrossEntropyLoss',loss_name='loss_ce',loss_weight=1.0),dict(type='DiceLoss',loss_name='loss_dice',loss_weight=3.0)]"


# ------------------------------------------------------------------------------------------------ the definition, float64
@pytest.mark.parametrize("drop_class", [-1, 3])
@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
def test_autograd_gradient_equals_the_closed_form(use_sigmoid, naive, drop_class):
    B, h, w, H, W, C = 2, 5, 7, 33, 45, 19
    lg = DH.rnd(B, h, w, C, seed=21, scale=2.0)
    lab = DH.labels(B, H, W, C, 22, all_ignored_image=True)   # image 1 is ignored altogether
    lab[0, 5, 5], lab[0, 6, 6] = 40, -3                       # a class >= C (an all-zero row), a negative label (class 0)
    ref = DH.dice(lg, lab, use_sigmoid, naive, eps=1e-3, drop_class=drop_class, loss_weight=3.0)
    closed = DH.closed_form_grad_p(ref, naive, drop_class, loss_weight=3.0)
    err = float((ref["grad_p"] - closed).abs().max()) / float(closed.abs().max())
    assert err < 1e-12, err
    # the ignored image: a = 0, its term of the loss is 1 - d with d = 0 (plain) or eps / s (naive)
    assert float(ref["a"][1]) == 0.0 and float(ref["c"][1]) == 0.0
    if naive:
        assert float(ref["coef"][1, 2]) > 0 and float(ref["grad"][1].abs().max()) > 0
    else:
        assert float(ref["d"][1]) == 0.0 and float(ref["grad"][1].abs().max()) == 0.0
    t = ref["t"]
    assert float(t[0, :, 5, 5].sum()) == 0.0 and float(t[0, 0, 6, 6]) == 1.0 and float(t[:, :, 2:4].sum()) == 0.0


def test_restatement_equals_mmseg_written_out():
    """mmseg's dice_loss / naive_dice_loss on flattened [N, C*H*W] inputs, written out independently of the helper's sums."""
    B, h, H, C = 2, 4, 16, 7
    lg, lab = DH.rnd(B, h, h, C, seed=23, scale=2.0), DH.labels(B, H, H, C, 24)
    for use_sigmoid, naive in DH.FORMS:
        ref = DH.dice(lg, lab, use_sigmoid, naive, eps=1e-3, loss_weight=0.7)
        up = DH.upsampled(lg, (H, H))
        p = (up.sigmoid() if use_sigmoid else up.softmax(1)).flatten(1)
        t = DH.one_hot(lab, C).flatten(1)
        a = torch.sum(p * t, 1)
        if naive:
            d = (2 * a + 1e-3) / (torch.sum(p, 1) + torch.sum(t, 1) + 1e-3)
        else:
            d = 2 * a / ((torch.sum(p * p, 1) + 1e-3) + (torch.sum(t * t, 1) + 1e-3))
        assert abs(ref["loss"] - float(0.7 * (1 - d).mean())) < 1e-14


# ------------------------------------------------------------------------------------------------ registry and config
def _head(kind, **extra):
    cfg = dict(linear=presets.linear_head, segformer=presets.segformer_head, vfm=presets.vfm_head)[kind](embed_dim=64, channels=128)
    cfg.update(extra)
    return cfg


def test_dice_loss_builds_with_the_mmseg_constructor():
    from vfmseg_amd.dice_loss import DiceLoss
    assert MODELS.get("DiceLoss") is DiceLoss
    mod = MODELS.build(dict(type="DiceLoss"))
    assert (mod.use_sigmoid, mod.naive_dice, mod.loss_weight, mod.ignore_index, mod.eps, mod.loss_name) == (True, False, 1.0, 255, 1e-3, "loss_dice")
    assert mod.drop_class(19) == -1
    mod = MODELS.build(dict(type="DiceLoss", use_sigmoid=False, activate=True, reduction="mean", naive_dice=True, loss_weight=3.0, ignore_index=4,
                            eps=1e-2, loss_name="loss_d2"))
    assert (mod.use_sigmoid, mod.naive_dice, mod.loss_weight, mod.eps, mod.loss_name) == (False, True, 3.0, 1e-2, "loss_d2")
    assert mod.drop_class(19) == 4 and mod.drop_class(4) == -1


@pytest.mark.parametrize("kind", ["linear", "segformer", "vfm"])
def test_a_loss_decode_list_builds_a_module_list(kind):
    from vfmseg_amd.dice_loss import DiceLoss
    from vfmseg_amd.heads import CrossEntropyLoss
    head = MODELS.build(_head(kind, loss_decode=presets.ce_dice_loss()))
    assert isinstance(head.loss_decode, torch.nn.ModuleList) and len(head.loss_decode) == 2
    ce, dice = head.loss_decode
    assert isinstance(ce, CrossEntropyLoss) and isinstance(dice, DiceLoss)
    assert (ce.loss_name, ce.loss_weight, dice.loss_name, dice.loss_weight) == ("loss_ce", 1.0, "loss_dice", 3.0)
    tup = MODELS.build(_head(kind, loss_decode=tuple(presets.ce_dice_loss(dice=0.5, naive_dice=True))))
    assert isinstance(tup.loss_decode, torch.nn.ModuleList) and tup.loss_decode[1].naive_dice and tup.loss_decode[1].loss_weight == 0.5


@pytest.mark.parametrize("kind", ["linear", "segformer", "vfm"])
def test_a_dict_loss_decode_builds_the_single_module_it_built_before(kind):
    from vfmseg_amd.heads import CrossEntropyLoss
    head = MODELS.build(_head(kind))
    assert type(head.loss_decode) is CrossEntropyLoss and head.loss_decode.loss_name == "loss_ce" and head.loss_decode.loss_weight == 1.0
    assert not any(k.startswith("loss_decode.") for k in head.state_dict())   # no new keys in a checkpoint


def test_cfg_options_line_of_the_readme_builds_the_list():
    from vfmseg_amd.config import Config, parse_cfg_options
    from vfmseg_amd.dice_loss import DiceLoss
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "dg_lora_dinov2_segformer.py"))
    assert isinstance(cfg.model.decode_head.loss_decode, dict)
    cfg.merge_from_dict(parse_cfg_options(["model.decode_head.loss_decode=" + CE_DICE]))
    assert isinstance(cfg.model.decode_head.loss_decode, list) and cfg.model.decode_head.loss_decode[1].type == "DiceLoss"
    head = MODELS.build(cfg.model.decode_head)
    assert isinstance(head.loss_decode[1], DiceLoss) and head.loss_decode[1].loss_weight == 3.0 and head.loss_decode[0].loss_name == "loss_ce"
    # the parser still reads what it read before
    assert parse_cfg_options(["a.b=1", "c=[1,2]", "d=str", "e=work_dirs/x", "f=1e-3", "g=None"]) == \
        {"a.b": 1, "c": [1, 2], "d": "str", "e": "work_dirs/x", "f": 1e-3, "g": None}


def test_the_list_in_a_config_file(tmp_path):
    from vfmseg_amd.config import Config
    path = tmp_path / "ce_dice.py"
    path.write_text("_base_ = %r\nmodel = dict(decode_head=dict(loss_decode=%s))\n"
                    % (os.path.join(ROOT, "configs", "dg_lora_dinov2_segformer.py"), CE_DICE))
    cfg = Config.fromfile(str(path))
    head = MODELS.build(cfg.model.decode_head)
    assert [m.loss_name for m in head.loss_decode] == ["loss_ce", "loss_dice"]


def test_refusals_name_their_option():
    for bad, name in ((dict(activate=False), "activate"), (dict(reduction="sum"), "reduction"), (dict(reduction="none"), "reduction")):
        with pytest.raises(NotImplementedError, match=name):
            MODELS.build(dict(type="DiceLoss", **bad))
    with pytest.raises(NotImplementedError, match="out_channels"):
        MODELS.build(_head("segformer", num_classes=2, out_channels=1, loss_decode=presets.ce_dice_loss()))
    with pytest.raises(NotImplementedError, match="out_channels"):
        MODELS.build(_head("segformer", num_classes=2, out_channels=1, loss_decode=dict(type="DiceLoss")))
    with pytest.raises(NotImplementedError, match="sampler"):
        MODELS.build(_head("linear", loss_decode=presets.ce_dice_loss(), sampler=dict(type="OHEMPixelSampler", thresh=0.7, min_kept=1000)))
    with pytest.raises(ValueError, match="loss_decode"):
        MODELS.build(_head("linear", loss_decode=[]))
    head = MODELS.build(_head("segformer", loss_decode=presets.ce_dice_loss()))
    with pytest.raises(NotImplementedError, match="seg_weight"):
        head.loss_by_feat(torch.zeros(1, 2, 2, 19), torch.zeros(1, 8, 8, dtype=torch.int64), seg_weight=torch.ones(1, 8, 8))


def test_loss_options_named_sees_lists():
    from vfmseg_amd.heads import loss_options_named
    assert loss_options_named(_head("linear")) == []
    assert loss_options_named(_head("linear", loss_decode=presets.ce_dice_loss())) == ["loss_decode list", "DiceLoss"]
    assert loss_options_named(_head("linear", loss_decode=dict(type="DiceLoss"))) == ["DiceLoss"]
    two_ce = [dict(type="CrossEntropyLoss", loss_name="loss_a"), dict(type="CrossEntropyLoss", loss_name="loss_b", avg_non_ignore=True)]
    assert loss_options_named(_head("linear", loss_decode=two_ce, sampler=dict(type="OHEMPixelSampler", thresh=0.7))) == \
        ["sampler", "loss_decode list", "avg_non_ignore"]
    assert loss_options_named(_head("linear", loss_decode=dict(type="CrossEntropyLoss", class_weight=[1.0] * 19))) == ["class_weight"]


@pytest.mark.parametrize("where", ["HRDAHead", "seg_head", "single_scale_head"])
def test_hrda_head_refuses_a_list(where):
    cfg = dict(type="HRDAHead", seg_head=presets.linear_head(64, 64), single_scale_head=presets.attention_head(64, 64), hr_loss_weight=0.1,
               scales=[1, 0.5])
    (cfg if where == "HRDAHead" else cfg[where])["loss_decode"] = presets.ce_dice_loss()
    with pytest.raises(NotImplementedError, match="loss_decode list"):
        MODELS.build(cfg)


def test_dacs_refuses_dice_on_its_decode_head():
    from tests import dacs_helpers as D
    cfg = D.dacs_config(0.9, depth=1)
    cfg["decode_head"]["loss_decode"] = presets.ce_dice_loss()
    with pytest.raises(NotImplementedError, match="DiceLoss"):
        MODELS.build(cfg)
