"""HRDA, CPU side: registry names, config parity with the reference's own file, state-dict keys, the crop-box stream, the float64
restatement of the fusion against the reference-made fixture (tests/golden/hrda.npz, tools/gen_hrda_golden.py), the unsupported options."""
import copy
import os

import numpy as np
import pytest
import torch

import vfmseg_amd  # noqa: F401
from tests import hrda_helpers as H
from tests.helpers import rel_err
from vfmseg_amd import presets
from vfmseg_amd.config import Config
from vfmseg_amd.registry import MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CFG = "/root/reference/configs/dg/gta2citys/dg_lora_dinov2_hrda_1024x1024.py"


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "hrda.npz"))


def _small(cfg, depth=2):
    cfg = copy.deepcopy(cfg)
    cfg["backbone"]["backbone"].update(depth=depth, out_indices=[0, 1, 1, 1] if depth == 2 else list(range(depth)))
    cfg["backbone"]["checkpoint"] = None
    return cfg


def test_registry_has_the_hrda_names():
    for name in ("HRDAEncoderDecoder", "FrozenHRDAEncoderDecoder", "HRDAHead", "AttentionHead"):
        assert MODELS.get(name) is not None, name


@pytest.mark.skipif(not os.path.exists(REF_CFG), reason="reference tree not present (GPU box)")
def test_reference_config_equals_preset_and_builds():
    from tests.test_reference_configs_cpu import ALLOWED, _diff, _plain
    cfg = Config.fromfile(REF_CFG)
    bad = [d for d in _diff(_plain(cfg.model), _plain(presets.dinov2_hrda())) if not any(a in d[0] for a in ALLOWED)]
    assert not bad, bad[:8]
    ours = Config.fromfile(os.path.join(ROOT, "configs", "dg_lora_dinov2_hrda.py"))
    assert not [d for d in _diff(_plain(cfg.model), _plain(ours.model)) if not any(a in d[0] for a in ALLOWED)]
    assert _plain(cfg.optim_wrapper) == _plain(ours.optim_wrapper) and _plain(cfg.param_scheduler) == _plain(ours.param_scheduler)
    model = MODELS.build(_small(cfg.model))
    assert type(model).__name__ == "HRDAEncoderDecoder" and model.scales == [0.5, 1]
    assert model.decode_head.enable_hr_crop and model.decode_head.scales == [0.5, 1]


def test_state_dict_keys_equal_the_reference(G):
    model = MODELS.build(_small(presets.dinov2_hrda(), depth=4))
    assert sorted(model.state_dict()) == list(G["model_param_names"])
    assert "decode_head.conv_seg.weight" in model.state_dict()
    head = MODELS.build(dict(presets.dinov2_hrda()["decode_head"], scales=[0.5, 1]))
    assert sorted(head.state_dict()) == list(G["head_param_names"])
    assert sorted(H.hrda_model_state_dict(4)) == list(G["model_param_names"])


def test_unused_conv_seg_is_frozen_like_the_reference_leaves_it(G):
    """hrda.py:72-76 keeps BaseDecodeHead's conv_seg and never calls it: in the reference it has no gradient, so AdamW never touches it.
    Here it must stay out of the optimiser's flat buffers (a zero gradient would still be weight-decayed)."""
    from vfmseg_amd.optim import param_options
    model = MODELS.build(_small(presets.dinov2_hrda())).train()
    assert list(G["train_no_grad"]) == ["decode_head.conv_seg.bias", "decode_head.conv_seg.weight"]
    opts = param_options(model, 1e-4, 0.05, presets.optim_cfg()["optim_wrapper"]["paramwise_cfg"])
    assert not any(k.startswith("decode_head.conv_seg") for k in opts)
    assert "decode_head.head.conv_seg.weight" in opts and "decode_head.scale_attention.conv_seg.weight" in opts
    n = sum(p.numel() for k, p in model.named_parameters() if p.requires_grad and "blocks.1." not in k)
    n4 = sum(p.numel() for k, p in MODELS.build(_small(presets.dinov2_hrda(), depth=4)).train().named_parameters() if p.requires_grad)
    assert n4 == int(G["train_n_trainable"][0]) and n < n4


def test_crop_boxes_follow_the_numpy_stream(G):
    seed = int(G["train_np_seed"][0])
    boxes = H.np_boxes(seed, 6)
    assert np.array_equal(np.array(boxes), G["train_boxes_stream"])
    assert tuple(G["train_box"]) == boxes[0]
    assert all(v % 8 == 0 for b in boxes for v in b) and len(set(boxes)) > 1
    from vfmseg_amd.segmentors import get_crop_bbox
    state = np.random.get_state()[1].copy()
    assert get_crop_bbox(512, 512, (512, 512), 8) == (0, 512, 0, 512)      # no draw when the image already has crop size
    assert np.array_equal(np.random.get_state()[1], state)


def test_scale_box_truncates():
    from vfmseg_amd.heads import scale_box
    assert scale_box((88, 600, 216, 728), 4) == (22, 150, 54, 182)
    assert scale_box((90, 602, 220, 732), 8.0) == (11, 75, 27, 91)


@pytest.mark.parametrize("case", ["inner", "corner", "nocrop", "wide"])
def test_float64_restatement_matches_the_reference(G, case):
    """tests/hrda_helpers.fuse_ref (the GPU tests' reference) against HRDAHead.forward of the reference run on the same logits in
    float64: fused, (1 - att) * lr and all three gradients."""
    k = f"fuse_{case}::"
    B, C, ha, wa, h, w, hc, wc, seed, y1, y2, x1, x2 = (int(v) for v in G[k + "shape"])
    lr, a, hr, dF = (t.double() for t in H.fuse_inputs(B, C, ha, wa, h, w, hc, wc, seed))
    box = None if y1 < 0 else (y1, y2, x1, x2)
    offset = (0, 0) if box is None else H.scale_box(box, 4)[::2]
    mask_box = None if box is None else H.scale_box(box, 8.0)
    got = H.fuse_ref_grads(lr, a, hr, offset, mask_box, dF)
    for name, t in zip(("fused", "lr_scaled", "d_lr", "d_a", "d_hr"), got):
        assert tuple(t.shape) == G[k + name].shape
        assert rel_err(t, G[k + name]) < 1e-6, (case, name)      # the fixture stores float64 results in fp32
    if box is not None:   # the mask is visible in this case
        no_mask = H.fuse_ref_grads(lr, a, hr, offset, mask_box, dF, drop="mask")
        assert rel_err(no_mask[0], G[k + "fused"]) > 1e-2


def test_fixture_can_see_the_feature(G):
    for case in H.HEAD_BOXES:
        mean, std = G[f"head_{case}::att_mean_std"]
        assert std >= 0.1 and 0.2 < mean < 0.8
        assert (G[f"head_{case}::fused_vs_uplr_vs_hr"] >= 0.3).all()
        assert int(G[f"head_{case}::bn_num_batches_tracked"][0]) == 2
    assert int(G["train_bn_num_batches_tracked"][0]) == 2
    # the recorded BatchNorm statistics are those after the two updates, not the initial ones
    for prefix, keys in (("decode_head.", ["train_"]), ("", ["head_inner::", "head_corner::"])):
        sd = H.hrda_head_state_dict(prefix=prefix)
        for n in ("running_mean", "running_var"):
            start = sd[prefix + "head.output_upscaling.1." + n][:8]
            for k in keys:
                assert rel_err(G[f"{k}bn_{n}_slice"], start) > 1e-2, (k, n)
    assert list(G["train_loss_keys"]) == ["decode.loss_seg", "decode.acc_seg", "decode.hr.loss_seg", "decode.hr.acc_seg"]


def test_unsupported_options_raise():
    head = presets.dinov2_hrda()["decode_head"]
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(head, single_scale_head="DAFormerHead"))
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(head, lr_loss_weight=0.1))
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(head, seg_head=dict(head["seg_head"], type="DAFormerHead")))
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(head, single_scale_head=dict(head["single_scale_head"], norm_cfg=dict(type="BN", requires_grad=True))))
    cfg = _small(presets.dinov2_hrda())
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(cfg, blur_hr_crop=True))
    for key in ("test_time_aug", "flip"):
        with pytest.raises(NotImplementedError):
            MODELS.build(dict(cfg, test_cfg=dict(cfg["test_cfg"], **{key: True})))


def test_accuracy_counts_every_pixel(G):
    """rein/models/heads/utils.py:35-80: 100 * correct / label.numel(), ignored pixels in the denominator.  The recorded accuracies are
    whole pixel counts over ALL pixels (they are not over the valid ones: the labels carry a 5 % ignore band) - what the GPU tests hold
    UpsampleCEAllFn to."""
    from vfmseg_amd.synth import synth_label
    lab = synth_label(2, 1024, seed=H.HEAD_SEED)
    valid = int((lab != 255).sum())
    assert valid < lab.numel()
    for case, box in H.HEAD_BOXES.items():
        acc = float(G[f"head_{case}::losses"][1])
        hits = acc * lab.numel() / 100.0
        assert abs(hits - round(hits)) < 0.05, hits
        hits_valid = acc * valid / 100.0
        assert abs(hits_valid - round(hits_valid)) > 0.05, "the recorded accuracy would also fit the valid-pixel denominator: case is blind"


def test_frozen_variant_freezes_the_backbone():
    cfg = _small(presets.dinov2_hrda())
    model = MODELS.build(dict(cfg, type="FrozenHRDAEncoderDecoder")).train()
    assert not model.backbone.training and not any(p.requires_grad for p in model.backbone.parameters())
    assert model.decode_head.training and any(p.requires_grad for p in model.decode_head.parameters())
