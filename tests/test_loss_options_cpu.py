"""The loss options of the fused cross-entropy (OHEM pixel sampler, class weights, avg_non_ignore) without a GPU:

- the float64 restatement of the semantics (tests/loss_options_helpers.py) against an independent formulation,
- the three-round histogram selection of vfmseg_amd/csrc/ohem_select.h as a stand-alone host program (tests/ohem_select_main.cpp, plain
  g++ under -fsanitize=undefined,address) against std::sort,
- the registry / config surface: what builds, what is refused and that every refusal names its option.
"""
import os
import subprocess

import pytest
import torch

import vfmseg_amd  # noqa: F401
from tests import loss_options_helpers as LO
from vfmseg_amd import presets
from vfmseg_amd.registry import MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OHEM = dict(type="OHEMPixelSampler", thresh=0.7, min_kept=100000)
CW19 = [0.5 + 0.1 * c for c in range(19)]


# ------------------------------------------------------------------------------------------------ the definition, float64
@pytest.mark.parametrize("thresh,min_kept", [(None, None), (0.05, 300), (0.7, 50), (0.3, 10 ** 6)])
@pytest.mark.parametrize("use_cw,avg_non_ignore", [(False, False), (False, True), (True, False), (True, True)])
def test_restatement_equals_the_independent_formulation(thresh, min_kept, use_cw, avg_non_ignore):
    B, h, H, C = 2, 8, 32, 19
    lg, lab = LO.rnd(B, h, h, C, seed=11, scale=2.0), LO.labels(B, H, H, C, 12)
    cw = CW19 if use_cw else None
    ref = LO.options(lg, lab, thresh, min_kept, cw, avg_non_ignore, loss_weight=0.4)
    other = LO.independent(lg, lab, ref["mask"] if thresh is not None else None, cw, avg_non_ignore, loss_weight=0.4)
    assert abs(ref["loss"] - other) < 1e-12 * max(1.0, abs(other))
    valid = lab != 255
    assert ref["n"] == int(valid.sum()) and not bool(ref["mask"][~valid].any())
    if thresh is not None:
        s = torch.sort(ref["p"][valid])[0]
        assert ref["k"] == min(min_kept * B, ref["n"] - 1) and ref["t"] == max(float(s[ref["k"]]), thresh)
        assert int(ref["mask"].sum()) == int((ref["p"][valid] < ref["t"]).sum())   # strict: the k-th pixel itself is kept only under thresh
    if not use_cw and not avg_non_ignore:
        assert ref["avg_factor"] == lab.numel()
    if use_cw:
        assert abs(ref["avg_factor"] - sum(CW19[int(c)] for c in lab[valid])) < 1e-9


def test_restatement_regimes_and_the_all_ignored_batch():
    B, h, H, C = 2, 8, 32, 19
    lg, lab = LO.rnd(B, h, h, C, seed=13, scale=2.0), LO.labels(B, H, H, C, 14)
    n = int((lab != 255).sum())
    reg = LO.regimes(lg, lab)
    above = LO.options(lg, lab, *reg["above"])      # the k-th value lies above thresh
    below = LO.options(lg, lab, *reg["below"])      # below it: t = thresh
    clamped = LO.options(lg, lab, *reg["clamped"])  # k = n - 1: t = the largest p, everything but the ties with it is kept
    assert above["t"] > reg["above"][0] and above["n_lt"] <= above["k"] and int(above["mask"].sum()) == above["k"]
    assert below["t"] == reg["below"][0] and below["n_lt"] > below["k"] and int(below["mask"].sum()) == below["n_lt"]
    assert clamped["k"] == n - 1 and int(clamped["mask"].sum()) == int((clamped["p"][lab != 255] < clamped["t"]).sum()) >= n - 2
    every = LO.options(lg, lab, 2.0, 50)
    plain = LO.options(lg, lab)
    assert every["loss"] == plain["loss"] and torch.equal(every["grad"], plain["grad"])
    none = LO.options(lg, torch.full_like(lab, 255), 0.7, 50, CW19, True)
    assert none["loss"] == 0.0 and float(none["grad"].abs().max()) == 0.0 and none["t"] == 0.7 and none["n"] == 0


# ------------------------------------------------------------------------------------------------ the selection on the host
def test_three_round_selection_equals_std_sort_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ohem_select_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "vfmseg_amd", "csrc"), os.path.join(ROOT, "tests", "ohem_select_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 600, r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ registry and config
def _head(kind, **extra):
    cfg = dict(linear=presets.linear_head, segformer=presets.segformer_head, vfm=presets.vfm_head)[kind](embed_dim=64, channels=128)
    cfg.update(extra)
    return cfg


@pytest.mark.parametrize("kind", ["linear", "segformer", "vfm"])
def test_sampler_config_builds_an_ohem_sampler_on_the_head(kind):
    from vfmseg_amd.loss_options import OHEMPixelSampler
    head = MODELS.build(_head(kind, sampler=dict(OHEM)))
    assert isinstance(head.sampler, OHEMPixelSampler)
    assert head.sampler.context is head and head.sampler.thresh == 0.7 and head.sampler.min_kept == 100000
    assert MODELS.build(_head(kind)).sampler is None
    assert MODELS.get("OHEMPixelSampler") is OHEMPixelSampler


def test_cfg_options_line_of_the_readme_turns_ohem_on():
    from vfmseg_amd.config import Config, parse_cfg_options
    from vfmseg_amd.loss_options import OHEMPixelSampler
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "dg_lora_dinov2_segformer.py"))
    assert cfg.model.decode_head.get("sampler") is None
    cfg.merge_from_dict(parse_cfg_options(["model.decode_head.sampler.type=OHEMPixelSampler", "model.decode_head.sampler.thresh=0.7",
                                           "model.decode_head.sampler.min_kept=100000"]))
    head = MODELS.build(cfg.model.decode_head)
    assert isinstance(head.sampler, OHEMPixelSampler) and (head.sampler.thresh, head.sampler.min_kept) == (0.7, 100000)


def test_cross_entropy_loss_builds_with_class_weight_and_avg_non_ignore():
    mod = MODELS.build(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4, class_weight=CW19, avg_non_ignore=True))
    assert mod.class_weight == CW19 and mod.avg_non_ignore is True and mod.has_options and mod.loss_weight == 0.4
    assert torch.equal(mod.class_weight_on("cpu", 19), torch.tensor(CW19, dtype=torch.float32))
    plain = MODELS.build(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))
    assert plain.class_weight is None and plain.avg_non_ignore is False and not plain.has_options
    head = MODELS.build(_head("linear", loss_decode=dict(type="CrossEntropyLoss", class_weight=CW19, avg_non_ignore=True)))
    assert head.loss_decode.has_options
    with pytest.raises(ValueError, match="class_weight"):
        mod.class_weight_on("cpu", 7)


def test_refusals_name_their_option():
    with pytest.raises(NotImplementedError, match="thresh=None"):
        MODELS.build(_head("linear", sampler=dict(type="OHEMPixelSampler", min_kept=100000)))
    with pytest.raises(NotImplementedError, match="class_weight"):
        MODELS.build(dict(type="CrossEntropyLoss", class_weight="weights.npy"))
    for bad in (dict(use_sigmoid=True), dict(reduction="sum")):
        with pytest.raises(NotImplementedError):
            MODELS.build(dict(type="CrossEntropyLoss", **bad))


@pytest.mark.parametrize("where", ["HRDAHead", "seg_head", "single_scale_head"])
@pytest.mark.parametrize("option", ["sampler", "class_weight", "avg_non_ignore"])
def test_hrda_head_refuses_the_loss_options(where, option):
    cfg = dict(type="HRDAHead", seg_head=presets.linear_head(64, 64), single_scale_head=presets.attention_head(64, 64), hr_loss_weight=0.1,
               scales=[1, 0.5])
    target = cfg if where == "HRDAHead" else cfg[where]
    if option == "sampler":
        target["sampler"] = dict(OHEM)
    else:
        target["loss_decode"] = dict(type="CrossEntropyLoss", **{option: CW19 if option == "class_weight" else True})
    with pytest.raises(NotImplementedError, match=option):
        MODELS.build(cfg)
    MODELS.build(dict(type="HRDAHead", seg_head=presets.linear_head(64, 64), single_scale_head=presets.attention_head(64, 64),
                      hr_loss_weight=0.1, scales=[1, 0.5]))   # the plain head still builds


def test_dacs_refuses_a_sampler_on_its_decode_head():
    from tests import dacs_helpers as D
    cfg = D.dacs_config(0.9, depth=1)
    cfg["decode_head"]["sampler"] = dict(OHEM)
    with pytest.raises(NotImplementedError, match="sampler"):
        MODELS.build(cfg)


def test_seg_weight_and_sampler_collide_in_loss_by_feat():
    head = MODELS.build(_head("segformer", sampler=dict(OHEM)))
    with pytest.raises(ValueError, match="sampler"):
        head.loss_by_feat(torch.zeros(1, 2, 2, 19), torch.zeros(1, 8, 8, dtype=torch.int64), seg_weight=torch.ones(1, 8, 8))
