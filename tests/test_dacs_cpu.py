"""DACS without a GPU: the registry builds the segmentor and the paired dataset from the new config, UDADataset yields pairs, the float64
helpers reproduce tests/golden/dacs.npz, and the option sets outside the HIP path are refused."""
import copy
import os
import tempfile

import numpy as np
import pytest
import torch

import vfmseg_amd  # noqa: F401
from tests import dacs_helpers as D
from tests import rcs_toy
from vfmseg_amd.config import Config
from vfmseg_amd.datasets import DataLoaderIter, UDADataset, pseudo_collate
from vfmseg_amd.registry import DATASETS, MODELS
from vfmseg_amd.synth import synth_label

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cfg():
    return Config.fromfile(os.path.join(ROOT, "configs", "uda_rein_dinov2_segformer.py"))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "dacs.npz"))


def _small(model_cfg):
    """the config's model at depth 1 (construction only)"""
    m = copy.deepcopy(dict(model_cfg))
    m["backbone"] = dict(m["backbone"], depth=1, out_indices=[0, 0, 0, 0])
    m["backbone"]["reins_config"] = dict(m["backbone"]["reins_config"], num_layers=1)
    m["backbone"].pop("init_cfg", None)
    return m


def test_registry_builds_dacs_from_the_config(cfg):
    from vfmseg_amd.uda import DACS
    m = cfg["model"]
    assert m["type"] == "DACS" and m["blur"] is False and m["color_jitter_probability"] >= 1
    assert (m["alpha"], m["pseudo_threshold"], m["pseudo_weight_ignore_top"], m["pseudo_weight_ignore_bottom"], m["mix"]) == (0.999, 0.968, 15, 120, "class")
    model = MODELS.build(_small(m))
    assert isinstance(model, DACS) and model.local_iter == 0
    keys = list(model.state_dict())
    head = sorted(k[len("decode_head."):] for k in keys if k.startswith("decode_head."))
    assert head and sorted(k[len("ema_head."):] for k in keys if k.startswith("ema_head.")) == head
    assert all(not p.requires_grad for p in model.ema_head.parameters()) and any(p.requires_grad for p in model.decode_head.parameters())
    assert model.ema_head.dropout_ratio == 0.0 and model.decode_head.dropout_ratio == 0.1


def test_registry_builds_the_paired_dataset_from_the_config(cfg):
    ds_cfg = dict(cfg["train_dataloader"]["dataset"])
    assert ds_cfg["type"] == "UDADataset" and ds_cfg["source"]["data_root"] == "data/gta/" and ds_cfg["target"]["data_root"] == "data/cityscapes/"
    assert ds_cfg["rare_class_sampling"] == dict(class_temp=0.01, min_crop_ratio=0.5, min_pixels=3000)
    with tempfile.TemporaryDirectory() as root:
        rcs_toy.write_stats(root, rcs_toy.label_maps())
        ds = DATASETS.build(dict(ds_cfg, source=rcs_toy.ToySource(root), target=rcs_toy.ToySource(root), rare_class_sampling=rcs_toy.RCS))
        assert isinstance(ds, UDADataset) and len(ds) == rcs_toy.N_FILES ** 2


@pytest.mark.parametrize("rcs", [False, True])
def test_uda_dataset_yields_pairs(rcs):
    with tempfile.TemporaryDirectory() as root:
        rcs_toy.write_stats(root, rcs_toy.label_maps())
        src, tgt = rcs_toy.ToySource(root), rcs_toy.ToySource(root)
        ds = UDADataset(src, tgt, rare_class_sampling=rcs_toy.RCS if rcs else None)
        np.random.seed(5)
        items = [ds[i] for i in (0, 7, 13, 100)]
        assert all(sorted(it) == ["img", "target_img"] for it in items)
        if rcs:
            # the target index is the np.random.choice that follows the source draw: replaying the stream finds it
            np.random.seed(5)
            src2, tgt2 = rcs_toy.ToySource(root), rcs_toy.ToySource(root)
            ds2 = UDADataset(src2, tgt2, rare_class_sampling=rcs_toy.RCS)
            again = [ds2[i] for i in (3, 3, 3, 3)]   # idx is ignored under RCS
            assert [a["target_img"]["index"] for a in again] == [it["target_img"]["index"] for it in items]
            assert [a["img"]["index"] for a in again] == [it["img"]["index"] for it in items]
            assert len({it["target_img"]["index"] for it in items}) > 1
        else:
            assert [it["img"]["index"] for it in items] == [0, 7, 1, 100 % rcs_toy.N_FILES]
            assert [it["target_img"]["index"] for it in items] == [0, 7, 1, 100 % rcs_toy.N_FILES]
        batch = pseudo_collate(items[:2])
        assert sorted(batch) == ["img", "target_img"]
        for half in batch.values():
            assert sorted(half) == ["data_samples", "inputs"] and len(half["inputs"]) == len(half["data_samples"]) == 2
        it = DataLoaderIter(ds, batch_size=2, num_workers=0, shuffle=False)
        b = next(it)
        assert sorted(b) == ["img", "target_img"] and len(b["img"]["data_samples"]) == 2


def test_helpers_reproduce_the_fixture(G):
    """From the recorded fp32 teacher logits of iteration 1, the float64 helpers give the recorded pseudo-labels (outside the undecided
    pixels), count (within the band) and - with the recorded masks' classes - the recorded mixed labels and weight sum."""
    k = "it1::"
    thr = float(G["pseudo_threshold"][0])
    low = torch.from_numpy(G[k + "ema_low"]).permute(0, 2, 3, 1)
    ref = D.pseudo_labels(low, (D.SIZE, D.SIZE), thr)
    count, total, band = (int(v) for v in G[k + "count_total_band"])
    assert total == D.BATCH * D.SIZE * D.SIZE and ref["n_band"] == band and abs(ref["count"] - count) <= band
    assert 0.2 < count / total < 0.8
    sub = lambda t: t[:, ::D.SUB, ::D.SUB]
    sure = ~torch.from_numpy(G[k + "unsure_sub"])
    assert torch.equal(sub(~ref["sure_label"]), ~sure) and int((~ref["sure_label"]).sum()) == int(G[k + "n_unsure"][0])
    assert torch.equal(sub(ref["label"])[sure], torch.from_numpy(G[k + "pseudo_label_sub"]).long()[sure])
    lab = synth_label(D.BATCH, D.SIZE, seed=D.SRC_SEED)[:, 0]
    mask_sub = torch.from_numpy(G[k + "mask_sub"]).long()
    chosen = [torch.unique(sub(lab)[b][mask_sub[b] > 0]).tolist() for b in range(D.BATCH)]   # (label blocks are 32 wide: every class shows at stride 8)
    mask = D.class_masks(lab, chosen)
    assert torch.equal(sub(mask), mask_sub) and torch.equal(mask.sum((1, 2)), torch.from_numpy(G[k + "mask_sum"]))
    for b in range(D.BATCH):
        assert 0 < len(chosen[b]) < len(torch.unique(lab[b]))
    img = torch.zeros(D.BATCH, 3, D.SIZE, D.SIZE)
    _, mixed_lbl, mix_weight = D.class_mix(img, img, lab, ref["label"], mask, count, total, D.IGNORE_TOP, D.IGNORE_BOTTOM)
    assert torch.equal(sub(mixed_lbl)[sure], torch.from_numpy(G[k + "mixed_lbl_sub"]).long()[sure])
    assert abs(mix_weight.double().sum().item() - float(G[k + "mix_weight_sum"][0])) <= 1e-6 * float(G[k + "mix_weight_sum"][0])
    assert float(G[k + "sensitivity"].min()) >= 0.1
    # EMA: a = 0.5 at iteration 1, alpha afterwards
    t, s = torch.tensor([1.0, -2.0]), torch.tensor([3.0, 2.0])
    assert torch.equal(D.ema(t, s, 1, D.ALPHA), torch.tensor([2.0, 0.0], dtype=torch.float64))
    assert torch.allclose(D.ema(t, s, 5000, D.ALPHA), 0.999 * t.double() + 0.001 * s.double(), rtol=0, atol=1e-15)


@pytest.mark.parametrize("bad,names", [
    (dict(blur=True), ("blur", "color_jitter_probability")),
    (dict(color_jitter_probability=0.2), ("blur", "color_jitter_probability")),
    (dict(mix="cut_mix"), ("cut_mix",)),
    (dict(decode_head=dict(type="HRDAHead")), ("HRDAHead",)),
])
def test_refused_option_sets_raise(cfg, bad, names):
    m = _small(cfg["model"])
    m.update(bad)
    with pytest.raises(NotImplementedError) as e:
        MODELS.build(m)
    assert all(n in str(e.value) for n in names)


def test_amp_and_data_parallel_are_refused_at_the_first_step(cfg):
    from vfmseg_amd.optim import AmpOptimWrapper, OptimWrapper
    model = MODELS.build(_small(cfg["model"]))

    class _Opt:
        _amp_sync = None

    for ow in (AmpOptimWrapper(_Opt()), OptimWrapper(_Opt(), grad_sync=lambda: None)):
        with pytest.raises(NotImplementedError, match="amp"):
            model.train_step(dict(img=None, target_img=None), ow)
