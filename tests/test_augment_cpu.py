"""Plan mode of the input pipeline (vfmseg_amd/datasets.py, Compose(device=True)) on the CPU: with the same seeds it delivers the host
chain's labels and metainfo, leaves np.random in the host chain's state, and decodes a file once under rare class sampling."""
import numpy as np
import pytest
import torch

import augment_helpers as H
from vfmseg_amd import datasets as D

SEEDS = 32


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("augment_cpu"))
    imgs, labs = H.write_folder(root, 2)
    return root, imgs, labs


def _pair(root, pipeline):
    return D.DATASETS.build(H.folder_cfg(root, pipeline, False)), D.DATASETS.build(H.folder_cfg(root, pipeline, True))


def _check_sample(a, b, src_img):
    ma, mb = a["data_samples"].metainfo, dict(b["data_samples"].metainfo)
    plan = mb.pop("aug_plan")
    assert "aug_plan" not in ma and set(ma) == set(mb)
    for k in ma:
        assert ma[k] == mb[k] and type(ma[k]) is type(mb[k]), (k, ma[k], mb[k])
    assert torch.equal(a["data_samples"].gt_sem_seg.data, b["data_samples"].gt_sem_seg.data)
    assert b["inputs"].dtype == torch.uint8 and np.array_equal(b["inputs"].numpy(), src_img)     # decoded, untouched, HWC, BGR
    assert tuple(plan["crop"][2:]) == tuple(ma["img_shape"]) == tuple(a["inputs"].shape[-2:])
    return plan


def test_plan_mode_equals_host_chain(folder):
    root, imgs, _ = folder
    host, dev = _pair(root, H.train_chain())
    plans = []
    for seed in range(SEEDS):
        np.random.seed(seed)
        a = host[seed % 2]
        sa = np.random.get_state()
        np.random.seed(seed)
        b = dev[seed % 2]
        assert H.same_rng(sa, np.random.get_state()), seed
        plans.append(_check_sample(a, b, imgs[seed % 2]))
        assert plans[-1]["resize"] == (200, 356) and plans[-1]["wide"] is D.convert_is_wide()
    H.assert_coverage(plans)


def test_convert_width_is_what_the_host_chain_computes():
    """PhotoMetricDistortion hands _convert what np.random.uniform returns - a Python float, so a float32 image stays float32 under numpy 1
    and 2 alike.  The probe must say what _convert really does: on draws where the two widths disagree, the host equals exactly one."""
    state = np.random.get_state()
    wide = D.convert_is_wide()
    assert H.same_rng(state, np.random.get_state())       # the probe leaves np.random alone
    x = np.arange(256, dtype=np.uint8)
    for lo, hi, as_alpha in ((0.5, 1.5, True), (-32, 32, False)):
        for v in H.straddling(lo, hi, as_alpha):
            np.random.seed(0)
            drawn = type(np.random.uniform(lo, hi))(v)       # the type the chain passes
            kw = dict(alpha=drawn) if as_alpha else dict(beta=drawn)
            host = D.PhotoMetricDistortion._convert(x, **kw)
            want, other = (H.convert_f64, H.convert_f32) if wide else (H.convert_f32, H.convert_f64)
            assert np.array_equal(host, want(x, **kw)) and not np.array_equal(host, other(x, **kw)), v


def test_plan_mode_label_index_vectors_are_nearest_interpolate():
    for n_in, n_out in ((150, 200), (150, 211), (267, 375), (1052, 1440), (1914, 2560), (64, 128), (267, 100)):
        want = torch.nn.functional.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None, None], size=(1, n_out), mode="nearest")
        assert np.array_equal(D.nearest_index(n_in, n_out), want.flatten().numpy().astype(np.int64)), (n_in, n_out)


def test_plan_mode_with_rare_class_sampling(folder, monkeypatch):
    """Through DGDataset: same samples, same stream, the same number of re-draws - and in plan mode each file is decoded once."""
    from PIL import Image
    root, imgs, _ = folder
    rcs = dict(class_temp=0.01, min_crop_ratio=2.0, min_pixels=600)    # more than 1200 pixels of the class in a 128^2 crop: often missed
    opens = []
    real_open = Image.open
    monkeypatch.setattr(Image, "open", lambda *a, **k: (opens.append(a[0]), real_open(*a, **k))[1])
    draws = {}

    def build(device):
        ds = D.DGDataset(H.folder_cfg(root, H.train_chain(), device), rare_class_sampling=rcs)
        inner, calls = type(ds.source).__getitem__, draws.setdefault(device, [])
        ds.source.__class__ = type("Counted", (type(ds.source),), dict(__getitem__=lambda self, i: (calls.append(i), inner(self, i))[1]))
        return ds

    host, dev = build(False), build(True)
    redrawn = 0
    for seed in range(SEEDS):
        np.random.seed(seed)
        n0, o0 = len(draws[False]), len(opens)
        a = host[0]
        sa, nh, oh = np.random.get_state(), len(draws[False]) - n0, len(opens) - o0
        np.random.seed(seed)
        n0, o0 = len(draws[True]), len(opens)
        b = dev[0]
        nd, od = len(draws[True]) - n0, len(opens) - o0
        assert H.same_rng(sa, np.random.get_state()) and nd == nh, (seed, nh, nd)
        idx = int(b["data_samples"].metainfo["img_path"][-7:-4])
        _check_sample(a, b, imgs[idx])
        assert oh == 2 * nh and od <= 2, (seed, oh, od)     # image + label per pipeline run on the host; once per file in plan mode
        redrawn += nh > 1
    assert redrawn >= 4, redrawn       # the toy statistics make the re-draw loop run


def test_eval_chain_is_expressible(folder):
    root, imgs, labs = folder
    host, dev = _pair(root, H.eval_chain())
    a, b = host[1], dev[1]
    plan = _check_sample(a, b, imgs[1])
    assert plan["resize"] == (200, 356) and plan["crop"] == (0, 0, 200, 356) and plan["flip"] == 0 and "brightness" not in plan
    assert np.array_equal(b["data_samples"].gt_sem_seg.data[0].numpy(), labs[1])      # loaded after the resize: untouched


@pytest.mark.parametrize("direction", ["horizontal", "vertical"])
def test_resize_and_flip_without_a_crop(folder, direction):
    """No crop between the resize and the flip: the whole resized label is gathered, then flipped; the plan's window is the whole image."""
    root, imgs, _ = folder
    chain = [dict(type="LoadImageFromFile"), dict(type="LoadAnnotations"), dict(type="Resize", scale=(375, 211)),
             dict(type="RandomFlip", prob=1.0, direction=direction), dict(type="PackSegInputs")]
    host, dev = _pair(root, chain)
    plan = _check_sample(host[0], dev[0], imgs[0])
    assert plan["crop"] == (0, 0, 211, 375) and plan["flip"] == (1 if direction == "horizontal" else 2)


@pytest.mark.parametrize("chain,name", [
    ([dict(type="LoadImageFromFile"), dict(type="RandomCrop", crop_size=64), dict(type="Resize", scale=(64, 64)), dict(type="PackSegInputs")], "Resize"),
    ([dict(type="LoadImageFromFile"), dict(type="Resize", scale=(64, 64)), dict(type="Resize", scale=(32, 32)), dict(type="PackSegInputs")], "Resize"),
    ([dict(type="LoadImageFromFile"), dict(type="RandomFlip", prob=0.5), dict(type="RandomCrop", crop_size=64), dict(type="PackSegInputs")], "RandomCrop"),
    ([dict(type="LoadImageFromFile"), dict(type="Blur"), dict(type="PackSegInputs")], "Blur"),
])
def test_inexpressible_chain_raises(chain, name):
    class Blur:
        def __call__(self, results):
            return results

    chain = [Blur() if t["type"] == "Blur" else t for t in chain]
    D.Compose(chain)     # the host form takes all of them
    with pytest.raises(ValueError, match=name):
        D.Compose(chain, device=True)


def test_switch(monkeypatch):
    monkeypatch.delenv("VFMSEG_AUG_DEVICE", raising=False)
    assert not D.device_augment_on({}) and not D.device_augment_on(None) and D.device_augment_on(dict(device_augment=True))
    from vfmseg_amd.config import parse_cfg_options      # --cfg-options train_dataloader.device_augment=True
    opts = parse_cfg_options(["train_dataloader.device_augment=True"])
    assert opts in ({"train_dataloader.device_augment": True}, {"train_dataloader": {"device_augment": True}})
    monkeypatch.setenv("VFMSEG_AUG_DEVICE", "0")
    assert not D.device_augment_on(dict(device_augment=True))
    monkeypatch.setenv("VFMSEG_AUG_DEVICE", "1")
    assert D.device_augment_on({})
