"""vfm_augment_u8 (csrc/augment.hip) and the device form of the training input pipeline: the resize against float64 and against the host
chain, the whole chain bit for bit against ops.preprocess_u8 of the host chain's crop, and the model-level wiring
(DataLoaderIter -> SegDataPreProcessor) with the switch on and off."""
import numpy as np
import pytest
import torch

import augment_helpers as H

pytestmark = pytest.mark.gpu

RESIZE = (211, 375)           # not dyadic
BOXES = ((0, 0, 128, 128), (211 - 128, 375 - 128, 128, 128), (40, 100, 128, 128))     # top left, touching bottom right, interior


def _augment(img, plan, size, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), swap=False, pad_val=0.0):
    from vfmseg_amd import ops
    out = torch.empty(3, size[0], size[1], dtype=torch.float32, device="cuda")
    ops.augment_u8(torch.from_numpy(np.ascontiguousarray(img)).cuda(), plan, out, mean, std, swap, pad_val)
    return out


@pytest.fixture(scope="module")
def images():
    return [H.make_image(s) for s in range(24)]


def test_resize_against_float64(images):
    """Distortion off, mean 0, std 1, no swap: every output is an integer within 0.5 + 2e-2 of the un-rounded float64 bilinear value
    (float32 source coordinates err by at most about 5e-5 pixel at this width, times a gradient of at most 255 per pixel)."""
    worst = 0.0
    for img in images:
        want = H.bilinear_f64(img, *RESIZE)
        for box in BOXES:
            for flip in (0, 1, 2):
                got = _augment(img, H.geometry_plan(RESIZE, box, flip), (128, 128)).cpu().numpy().transpose(1, 2, 0).astype(np.float64)
                ref = H.flipped(want[box[0]:box[0] + 128, box[1]:box[1] + 128], flip)
                assert np.array_equal(got, np.rint(got)) and got.min() >= 0 and got.max() <= 255
                err = np.abs(got - ref).max()
                assert err <= 0.5 + 2e-2, (box, flip, err)
                worst = max(worst, err)
    print("largest distance from the float64 value", worst)


def test_resize_against_host_chain(images):
    """Within one grey level of datasets._resize + crop + flip everywhere; unequal at no more than 1e-3 of the values (a correctly
    rounded float64 resize differs from the host at 1.2e-4 of them: room for a correct kernel, none for a wrong tap)."""
    from vfmseg_amd.datasets import _resize
    unequal = total = 0
    for img in images:
        host = _resize(img, RESIZE, "bilinear").astype(np.int32)
        for box in BOXES:
            for flip in (0, 1, 2):
                got = _augment(img, H.geometry_plan(RESIZE, box, flip), (128, 128)).cpu().numpy().transpose(1, 2, 0).astype(np.int32)
                d = np.abs(got - H.flipped(host[box[0]:box[0] + 128, box[1]:box[1] + 128], flip))
                assert d.max() <= 1, (box, flip, d.max())
                unequal += int((d != 0).sum())
                total += d.size
    print("unequal share", unequal / total)
    assert unequal / total <= 1e-3, unequal / total


# dyadic weights: every stage is exactly computable.  (source h, w), Resize scale (w, h), crop_size, flip direction, preprocessor size
EXACT = {"no_resize": ((150, 267), None, 128, "horizontal", (128, 128)),
         "x4_3": ((150, 267), (356, 200), 128, "vertical", (128, 128)),
         "x2_padded": ((64, 96), (192, 128), (160, 144), "horizontal", (160, 160))}     # resized height 128 < crop height 160; width padded 144 -> 160


@pytest.mark.parametrize("case", sorted(EXACT))
def test_whole_chain_bit_exact(case, tmp_path):
    """32 seeds: the kernel output equals ops.preprocess_u8 of the host chain's crop at the same seed, bit for bit; padding is pad_val;
    the label is the host's."""
    from vfmseg_amd import ops
    from vfmseg_amd.datasets import DATASETS
    (h, w), scale, crop, direction, size = EXACT[case]
    imgs, _ = H.write_folder(str(tmp_path), 2, h, w)
    chain = H.train_chain(scale, crop, direction)
    host, dev = DATASETS.build(H.folder_cfg(str(tmp_path), chain, False)), DATASETS.build(H.folder_cfg(str(tmp_path), chain, True))
    pad_val, plans = -3.25, []
    for seed in range(32):
        np.random.seed(seed)
        a = host[seed % 2]
        np.random.seed(seed)
        b = dev[seed % 2]
        plan = b["data_samples"].metainfo["aug_plan"]
        plans.append(plan)
        want = torch.empty(3, *size, dtype=torch.float32, device="cuda")
        ops.preprocess_u8(a["inputs"].cuda().contiguous(), want, H.MEAN, H.STD, True, pad_val)
        got = _augment(b["inputs"].numpy(), plan, size, H.MEAN, H.STD, True, pad_val)
        assert torch.equal(got, want), (seed, plan, int((got != want).sum()), float((got - want).abs().max()))
        ch, cw = a["inputs"].shape[-2:]
        assert (ch, cw) == tuple(plan["crop"][2:])
        assert bool((got[:, ch:] == pad_val).all()) and bool((got[:, :, cw:] == pad_val).all())
        assert torch.equal(a["data_samples"].gt_sem_seg.data, b["data_samples"].gt_sem_seg.data)
    if case == "x2_padded":
        assert (ch, cw) == (128, 144)
    H.assert_coverage(plans)


def _host_photometric(img, plan, convert):
    """PhotoMetricDistortion.__call__ with the plan's parameters and `convert` in the place of _convert."""
    from vfmseg_amd.datasets import bgr2hsv_u8, hsv2bgr_u8
    if plan.get("brightness", (0,))[0]:
        img = convert(img, beta=plan["brightness"][1])
    if plan.get("contrast", (0,))[0] == 1:
        img = convert(img, alpha=plan["contrast"][1])
    if plan.get("saturation", (0,))[0]:
        hsv = bgr2hsv_u8(img)
        hsv[..., 1] = convert(hsv[..., 1], alpha=plan["saturation"][1])
        img = hsv2bgr_u8(hsv)
    if plan.get("contrast", (0,))[0] == 2:
        img = convert(img, alpha=plan["contrast"][1])
    return img


@pytest.mark.parametrize("step", ["brightness", "contrast_early", "contrast_late", "saturation"])
def test_convert_in_both_widths(step):
    """_convert parameters at which the float32 and the float64 form land on different sides of an integer (found by search over the grey
    levels, augment_helpers.straddling): the kernel follows plan["wide"] - float32 is what the host chain computes with the Python float
    np.random.uniform returns, and there the real _convert is the expectation; float64 is the branch for a numpy that would widen."""
    from vfmseg_amd.datasets import PhotoMetricDistortion, convert_is_wide
    assert not convert_is_wide()
    img = H.make_image(7, 64, 256)
    img[1] = np.arange(256, dtype=np.uint8)[:, None]       # every grey level, so that every straddling level is hit
    img[2, :, 1] = np.arange(256, dtype=np.uint8)           # ... and saturated colours of every value
    img[2, :, 0], img[2, :, 2] = 0, 255
    vals = H.straddling(-32, 32, False) if step == "brightness" else H.straddling(0.5, 1.5, True)
    for v in vals:
        base = dict(resize=None, crop=(0, 0, 64, 256), flip=0)
        plan = dict(base, **{"brightness": dict(brightness=(1, v)), "contrast_early": dict(contrast=(1, v)), "contrast_late": dict(contrast=(2, v)),
                             "saturation": dict(saturation=(1, v))}[step])
        want32 = _host_photometric(img, plan, PhotoMetricDistortion._convert)       # the host's own
        assert np.array_equal(want32, _host_photometric(img, plan, H.convert_f32))
        want64 = _host_photometric(img, plan, H.convert_f64)
        assert not np.array_equal(want32, want64)       # the case separates the widths
        for wide, want in ((False, want32), (True, want64)):
            got = _augment(img, dict(plan, wide=wide), (64, 256)).cpu().numpy().transpose(1, 2, 0)
            assert np.array_equal(got, want.astype(np.float32)), (step, v, wide, int((got != want).sum()))


def test_unaligned_output_takes_the_scalar_stores():
    """An output whose width is no multiple of four: same values as the vectorised form on the common part."""
    img = H.make_image(3)
    plan = dict(H.geometry_plan((200, 356), (7, 11, 120, 126), 1), brightness=(1, -11.5), contrast=(2, 1.25), saturation=(1, 0.75), hue=(1, -7))
    a, b = _augment(img, plan, (121, 127), H.MEAN, H.STD, True, 1.5), _augment(img, plan, (124, 128), H.MEAN, H.STD, True, 1.5)
    assert torch.equal(a[:, :120, :126], b[:, :120, :126]) and bool((a[:, 120:] == 1.5).all()) and bool((a[:, :, 126:] == 1.5).all())


@pytest.mark.parametrize("plan", [dict(resize=(200, 356), crop=(100, 0, 128, 128)), dict(resize=(200, 356), crop=(0, 300, 128, 128)),
                                  dict(resize=None, crop=(0, 0, 151, 128)), dict(resize=(200, 356), crop=(-1, 0, 64, 64)),
                                  dict(resize=(200, 356), crop=(0, 0, 129, 128))])
def test_box_outside_the_resize_target_is_refused(plan):
    """VFM_E_SHAPE (-2) from the C entry, before any launch: the output keeps its fill."""
    from vfmseg_amd import lib as L, ops
    out = torch.full((3, 128, 128), 7.0, device="cuda")
    with pytest.raises(L.HipError, match=r"\(-2\)"):
        ops.augment_u8(torch.from_numpy(H.make_image(0)).cuda(), plan, out, H.MEAN, H.STD, True, 0.0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("augment_gpu"))
    H.write_folder(root, 4)
    return root


def _pre():
    from vfmseg_amd.segmentors import SegDataPreProcessor
    return SegDataPreProcessor(mean=H.MEAN, std=H.STD, size=(128, 128), pad_val=0, seg_pad_val=255, bgr_to_rgb=True)


def _same_batch(a, b):
    assert torch.equal(a["inputs"], b["inputs"]) and len(a["data_samples"]) == len(b["data_samples"])
    for sa, sb in zip(a["data_samples"], b["data_samples"]):
        assert torch.equal(sa.gt_sem_seg.data, sb.gt_sem_seg.data)
        assert sa.metainfo == sb.metainfo, (sa.metainfo, sb.metainfo)


def _batches(dataset_cfg, device, n=3):
    from vfmseg_amd.datasets import DataLoaderIter
    np.random.seed(11)
    loader = DataLoaderIter(dataset_cfg, batch_size=2, num_workers=0, seed=5, device_augment=device)
    pre = _pre()
    out = []
    for _ in range(n):
        batch = next(loader)
        halves = batch if "inputs" in batch else None
        out.append(pre(batch, True) if halves is not None else {k: pre(v, True) for k, v in batch.items()})
    return out, np.random.get_state()


def test_loader_and_preprocessor_on_and_off(folder, monkeypatch):
    monkeypatch.delenv("VFMSEG_AUG_DEVICE", raising=False)
    cfg = H.folder_cfg(folder, H.train_chain(), False)
    (off, s_off), (on, s_on) = _batches(cfg, False), _batches(cfg, True)
    assert H.same_rng(s_off, s_on)
    for a, b in zip(off, on):
        _same_batch(a, b)
        assert tuple(b["inputs"].shape) == (2, 3, 128, 128) and "aug_plan" not in b["data_samples"][0].metainfo


def test_uda_pairs_on_and_off(folder, monkeypatch):
    monkeypatch.delenv("VFMSEG_AUG_DEVICE", raising=False)
    one = H.folder_cfg(folder, H.train_chain(), False)
    cfg = dict(type="UDADataset", source=one, target=one)
    (off, s_off), (on, s_on) = _batches(cfg, False, n=2), _batches(cfg, True, n=2)
    assert H.same_rng(s_off, s_on)
    for a, b in zip(off, on):
        for half in ("img", "target_img"):
            _same_batch(a[half], b[half])


def test_validation_sample_through_the_test_chain(folder):
    from vfmseg_amd.datasets import DATASETS
    pre = _pre()
    host, dev = DATASETS.build(H.folder_cfg(folder, H.eval_chain(), False)), DATASETS.build(H.folder_cfg(folder, H.eval_chain(), True))
    for i in (0, 3):
        a, b = host[i], dev[i]
        da = pre(dict(inputs=[a["inputs"]], data_samples=[a["data_samples"]]), False)
        db = pre(dict(inputs=[b["inputs"]], data_samples=[b["data_samples"]]), False)
        _same_batch(da, db)
        m = db["data_samples"][0].metainfo
        assert m["ori_shape"] == (150, 267) and m["scale_factor"] == (356 / 267, 200 / 150) and m["img_shape"] == (200, 356)
        assert tuple(db["inputs"].shape) == (1, 3, 200, 356)
