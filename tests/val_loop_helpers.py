"""Shared by tests/test_val_loop_gpu.py and its worker (tests/val_loop_worker.py): a depth-2 DINOv2 + LoRA + LinearHead segmentor at
512^2, a folder tree of three 470 x 600 images (keep-ratio resize to 401 x 512, padded to 512 x 512 by the data preprocessor, so
that predictions come back through padding removal and a resize to ori_shape), and the configs built from them."""
import copy
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 470, 600
KEYS = ["citys"]


def model_cfg(dropout=True):
    from vfmseg_amd import presets
    cfg = presets.dinov2_linear(depth=2)
    cfg["backbone"]["backbone"]["out_indices"] = [0, 1, 1, 1]
    cfg["data_preprocessor"] = dict(cfg["data_preprocessor"], test_cfg=dict(size_divisor=512))
    if not dropout:      # two ranks draw other masks than one process with the global batch
        cfg["backbone"]["Lora_config"]["lora_dropout"] = 0.0
        cfg["decode_head"]["dropout_ratio"] = 0.0
    return cfg


def tree(root, n=3):
    """n images citys_<i>.png with labels (rows of 255 on top), Cityscapes-shaped"""
    from PIL import Image
    rng = np.random.RandomState(0)
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "labels"))
    for i in range(n):
        base = rng.randint(0, 256, (H // 50 + 1, W // 50 + 1, 3), dtype=np.uint8)
        img = np.kron(base, np.ones((50, 50, 1), np.uint8))[:H, :W]
        lab = rng.randint(0, 19, (H // 100 + 1, W // 100 + 1), dtype=np.uint8)
        lab = np.kron(lab, np.ones((100, 100), np.uint8))[:H, :W].copy()
        lab[:40] = 255
        Image.fromarray(img).save(os.path.join(root, "images", f"citys_{i}.png"))
        Image.fromarray(lab).save(os.path.join(root, "labels", f"citys_{i}_labelTrainIds.png"))
    return root


def test_dataset(root):
    pipe = [dict(type="LoadImageFromFile"), dict(type="Resize", scale=(512, 512), keep_ratio=True), dict(type="LoadAnnotations"),
            dict(type="PackSegInputs")]
    return dict(type="CityscapesDataset", data_root=root, data_prefix=dict(img_path="images", seg_map_path="labels"), img_suffix=".png",
                seg_map_suffix="_labelTrainIds.png", pipeline=pipe)


def evaluator():
    return dict(type="DGIoUMetric", iou_metrics=["mIoU"], dataset_keys=list(KEYS))


def build_model(checkpoint=None, dropout=True):
    """the model tools/test.py builds: synthetic weights, then the checkpoint's"""
    import torch
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.synth import synth_like
    model = MODELS.build(copy.deepcopy(model_cfg(dropout)))
    sd = synth_like(model.state_dict())
    if checkpoint:
        sd.update(torch.load(checkpoint, map_location="cpu")["state_dict"])
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def train_cfg(work_dir, max_iters, val_interval=None, batch_size=2, save_best=None, dropout=True, val_images=2):
    from vfmseg_amd import presets
    oc = presets.optim_cfg()
    tc = dict(type="IterBasedTrainLoop", max_iters=max_iters)
    if val_interval:
        tc["val_interval"] = val_interval
    if not dropout:
        # the two-rank comparison: eps 1 makes AdamW's first updates smooth in the gradient (at 1e-8 they are sign-like and turn the
        # last-bit differences between the worlds' fp32 sums into +-lr steps of the parameters)
        oc["optim_wrapper"]["optimizer"]["eps"] = 1.0
    cfg = dict(model=model_cfg(dropout), optim_wrapper=oc["optim_wrapper"], param_scheduler=oc["param_scheduler"], randomness=dict(seed=0),
               work_dir=work_dir, train_cfg=tc, train_dataloader=dict(batch_size=batch_size), val_cfg=dict(type="ValLoop", synthetic_images=val_images),
               val_evaluator=[evaluator()], default_hooks=dict(checkpoint=dict(type="CheckpointHook", by_epoch=False, interval=2)))
    if save_best:
        cfg["default_hooks"]["checkpoint"]["save_best"] = save_best
    return cfg


def write_config(path, root):
    """a config file for tools/test.py"""
    with open(path, "w") as f:
        f.write(f"model = {model_cfg()!r}\ntest_dataloader = dict(batch_size=1, num_workers=0, dataset={test_dataset(root)!r})\n"
                f"test_evaluator = {evaluator()!r}\n")
    return path


def records(work_dir):
    return [json.loads(l) for l in open(os.path.join(work_dir, "scalars_rank0.jsonl"))]
