#!/usr/bin/env python
"""Evaluation entry point (tools/test.py:19-145): CONFIG CHECKPOINT [--backbone PTH --work-dir --out DIR --show --show-dir DIR
--wait-time S --cfg-options ... --launcher ... --tta].
Runs the configured test mode (ms_slide_inference / slide) over the config's test_dataloader.dataset when its data_root exists
(test pipeline: LoadImageFromFile, Resize(keep_ratio), LoadAnnotations, PackSegInputs -> SegDataPreProcessor -> predict ->
postprocess to ori_shape), else over synthetic images, and reports mIoU against the labels (mmseg IoUMetric / DGIoUMetric
semantics) and ms/img.  One loop for both (vfmseg_amd.evaluation.evaluate); with --launcher pytorch / WORLD_SIZE > 1
(bash tools/dist_test.sh CONFIG CHECKPOINT GPUS) every rank scores its share and rank 0 prints the summed result."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("checkpoint", nargs="?")
    ap.add_argument("--backbone", help="backbone .pth merged under 'backbone.' (LoadBackboneHook semantics)")
    ap.add_argument("--work-dir")
    ap.add_argument("--cfg-options", nargs="+")
    ap.add_argument("--out", type=str, help="directory for the predicted label maps (PNG, one per image; mmseg IoUMetric output_dir)")
    ap.add_argument("--show", action="store_true", help="accepted for CLI parity; there is no display here: use --show-dir")
    ap.add_argument("--show-dir", help="directory for colour-painted predictions (Cityscapes palette)")
    ap.add_argument("--wait-time", type=float, default=2)
    ap.add_argument("--launcher", choices=["none", "pytorch", "slurm", "mpi"], default="none")
    ap.add_argument("--tta", action="store_true", help="test-time augmentation from the config's tta_pipeline (scales x flip, mean of softmax)")
    ap.add_argument("--local_rank", "--local-rank", type=int, default=0)
    ap.add_argument("--images", type=int, default=None,
                    help="evaluate only the first N samples (default: the whole test set on real data, 4 synthetic images otherwise)")
    ap.add_argument("--size", type=int, nargs=2, default=[1024, 1024])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "bf16x3", "fp16"])
    ap.add_argument("--data", choices=["auto", "synthetic", "real"], default="auto")
    a = ap.parse_args()
    if "LOCAL_RANK" not in os.environ:
        os.environ["LOCAL_RANK"] = str(a.local_rank)
    import numpy as np
    import torch
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd.config import Config, parse_cfg_options
    from vfmseg_amd.registry import METRICS
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.synth import synth_like
    from vfmseg_amd import lib as hiplib, parallel
    from vfmseg_amd.evaluation import dataset_size, evaluate, synthetic_set
    set_compute_dtype(a.dtype)
    # several ranks (--launcher pytorch / WORLD_SIZE > 1, tools/dist_test.sh): rank r scores the samples r, r + world, ...; one
    # all-reduce sums the confusion counts and only rank 0 prints
    rank, world, local = parallel.init_from_env() if (a.launcher == "pytorch" or int(os.environ.get("WORLD_SIZE", "1")) > 1) else (0, 1, int(os.environ["LOCAL_RANK"]))
    cfg = Config.fromfile(a.config)
    cfg.merge_from_dict(parse_cfg_options(a.cfg_options))
    model = MODELS.build(cfg["model"])
    sd = synth_like(model.state_dict())
    if a.checkpoint:
        ck = torch.load(a.checkpoint, map_location="cpu")   # (weights-only: Runner checkpoints keep their RNG states as tensors / numbers)
        sd.update(ck.get("state_dict", ck))
    if a.backbone:
        sd.update({"backbone." + k: v for k, v in torch.load(a.backbone, map_location="cpu").items()})
    model.load_state_dict(sd, strict=False)
    dev_index = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    hiplib.set_device_index(dev_index)
    model = model.cuda().eval()
    tta = None
    if a.tta:   # tools/test.py:131-134 swaps in cfg.tta_pipeline / cfg.tta_model (mmseg SegTTAModel: mean of the views' softmax)
        if "tta_pipeline" not in cfg:
            raise SystemExit("--tta: the config defines no tta_pipeline (the reference raises on cfg.tta_pipeline too)")
        from vfmseg_amd.segmentors import tta_views
        tta = tta_views(cfg["tta_pipeline"])
    for d in (a.out, a.show_dir):
        if d:
            os.makedirs(d, exist_ok=True)

    class TTAModel:
        """--tta needs the logits of every view (mean of softmax): predict_tta, then the counts process() takes (metrics.confusion)."""
        training = False
        data_preprocessor = model.data_preprocessor

        def eval(self):
            return self

        def train(self, mode=True):
            return self

        def parameters(self):
            return model.parameters()

        def predict_labels(self, inputs, samples, hist=None, num_classes=None, ignore_index=255):
            from vfmseg_amd.metrics import confusion
            from vfmseg_amd.segmentors import predict_tta
            out = predict_tta(model, inputs, samples, tta)
            for o in out:
                if hist is not None and hasattr(o, "gt_sem_seg"):
                    confusion(o.pred_sem_seg.data.squeeze(), o.gt_sem_seg.data.squeeze(), num_classes, ignore_index, out=hist)
            return out

    def dump(out, idx):
        if not (a.out or a.show_dir):
            return
        from PIL import Image
        from vfmseg_amd.datasets import CITYSCAPES_PALETTE
        for j, o in enumerate(out):
            pred = o.pred_sem_seg.data.squeeze().to(torch.uint8).cpu().numpy()
            name = os.path.splitext(os.path.basename(str((o.metainfo or {}).get("img_path") or (o.metainfo or {}).get("seg_map_path") or f"{idx}_{j}")))[0]
            if a.out:
                Image.fromarray(pred).save(os.path.join(a.out, name + ".png"))
            if a.show_dir:
                pal = np.asarray(CITYSCAPES_PALETTE, dtype=np.uint8)
                Image.fromarray(pal[np.minimum(pred, len(pal) - 1)]).save(os.path.join(a.show_dir, name + ".png"))
    ev = cfg.get("test_evaluator") or cfg.get("val_evaluator") or dict(type="IoUMetric")
    ev = dict(ev[0] if isinstance(ev, (list, tuple)) else ev)
    metric = METRICS.build(ev)      # DGIoUMetric (rein/dg_metrics.py) with the config's dataset_keys, or mmseg's IoUMetric
    keys = list(getattr(metric, "dataset_keys", [])) or ["synthetic"]
    dl = dict(cfg.get("test_dataloader") or cfg.get("val_dataloader") or {})
    ds_cfg = dl.get("dataset")
    root = (ds_cfg.get("source", ds_cfg) if isinstance(ds_cfg, dict) else {}).get("data_root") if ds_cfg else None
    real = a.data == "real" or (a.data == "auto" and root and os.path.isdir(root))
    if real:
        from vfmseg_amd.datasets import DataLoaderIter, device_augment_on
        data = DataLoaderIter(ds_cfg, 1, dl.get("num_workers", 0), shuffle=False, rank=rank, world=world, infinite=False,
                              device_augment=device_augment_on(dl))   # test_dataloader.device_augment / VFMSEG_AUG_DEVICE
        if hasattr(data.dataset, "metainfo"):
            metric.dataset_meta = dict(classes=data.dataset.metainfo["classes"])
        limit = a.images      # only when --images was given: the reference evaluates the whole test_dataloader
    else:
        data, limit = synthetic_set(a.images or 4, tuple(a.size), keys), None
    res, info = evaluate(model if tta is None else TTAModel(), data, metric, rank, world, limit=limit, on_output=dump)
    res = dict(res)
    res["ms_per_img"] = 1e3 * info["seconds"] / max(info["samples"], 1)     # the ranks' summed prediction time over the summed samples
    res["evaluated_samples"] = info["samples"]
    if real:
        res["dataset_size"] = dataset_size(data)
    if rank == 0:
        print(res)


if __name__ == "__main__":
    main()
