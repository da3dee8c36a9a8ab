#!/usr/bin/env python
"""Timing of the training input pipeline in its two forms (run in a fresh process under a time limit, e.g.
`timeout -k 10 500 python tools/augment_time.py`), at the reference's GTA geometry (configs/_base_/datasets/gta_1024x1024.py): a 1052 x 1914
image resized to 1440 x 2560, a 1024^2 crop, flip, photometric distortion.  The images are synthetic PNGs written to a temporary folder.

1. The host chain (Resize -> RandomCrop -> RandomFlip -> PhotoMetricDistortion -> PackSegInputs on decoded arrays), ms per sample, one thread.
2. Plan mode of the same chain (datasets.Compose(device=True)), ms per sample.
3. vfm_augment_u8, us per sample and bytes/s (the fp32 output written plus the source window read), device events around `--reps` launches,
   next to the host's enqueue time per call (when the two agree the figure is the launch rate, not the kernel); sources and outputs rotate
   through a ring larger than the 256-MB last-level cache.
4. DataLoaderIter (num_workers=0) -> SegDataPreProcessor, samples/s, in both modes (decode included).

The forms alternate over `--rounds` rounds after one dropped round; median, min, max and every round are logged as JSON lines."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from segformer_time import _spread, _time  # noqa: E402

HS, WS, RESIZE, CROP = 1052, 1914, (1440, 2560), 1024
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
COPY_RATE = 6.29e12    # bytes/s of a device-to-device copy on this chip (MI355X_MICROARCH.md)


def write_folder(root, n):
    from PIL import Image
    os.makedirs(os.path.join(root, "img"))
    os.makedirs(os.path.join(root, "ann"))
    for i in range(n):
        rng = np.random.RandomState(i)
        gh, gw = -(-HS // 32), -(-WS // 32)
        img = np.clip(np.kron(rng.randint(0, 256, (gh, gw, 3)), np.ones((32, 32, 1)))[:HS, :WS] + rng.randint(-20, 21, (HS, WS, 3)), 0, 255)
        lab = np.kron(rng.randint(0, 19, (gh, gw)), np.ones((32, 32)))[:HS, :WS]
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(root, "img", f"{i}.png"))
        Image.fromarray(lab.astype(np.uint8)).save(os.path.join(root, "ann", f"{i}.png"))


def chain():
    return [dict(type="LoadImageFromFile"), dict(type="LoadAnnotations"), dict(type="Resize", scale=(RESIZE[1], RESIZE[0])),
            dict(type="RandomCrop", crop_size=CROP, cat_max_ratio=0.75), dict(type="RandomFlip", prob=0.5), dict(type="PhotoMetricDistortion"),
            dict(type="PackSegInputs")]


def folder_cfg(root):
    return dict(type="BaseSegDataset", data_root=root, data_prefix=dict(img_path="img", seg_map_path="ann"), img_suffix=".png", seg_map_suffix=".png",
                pipeline=chain())


def host_times(root, samples, rounds):
    """ms per sample of the chain after the decode, host form and plan mode alternating, one thread."""
    from vfmseg_amd.datasets import DATASETS
    ds = DATASETS.build(folder_cfg(root))
    loads, rest = ds.pipeline.transforms[:2], ds.pipeline.transforms[2:]
    decoded = []
    t0 = time.perf_counter()
    for i in range(len(ds)):
        item = dict(ds.data_list[i], seg_fields=[])
        decoded.append(loads[1](loads[0](item)))
    decode_ms = 1e3 * (time.perf_counter() - t0) / len(ds)
    vals = {"host_chain_ms": [], "plan_mode_ms": []}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    for rnd in range(rounds + 1):
        for key in vals:
            np.random.seed(rnd)
            t0 = time.perf_counter()
            for k in range(samples):
                res = dict(decoded[k % len(decoded)], seg_fields=["gt_seg_map"])
                if key == "plan_mode_ms":
                    res = loads[0].plan(dict(res, _decoded={("img", res["img_path"]): res["img"]}))
                for t in rest:
                    res = t.plan(res) if key == "plan_mode_ms" else t(res)
            if rnd:
                vals[key].append(1e3 * (time.perf_counter() - t0) / samples)
    torch.set_num_threads(threads)
    rec = dict(what=f"transform chain after the decode, ms per sample, one thread (the plan-mode figure also holds LoadImageFromFile.plan on a "
                    f"cache hit, which opens the plan; the host figure starts after the loads), {samples} samples per round ({HS} x {WS} -> {RESIZE[0]} x {RESIZE[1]}, "
                    f"{CROP}^2 crop, cat_max_ratio 0.75, flip, photometric distortion)", decode_ms_per_sample=round(decode_ms, 1))
    rec.update({k: _spread(v) for k, v in vals.items()})
    print(json.dumps(rec), flush=True)


def kernel_time(reps, rounds):
    from vfmseg_amd import ops
    g = torch.Generator().manual_seed(1)
    srcs = [torch.randint(0, 256, (HS, WS, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(8)]
    outs = [torch.empty(3, CROP, CROP, device="cuda") for _ in range(24)]    # 24 x 12.6 MB: beyond the last-level cache
    plans = {"geometry_only": dict(resize=RESIZE, crop=(208, 768, CROP, CROP), flip=1, wide=False),
             "all_steps": dict(resize=RESIZE, crop=(208, 768, CROP, CROP), flip=1, wide=False, brightness=(1, 12.5), contrast=(2, 1.2),
                               saturation=(1, 0.8), hue=(1, -9))}
    it = [0]

    def run(plan):
        def f():
            it[0] += 1
            ops.augment_u8(srcs[it[0] % len(srcs)], plan, outs[it[0] % len(outs)], MEAN, STD, True, 0.0)
        return f

    def enqueue_us(fn):
        """host time of one call (Python binding + launch), the queue drained before and after: a floor for the device-event figure"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        return 1e6 * t / reps

    vals = {k: [] for k in plans}
    host = {k: [] for k in plans}
    for rnd in range(rounds + 1):
        for k, p in plans.items():
            t, th = _time(run(p), reps), enqueue_us(run(p))
            if rnd:
                vals[k].append(t)
                host[k].append(th)
    window = int(CROP * HS / RESIZE[0] + 2) * int(CROP * WS / RESIZE[1] + 2) * 3
    nbytes = 3 * CROP * CROP * 4 + window
    rec = dict(what="vfm_augment_u8, us per sample (one launch)", bytes_per_sample=nbytes, bytes_written=3 * CROP * CROP * 4, source_window_bytes=window,
               copy_rate_bytes_per_s=COPY_RATE)
    for k, v in vals.items():
        rec[k + "_us"] = _spread(v)
        rec[k + "_host_enqueue_us"] = _spread(host[k])
        rec[k + "_bytes_per_s"] = round(nbytes / (rec[k + "_us"]["median"] * 1e-6), -9)
        rec[k + "_share_of_copy_rate"] = round(rec[k + "_bytes_per_s"] / COPY_RATE, 3)
    print(json.dumps(rec), flush=True)


def loader_rates(root, batches, rounds):
    from vfmseg_amd.datasets import DataLoaderIter
    from vfmseg_amd.segmentors import SegDataPreProcessor
    pre = SegDataPreProcessor(mean=MEAN, std=STD, size=(CROP, CROP), pad_val=0, seg_pad_val=255, bgr_to_rgb=True)
    vals = {"host": [], "device": []}
    for rnd in range(rounds + 1):
        for key in vals:
            np.random.seed(rnd)
            loader = DataLoaderIter(folder_cfg(root), batch_size=2, num_workers=0, seed=rnd, device_augment=key == "device")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batches):
                pre(next(loader), True)
            torch.cuda.synchronize()
            if rnd:
                vals[key].append(2 * batches / (time.perf_counter() - t0))
    rec = dict(what=f"DataLoaderIter(num_workers=0) -> SegDataPreProcessor, samples/s (PNG decode included), {batches} batches of 2 per round")
    rec.update({"samples_per_s_" + k: _spread(v) for k, v in vals.items()})
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--samples", type=int, default=6, help="samples per round of the host timings")
    ap.add_argument("--batches", type=int, default=3, help="batches of two per round of the loader timing")
    ap.add_argument("--rounds", type=int, default=3, help="reported rounds per figure (after one dropped round)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_time.py measures on the GPU; none found")
    import vfmseg_amd  # noqa: F401
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          reps=a.reps, numpy=np.__version__, torch_threads=torch.get_num_threads())), flush=True)
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, 2)
        host_times(root, a.samples, a.rounds)
        kernel_time(a.reps, a.rounds)
        loader_rates(root, a.batches, a.rounds)


if __name__ == "__main__":
    main()
