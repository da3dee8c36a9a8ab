"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py: the test images (smooth blocks plus noise, as oracle/gen_transform_fixture.py
makes them, with the colour-space corner cases in row 0), toy dataset folders, the float64 bilinear expectation written from the sampling
formula (no code shared with the product), and the coverage assertion over the drawn plans."""
import json
import os

import numpy as np

H0, W0 = 150, 267
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def make_image(s, h=H0, w=W0):
    rng = np.random.RandomState(1000 + s)
    gh, gw = -(-h // 8), -(-w // 8)    # 19 x 34 at 150 x 267
    base = np.kron(rng.randint(0, 256, (gh, gw, 3)), np.ones((8, 8, 1)))[:h, :w]
    img = np.clip(base + rng.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    img[0, 0] = (0, 0, 0)
    img[0, 1] = (255, 255, 255)
    img[0, 2] = (128, 128, 128)      # grey: saturation 0, hue undefined
    img[0, 3] = (0, 0, 255)          # pure red (BGR)
    img[0, 4] = (200, 50, 200)       # the maximum is shared by blue and red
    img[0, 5] = (50, 200, 200)       # ... by green and red
    return img


def make_label(s, h=H0, w=W0):
    rng = np.random.RandomState(5000 + s)
    gh, gw = -(-h // 8), -(-w // 8)
    lab = np.kron(rng.randint(0, 19, (gh, gw)), np.ones((8, 8)))[:h, :w].astype(np.uint8)
    lab[:3] = 255
    return lab


def write_folder(root, n=2, h=H0, w=W0, first=0):
    """n PNG pairs under root/img, root/ann (+ the two rare-class-sampling json files of the reference's converters); returns the arrays."""
    from PIL import Image
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    os.makedirs(os.path.join(root, "ann"), exist_ok=True)
    imgs, labs, stats, swc = [], [], [], {}
    for i in range(n):
        img, lab = make_image(first + i, h, w), make_label(first + i, h, w)
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(os.path.join(root, "img", f"{i:03d}.png"))    # files hold RGB
        Image.fromarray(lab).save(os.path.join(root, "ann", f"{i:03d}.png"))
        imgs.append(img)
        labs.append(lab)
        row = {"file": f"ann/{i:03d}.png"}
        for c in range(19):
            k = int((lab == c).sum())
            if k:
                row[str(c)] = k
                swc.setdefault(str(c), []).append([row["file"], k])
        stats.append(row)
    with open(os.path.join(root, "sample_class_stats.json"), "w") as f:
        json.dump(stats, f)
    with open(os.path.join(root, "samples_with_class.json"), "w") as f:
        json.dump(swc, f)
    return imgs, labs


def train_chain(scale=(356, 200), crop=128, flip_dir="horizontal"):
    p = [dict(type="LoadImageFromFile"), dict(type="LoadAnnotations")]
    if scale is not None:
        p.append(dict(type="Resize", scale=scale))
    p += [dict(type="RandomCrop", crop_size=crop, cat_max_ratio=0.75), dict(type="RandomFlip", prob=0.5, direction=flip_dir),
          dict(type="PhotoMetricDistortion"), dict(type="PackSegInputs")]
    return p


def eval_chain(scale=(356, 200)):
    return [dict(type="LoadImageFromFile"), dict(type="Resize", scale=scale, keep_ratio=True), dict(type="LoadAnnotations"),
            dict(type="PackSegInputs")]


def folder_cfg(root, pipeline, device):
    return dict(type="BaseSegDataset", data_root=root, data_prefix=dict(img_path="img", seg_map_path="ann"), img_suffix=".png",
                seg_map_suffix=".png", pipeline=pipeline, device_augment=device)


def same_rng(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def assert_coverage(plans):
    """Every photometric step on and off, both contrast positions, a negative hue shift, both flip states."""
    for key in ("brightness", "saturation", "hue"):
        assert {bool(p[key][0]) for p in plans} == {True, False}, key
    assert {p["contrast"][0] for p in plans} == {0, 1, 2}
    assert any(p["hue"][0] and p["hue"][1] < 0 for p in plans) and any(p["hue"][0] and p["hue"][1] > 0 for p in plans)
    assert {p["flip"] != 0 for p in plans} == {True, False}


def bilinear_f64(img, oh, ow):
    """Un-rounded float64 bilinear resize at half-pixel centres with edge clamp (cv2.INTER_LINEAR's sampling positions)."""
    h, w = img.shape[:2]
    ys = np.clip((np.arange(oh, dtype=np.float64) + 0.5) * h / oh - 0.5, 0.0, h - 1.0)
    xs = np.clip((np.arange(ow, dtype=np.float64) + 0.5) * w / ow - 0.5, 0.0, w - 1.0)
    y0, x0 = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    f = img.astype(np.float64)
    rows0, rows1 = f[y0], f[y1]
    top = rows0[:, x0] * (1.0 - fx) + rows0[:, x1] * fx
    bot = rows1[:, x0] * (1.0 - fx) + rows1[:, x1] * fx
    return top * (1.0 - fy) + bot * fy


def geometry_plan(resize, box, flip):
    return dict(resize=resize, crop=box, flip=flip, wide=False)


def convert_f32(x, alpha=1.0, beta=0.0):
    """clip(x * alpha + beta).astype(uint8) with every operand and operation in float32 - written out, not left to numpy's promotion."""
    v = x.astype(np.float32) * np.float32(alpha) + np.float32(beta)
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8)


def convert_f64(x, alpha=1.0, beta=0.0):
    """The same in float64."""
    return np.clip(x.astype(np.float64) * np.float64(alpha) + np.float64(beta), 0.0, 255.0).astype(np.uint8)


def straddling(lo, hi, as_alpha, n=4):
    """n parameters of _convert in [lo, hi] for which its float32 and its float64 form disagree on some grey level, because the result lands
    on different sides of an integer in the two widths.  alpha: the first n such of 20000 draws of uniform(lo, hi) (about 1e-3 of the draws
    are).  beta: the float64 neighbours below integers - they round to the integer in float32 (such draws are rare: constructed)."""
    x = np.arange(256, dtype=np.uint8)
    if as_alpha:
        cand = (float(v) for v in np.random.RandomState(0).uniform(lo, hi, 20000))
    else:
        cand = (float(np.nextafter(np.float64(k), -np.inf)) for k in (13, -7, 31, -20, 5, -1))
    out = []
    for v in cand:
        kw = dict(alpha=v) if as_alpha else dict(beta=v)
        if lo <= v <= hi and (convert_f32(x, **kw) != convert_f64(x, **kw)).any():
            out.append(v)
            if len(out) == n:
                break
    assert len(out) == n
    return out


def flipped(a, flip):
    return a if flip == 0 else np.flip(a, 1 if flip == 1 else 0)
