"""Segmentors on the HIP path.  MsVFMEncoderDecoder mirrors rein/models/segmentors/Ms_VFM_encoder_decoder.py:62-474
(multi-scale training: LR pass + HR crop, two heads; coarse-to-fine gated sliding inference); EncoderDecoder /
LoraBackboneEncoderDecoder mirror the mmseg base class slice the reference configs use (SURVEY App. D,
rein/models/segmentors/Lora_encoder_decoder.py:12-44)."""
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .heads import FeatPack
from .precision import compute_dtype
from .registry import MODELS


class PixelData:
    def __init__(self, data):
        self.data = data


class SegDataSample:
    """Minimal stand-in for mmseg.structures.SegDataSample: `.gt_sem_seg.data` [1,H,W] int64 and `.metainfo`."""

    def __init__(self, gt_sem_seg=None, metainfo=None):
        if gt_sem_seg is not None:
            self.gt_sem_seg = PixelData(gt_sem_seg)
        self.metainfo = metainfo or {}

    def set_metainfo(self, d):
        self.metainfo.update(d)


class CfgDict(dict):
    """dict with attribute access (mmengine ConfigDict subset used by the segmentors)."""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = CfgDict(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


@MODELS.register_module()
class SegDataPreProcessor(nn.Module):
    """mmseg SegDataPreProcessor (1.2.2 semantics, restated): decoded uint8 CHW images are channel-swapped (bgr_to_rgb),
    normalised and padded right/bottom to `size` with pad_val by one HIP kernel per sample (vfm_preprocess_u8), labels are
    padded with seg_pad_val, and img_shape / pad_shape / padding_size land in the sample's metainfo (stack_batch).
    Float inputs are taken as already-normalised images (the synthetic benchmark path) and only stacked.  A sample of the device pipeline
    (metainfo["aug_plan"], datasets.Compose(device=True)) is a decoded uint8 HWC image: vfm_augment_u8 runs the training chain on it first."""

    def __init__(self, mean=None, std=None, size=None, size_divisor=None, pad_val=0, seg_pad_val=255, bgr_to_rgb=False,
                 rgb_to_bgr=False, batch_augments=None, test_cfg=None):
        super().__init__()
        assert not (bgr_to_rgb and rgb_to_bgr)
        self.size, self.size_divisor, self.pad_val, self.seg_pad_val = size, size_divisor, pad_val, seg_pad_val
        self.channel_swap = bool(bgr_to_rgb or rgb_to_bgr)
        self.test_cfg = test_cfg
        self.mean_l = list(mean) if mean is not None else [0.0, 0.0, 0.0]
        self.std_l = list(std) if std is not None else [1.0, 1.0, 1.0]
        self.register_buffer("mean", torch.tensor(self.mean_l).view(-1, 1, 1), False)
        self.register_buffer("std", torch.tensor(self.std_l).view(-1, 1, 1), False)

    def _target(self, shapes, training):
        h, w = max(s[0] for s in shapes), max(s[1] for s in shapes)
        if training and self.size is not None:
            h, w = max(h, self.size[-2]), max(w, self.size[-1])
        div = self.size_divisor if training else (self.test_cfg or {}).get("size_divisor") if self.test_cfg else None
        if div:
            h, w = (h + div - 1) // div * div, (w + div - 1) // div * div
        return h, w

    def forward(self, data, training=False):
        inputs, samples = data["inputs"], data.get("data_samples")
        if torch.is_tensor(inputs) and inputs.dtype == torch.float32:
            return dict(inputs=inputs.cuda(non_blocking=True).contiguous(), data_samples=samples)
        imgs = list(inputs)
        if imgs[0].dtype == torch.float32:
            return dict(inputs=torch.stack(imgs, 0).cuda(non_blocking=True).contiguous(), data_samples=samples)
        if imgs[0].dtype != torch.uint8:
            raise TypeError(f"SegDataPreProcessor: expected uint8 or float32 images, got {imgs[0].dtype}")
        # a sample of the device pipeline (datasets.Compose(device=True)) is the decoded HWC image plus metainfo["aug_plan"]: resize, crop,
        # flip and photometric distortion run in the kernel that normalises and pads (ops.augment_u8); its shape is the plan's crop
        plans = [None if samples is None else (getattr(samples[i], "metainfo", None) or {}).get("aug_plan") for i in range(len(imgs))]
        shapes = [tuple(im.shape[-2:]) if p is None else tuple(p["crop"][2:]) for im, p in zip(imgs, plans)]
        hp, wp = self._target(shapes, training)
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty(len(imgs), 3, hp, wp, dtype=torch.float32, device=dev)
        for i, im in enumerate(imgs):
            if plans[i] is None:
                ops.preprocess_u8(im.to(dev, non_blocking=True).contiguous(), out[i], self.mean_l, self.std_l, self.channel_swap, self.pad_val)
            else:
                ops.augment_u8(im.to(dev, non_blocking=True).contiguous(), plans[i], out[i], self.mean_l, self.std_l, self.channel_swap, self.pad_val)
            if samples is not None:
                s_ = samples[i]
                h, w = shapes[i]
                gt = getattr(s_, "gt_sem_seg", None)
                g = None if gt is None else (gt if torch.is_tensor(gt) else gt.data)
                if training and g is not None and tuple(g.shape[-2:]) != (hp, wp):   # (test mode: stack_batch pads the images only)
                    pad = torch.full(tuple(g.shape[:-2]) + (hp, wp), self.seg_pad_val, dtype=g.dtype, device=g.device)
                    pad[..., :g.shape[-2], :g.shape[-1]] = g
                    s_.gt_sem_seg = PixelData(pad)
                meta = dict(getattr(s_, "metainfo", {}) or {})
                meta.pop("aug_plan", None)    # consumed: what is left is the host chain's metainfo
                meta.update(img_shape=(hp, wp), pad_shape=(hp, wp), padding_size=(0, wp - w, 0, hp - h))
                meta.setdefault("ori_shape", (h, w))
                s_.metainfo = meta
        return dict(inputs=out, data_samples=samples)


def get_crop_bbox(img_h, img_w, crop_size, divisible=1):
    """Ms_VFM_encoder_decoder.py:34-46 (np.random: same RNG stream as the reference)."""
    assert crop_size[0] > 0 and crop_size[1] > 0
    if img_h == crop_size[-2] and img_w == crop_size[-1]:
        return (0, img_h, 0, img_w)
    margin_h = max(img_h - crop_size[-2], 0)
    margin_w = max(img_w - crop_size[-1], 0)
    offset_h = np.random.randint(0, (margin_h + 1) // divisible) * divisible
    offset_w = np.random.randint(0, (margin_w + 1) // divisible) * divisible
    return offset_h, offset_h + crop_size[0], offset_w, offset_w + crop_size[1]


def gate_cannot_fire(threadshod, conf):
    """ms_inference's gate keeps a window's coarse logits when the fraction of its pixels whose max softmax exceeds `threadshod` reaches
    `conf` (Ms_VFM_encoder_decoder.py:430-461).  No softmax exceeds 1 and no fraction exceeds 1: with threadshod >= 1 (and conf > 0) or
    conf > 1 every window is refined whatever the coarse logits say - the case in which the coarse pass may run beside the window pass."""
    return conf > 1.0 or (threadshod >= 1.0 and conf > 0.0)


def add_prefix(d, prefix):
    return {f"{prefix}.{k}": v for k, v in d.items()}


def grid_boxes(h_img, w_img, crop, stride):
    h_crop, w_crop = crop
    h_stride, w_stride = stride
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    out = []
    for hi in range(h_grids):
        for wi in range(w_grids):
            y2 = min(hi * h_stride + h_crop, h_img)
            x2 = min(wi * w_stride + w_crop, w_img)
            out.append((max(y2 - h_crop, 0), y2, max(x2 - w_crop, 0), x2))
    return out


@MODELS.register_module()
class EncoderDecoder(nn.Module):
    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None,
                 data_preprocessor=None, pretrained=None, init_cfg=None):
        super().__init__()
        if neck is not None or auxiliary_head is not None:
            raise NotImplementedError("neck / auxiliary_head are outside the hot path")
        self.data_preprocessor = MODELS.build(data_preprocessor or dict(type="SegDataPreProcessor"))
        self.backbone = MODELS.build(backbone)
        self.decode_head = MODELS.build(decode_head)
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.out_channels = self.decode_head.out_channels
        self.train_cfg, self.test_cfg = CfgDict(train_cfg), CfgDict(test_cfg)
        self.with_neck = False
        if type(self.backbone).__name__ == "DinoVisionTransformer":   # the bare backbone: its init_cfg is the pretrained base
            self._load_backbone_init_cfg(backbone)

    # full fine-tuning of a bare DinoVisionTransformer: the segmentors that send the backbone over several inputs per step or train it
    # against a teacher (MsVFMEncoderDecoder, HRDAEncoderDecoder, DACS) refuse it by name
    _full_finetune_ok = True

    def _load_backbone_init_cfg(self, backbone):
        """backbone init_cfg=dict(type='Pretrained', checkpoint=PATH | state dict) -> the backbone's weights, strictly: a file whose keys
        do not match is an error, not an untrained base.  A backbone that reads its own init_cfg (ReinsDinoVisionTransformer) or has been
        loaded already is left alone."""
        ic = backbone.get("init_cfg") if isinstance(backbone, dict) else None
        ck = ic.get("checkpoint") if isinstance(ic, dict) else None
        if ck is not None and getattr(self.backbone, "pretrained", None) is None:
            if ic.get("type", "Pretrained") != "Pretrained":
                raise NotImplementedError(f"init_cfg type {ic.get('type')!r}: only dict(type='Pretrained', checkpoint=...) is read")
            sd = torch.load(ck, map_location="cpu") if isinstance(ck, (str, os.PathLike)) else ck
            sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
            self.backbone.load_state_dict(sd, strict=True)
            self.backbone.pretrained = ck if isinstance(ck, (str, os.PathLike)) else "<state dict>"

    # ---- features
    def _tokens(self, jobs):
        bb = self.backbone
        if hasattr(bb, "forward_tokens"):
            if bb.__class__.__name__ == "LoRABackbone":
                xcat, (hp, wp) = bb.forward_tokens(jobs)
            elif hasattr(bb, "adapter_training"):   # a ViT that carries its own adapters (Rein) says whether they are being trained
                xcat, (hp, wp) = bb.forward_tokens(jobs, training=bb.adapter_training())
            elif getattr(bb, "full_training", None) is not None and bb.full_training() and torch.is_grad_enabled():
                # a bare DinoVisionTransformer in train() mode: every base weight trains (full fine-tuning); eval() / no_grad calls stay
                # on the prediction path below
                if not self._full_finetune_ok:
                    raise NotImplementedError(
                        f"{type(self).__name__} over a bare DinoVisionTransformer in train() mode (full fine-tuning): only EncoderDecoder "
                        "(whole / slide) trains the base; wrap the backbone (LoRABackbone, ReinsDinoVisionTransformer) or use the "
                        "frozen-backbone segmentor")
                xcat, (hp, wp) = bb.forward_tokens(jobs, training=True)
            else:
                xcat, (hp, wp) = bb.forward_tokens(jobs, training=False)
            return xcat, hp, wp
        raise NotImplementedError(type(bb))

    def extract_feat(self, inputs):
        xcat, hp, wp = self._tokens([(inputs, None)])
        return FeatPack(xcat, inputs.shape[0], hp, wp)

    # ---- mmengine BaseModel surface
    def forward(self, inputs, data_samples=None, mode="tensor"):
        if mode == "loss":
            return self.loss(inputs, data_samples)
        if mode == "predict":
            return self.predict(inputs, data_samples)
        return self.decode_head.forward(self.extract_feat(inputs))

    def loss(self, inputs, data_samples):
        fp = self.extract_feat(inputs)
        seg_label = self.decode_head._stack_batch_gt(data_samples).cuda()
        return add_prefix(self.decode_head.loss(fp, seg_label), "decode")

    def parse_losses(self, losses):
        total = None
        log = {}
        for k, v in losses.items():
            log[k] = v
            if "loss" in k:
                total = v if total is None else total + v
        log["loss"] = total
        return total, log

    def train_step(self, data, optim_wrapper):
        data = self.data_preprocessor(data, True)
        losses = self.forward(data["inputs"], data["data_samples"], mode="loss")
        total, log = self.parse_losses(losses)
        optim_wrapper.update_params(total)
        # mmengine's parse_losses returns detached log_vars: after the update nobody may backpropagate through them again
        return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in log.items()}

    def encode_decode(self, inputs, batch_img_metas):
        return self.decode_head.predict(self.extract_feat(inputs), batch_img_metas, self.test_cfg)

    def whole_inference(self, inputs, batch_img_metas):
        return self.encode_decode(inputs, batch_img_metas)

    @staticmethod
    def _window_batch(seg, boxes):
        """[len(boxes) * B, C, hc, wc]: the windows (y1, y2, x1, x2) of the NCHW map seg, window-major, contiguous."""
        B, C = seg.shape[:2]
        hc, wc = boxes[0][1] - boxes[0][0], boxes[0][3] - boxes[0][2]
        out = torch.empty(len(boxes) * B, C, hc, wc, dtype=torch.float32, device=seg.device)
        for j, (y1, y2, x1, x2) in enumerate(boxes):
            win = seg[:, :, y1:y2, x1:x2]
            ops.strided_copy(win, out[j * B:(j + 1) * B], (B, C, hc, wc), (win.stride(0), win.stride(1), win.stride(2), 1),
                             (C * hc * wc, hc * wc, wc, 1))
        return out

    @staticmethod
    def _gate_counts(seg, boxes, thr, cnt):
        """cnt[j] += the number of pixels of window boxes[j] = (y1, y2, x1, x2) of the NCHW map seg whose max softmax exceeds thr:
        all windows in one pass (up to 16), else one pass per window."""
        if len(boxes) <= 16:
            ops.conf_gate_windows(seg, [(y1, x1, y2 - y1, x2 - x1) for (y1, y2, x1, x2) in boxes], thr, cnt)
        else:
            for j, (y1, y2, x1, x2) in enumerate(boxes):
                ops.conf_gate_count(seg, (y1, x1, y2 - y1, x2 - x1), thr, cnt[j:j + 1])
        return cnt

    @staticmethod
    def _merge_windows(wins, B, C, H, W, dev):
        """mmseg's slide merge (preds[window] += resize(window logits); count += 1; preds / count) over `wins` = [(logits, nchw, (y0, x0, hc,
        wc))] in accumulation order: one gather pass (vfm_slide_gather), or the per-window accumulate + finalize when the table does not fit."""
        preds = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        if ops.slide_gather(wins, preds):
            return preds
        preds.zero_()
        count = torch.zeros(B, 1, H, W, dtype=torch.float32, device=dev)
        for t, nchw, box in wins:
            h, w = (t.shape[2], t.shape[3]) if nchw else (t.shape[1], t.shape[2])
            ops.slide_accumulate(t, nchw, B, h, w, C, preds, count, box)
        ops.slide_finalize(preds, count)
        return preds

    def slide_inference(self, inputs, batch_img_metas):
        B, _, H, W = inputs.shape
        # the windows are independent: ONE batched backbone + head pass over all of them (rows = window-major), then the
        # resize-and-merge of the windows.  Same arithmetic as mmseg's sequential loop, far better GEMM shapes.
        boxes = grid_boxes(H, W, self.test_cfg.crop_size, self.test_cfg.stride)
        xcat, hp, wp = self._tokens([(inputs, b) for b in boxes])
        lg = self.decode_head.forward_tokens(FeatPack(xcat, B * len(boxes), hp, wp))  # NHWC low-res, [nwin*B, h, w, C]
        wins = [(lg[j * B:(j + 1) * B], False, (y1, x1, y2 - y1, x2 - x1)) for j, (y1, y2, x1, x2) in enumerate(boxes)]
        return self._merge_windows(wins, B, self.out_channels, H, W, inputs.device)

    def inference(self, inputs, batch_img_metas):
        mode = self.test_cfg.get("mode", "whole")
        assert mode in ("slide", "whole")
        return self.slide_inference(inputs, batch_img_metas) if mode == "slide" else self.whole_inference(inputs, batch_img_metas)

    @torch.no_grad()
    def predict(self, inputs, data_samples=None):
        if data_samples is not None and len(data_samples) and getattr(data_samples[0], "metainfo", None):
            metas = [d.metainfo for d in data_samples]
        else:
            metas = [dict(ori_shape=inputs.shape[2:], img_shape=inputs.shape[2:], pad_shape=inputs.shape[2:],
                          padding_size=[0, 0, 0, 0])] * inputs.shape[0]
        seg_logits = self.inference(inputs, metas)
        return self.postprocess_result(seg_logits, data_samples, metas)

    def postprocess_result(self, seg_logits, data_samples, metas):
        """mmseg EncoderDecoder/BaseSegmentor.postprocess_result (1.2.2, restated; reached from tools/test.py:96-145): per
        image remove the padding recorded by the data preprocessor (`img_padding_size` / `padding_size` = left, right, top,
        bottom), undo a test-time flip, resize the logits bilinearly to `ori_shape`, argmax -> `seg_logits` / `pred_sem_seg`."""
        B, C, H, W = seg_logits.shape
        out = []
        plain = True
        for i in range(B):
            m = metas[i] if metas else {}
            pad = m.get("img_padding_size", m.get("padding_size", [0, 0, 0, 0]))
            ori = tuple(m.get("ori_shape", (H, W)))[:2]
            if any(int(v) for v in pad) or m.get("flip") or ori != (H, W):
                plain = False
        if plain:  # synthetic / already-sized inputs: one argmax launch over the batch, no copies
            am = torch.empty(B, H, W, dtype=torch.uint8, device=seg_logits.device)
            ops.slide_finalize(seg_logits, None, am)
            per_img = [(seg_logits[i], am[i:i + 1]) for i in range(B)]
        else:
            per_img = []
            for i in range(B):
                m = metas[i] if metas else {}
                pl, pr, pt, pb = [int(v) for v in m.get("img_padding_size", m.get("padding_size", [0, 0, 0, 0]))]
                h, w = H - pt - pb, W - pl - pr
                win = seg_logits[i, :, pt:H - pb, pl:W - pr]
                cur = torch.empty(1, C, h, w, dtype=torch.float32, device=seg_logits.device)
                sstr = [win.stride(0), win.stride(1), win.stride(2)]
                src = win
                if m.get("flip"):
                    fd = m.get("flip_direction", "horizontal")
                    assert fd in ("horizontal", "vertical")
                    if fd == "horizontal":   # read each row backwards: start at its last element, stride -1
                        src, sstr = win[:, :, w - 1:], [win.stride(0), win.stride(1), -win.stride(2)]
                    else:
                        src, sstr = win[:, h - 1:, :], [win.stride(0), -win.stride(1), win.stride(2)]
                ops.strided_copy(src, cur, (C, h, w), sstr, (h * w, w, 1))
                oh, ow = tuple(m.get("ori_shape", (h, w)))[:2]
                if (oh, ow) != (h, w):
                    res = torch.empty(1, C, oh, ow, dtype=torch.float32, device=seg_logits.device)
                    ops.resize_bilinear(cur, True, 1, h, w, C, res, 1, (oh, ow))
                    cur = res
                am = torch.empty(1, oh, ow, dtype=torch.uint8, device=seg_logits.device)
                ops.slide_finalize(cur, None, am)
                per_img.append((cur[0], am))
        for i in range(B):
            ds = data_samples[i] if data_samples else SegDataSample()
            ds.seg_logits = PixelData(per_img[i][0])
            ds.pred_sem_seg = PixelData(per_img[i][1])
            out.append(ds)
        return out

    @torch.no_grad()
    def predict_labels(self, inputs, data_samples=None, hist=None, num_classes=None, ignore_index=255):
        """predict() for callers that need the label map and not the logits (the evaluation loop): the same inference(), then per
        image ONE vfm_postprocess_argmax launch that reads the un-padded window of the logits in place, undoes the flip, samples at
        `ori_shape` and takes the argmax - no cropped copy, no full-resolution logits.  Returns samples carrying only `pred_sem_seg`
        (uint8 [1, oh, ow]).  hist (int64 [(num_classes+1)*num_classes], device): the confusion counts of every sample that has a
        `gt_sem_seg` are added to it in the same launch.  VFMSEG_POST_FUSED=0: the composition of the existing ops
        (postprocess_result + metrics.confusion), same values."""
        if data_samples is not None and len(data_samples) and getattr(data_samples[0], "metainfo", None):
            metas = [d.metainfo for d in data_samples]
        else:
            metas = [dict(ori_shape=inputs.shape[2:], img_shape=inputs.shape[2:], pad_shape=inputs.shape[2:],
                          padding_size=[0, 0, 0, 0])] * inputs.shape[0]
        seg_logits = self.inference(inputs, metas)
        B, C, H, W = seg_logits.shape
        assert hist is None or num_classes is not None
        fused = post_fused_default() and C <= 32

        def label_of(ds):
            gt = getattr(ds, "gt_sem_seg", None) if ds is not None else None
            if gt is None or hist is None:
                return None
            g = (gt if torch.is_tensor(gt) else gt.data).to(seg_logits.device)
            return (g if g.dtype in (torch.uint8, torch.int64) else g.long()).contiguous()

        out = []
        if not fused:
            from .metrics import confusion
            for ds in self.postprocess_result(seg_logits, data_samples, metas):
                pred = ds.pred_sem_seg.data
                res = SegDataSample(metainfo=ds.metainfo)
                if hasattr(ds, "gt_sem_seg"):
                    res.gt_sem_seg = ds.gt_sem_seg
                res.pred_sem_seg = PixelData(pred)
                lab = label_of(ds)
                if lab is not None:
                    confusion(pred, lab, num_classes, ignore_index, out=hist)
                out.append(res)
            return out
        for i in range(B):
            m = metas[i] if metas else {}
            pl, pr, pt, pb = [int(v) for v in m.get("img_padding_size", m.get("padding_size", [0, 0, 0, 0]))]
            h, w = H - pt - pb, W - pl - pr
            flip = 0
            if m.get("flip"):
                fd = m.get("flip_direction", "horizontal")
                assert fd in ("horizontal", "vertical")
                flip = 1 if fd == "horizontal" else 2
            oh, ow = tuple(m.get("ori_shape", (h, w)))[:2]
            ds = data_samples[i] if data_samples else None
            lab = label_of(ds)
            pred = ops.postprocess_argmax(seg_logits[i], (pt, pl, h, w), flip, (oh, ow), label=lab, hist=None if lab is None else hist,
                                          num_classes=num_classes, ignore_index=ignore_index)
            res = SegDataSample(metainfo=m)
            if ds is not None and hasattr(ds, "gt_sem_seg"):
                res.gt_sem_seg = ds.gt_sem_seg
            res.pred_sem_seg = PixelData(pred.view(1, oh, ow))
            out.append(res)
        return out


def post_fused_default():
    """VFMSEG_POST_FUSED (A/B knob, default 1): predict_labels runs vfm_postprocess_argmax; 0 composes the existing ops."""
    return os.environ.get("VFMSEG_POST_FUSED", "1") != "0"


def tta_views(tta_pipeline):
    """(ratio, flip) views of an mmseg `tta_pipeline` (the TestTimeAug entry: a list of Resize alternatives x a list of RandomFlip
    alternatives; tools/test.py:131-134 installs it under --tta)."""
    ratios, flips = [1.0], [False]
    for t in tta_pipeline:
        if t.get("type") != "TestTimeAug":
            continue
        for alts in t["transforms"]:
            kinds = {a_.get("type") for a_ in alts}
            if kinds == {"Resize"}:
                ratios = [float(a_.get("scale_factor", 1.0)) for a_ in alts]
            elif kinds == {"RandomFlip"}:
                flips = [float(a_.get("prob", 0.0)) >= 1.0 for a_ in alts]
    return [(r, f) for r in ratios for f in flips]


@torch.no_grad()
def predict_tta(model, inputs, data_samples, views):
    """mmseg SegTTAModel.merge_preds (restated): every view is predicted and post-processed back to `ori_shape` (the flip is undone
    there), the views' class softmax is averaged, argmax.  Views are produced from the loaded tensor (bilinear resize, flip)."""
    B, C, H, W = inputs.shape
    acc = None
    for ratio, flip in views:
        x = inputs
        if ratio != 1.0:
            h, w = int(H * ratio + 0.5), int(W * ratio + 0.5)
            y = torch.empty(B, C, h, w, dtype=torch.float32, device=inputs.device)
            ops.resize_bilinear(inputs.contiguous(), True, B, H, W, C, y, 1, (h, w))
            x = y
        if flip:
            x = torch.flip(x, dims=[3]).contiguous()
        samples = []
        for i in range(B):
            m = dict((data_samples[i].metainfo if data_samples else None) or {})
            m.setdefault("ori_shape", (H, W))
            m.update(img_shape=tuple(x.shape[2:]), pad_shape=tuple(x.shape[2:]), padding_size=[0, 0, 0, 0], flip=flip, flip_direction="horizontal")
            samples.append(SegDataSample(metainfo=m))
        out = model.predict(x, samples)
        probs = [o.seg_logits.data.softmax(dim=0) for o in out]
        acc = probs if acc is None else [a_ + p_ for a_, p_ in zip(acc, probs)]
    res = []
    for i in range(B):
        ds = data_samples[i] if data_samples else SegDataSample()
        mean = acc[i] / len(views)
        ds.seg_logits = PixelData(mean)
        ds.pred_sem_seg = PixelData(mean.argmax(dim=0, keepdim=True))
        res.append(ds)
    return res


@MODELS.register_module()
class LoraBackboneEncoderDecoder(EncoderDecoder):
    """Lora_encoder_decoder.py:12-44: plain EncoderDecoder whose backbone is LoRA-wrapped."""

    def __init__(self, Lora_config, checkpoint=None, backbone=None, **kw):
        super().__init__(backbone=dict(type="LoRABackbone", backbone=backbone, checkpoint=checkpoint, Lora_config=Lora_config), **kw)


@MODELS.register_module()
class FrozenBackboneEncoderDecoder(EncoderDecoder):
    """rein/models/segmentors/frozen_encoder_decoder.py:19-34: the backbone stays in eval mode, none of its parameters train, and its
    taps are computed without a graph.  The checkpoint still holds the whole model."""

    def __init__(self, backbone, **kw):
        super().__init__(backbone=backbone, **kw)
        # dinov2_SegFormer_frozen.py: the frozen weights arrive through the backbone's init_cfg=dict(type="Pretrained", checkpoint=PATH);
        # a backbone that reads its own init_cfg (ReinsDinoVisionTransformer) has loaded them already
        self._load_backbone_init_cfg(backbone)   # a file whose keys do not match is an error, not an untrained frozen base
        self.train(self.training)   # frozen from construction on: an optimiser built before the first train() sees no backbone parameter

    def train(self, mode=True):
        super().train(mode)
        self.backbone.eval()
        for p in self.backbone.parameters():
            p.requires_grad = False
        return self

    def _tokens(self, jobs):
        with torch.no_grad():
            xcat, hp, wp = super()._tokens(jobs)
            cd = compute_dtype()
            if self.training and xcat.dtype != cd:
                # fp16 mode: a backbone that runs without a graph hands out fp32 taps (precision.eval_heads_fp32, meant for predictions);
                # the train step keeps 16-bit heads, as the reference's autocast does
                taps = torch.empty(xcat.shape, dtype=cd, device=xcat.device)
                xcat = ops.cast(xcat, taps)
        return xcat.detach(), hp, wp


@MODELS.register_module()
class MsVFMEncoderDecoder(EncoderDecoder):
    _full_finetune_ok = False   # a bare DinoVisionTransformer in train() mode is refused by name (EncoderDecoder._tokens)

    def __init__(self, backbone, decode_head, aux_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None, scales=[1], hr_crop_size=None, crop_coord_divisible=1, feature_scale=1,
                 data_preprocessor=None, debug=False, debug_interval=100, detail_loss=1.0):
        super().__init__(backbone=backbone, decode_head=decode_head, neck=neck, auxiliary_head=auxiliary_head,
                         train_cfg=train_cfg, test_cfg=test_cfg, data_preprocessor=data_preprocessor)
        self.local_iter = 0
        self.scales = sorted(scales)
        assert len(self.scales) <= 2, "Only up to 2 scales are supported."
        self.feature_scale = feature_scale
        self.crop_size = hr_crop_size
        self.crop_coord_divisible = crop_coord_divisible
        self.hr_crop_box = None
        self.fixed_crop_box = None  # parity tests / benchmarks pin the RNG consumer
        self.aux_decoder = MODELS.build(aux_head)
        self.detail_loss = detail_loss

    # ---- training (Ms_VFM_encoder_decoder.py:125-200)
    def loss(self, inputs, data_samples):
        return self.forward_train(inputs, data_samples)

    def forward_train(self, img, data_samples):
        B, _, H, W = img.shape
        s0, s1 = self.scales
        assert s1 == 1 and self.crop_size is not None
        lh, lw = int(H * s0), int(W * s0)
        lr_img = torch.empty(B, 3, lh, lw, dtype=torch.float32, device=img.device)
        ops.resize_bilinear(img, True, B, H, W, 3, lr_img, 1, (lh, lw), scale_factor=s0)
        box =self.fixed_crop_box or get_crop_bbox(H, W, self.crop_size, self.crop_coord_divisible)
        self.hr_crop_box = box
        y1, y2, x1, x2 = box
        assert (lh, lw) == (y2 - y1, x2 - x1), "LR pass and HR crop must share the token grid to be batched"
        # one batched backbone call: rows [0, B*P) = LR pass, [B*P, 2*B*P) = HR crop
        xcat, hp, wp = self._tokens([(lr_img, None), (img, box)])
        P = hp * wp
        lr_fp, hr_fp = FeatPack(xcat[:B * P], B, hp, wp), FeatPack(xcat[B * P:], B, hp, wp)
        seg_label = self.decode_head._stack_batch_gt(data_samples).to(img.device).squeeze(1).contiguous()  # [B,H,W]
        lr_gt = torch.empty(B, lh, lw, dtype=torch.int64, device=img.device)
        hr_gt = torch.empty(B, y2 - y1, x2 - x1, dtype=torch.int64, device=img.device)
        ops.label_resize(seg_label, lr_gt, (lh, lw))                               # get_lr_seg: nearest 0.5x
        ops.label_resize(seg_label, hr_gt, (H, W), (y1, x1, y2 - y1, x2 - x1))     # get_hr_seg: crop
        losses = {}
        lr_low = self.decode_head.forward_tokens(lr_fp)                            # [B, 4hp, 4wp, C] fp32
        loss_lr = self.decode_head._loss_from_lowres(lr_low, lr_gt.unsqueeze(1), False)
        losses.update(add_prefix(loss_lr, "decode_lr"))
        # get_seg_logits (:160-167): detached full-res LR logits cropped at box/2 -> context for the detail head
        assert all(v % 2 == 0 for v in box)
        cy, cx, ch, cw = y1 // 2, x1 // 2, (y2 - y1) // 2, (x2 - x1) // 2
        Bc, h4, w4, C = lr_low.shape
        ctx = torch.empty(B, C, ch, cw, dtype=torch.float32, device=img.device)
        ops.resize_bilinear(lr_low.detach(), False, B, h4, w4, C, ctx, 1, (lh, lw), (cy, cx, ch, cw))
        hr_low = self.aux_decoder.forward_tokens(hr_fp, ctx)
        loss_hr = self.aux_decoder._loss_from_lowres(hr_low, hr_gt.unsqueeze(1), False)
        if self.detail_loss != 1.0:
            loss_hr["loss_ce"] = loss_hr["loss_ce"] * self.detail_loss
        losses.update(add_prefix(loss_hr, "decode_hr"))
        self.local_iter += 1
        return losses

    # ---- inference (Ms_VFM_encoder_decoder.py:268-332, 400-466)
    def enc_dec(self, inputs, context=None, box=None):
        B = inputs.shape[0]
        xcat, hp, wp = self._tokens([(inputs, box)])
        fp = FeatPack(xcat, B, hp, wp)
        if context is None:
            return self.decode_head.forward_tokens(fp)
        return self.aux_decoder.forward_tokens(fp, context)

    def inference(self, inputs, batch_img_metas):
        """Ms_VFM_encoder_decoder.py:276-332: the four test modes."""
        mode = self.test_cfg.get("mode", "lr_slide_inference")
        assert mode in ("lr_slide_inference", "hr_slide_inference", "msfull_slide_inference", "ms_slide_inference")
        if mode == "ms_slide_inference":
            return self.ms_inference(inputs, batch_img_metas)
        if mode == "hr_slide_inference":
            return self.slide_inference(inputs, batch_img_metas)
        if mode == "lr_slide_inference":
            return self.lr_slide_inference(inputs, batch_img_metas)
        return self.msfull_slide_inference(inputs, batch_img_metas)

    def _resize_nchw(self, x, size, scale_factor=None):
        B, C, H, W = x.shape
        out = torch.empty(B, C, size[0], size[1], dtype=torch.float32, device=x.device)
        ops.resize_bilinear(x, True, B, H, W, C, out, 1, tuple(size), scale_factor=scale_factor)
        return out

    def lr_slide_inference(self, inputs, batch_img_metas):
        """:280-283: 0.5x bilinear input, the base class' sliding LinearHead pass, 2x bilinear logits."""
        B, _, H, W = inputs.shape
        lh, lw = int(H * 0.5), int(W * 0.5)    # F.interpolate(scale_factor=0.5): floor(size * scale), sampled at source scale 2
        lr = self.slide_inference(self._resize_nchw(inputs, (lh, lw), scale_factor=0.5), batch_img_metas)
        return self._resize_nchw(lr, (int(lh * 2), int(lw * 2)), scale_factor=2.0)

    # ---- coarse pass beside the window pass
    # When every window is refined whatever the coarse logits say (msfull_slide_inference; ms_slide_inference with a gate that cannot
    # fire: threadshod >= 1 or conf > 1), the windows' backbone pass does not depend on the coarse pass: only the VFMHead's context does.
    # The coarse pass (one 512 x 1024 image: GEMMs of 136-544 tiles, attention with 272 blocks - half the chip idle) then runs on a side
    # stream beside the nine-window pass and is joined in front of the head.  Same kernels on the same data: bit-identical predictions.
    # The first prediction after a weight change runs on one stream (it builds the packed / merged weights both passes read).
    _side = {"stream": None}

    def _overlap_ok(self):
        from .optim import PARAM_EPOCH
        if os.environ.get("VFMSEG_EVAL_OVERLAP", "1") == "0" or not torch.cuda.is_available():
            return False
        key = (PARAM_EPOCH[0], self.training)
        if getattr(self, "_overlap_key", None) != key:
            self._overlap_key = key
            return False
        return True

    def _coarse_beside(self, coarse_fn, window_fn):
        """(coarse_fn(), window_fn()): on one stream, or coarse_fn on the side stream while window_fn runs here (joined before returning)."""
        if not self._overlap_ok():
            return coarse_fn(), window_fn()
        if self._side["stream"] is None:
            self._side["stream"] = torch.cuda.Stream()
        side, main = self._side["stream"], torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            seg = coarse_fn()
        out = window_fn()
        main.wait_stream(side)
        seg.record_stream(main)
        return seg, out

    def msfull_slide_inference(self, inputs, batch_img_metas):
        """:286-328: coarse sliding LinearHead pass on the input squeezed to (512, 1024), logits resized to the input size,
        then EVERY window refined by the VFMHead with its coarse logits as context (no confidence gate; the decoder's query mask
        stays enabled here - only ms_inference turns it off, :422-423).  All windows go through one batched pass."""
        B, _, H, W = inputs.shape
        C = self.out_channels
        dev = inputs.device
        boxes = grid_boxes(H, W, self.test_cfg.crop_size, self.test_cfg.stride)
        hc, wc = boxes[0][1] - boxes[0][0], boxes[0][3] - boxes[0][2]
        assert all((b[1] - b[0], b[3] - b[2]) == (hc, wc) for b in boxes)
        seg, (xcat, hp, wp) = self._coarse_beside(
            lambda: self._resize_nchw(self.slide_inference(self._resize_nchw(inputs, (512, 1024)), batch_img_metas), (H, W)),
            lambda: self._tokens([(inputs, b) for b in boxes]))
        if self.aux_decoder.ctx_windows_ok(seg, boxes, hp, wp):   # the context windows are sampled straight out of the coarse map
            lg = self.aux_decoder.forward_tokens(FeatPack(xcat, B * len(boxes), hp, wp), None, ctx_windows=(seg, boxes))
        else:
            lg = self.aux_decoder.forward_tokens(FeatPack(xcat, B * len(boxes), hp, wp), self._window_batch(seg, boxes))
        wins = [(lg[j * B:(j + 1) * B], False, (y1, x1, hc, wc)) for j, (y1, y2, x1, x2) in enumerate(boxes)]
        self.hr_crop_box = boxes[-1]
        return self._merge_windows(wins, B, C, H, W, dev)

    def ms_inference(self, inputs, batch_img_metas):
        """Ms_VFM_encoder_decoder.py:400-466.  Stage 0: whole-image pass at a hard-coded (512, 1024) through the
        LinearHead, bilinear to the image size.  Stage 1: per 512^2 window, confidence gate (fraction of pixels whose
        max softmax exceeds `threadshod`; one device->host sync per window, as in the reference) and, when below
        `conf`, the VFMHead refinement with that window's coarse logits as context; sliding accumulate."""
        thr = self.test_cfg.get("threadshod", 1.0)
        conf = self.test_cfg.get("conf", 1.0)
        B, _, H, W = inputs.shape
        dev = inputs.device
        C = self.out_channels

        def coarse():
            small = torch.empty(B, 3, 512, 1024, dtype=torch.float32, device=dev)
            ops.resize_bilinear(inputs, True, B, H, W, 3, small, 1, (512, 1024))
            lg0 = self.enc_dec(small)                                   # NHWC low-res logits of the coarse pass
            seg = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
            ops.resize_bilinear(lg0, False, B, lg0.shape[1], lg0.shape[2], C, seg, 1, (H, W))  # predict_by_feat -> image size
            return seg

        boxes = grid_boxes(H, W, self.test_cfg.crop_size, self.test_cfg.stride)
        # a gate that cannot fire (no pixel's max softmax exceeds 1; no fraction reaches a conf above 1): every window is refined
        all_refined = gate_cannot_fire(thr, conf)
        early = None
        if all_refined:
            seg, early = self._coarse_beside(coarse, lambda: self._tokens([(inputs, b) for b in boxes]))
        else:
            seg = coarse()
        dec = getattr(self.aux_decoder, "transformer_decoder", None)
        had_mask = getattr(dec, "mask_enable", None)
        if had_mask is not None:
            dec.mask_enable = False
        cnt = torch.zeros(len(boxes), dtype=torch.int32, device=dev)
        self.last_refined = []
        try:
            # all gates depend only on the coarse logits: evaluate them together (ONE pass over the map and ONE device->host sync
            # instead of one of each per window), then refine the selected windows in one batched backbone + VFMHead pass
            if all_refined:          # (no gate to evaluate, no device->host sync)
                refine = list(range(len(boxes)))
            else:
                self._gate_counts(seg, boxes, thr, cnt)
                fracs = [c / float(B * (b[1] - b[0]) * (b[3] - b[2])) for c, b in zip(cnt.tolist(), boxes)]
                refine = [j for j, f in enumerate(fracs) if f < conf]
            hc, wc = boxes[0][1] - boxes[0][0], boxes[0][3] - boxes[0][2]
            assert all((b[1] - b[0], b[3] - b[2]) == (hc, wc) for b in boxes)
            if refine:
                xcat, hp, wp = early if early is not None else self._tokens([(inputs, boxes[j]) for j in refine])
                rboxes = [boxes[j] for j in refine]
                if self.aux_decoder.ctx_windows_ok(seg, rboxes, hp, wp):   # context windows sampled straight out of the coarse map
                    lg = self.aux_decoder.forward_tokens(FeatPack(xcat, B * len(refine), hp, wp), None, ctx_windows=(seg, rboxes))
                else:
                    lg = self.aux_decoder.forward_tokens(FeatPack(xcat, B * len(refine), hp, wp), self._window_batch(seg, rboxes))   # [nref*B, hp, wp, C]
            keep = [j for j in range(len(boxes)) if j not in refine]
            kctx = self._window_batch(seg, [boxes[j] for j in keep]) if keep else None   # confident windows keep their coarse logits
            wins = []
            for j, (y1, y2, x1, x2) in enumerate(boxes):
                if j in refine:
                    k = refine.index(j)
                    wins.append((lg[k * B:(k + 1) * B], False, (y1, x1, hc, wc)))
                    self.last_refined.append((y1, y2, x1, x2))
                else:
                    k = keep.index(j)
                    wins.append((kctx[k * B:(k + 1) * B], True, (y1, x1, hc, wc)))
                self.hr_crop_box = (y1, y2, x1, x2)
            preds = self._merge_windows(wins, B, C, H, W, dev)
        finally:
            if had_mask is not None:
                dec.mask_enable = had_mask
        return preds


@MODELS.register_module()
class HRDAEncoderDecoder(EncoderDecoder):
    """rein/models/segmentors/hrda_encoder_decoder.py:62-447 (the HRDA multi-resolution baseline): the half-size image and a random
    full-resolution crop (training) or overlapping full-resolution crops (prediction) go through ONE backbone call; the HRDAHead fuses
    their logits by a learned scale attention."""
    _full_finetune_ok = False   # a bare DinoVisionTransformer in train() mode is refused by name (EncoderDecoder._tokens)

    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None, scales=[1], hr_crop_size=None, hr_slide_inference=True, hr_slide_overlapping=True,
                 crop_coord_divisible=1, blur_hr_crop=False, feature_scale=1, data_preprocessor=None):
        if blur_hr_crop:
            raise NotImplementedError("HRDAEncoderDecoder: blur_hr_crop is not used by the reference config and not implemented")
        if (test_cfg or {}).get("test_time_aug", False) or (test_cfg or {}).get("flip", False):
            raise NotImplementedError("HRDAEncoderDecoder: test_time_aug / flip inside slide_inference are not implemented (use tools/test.py --tta)")
        scales = sorted(scales)
        decode_head = dict(decode_head)
        decode_head["scales"] = scales
        decode_head["enable_hr_crop"] = hr_crop_size is not None
        decode_head["hr_slide_inference"] = hr_slide_inference
        super().__init__(backbone=backbone, decode_head=decode_head, neck=neck, auxiliary_head=auxiliary_head, train_cfg=train_cfg,
                         test_cfg=test_cfg, data_preprocessor=data_preprocessor)
        assert len(scales) == 2 and scales[1] == 1, "HRDA runs on two scales, the larger one the image itself"
        self.local_iter = 0
        self.scales = scales
        self.feature_scale = feature_scale
        self.crop_size = hr_crop_size
        self.hr_slide_inference = hr_slide_inference
        self.hr_slide_overlapping = hr_slide_overlapping
        self.crop_coord_divisible = crop_coord_divisible
        self.orginal_slide_inference = self.test_cfg.get("orginal_slide_inference", False)
        self.fixed_crop_box = None      # tests pin the RNG consumer
        self.last_crop_box = None
        self.sequential_windows = False  # one backbone call per outer slide window instead of one for all of them (same sums)

    # ---- features
    def _hr_tokens(self, jobs):
        return self._tokens(jobs)

    def _lr_image(self, img):
        B, _, H, W = img.shape
        s = self.scales[0]
        lh, lw = int(H * s), int(W * s)
        lr_img = torch.empty(B, 3, lh, lw, dtype=torch.float32, device=img.device)
        return ops.resize_bilinear(img, True, B, H, W, 3, lr_img, 1, (lh, lw), scale_factor=s)   # F.interpolate(scale_factor=s): source scale 1/s

    # ---- training (:305-392)
    def loss(self, inputs, data_samples):
        return self.forward_train(inputs, data_samples)

    def forward_train(self, img, data_samples):
        B, _, H, W = img.shape
        assert self.crop_size is not None, "training needs hr_crop_size"
        lr_img = self._lr_image(img)
        box = self.fixed_crop_box or get_crop_bbox(H, W, self.crop_size, self.crop_coord_divisible)
        self.last_crop_box = box
        y1, y2, x1, x2 = box
        assert tuple(lr_img.shape[2:]) == (y2 - y1, x2 - x1), "LR pass and HR crop must share the token grid to be batched"
        xcat, hp, wp = self._hr_tokens([(lr_img, None), (img, box)])
        P = hp * wp
        feats = [FeatPack(xcat[:B * P], B, hp, wp), FeatPack(xcat[B * P:], B, hp, wp)]
        self.decode_head.set_hr_crop_box(box)
        try:
            losses = add_prefix(self.decode_head.loss(feats, data_samples, self.train_cfg), "decode")
        finally:
            self.decode_head.reset_crop()
        self.local_iter += 1
        return losses

    # ---- prediction (:125-150, 275-303)
    def _crop_boxes(self, H, W):
        stride = [e // 2 for e in self.crop_size] if self.hr_slide_overlapping else list(self.crop_size)
        return grid_boxes(H, W, self.crop_size, stride)

    def fused_lowres(self, img):
        """The head's fused logits of whole images, NHWC [B, H/4, W/4, classes]: LR pass on the half-size image, HR pass over the
        `hr_crop_size` crops (stride crop / 2 when overlapping), everything that shares a token grid in one backbone call."""
        B, _, H, W = img.shape
        self.decode_head.reset_crop()
        if self.orginal_slide_inference:
            return self.decode_head.head.forward_tokens(self.extract_feat(img))
        lr_img = self._lr_image(img)
        if not self.hr_slide_inference:
            lr_x, hp, wp = self._hr_tokens([(lr_img, None)])
            hr_x, hph, wph = self._hr_tokens([(img, None)])
            return self.decode_head.forward_test([FeatPack(lr_x, B, hp, wp), FeatPack(hr_x, B, hph, wph)])
        boxes = self._crop_boxes(H, W)
        if tuple(lr_img.shape[2:]) == tuple(self.crop_size):
            xcat, hp, wp = self._hr_tokens([(lr_img, None)] + [(img, b) for b in boxes])
            P = hp * wp
            lr_fp, hr_fp = FeatPack(xcat[:B * P], B, hp, wp), FeatPack(xcat[B * P:], B * len(boxes), hp, wp)
        else:
            lr_x, hp, wp = self._hr_tokens([(lr_img, None)])
            hr_x, hph, wph = self._hr_tokens([(img, b) for b in boxes])
            lr_fp, hr_fp = FeatPack(lr_x, B, hp, wp), FeatPack(hr_x, B * len(boxes), hph, wph)
        return self.decode_head.forward_test([lr_fp, dict(features=hr_fp, boxes=[list(b) for b in boxes])])

    def encode_decode(self, inputs, batch_img_metas, upscale_pred=True):
        lg = self.fused_lowres(inputs)
        if not upscale_pred:
            return lg.permute(0, 3, 1, 2)
        B, h, w, C = lg.shape
        out = torch.empty(B, C, inputs.shape[2], inputs.shape[3], dtype=torch.float32, device=inputs.device)
        return ops.resize_bilinear(lg, False, B, h, w, C, out, 1, tuple(inputs.shape[2:]))

    def slide_inference(self, inputs, batch_img_metas):
        """mmseg's slide merge over `test_cfg.crop_size` windows (batched_slide=True and the per-window loop have the same arithmetic):
        the windows are a batch - one backbone call for the LR images and HR crops of all of them - unless `sequential_windows`."""
        B, _, H, W = inputs.shape
        boxes = grid_boxes(H, W, self.test_cfg.crop_size, self.test_cfg.stride)
        if self.sequential_windows:
            lgs = [self.fused_lowres(self._window_batch(inputs, [b])) for b in boxes]
        else:
            lg = self.fused_lowres(self._window_batch(inputs, boxes))
            lgs = [lg[j * B:(j + 1) * B] for j in range(len(boxes))]
        wins = [(lgs[j], False, (y1, x1, y2 - y1, x2 - x1)) for j, (y1, y2, x1, x2) in enumerate(boxes)]
        return self._merge_windows(wins, B, self.out_channels, H, W, inputs.device)


@MODELS.register_module()
class FrozenHRDAEncoderDecoder(HRDAEncoderDecoder):
    """hrda_encoder_decoder.py:450-464: the backbone stays in eval mode, runs without a graph and none of its parameters train."""

    def train(self, mode=True):
        super().train(mode)
        self.backbone.eval()
        for p in self.backbone.parameters():
            p.requires_grad = False
        return self

    def _hr_tokens(self, jobs):
        with torch.no_grad():
            xcat, hp, wp = self._tokens(jobs)
        return xcat.detach(), hp, wp
