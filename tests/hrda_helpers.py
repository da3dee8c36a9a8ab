"""Shared by the HRDA tests and tools/gen_hrda_golden.py: a torch restatement of the HRDA fusion (rein/models/heads/hrda.py:149-191) on
F.interpolate + autograd in any dtype - float64 is the GPU tests' reference, pinned to the reference-made fixture by
tests/test_hrda_cpu.py - and the synthetic parameter recipe of the HRDA model (LoRA DINOv2 + HRDAHead)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import model_shapes
from vfmseg_amd.synth import synth_state_dict

HEAD_SEED, NP_SEED = 4100, 12
TRAIN_SEED, EVAL_SEED = 41, 43   # synth_image / synth_label seeds of the segmentor-level fixtures
# head-level cases of the fixture: HR crop boxes in image pixels of a 1024^2 image (crop 512^2, multiples of 8)
HEAD_BOXES = {"inner": (200, 712, 328, 840), "corner": (512, 1024, 512, 1024)}
ATT_WEIGHT_SCALE = 0.05   # scale_attention.conv_seg.weight: logits of order 1, so the attention is neither flat nor saturated


def scale_box(box, scale):
    return tuple(int(v / scale) for v in box)


def fuse_ref(lr, a, hr, offset, mask_box, drop=None):
    """NHWC in / out, dtype of the inputs.  -> (fused [B,2h,2w,C], (1 - att) * lr [B,h,w,C]).  `drop` removes one term of the formula:
    'mask' (no crop mask), 'hr_ins' (no HR contribution), 'one_minus_att' (lr is not scaled down)."""
    lr_, a_, hr_ = (t.permute(0, 3, 1, 2) for t in (lr, a, hr))
    B, C, h, w = lr_.shape
    att = F.interpolate(torch.sigmoid(a_), size=(h, w), mode="bilinear", align_corners=False)
    if mask_box is not None and drop != "mask":
        mask = torch.zeros(B, 1, h, w, dtype=lr.dtype, device=lr.device)
        mask[:, :, mask_box[0]:mask_box[1], mask_box[2]:mask_box[3]] = 1
        att = att * mask
    lrs = lr_ if drop == "one_minus_att" else (1 - att) * lr_
    up_lr = F.interpolate(lrs, scale_factor=2, mode="bilinear", align_corners=False)
    up_att = F.interpolate(att, scale_factor=2, mode="bilinear", align_corners=False)
    if tuple(hr_.shape[2:]) == (2 * h, 2 * w) and tuple(offset) == (0, 0):
        ins = hr_
    else:
        ins = F.pad(hr_, (offset[1], 2 * w - offset[1] - hr_.shape[3], offset[0], 2 * h - offset[0] - hr_.shape[2]))
    fused = up_lr if drop == "hr_ins" else up_att * ins + up_lr
    return fused.permute(0, 2, 3, 1), lrs.permute(0, 2, 3, 1)


def fuse_ref_grads(lr, a, hr, offset, mask_box, d_fused, drop=None):
    """(fused, lr_scaled, d_lr, d_a, d_hr) of fuse_ref under autograd in the dtype of the inputs.  drop='sig_grad': d_a without s (1 - s)."""
    lr, a, hr = (t.detach().clone().requires_grad_(True) for t in (lr, a, hr))
    fused, lrs = fuse_ref(lr, a, hr, offset, mask_box, None if drop == "sig_grad" else drop)
    fused.backward(d_fused)
    d_a = a.grad if a.grad is not None else torch.zeros_like(a)
    if drop == "sig_grad":
        s = torch.sigmoid(a.detach())
        d_a = d_a / (s * (1 - s))
    zero = torch.zeros_like
    return fused.detach(), lrs.detach(), lr.grad, d_a, hr.grad if hr.grad is not None else zero(hr)


def fuse_inputs(B, C, ha, wa, h, w, hc, wc, seed):
    g = torch.Generator().manual_seed(seed)
    lr = 2.0 * torch.randn(B, h, w, C, generator=g)
    a = 1.5 * torch.randn(B, ha, wa, C, generator=g)
    hr = 2.0 * torch.randn(B, hc, wc, C, generator=g)
    dF = torch.randn(B, 2 * h, 2 * w, C, generator=g)
    return lr, a, hr, dF


# ---------------------------------------------------------------------------------------------- parameters
def hrda_head_shapes(dim=1024, ch=256, num_classes=19, prefix="decode_head."):
    lin = {k[len("decode_head."):]: v for k, v in model_shapes(1, dim).items() if k.startswith("decode_head.")}
    s = {prefix + "conv_seg.weight": (num_classes, ch, 1, 1), prefix + "conv_seg.bias": (num_classes,)}
    for k, v in lin.items():
        s[prefix + "head." + k] = v
    s[prefix + "head.conv_seg.weight"] = (num_classes, dim // 4, 1, 1)
    a = prefix + "scale_attention."
    s[a + "conv_seg.weight"] = (num_classes, ch, 1, 1)
    s[a + "conv_seg.bias"] = (num_classes,)
    s[a + "fusion_conv.conv.weight"] = (ch, 4 * dim, 1, 1)
    s[a + "fusion_conv.gn.weight"] = (ch,)
    s[a + "fusion_conv.gn.bias"] = (ch,)
    return s


def hrda_head_state_dict(prefix="decode_head."):
    sd = synth_state_dict(hrda_head_shapes(prefix=prefix))
    sd[prefix + "scale_attention.conv_seg.weight"] = sd[prefix + "scale_attention.conv_seg.weight"] * ATT_WEIGHT_SCALE
    return sd


def hrda_model_state_dict(depth=4, dim=1024):
    """HRDAEncoderDecoder(LoRABackbone(DinoVisionTransformer), HRDAHead): the backbone as tests.helpers.full_state_dict builds it."""
    from tests.helpers import full_state_dict
    sd = {k: v for k, v in full_state_dict(depth, dim).items() if k.startswith("backbone.")}
    sd.update(hrda_head_state_dict())
    return sd


def head_feats(seed=HEAD_SEED, b=2):
    """(LR taps, HR taps): two lists of four [b, 1024, 32, 32] maps"""
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(b, 1024, 32, 32, generator=g) for _ in range(4)], [torch.randn(b, 1024, 32, 32, generator=g) for _ in range(4)])


def sample_grid(t, step=37):
    """every `step`-th element of the flattened tensor (the logit sample the inference fixtures share)"""
    return t.detach().reshape(-1)[::step].cpu().numpy()


def np_boxes(seed, n, img=1024, crop=(512, 512), div=8):
    from vfmseg_amd.segmentors import get_crop_bbox
    np.random.seed(seed)
    return [get_crop_bbox(img, img, crop, div) for _ in range(n)]
