"""Shared by the SegFormer-head tests and tools/gen_segformer_golden.py (no reference tree needed): the synthetic parameter recipe of the
three models (LoRA / Rein / frozen DINOv2 + SegformerHead), the seeded head inputs, and a torch restatement of mmseg 1.2.2's SegformerHead
and BaseDecodeHead.loss written from their formulas, in any dtype - float64 is the GPU tests' reference, pinned to the fixture
(tests/golden/segformer.npz) by tests/test_segformer_cpu.py."""
import torch
import torch.nn.functional as F

from tests.helpers import full_state_dict
from tests.rein_helpers import bare_dinov2_state_dict, rein_backbone_state_dict
from vfmseg_amd.synth import synth_state_dict

HEAD_SEED = 5200
TRAIN_SEED, EVAL_SEED = 51, 53   # synth_image / synth_label seeds of the segmentor-level fixtures
DEPTH = 4
KINDS = ("lora", "rein", "frozen")
HEAD_KEYS = ([f"convs.{i}.{n}" for i in range(4) for n in ("conv.weight", "gn.weight", "gn.bias")]
             + ["fusion_conv.conv.weight", "fusion_conv.gn.weight", "fusion_conv.gn.bias", "conv_seg.weight", "conv_seg.bias"])
# image sizes of the slide fixtures (512 windows, stride 341): two windows and nine
SLIDE_SIZES = ((512, 768), (1024, 1024))


def head_shapes(dim=1024, ch=256, num_classes=19, prefix="decode_head."):
    s = {prefix + "conv_seg.weight": (num_classes, ch, 1, 1), prefix + "conv_seg.bias": (num_classes,),
         prefix + "fusion_conv.conv.weight": (ch, 4 * ch, 1, 1), prefix + "fusion_conv.gn.weight": (ch,), prefix + "fusion_conv.gn.bias": (ch,)}
    for i in range(4):
        s[prefix + f"convs.{i}.conv.weight"] = (ch, dim, 1, 1)
        s[prefix + f"convs.{i}.gn.weight"] = (ch,)
        s[prefix + f"convs.{i}.gn.bias"] = (ch,)
    return s


def head_state_dict(prefix="decode_head."):
    sd = synth_state_dict(head_shapes(prefix=prefix))
    for k in sd:   # GroupNorm biases of order 0.3: ReLU then cuts a visible share of every branch (synth's 0.02 would cut exactly half)
        if k.endswith(".gn.bias"):
            sd[k] = sd[k] * 15.0
    return sd


def model_config(kind, depth=DEPTH):
    """The preset of `kind` at reduced depth with the taps inside it, dropout and LoRA dropout zero (as the fixture's reference models)."""
    from vfmseg_amd import presets
    cfg = {"lora": presets.dinov2_segformer, "rein": presets.rein_dinov2_segformer, "frozen": presets.frozen_dinov2_segformer}[kind](depth=depth)
    cfg["backbone"]["out_indices"] = list(range(4)) if depth >= 4 else [min(i, depth - 1) for i in range(4)]
    cfg["backbone"].pop("init_cfg", None)
    if kind == "lora":
        cfg["Lora_config"]["lora_dropout"] = 0.0
    cfg["decode_head"]["dropout_ratio"] = 0.0
    return cfg


def model_state_dict(kind, depth=DEPTH):
    if kind == "lora":
        sd = {k: v for k, v in full_state_dict(depth).items() if k.startswith("backbone.")}
    elif kind == "rein":
        sd = {"backbone." + k: v for k, v in rein_backbone_state_dict(depth).items()}
    else:
        sd = {"backbone." + k: v for k, v in bare_dinov2_state_dict(depth).items()}
    sd.update(head_state_dict())
    return sd


def head_feats(seed=HEAD_SEED, b=2, dim=1024, h=32, w=32):
    """four [b, dim, h, w] taps; the later taps are louder, as the residual stream of a ViT grows with depth"""
    g = torch.Generator().manual_seed(seed)
    return [(1.0 + 0.5 * i) * torch.randn(b, dim, h, w, generator=g) for i in range(4)]


def head_forward(sd, feats, dtype=torch.float64, groups=32, eps=1e-5, prefix="", drop=None):
    """SegformerHead.forward (eval mode, or train mode with dropout 0) on NCHW taps of one size: NCHW logits.  `drop` removes one term:
    'relu' (no activation in the branches), 'fusion_gn' (no norm after the fusion conv)."""
    p = {k[len(prefix):]: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    outs = []
    for i, x in enumerate(feats):
        y = F.conv2d(x.to(dtype), p[f"convs.{i}.conv.weight"])
        y = F.group_norm(y, groups, p[f"convs.{i}.gn.weight"], p[f"convs.{i}.gn.bias"], eps)
        y = y if drop == "relu" else F.relu(y)
        if y.shape[2:] != feats[0].shape[2:]:
            y = F.interpolate(y, size=feats[0].shape[2:], mode="bilinear", align_corners=False)
        outs.append(y)
    y = F.conv2d(torch.cat(outs, 1), p["fusion_conv.conv.weight"])
    if drop != "fusion_gn":
        y = F.group_norm(y, groups, p["fusion_conv.gn.weight"], p["fusion_conv.gn.bias"], eps)
    y = F.relu(y)
    return F.conv2d(y, p["conv_seg.weight"], p["conv_seg.bias"])


def head_loss(logits, label, ignore_index=255):
    """BaseDecodeHead.loss_by_feat: bilinear resize to the label, CE averaged over ALL pixels (ignored ones add 0), mmseg `accuracy`."""
    lab = label.squeeze(1)
    up = F.interpolate(logits, size=lab.shape[1:], mode="bilinear", align_corners=False)
    loss = F.cross_entropy(up, lab, reduction="none", ignore_index=ignore_index).mean()
    valid = lab != ignore_index
    correct = (up.argmax(1) == lab)[valid].to(logits.dtype).sum()
    acc = correct * (100.0 / (valid.sum() + torch.finfo(torch.float32).eps))
    return loss, acc


def head_ref_grads(sd, feats, label, dtype=torch.float64):
    """(logits, loss, acc, {param: grad}, [tap grads]) of the restatement under autograd."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    taps = [t.detach().to(dtype).requires_grad_(True) for t in feats]
    logits = head_forward(p, taps, dtype)
    loss, acc = head_loss(logits, label)
    loss.backward()
    return logits.detach(), loss.detach(), acc.detach(), {k: v.grad for k, v in p.items()}, [t.grad for t in taps]
