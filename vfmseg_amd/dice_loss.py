"""mmseg 1.2.2 DiceLoss (losses/dice_loss.py) on the fused loss path.

With v = bilinear_up(logits) [B,C,H,W], p = sigmoid(v) or softmax(v, dim=1) and t = one_hot(clamp(label, 0, C), C + 1)[..., :C] - a label
of 255, or any label >= C, is an all-zero row whose pixel stays in the sums of p; the module's `ignore_index` names a class CHANNEL that is
dropped from p and t, not a label - per image n, over all classes and pixels:

    a = sum p t;   b = sum p^2 + eps, c = sum t + eps, d = 2a / (b + c)     (naive_dice: b = sum p, c = sum t, d = (2a + eps) / (b + c + eps))
    loss = loss_weight * mean_n (1 - d_n)

VFMSEG_DICE_FUSED=1 (default) runs three HIP launches that never hold the [B,C,H,W] logits (ops.upsample_dice); =0 composes the same loss
from ops.resize_bilinear, torch's softmax / sigmoid and torch autograd on the full-resolution tensor, as mmseg writes it (cross-check and
timing partner)."""
import os

import torch
import torch.nn as nn

from . import functional as Fh
from . import ops
from .registry import MODELS

ACC_EPS = 2.0 ** -23   # torch.finfo(torch.float32).eps: mmseg `accuracy`


def fused_default():
    return os.environ.get("VFMSEG_DICE_FUSED", "1") != "0"


class _UpsampleFn(torch.autograd.Function):
    """[B,h,w,C] fp32 -> bilinear (align_corners=False) NCHW [B,C,H,W]: the composed form's first step, with the adjoint through ATen."""

    @staticmethod
    def forward(ctx, logits_nhwc, size):
        lg = logits_nhwc.contiguous()
        B, h, w, C = lg.shape
        full = torch.empty(B, C, size[0], size[1], dtype=torch.float32, device=lg.device)
        ops.resize_bilinear(lg, False, B, h, w, C, full, 1, tuple(size))
        ctx.geo = (B, C, h, w, int(size[0]), int(size[1]))
        return full

    @staticmethod
    def backward(ctx, dfull):
        B, C, h, w, H, W = ctx.geo
        d = torch.ops.aten.upsample_bilinear2d_backward(dfull.contiguous(), [H, W], [B, C, h, w], False, None, None)
        return d.permute(0, 2, 3, 1).contiguous(), None


def composed(logits_nhwc, label, use_sigmoid, naive, eps, drop_class, loss_weight, ignore_label=255):
    """(loss, acc_seg) as mmseg computes them, on the full-resolution logits (they, their activation and both gradients live in memory)."""
    B, h, w, C = logits_nhwc.shape
    full = _UpsampleFn.apply(logits_nhwc, tuple(label.shape[1:]))
    p = torch.sigmoid(full) if use_sigmoid else torch.softmax(full, dim=1)
    t = torch.nn.functional.one_hot(torch.clamp(label, 0, C), C + 1)[..., :C].permute(0, 3, 1, 2).to(p.dtype)
    if 0 <= drop_class < C:
        keep = [c for c in range(C) if c != drop_class]
        p, t = p[:, keep], t[:, keep]
    p, t = p.reshape(B, -1), t.reshape(B, -1)
    a = (p * t).sum(1)
    if naive:
        d = (2 * a + eps) / (p.sum(1) + t.sum(1) + eps)
    else:
        d = 2 * a / ((p * p).sum(1) + eps + t.sum(1) + eps)
    loss = loss_weight * (1 - d).mean()
    with torch.no_grad():
        valid = label != ignore_label
        hits = ((full.argmax(1) == label) & valid).sum().to(torch.float32)
        acc = (hits * (100.0 / (valid.sum().to(torch.float32) + ACC_EPS))).view(1)
    return loss, acc


@MODELS.register_module()
class DiceLoss(nn.Module):
    """mmseg 1.2.2 DiceLoss(use_sigmoid, activate, reduction, naive_dice, loss_weight, ignore_index, eps, loss_name); reduction 'mean' with the
    activation inside the loss.  `ignore_index` is a class channel (255 with up to 32 classes: none)."""

    def __init__(self, use_sigmoid=True, activate=True, reduction="mean", naive_dice=False, loss_weight=1.0, ignore_index=255, eps=1e-3,
                 loss_name="loss_dice"):
        super().__init__()
        if not activate:
            raise NotImplementedError("DiceLoss: activate=False (probabilities handed in by the caller) is not on the HIP path: the kernels "
                                      "activate the up-sampled logits in registers")
        if reduction != "mean":
            raise NotImplementedError(f"DiceLoss: reduction={reduction!r}: only reduction='mean' (the mean over the images) is implemented")
        self.use_sigmoid, self.naive_dice = bool(use_sigmoid), bool(naive_dice)
        self.loss_weight, self.eps, self._loss_name = loss_weight, float(eps), loss_name
        self.ignore_index = ignore_index
        self.fused = fused_default()

    @property
    def loss_name(self):
        return self._loss_name

    def drop_class(self, num_classes):
        """The class channel left out of the sums, or -1."""
        ii = self.ignore_index
        return int(ii) if ii is not None and 0 <= ii < num_classes else -1

    def loss_lowres(self, logits_nhwc, label, ignore_label=255):
        """(loss, acc_seg) on NHWC logits at any resolution up to the label's; ignore_label is the label the ACCURACY skips."""
        C = logits_nhwc.shape[-1]
        if C == 1:
            raise NotImplementedError("DiceLoss: out_channels == 1 (mmseg's binary form, which skips the one-hot expansion) is not implemented")
        args = (self.use_sigmoid, self.naive_dice, self.eps, self.drop_class(C), self.loss_weight, ignore_label)
        if self.fused:
            return Fh.UpsampleDiceFn.apply(logits_nhwc, label, *args)
        return composed(logits_nhwc, label, *args)

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, ignore_index=255, **kw):
        """pred NCHW fp32 at label resolution (API parity, as CrossEntropyLoss.forward); the heads use the low-resolution path instead.
        The `ignore_index` argument is unused, as in mmseg."""
        if weight is not None or avg_factor is not None:
            raise NotImplementedError("DiceLoss.forward: weight= / avg_factor= (per-image weights) are not implemented")
        if reduction_override not in (None, "mean"):
            raise NotImplementedError(f"DiceLoss.forward: reduction_override={reduction_override!r}: only 'mean' is implemented")
        lg = torch.empty(pred.shape[0], pred.shape[2], pred.shape[3], pred.shape[1], dtype=torch.float32, device=pred.device)
        ops.permute_copy(pred.detach(), (0, 2, 3, 1), lg)
        label = (target.squeeze(1) if target.dim() == 4 else target).contiguous()
        return self.loss_lowres(lg, label)[0]
