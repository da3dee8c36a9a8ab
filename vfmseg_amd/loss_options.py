"""The loss options of the decode heads' fused cross-entropy: mmseg 1.2.2's OHEMPixelSampler (thresh branch),
CrossEntropyLoss(class_weight=, avg_non_ignore=).

Every option becomes a per-pixel fp32 weight map [B,H,W] plus one device scalar: the map goes through the weighted loss kernels
(vfm_upsample_ce_w), the scalar B*H*W / (avg_factor + eps) rescales their loss and gradient (functional.UpsampleCENormFn).  With

    p_i = softmax(bilinear_up(logits))_i[y_i],  n = #valid,  k = min(min_kept * B, n - 1),  t = max(sorted valid p [k], thresh)  (thresh if n == 0)
    w_i = [valid and p_i < t] * class_weight[y_i]          avg_factor = sum_valid class_weight[y_i]  |  n (avg_non_ignore)  |  B*H*W
    loss = loss_weight * sum_i w_i * -log p_i / (avg_factor + 2^-23)

VFMSEG_OHEM_FUSED=1 (default) builds the map with three HIP passes at label resolution that never hold the [B,C,H,W] logits (ops.ohem_weight /
ops.label_weight: k, n, t and the normaliser stay on the device, no host read); =0 composes the same map from ops.resize_bilinear,
torch.softmax, gather and torch.sort as mmseg writes it (cross-check and timing partner; it synchronises)."""
import os

import torch

from . import functional as Fh
from . import ops
from .registry import MODELS

EPS = 2.0 ** -23


def fused_default():
    return os.environ.get("VFMSEG_OHEM_FUSED", "1") != "0"


@MODELS.register_module()
class OHEMPixelSampler:
    """mmseg OHEMPixelSampler(context, thresh, min_kept): keep the valid pixels whose probability of their label is below
    t = max(thresh, the (min_kept * batch)-th smallest such probability): at least min_kept per image are kept when there are that many.
    Sampling is per batch, per rank, on detached logits."""

    def __init__(self, context, thresh=None, min_kept=100000):
        if thresh is None:
            raise NotImplementedError("OHEMPixelSampler: thresh=None (the branch that ranks pixels by their loss) is not on the HIP path; "
                                      "set thresh (mmseg's configs use thresh=0.7)")
        assert min_kept > 1
        self.context, self.thresh, self.min_kept = context, float(thresh), int(min_kept)
        self.fused = fused_default()

    def sample_lowres(self, logits_nhwc, label):
        """logits fp32 [B,h,w,C] (any resolution up to the label's), label int64 [B,H,W] -> weight fp32 [B,H,W] of zeros and ones."""
        weight, _, _ = pixel_weights(logits_nhwc, label, self.context.ignore_index, sampler=self)
        return weight

    def sample(self, seg_logit, seg_label):
        """mmseg's signature: seg_logit NCHW at label size, seg_label [B,1,H,W] -> seg_weight [B,H,W]."""
        B, C, H, W = seg_logit.shape
        lg = torch.empty(B, H, W, C, dtype=torch.float32, device=seg_logit.device)
        ops.permute_copy(seg_logit.detach(), (0, 2, 3, 1), lg)
        label = (seg_label.squeeze(1) if seg_label.dim() == 4 else seg_label).contiguous()
        return self.sample_lowres(lg, label)


def _composed(lg, label, ignore_index, sampler, class_weight, avg_non_ignore, pix_weight):
    """The map and normaliser as mmseg computes them, on the full-resolution logits."""
    B, h, w, C = lg.shape
    H, W = label.shape[1:]
    valid = label != ignore_index
    lab0 = torch.where(valid, label, torch.zeros_like(label))
    weight = valid.to(torch.float32)
    info = {}
    if sampler is not None:
        full = torch.empty(B, C, H, W, dtype=torch.float32, device=lg.device)
        ops.resize_bilinear(lg, False, B, h, w, C, full, 1, (H, W))
        p = torch.softmax(full, dim=1).gather(1, lab0.unsqueeze(1)).squeeze(1)
        pv = p[valid]
        t = torch.full((1,), sampler.thresh, dtype=torch.float32, device=lg.device)
        if pv.numel() > 0:
            s, _ = pv.sort()
            t = torch.clamp(s[min(sampler.min_kept * B, pv.numel() - 1)], min=sampler.thresh).view(1)
        weight = weight * (p < t).to(torch.float32)
        info.update(p=torch.where(valid, p, torch.full_like(p, -1.0)), t=t)
    norm = None
    if class_weight is not None:
        cw = class_weight[lab0] * valid
        weight = weight * cw
        avg = cw.double().sum()
    elif avg_non_ignore:
        avg = valid.sum().double()
    if class_weight is not None or avg_non_ignore:
        norm = torch.stack([label.numel() / (avg + EPS), avg]).to(torch.float32)
    if pix_weight is not None:
        weight = weight * pix_weight
    return weight.contiguous(), norm, info


def pixel_weights(logits_nhwc, label, ignore_index, sampler=None, class_weight=None, avg_non_ignore=False, pix_weight=None):
    """(weight fp32 [B,H,W] or None (all ones), norm fp32 [2] on the device or None (the mean over all pixels stands), info) for the options
    given: sampler an OHEMPixelSampler, class_weight fp32 [C] on the device, pix_weight fp32 [B,H,W] (mmseg's `weight=`)."""
    lg = logits_nhwc.detach().contiguous()
    B, C = lg.shape[0], lg.shape[-1]
    need_norm = class_weight is not None or avg_non_ignore
    fused = sampler.fused if sampler is not None else fused_default()
    if not fused:
        return _composed(lg, label, ignore_index, sampler, class_weight, avg_non_ignore, pix_weight)
    if sampler is not None:
        weight, p, t, state, norm, counts = ops.ohem_weight(lg, label, sampler.thresh, sampler.min_kept * B, ignore_index, class_weight,
                                                            pix_weight, avg_non_ignore, want_norm=need_norm)
        return weight, norm, dict(p=p, t=t, state=state, counts=counts)
    want_weight = class_weight is not None or pix_weight is not None
    weight, norm, counts = ops.label_weight(label, C, None, None, class_weight, pix_weight, ignore_index, avg_non_ignore,
                                            want_weight=want_weight, want_norm=need_norm)
    return weight, norm, dict(counts=counts)


def loss_with_options(logits_nhwc, label, ignore_index, loss_weight, sampler=None, class_weight=None, avg_non_ignore=False, pix_weight=None):
    """(loss, acc_seg) of the fused low-resolution cross-entropy under the options.  With none of them this is what the heads called before
    the options existed, untouched: UpsampleCEFn, or UpsampleCEWeightedFn for a pixel weight alone."""
    if pix_weight is not None:
        pix_weight = pix_weight.float().contiguous()
    if sampler is None and class_weight is None and not avg_non_ignore:
        if pix_weight is None:
            return Fh.UpsampleCEFn.apply(logits_nhwc, label, ignore_index, loss_weight)
        return Fh.UpsampleCEWeightedFn.apply(logits_nhwc, label, pix_weight, ignore_index, loss_weight)
    weight, norm, _ = pixel_weights(logits_nhwc, label, ignore_index, sampler, class_weight, avg_non_ignore, pix_weight)
    if norm is None:
        return Fh.UpsampleCEWeightedFn.apply(logits_nhwc, label, weight, ignore_index, loss_weight)
    return Fh.UpsampleCENormFn.apply(logits_nhwc, label, weight, norm, ignore_index, loss_weight)
