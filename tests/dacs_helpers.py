"""Float64 torch restatements of the DACS glue (rein/models/uda/dacs.py:264-299, dacs_transforms.py:96-126) that tests/test_dacs_*.py compare
the HIP kernels and the DACS segmentor against.  Nothing here touches the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

BAND = 1e-5   # pixels whose float64 decision margin is below this may fall either way in fp32

# ---- the recipe of tests/golden/dacs.npz (tools/gen_dacs_golden.py drives the reference's DACS.forward_train with it)
SRC_SEED, TGT_SEED, PY_SEED, NP_SEED = 61, 67, 7, 89          # synth_image / synth_label seeds, random.seed, np.random.seed (89: of seeds 0..199 the one whose class draws leave the most unmixed pixels in the ignore rows in both iterations; with 11 the rows moved loss_tgt by 9.7 % at iteration 1)
SIZE, BATCH, IGNORE_TOP, IGNORE_BOTTOM, ALPHA = 512, 2, 15, 120, 0.999
OPTIM = dict(type="AdamW", lr=3e-4, weight_decay=0.0, eps=1.0, betas=(0.9, 0.999))   # eps 1: the first update is smooth in the gradient; lr 3e-4 keeps iteration 1 near the threshold chosen at iteration 0 (at 1e-2 the ratio left the band, 0.70 -> 0.92; at 1e-3 the ignore rows moved loss_tgt by 9.8 %, under the 10 % the fixture must show)
SUB = 8                                                        # label maps are recorded at every SUB-th row and column
LOG_KEYS = ("total_loss", "decode.loss_src", "decode.acc_src", "decode.loss_tgt", "decode.acc_tgt")


def dacs_config(pseudo_threshold, depth=None):
    """The Rein DINOv2 + SegformerHead DACS model of the fixture: the preset at reduced depth, dropout zero, the fixture's ignore rows."""
    from tests import segformer_helpers as S
    from vfmseg_amd import presets
    cfg = S.model_config("rein", S.DEPTH if depth is None else depth)
    uda = presets.uda_rein_dinov2_segformer()
    cfg.update({k: uda[k] for k in uda if k not in cfg or k == "type"})
    cfg.update(pseudo_threshold=float(pseudo_threshold), pseudo_weight_ignore_top=IGNORE_TOP, pseudo_weight_ignore_bottom=IGNORE_BOTTOM,
               alpha=ALPHA, blur=False, color_jitter_probability=1.0)
    return cfg


def dacs_state_dict():
    """The weights of the fixture: tests/segformer_helpers' Rein model with conv_seg scaled by 0.01.  The synthetic head's logits have a standard
    deviation of 23, which saturates every softmax (median max-probability 1.0: no threshold could split the pixels).  At a hundredth the
    softmax is flat enough that a pseudo-labelled pixel costs about as much as a source-labelled one (both near log 19); only then does the
    pseudo-weighted part of loss_tgt - and with it the ignore rows - carry a tenth of the loss (at a tenth of the scale the rows moved it
    by 1.7 %)."""
    from tests import segformer_helpers as S
    sd = S.model_state_dict("rein")
    for k in ("decode_head.conv_seg.weight", "decode_head.conv_seg.bias"):
        sd[k] = sd[k] * 0.01
    return sd


def upsample_ce_w(logits_nhwc, label, weight=None, ignore_index=255):
    """mmseg CrossEntropyLoss(weight=seg_weight, reduction='mean', avg_non_ignore=False) on bilinear-upsampled logits, float64:
    (loss, d loss / d logits_nhwc, [hits, valid]).  The counters are unweighted."""
    lg = logits_nhwc.detach().double().requires_grad_(True)
    up = F.interpolate(lg.permute(0, 3, 1, 2), size=label.shape[1:], mode="bilinear", align_corners=False)
    per = F.cross_entropy(up, label, reduction="none", ignore_index=ignore_index)
    if weight is not None:
        per = per * weight.double()
    loss = per.mean()
    loss.backward()
    valid = label != ignore_index
    hits = int(((up.argmax(1) == label) & valid).sum())
    return loss.item(), lg.grad, [hits, int(valid.sum())]


def teacher_probs(logits_nhwc, size):
    """float64 softmax of the bilinear-upsampled teacher logits, [B,C,H,W] (predict_by_feat + torch.softmax)."""
    up = F.interpolate(logits_nhwc.double().permute(0, 3, 1, 2), size=tuple(size), mode="bilinear", align_corners=False)
    return torch.softmax(up, dim=1)


def pseudo_labels(logits_nhwc, size, thr):
    """-> dict(label, prob, count, sure_label [bool: top-2 margin >= BAND], n_band [pixels with |max prob - thr| < BAND]), float64."""
    sm = teacher_probs(logits_nhwc, size)
    top2 = sm.topk(2, dim=1).values
    prob, label = torch.max(sm, dim=1)
    return dict(label=label, prob=prob, count=int((prob >= thr).sum()), sure_label=(top2[:, 0] - top2[:, 1]) >= BAND,
                n_band=int(((prob - thr).abs() < BAND).sum()))


def class_sets(label):
    """per image the sorted list of label values present (torch.unique; the ignore label is a class)."""
    return [torch.unique(l).tolist() for l in label]


def draw_classes(class_lists):
    """get_class_masks' draw: np.random.choice(n, int((n + n % 2) / 2), replace=False) per image, over the sorted classes."""
    out = []
    for classes in class_lists:
        n = len(classes)
        pick = np.random.choice(n, int((n + n % 2) / 2), replace=False)
        out.append([int(classes[int(i)]) for i in pick])
    return out


def class_masks(label, chosen):
    """generate_class_mask per image: int64 [B,H,W], 1 where the label's class is chosen."""
    return torch.stack([torch.isin(l, torch.tensor(c, dtype=torch.int64)) for l, c in zip(label, chosen)]).long()


def class_mix(src_img, tgt_img, src_lbl, pseudo_lbl, mask, count, total, ignore_top, ignore_bottom):
    """one_mix three times + the pseudo-weight set-up (dacs.py:270-299), with the reference's own formulas in the input dtypes:
    (mixed_img, mixed_lbl, mix_weight).  ratio is the Python double count / total, cast to fp32 when it multiplies the fp32 ones."""
    ratio = count / total
    pseudo_weight = ratio * torch.ones(pseudo_lbl.shape)
    if ignore_top > 0:
        pseudo_weight[:, :ignore_top, :] = 0
    if ignore_bottom > 0:
        pseudo_weight[:, -ignore_bottom:, :] = 0
    gt_weight = torch.ones_like(pseudo_weight)
    m = mask.unsqueeze(1)
    return m * src_img + (1 - m) * tgt_img, mask * src_lbl + (1 - mask) * pseudo_lbl, mask * gt_weight + (1 - mask) * pseudo_weight


def ema(teacher, student, it, alpha):
    """_update_ema in float64."""
    a = min(1 - 1 / (it + 1), alpha)
    return a * teacher.double() + (1 - a) * student.double()
