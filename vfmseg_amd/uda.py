"""DACS self-training (rein/models/uda/dacs.py:40-365, dacs_transforms.py:96-126) on the HIP path: an EMA teacher head, pseudo-labels from
its logits, a ClassMix of source and target, a per-pixel-weighted cross-entropy on the mixed image, two backward passes into one optimiser step.

Per step (the reference's order): EMA init / update -> source forward + backward -> target features from the STUDENT backbone under no_grad
through the teacher head with dropout off -> pseudo-labels and the confident-pixel ratio -> class masks -> mix -> mixed forward + backward
with mix_weight -> one optimiser step, zero_grad.

VFMSEG_DACS_FUSED=1 (default) runs the glue as three HIP passes (vfm_pseudo_label, vfm_class_presence, vfm_class_mix: the full-resolution
teacher logits never exist and the ratio never visits the host); =0 composes the same steps from ops.resize_bilinear and torch, as the
reference writes them (cross-check and A/B partner).  Both forms take the loss through vfm_upsample_ce_w.

Out of scope, each refused with an error: colour jitter / Gaussian blur (the reference's kornia import is commented out, so those branches
raise NameError there), cut_mix, HRDAHead / Mask2Former heads, AmpOptimWrapper and data parallelism, the debug figure."""
import os
import random
from copy import deepcopy

import numpy as np
import torch

from . import ops
from .registry import MODELS
from .segmentors import EncoderDecoder

_KEYS = ("alpha", "pseudo_threshold", "pseudo_weight_ignore_top", "pseudo_weight_ignore_bottom", "mix", "blur", "color_jitter_strength",
         "color_jitter_probability", "debug_img_interval", "print_grad_magnitude")
_HEADS = ("SegformerHead", "LinearHead")


def fused_default():
    return os.environ.get("VFMSEG_DACS_FUSED", "1") != "0"


def choose_classes(class_lists):
    """get_class_masks' host draw (dacs_transforms.py:96-105): per image np.random.choice(n, int((n + n % 2) / 2), replace=False) over the
    sorted present classes.  -> per image the list of chosen classes."""
    out = []
    for classes in class_lists:
        n = len(classes)
        pick = np.random.choice(n, int((n + n % 2) / 2), replace=False)
        out.append([int(classes[int(i)]) for i in pick])
    return out


@MODELS.register_module()
class DACS(EncoderDecoder):
    _full_finetune_ok = False   # a bare DinoVisionTransformer in train() mode is refused by name (EncoderDecoder._tokens)

    def __init__(self, **cfg):
        missing = [k for k in _KEYS if k not in cfg]
        if missing:
            raise KeyError(f"DACS: missing config keys {missing}")
        if cfg["blur"] or cfg["color_jitter_probability"] < 1:
            raise NotImplementedError("DACS: blur and color_jitter_probability: Gaussian blur and colour jitter are not on the HIP path (the reference's "
                                      "kornia branches cannot run either); set blur=False and color_jitter_probability >= 1")
        if cfg["mix"] != "class":
            raise NotImplementedError(f"DACS: mix={cfg['mix']!r}: only the class mix (one_mix over get_class_masks) is on the HIP path, cut_mix is not")
        head_type = dict(cfg["decode_head"]).get("type")
        if head_type not in _HEADS:
            raise NotImplementedError(f"DACS: decode_head type {head_type!r}: the self-training loop runs with {' / '.join(_HEADS)} "
                                      "(HRDAHead and Mask2Former heads are not on this path)")
        if dict(cfg["decode_head"]).get("sampler") is not None:
            raise NotImplementedError("DACS: decode_head sampler=: the mixed-image loss passes seg_weight (the pseudo-label weight), and a pixel "
                                      "sampler would set the same weights (mmseg lets the sampler overwrite them); remove the sampler")
        ld = dict(cfg["decode_head"]).get("loss_decode")
        if isinstance(ld, (list, tuple)) or (isinstance(ld, dict) and ld.get("type") == "DiceLoss"):
            raise NotImplementedError("DACS: decode_head loss_decode list / DiceLoss: the mixed-image loss passes seg_weight (the pseudo-label "
                                      "weight), which mmseg's DiceLoss cannot take; the self-training loop runs with one CrossEntropyLoss")
        super().__init__(backbone=cfg["backbone"], decode_head=cfg["decode_head"], train_cfg=cfg.get("train_cfg"),
                         test_cfg=cfg.get("test_cfg"), data_preprocessor=cfg.get("data_preprocessor"))
        self.local_iter = 0   # a plain attribute, as in the reference: a resumed run starts at 0 and re-initialises the teacher from the student
        self.alpha = cfg["alpha"]
        self.pseudo_threshold = cfg["pseudo_threshold"]
        self.psweight_ignore_top = cfg["pseudo_weight_ignore_top"]
        self.psweight_ignore_bottom = cfg["pseudo_weight_ignore_bottom"]
        self.mix = cfg["mix"]
        self.blur = cfg["blur"]
        self.color_jitter_s = cfg["color_jitter_strength"]
        self.color_jitter_p = cfg["color_jitter_probability"]
        self.debug_img_interval = cfg["debug_img_interval"]     # accepted; the debug figure is not drawn
        self.print_grad_magnitude = cfg["print_grad_magnitude"]
        self.work_dir = cfg.get("work_dir")
        self.mean = self.std = None
        self.ema_head = MODELS.build(deepcopy(cfg["decode_head"]))
        self.ema_head.requires_grad_(False)   # (the reference does this at iteration 0; here the optimiser must never own the teacher)
        self.ema_head.dropout_ratio = 0.0     # dacs.py:254-258 turns the teacher's dropout modules off and nothing else
        self.fused = fused_default()
        self.keep_mask = False                # tests / tools: also write the mix mask in the fused form
        self._ema_flat = None
        self._ema_src = None
        self._count = None
        self._last = {}

    # ---- teacher
    def get_ema_model(self):
        return self.ema_head

    def get_model(self):
        return self

    def _student_slice(self, optim_wrapper):
        """The decode head's contiguous slice of FusedAdamW.flat, and the (name, offset in the slice, size) of its parameters."""
        opt = getattr(optim_wrapper, "optimizer", None)
        if opt is None or not hasattr(opt, "bucket_slices"):
            raise TypeError("DACS: the EMA teacher mirrors the decode head's slice of FusedAdamW's flat parameter buffer; "
                            f"got optimiser {type(opt).__name__}")
        cuts = [c for c in opt.bucket_slices() if c[0] == "decode_head"]
        assert len(cuts) == 1, cuts
        _, a, b = cuts[0]
        lay = [(n, o - a, s) for n, o, s in zip(opt.names, opt.offsets[:-1], opt.sizes) if a <= o < b]
        stray = [n for n, _, _ in lay if not n.startswith("decode_head.")]
        if stray:
            raise NotImplementedError(f"DACS: trainable parameters outside decode_head in its gradient bucket: {stray[:3]}")
        return opt.flat[a:b], lay

    def _init_ema_weights(self, optim_wrapper):
        """Teacher <- student (dacs.py:117-129).  The teacher's parameters are re-pointed into ONE flat fp32 buffer laid out like the student
        head's slice of the optimiser's flat buffer, so that the update is one axpby."""
        src, lay = self._student_slice(optim_wrapper)
        named = dict(self.ema_head.named_parameters())
        want = {"decode_head." + n for n in named}
        assert want == {n for n, _, _ in lay}, "teacher / student parameter sets differ"
        if self._ema_flat is None or self._ema_flat.numel() != src.numel() or self._ema_flat.device != src.device:
            self._ema_flat = torch.zeros_like(src)
            for n, o, s in lay:
                p = named[n[len("decode_head."):]]
                p.requires_grad_(False)
                p.data = self._ema_flat[o:o + s].view(p.shape)
        self._ema_src = src
        self._ema_flat.copy_(src)
        self._teacher_changed()

    def _update_ema(self, it):
        """teacher = a * teacher + (1 - a) * student, a = min(1 - 1 / (it + 1), alpha) (dacs.py:131-143): one launch over the flat buffers."""
        a = min(1 - 1 / (it + 1), self.alpha)
        ops.axpby(self._ema_src, 1 - a, self._ema_flat, a)
        self._teacher_changed()

    @staticmethod
    def _teacher_changed():
        from .optim import PARAM_EPOCH
        PARAM_EPOCH[0] += 1   # the weight-pack caches key on it: the teacher's weights changed behind torch's version counters

    def _teacher_logits(self, target_img):
        """Low-resolution teacher logits NHWC [B,h,w,C] of the target image: student backbone (as it is: train mode), teacher head, no_grad."""
        from . import backbones
        pending = backbones._PENDING_BACKWARD[0]
        with torch.no_grad():
            fp = self.extract_feat(target_img)
            lg = self.ema_head.forward_tokens(fp).contiguous()
        backbones._PENDING_BACKWARD[0] = pending   # that forward will never see its backward
        return lg

    # ---- one loss + backward (dacs.py:151-181)
    def train_and_update(self, optim_wrapper, log_vars, img, seg_label, seg_weight=None, suffix=""):
        fp = self.extract_feat(img)
        logits = self.decode_head.forward_tokens(fp)
        loss = self.decode_head.loss_by_feat(logits, seg_label, seg_weight)
        parsed, log = self.parse_losses(loss)
        log_vars["total_loss"] = log_vars["total_loss"] + parsed.detach()
        log_vars[f"decode.loss_{suffix}"] = log[self.decode_head.loss_decode.loss_name].detach()
        log_vars[f"decode.acc_{suffix}"] = log["acc_seg"].detach().reshape(())
        optim_wrapper.backward(optim_wrapper.scale_loss(parsed))

    def train_step(self, data, optim_wrapper):
        from .optim import AmpOptimWrapper
        if isinstance(optim_wrapper, AmpOptimWrapper) or getattr(optim_wrapper, "grad_sync", None) is not None:
            raise NotImplementedError("DACS: --amp (AmpOptimWrapper) and data parallelism are not supported: two backward passes per step do not "
                                      "fit the loss scaler's and GradSync's one-backward step")
        if getattr(optim_wrapper, "_accumulative_counts", 1) != 1:
            raise NotImplementedError(f"DACS: optim_wrapper.accumulative_counts={optim_wrapper._accumulative_counts} has no meaning here: the "
                                      "reference's DACS.train_step calls step() and zero_grad() unconditionally after its two backward "
                                      "passes (clip_grad works: it is applied inside step())")
        self.mean, self.std = self.data_preprocessor.mean, self.data_preprocessor.std
        img = self.data_preprocessor(data["img"], True)
        target_img = self.data_preprocessor(data["target_img"], True)
        log_vars = self.forward_train(img, target_img, optim_wrapper)
        optim_wrapper.step()
        optim_wrapper.zero_grad()
        return log_vars

    def forward_train(self, img_dict, target_img_dict, optim_wrapper=None):
        img, target_img = img_dict["inputs"], target_img_dict["inputs"]
        B, _, H, W = img.shape
        assert target_img.shape == img.shape, "source and target crops share one size"
        dev = img.device
        gt = torch.stack([s.gt_sem_seg.data for s in img_dict["data_samples"]]).to(dev)   # [B,1,H,W]
        gt_lbl = gt.reshape(B, H, W).contiguous()
        fused = self.fused
        log_vars = {"total_loss": torch.zeros((), device=dev)}

        if self.local_iter == 0:
            self._init_ema_weights(optim_wrapper)
        if self.local_iter > 0:
            self._update_ema(self.local_iter)

        # host draws in the reference's order (dacs.py:238-246); neither value is used: jitter and blur are off
        random.uniform(0, 1)
        _ = random.uniform(0, 1) if self.blur else 0

        # the class sets leave for the host now, so that the wait at the class-mask step covers nothing of this step's forward / backward work
        if fused:
            bits_host = torch.empty(B, 8, dtype=torch.int32, pin_memory=True)
            bits_host.copy_(ops.class_presence(gt_lbl), non_blocking=True)
            bits_ready = torch.cuda.Event()
            bits_ready.record()

        self.train_and_update(optim_wrapper, log_vars, img, gt, suffix="src")

        ema_logits = self._teacher_logits(target_img)
        total = B * H * W
        if fused:
            if self._count is None or self._count.device != dev:
                self._count = torch.zeros(1, dtype=torch.int32, device=dev)
            count = self._count
            count.zero_()
            pseudo_label, _ = ops.pseudo_label(ema_logits, (H, W), self.pseudo_threshold, count)
            bits_ready.synchronize()
            chosen = choose_classes(ops.class_bits_to_lists(bits_host))
            chosen_bits = ops.class_lists_to_bits(chosen, dev)
            mixed_img, mixed_lbl, mix_weight, mask = ops.class_mix(img, target_img, gt_lbl, pseudo_label, chosen_bits, count, total,
                                                                   self.psweight_ignore_top, self.psweight_ignore_bottom, want_mask=self.keep_mask)
        else:
            pseudo_label, count, mixed_img, mixed_lbl, mix_weight, mask = self._composed_mix(img, target_img, gt_lbl, ema_logits)
        self._last = dict(pseudo_label=pseudo_label, mask=mask, mix_weight=mix_weight, mixed_lbl=mixed_lbl, count=count.clone(), total=total)

        self.train_and_update(optim_wrapper, log_vars, mixed_img, mixed_lbl, mix_weight, suffix="tgt")
        self.local_iter += 1
        return log_vars

    def _composed_mix(self, img, target_img, gt_lbl, ema_logits):
        """Steps 4-6 as the reference writes them, from ops.resize_bilinear and torch: full-resolution logits, softmax, max, the ratio (kept on
        the device), torch.unique class sets, the three one_mix products."""
        B, _, H, W = img.shape
        h, w, C = ema_logits.shape[1:]
        full = torch.empty(B, C, H, W, dtype=torch.float32, device=img.device)
        ops.resize_bilinear(ema_logits, False, B, h, w, C, full, 1, (H, W))
        pseudo_prob, pseudo_label = torch.max(torch.softmax(full, dim=1), dim=1)
        count = pseudo_prob.ge(self.pseudo_threshold).sum().to(torch.int32).reshape(1)
        ratio = (count.double() / float(B * H * W)).float()
        pseudo_weight = ratio * torch.ones(pseudo_prob.shape, device=img.device)
        if self.psweight_ignore_top > 0:
            pseudo_weight[:, :self.psweight_ignore_top, :] = 0
        if self.psweight_ignore_bottom > 0:
            pseudo_weight[:, -self.psweight_ignore_bottom:, :] = 0
        chosen = choose_classes([torch.unique(l).cpu().tolist() for l in gt_lbl])
        mask = torch.stack([torch.isin(l, torch.tensor(c, dtype=torch.int64, device=l.device)) for l, c in zip(gt_lbl, chosen)]).long()
        m_img = mask.unsqueeze(1)
        mixed_img = m_img * img + (1 - m_img) * target_img
        mixed_lbl = mask * gt_lbl + (1 - mask) * pseudo_label
        mix_weight = mask * torch.ones_like(pseudo_weight) + (1 - mask) * pseudo_weight
        return pseudo_label, count, mixed_img.contiguous(), mixed_lbl.contiguous(), mix_weight.contiguous(), mask.to(torch.uint8)
