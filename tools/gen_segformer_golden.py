"""Writes tests/golden/segformer.npz: the SegFormer-head baselines (LoRA / Rein / frozen DINOv2 + SegformerHead) computed by the
REFERENCE's own modules imported through oracle/ref_shim.py - FrozenBackboneEncoderDecoder, LoraBackboneEncoderDecoder,
ReinsDinoVisionTransformer / LoRAReins, DinoVisionTransformer.  Data only: slices, whole-tensor statistics, losses, gradient norms and
parameter names.  Runs where the reference tree exists; the tests read the .npz and tests/segformer_helpers.py only.

    python tools/gen_segformer_golden.py

mmseg is not installed, and the shim's BaseDecodeHead has no `loss`: SegformerHead and BaseDecodeHead.loss (mmseg 1.2.2) are RESTATED
below on the shim's BaseDecodeHead / ConvModule / resize / accuracy - the head is "pinned by restatement", everything around it is the
reference's code.  The generator ASSERTS that the fixture can see the head: every branch, the fusion norm and the ReLU move the logits."""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import segformer_helpers as S  # noqa: E402
from tests.helpers import sl, stats  # noqa: E402
from tests.rein_helpers import bare_dinov2_state_dict  # noqa: E402
from vfmseg_amd import presets  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


class SegformerHead(ref_shim.BaseDecodeHead):
    """mmseg 1.2.2 decode_heads/segformer_head.py, restated."""

    def __init__(self, interpolate_mode="bilinear", **kwargs):
        super().__init__(input_transform="multiple_select", **kwargs)
        self.interpolate_mode = interpolate_mode
        num_inputs = len(self.in_channels)
        assert num_inputs == len(self.in_index)
        self.convs = nn.ModuleList([ref_shim.ConvModule(in_channels=self.in_channels[i], out_channels=self.channels, kernel_size=1, stride=1,
                                                        norm_cfg=self.norm_cfg, act_cfg=self.act_cfg) for i in range(num_inputs)])
        self.fusion_conv = ref_shim.ConvModule(in_channels=self.channels * num_inputs, out_channels=self.channels, kernel_size=1,
                                               norm_cfg=self.norm_cfg)

    def forward(self, inputs):
        inputs = self._transform_inputs(inputs)
        outs = []
        for idx in range(len(inputs)):
            x = inputs[idx]
            conv = self.convs[idx]
            outs.append(ref_shim.resize(input=conv(x), size=inputs[0].shape[2:], mode=self.interpolate_mode, align_corners=self.align_corners))
        out = self.fusion_conv(torch.cat(outs, dim=1))
        return self.cls_seg(out)

    def loss_by_feat(self, seg_logits, seg_label):
        """BaseDecodeHead.loss_by_feat (one loss module, no sampler)."""
        seg_logits = ref_shim.resize(input=seg_logits, size=seg_label.shape[2:], mode="bilinear", align_corners=self.align_corners)
        seg_label = seg_label.squeeze(1)
        loss = {self.loss_decode.loss_name: self.loss_decode(seg_logits, seg_label, weight=None, ignore_index=self.ignore_index)}
        loss["acc_seg"] = ref_shim.accuracy(seg_logits, seg_label, ignore_index=self.ignore_index)
        return loss

    def loss(self, inputs, seg_label, train_cfg=None):
        return self.loss_by_feat(self.forward(inputs), seg_label)


def _models():
    M = ref_shim.load_all()
    ref_shim.ref_import("models.backbones.reins")
    ref_shim.ref_import("models.backbones.reins_dinov2")
    ref_shim.ref_import("models.segmentors.Lora_encoder_decoder")
    ref_shim.ref_import("models.segmentors.frozen_encoder_decoder")
    M.register_module(module=SegformerHead)
    M.register_module(name="EncoderDecoder", module=ref_shim.EncoderDecoder)
    return M


def _zero_dropout(m):
    for mod in m.modules():
        if isinstance(mod, (nn.Dropout, nn.Dropout2d)):
            mod.p = 0.0


def _range_dist(a, b):
    return ((a - b).abs().max() / a.abs().max()).item()


def _grad2d(g):
    return g.reshape(g.shape[0], -1) if g.dim() > 1 else g


# ------------------------------------------------------------------------------------------------ head level (float64)
def gen_head(M, out):
    head = M.build(presets.segformer_head()).double()
    sd = S.head_state_dict(prefix="")
    assert sorted(head.state_dict()) == sorted(S.HEAD_KEYS) == sorted(sd), set(head.state_dict()) ^ set(sd)
    out["head_param_names"] = np.array(sorted(head.state_dict()))
    head.load_state_dict({k: v.double() for k, v in sd.items()})
    head.train()
    _zero_dropout(head)
    feats = [t.double().requires_grad_(True) for t in S.head_feats()]
    lab = synth_label(2, 512, seed=S.HEAD_SEED)
    logits = head.forward(feats)
    losses = head.loss_by_feat(logits, lab)
    losses["loss_ce"].backward()
    out["head::logits_stats"], out["head::logits_slice"] = stats(logits), sl(logits).astype(np.float32)
    out["head::logits_grid"] = logits.detach()[:, :, 3::8, 5::8].numpy().astype(np.float32)
    out["head::loss_acc"] = np.array([losses["loss_ce"].item(), losses["acc_seg"].item()])
    for n, p in head.named_parameters():
        assert p.grad is not None, n
        out[f"head::grad_slice::{n}"] = sl(_grad2d(p.grad)).astype(np.float32)
        out[f"head::grad_norm::{n}"] = np.array([p.grad.norm().item()])
    for i, t in enumerate(feats):
        out[f"head::tap_grad_norm::{i}"] = np.array([t.grad.norm().item()])
        out[f"head::tap_grad_slice::{i}"] = sl(t.grad[:, :, 8:, 8:]).astype(np.float32)
    head.eval()
    with torch.no_grad():
        ev = head.forward([t.detach() for t in feats])
        out["head::eval_logits_stats"], out["head::eval_logits_slice"] = stats(ev), sl(ev).astype(np.float32)
        # what the fixture must be able to see: every branch, the branch ReLU, the fusion norm
        sens = []
        for i in range(4):
            keep = head.convs[i].conv.weight.data.clone()
            head.convs[i].conv.weight.data.mul_(-1.0)
            sens.append(_range_dist(ev, head.forward([t.detach() for t in feats])))
            head.convs[i].conv.weight.data.copy_(keep)
        assert min(sens) >= 0.1, sens
        no_relu = S.head_forward(sd, S.head_feats(), drop="relu")
        no_gn = S.head_forward(sd, S.head_feats(), drop="fusion_gn")
        d_relu, d_gn = _range_dist(ev, no_relu), _range_dist(ev, no_gn)
        assert d_relu >= 0.1 and d_gn >= 0.1, (d_relu, d_gn)
        out["head::sensitivity"] = np.array(sens + [d_relu, d_gn])
        assert _range_dist(ev, S.head_forward(sd, S.head_feats())) < 1e-9, "tests/segformer_helpers.head_forward drifted from the restated head"
    print("head: loss / acc", out["head::loss_acc"], "sensitivity (branch 0-3 sign flip, no ReLU, no fusion GN)", np.round(out["head::sensitivity"], 3))


# ------------------------------------------------------------------------------------------------ segmentors
def build_reference_model(M, kind):
    cfg = S.model_config(kind)
    want = S.model_state_dict(kind)
    if kind == "lora":
        with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
            torch.save(bare_dinov2_state_dict(S.DEPTH), f.name)
            cfg["checkpoint"] = f.name
        model = M.build(cfg)
        os.unlink(cfg["checkpoint"])
    else:
        model = M.build(cfg)
    if kind == "lora":   # the reference wraps the backbone itself (backbone.base_model.model.*), this tree wraps it in a LoRABackbone (backbone.model.base_model.model.*)
        want = {k.replace("backbone.model.base_model.", "backbone.base_model.", 1): v for k, v in want.items()}
    model.load_state_dict(want, strict=False)   # (the Rein backbone's state_dict lists only its `reins` keys)
    have = dict(model.named_parameters())
    have.update(dict(model.named_buffers()))
    assert set(want) <= set(have), sorted(set(want) - set(have))[:6]
    for k, v in want.items():
        assert torch.equal(have[k].detach(), v), k
    return model


def gen_train_step(model, kind, out):
    model.zero_grad()
    model.train()
    _zero_dropout(model)
    img, lab = synth_image(2, 512, seed=S.TRAIN_SEED), synth_label(2, 512, seed=S.TRAIN_SEED)
    feats = model.extract_feat(img)
    if kind == "frozen":
        assert not model.backbone.training and all(not t.requires_grad for t in feats)
    losses = model.decode_head.loss(list(feats), lab)
    losses["loss_ce"].backward()
    k = f"{kind}::"
    out[k + "train_loss_acc"] = np.array([losses["loss_ce"].item(), losses["acc_seg"].item()])
    norms, n_train, nograd = {"backbone": 0.0, "head": 0.0}, 0, []
    ours = (lambda n: n.replace("backbone.base_model.", "backbone.model.base_model.", 1)) if kind == "lora" else (lambda n: n)   # this tree's key names
    for n, p in model.named_parameters():
        n = ours(n)
        if not p.requires_grad:
            assert p.grad is None, n
            continue
        if p.grad is None:
            nograd.append(n)
            continue
        n_train += p.numel()
        norms["head" if n.startswith("decode_head.") else "backbone"] += p.grad.double().pow(2).sum().item()
        if "blocks.0." in n or f"blocks.{S.DEPTH - 1}." in n or n.startswith("decode_head") or ".reins." in n:
            out[k + f"train_grad_slice::{n}"] = sl(_grad2d(p.grad) if p.grad.dim() else p.grad.reshape(1))
            out[k + f"train_grad_norm::{n}"] = np.array([p.grad.double().norm().item()])
    out[k + "train_grad_norms"] = np.sqrt(np.array([norms["backbone"], norms["head"]]))
    out[k + "train_n_trainable"], out[k + "train_no_grad"] = np.array([n_train]), np.array(sorted(nograd))
    out[k + "trainable_names"] = np.array(sorted(ours(n) for n, p in model.named_parameters() if p.requires_grad))
    if kind == "frozen":
        assert norms["backbone"] == 0.0 and all(n.startswith("decode_head.") for n in out[k + "trainable_names"])
    print(kind, "train step: loss / acc", out[k + "train_loss_acc"], "grad norms (backbone, head)", out[k + "train_grad_norms"], "no grad:", nograd)


def _record_logits(out, key, logits):
    top2 = logits.topk(2, dim=1)[0]
    margin = ((top2[:, 0] - top2[:, 1]) / (logits.max() - logits.min()))[0]
    H, W = logits.shape[2:]
    out[key + "logits_stats"] = stats(logits)
    out[key + "logits_grid"] = logits[0, :, 5::64, 5::64].numpy().copy()
    out[key + "logits_slice"] = sl(logits[0, :, H // 2 - 4:, W // 2 - 4:])   # straddles the window seams
    out[key + "pred_sub16"] = logits.argmax(1)[0, ::16, ::16].numpy().astype(np.uint8)
    out[key + "margin_sub16"] = margin[::16, ::16].numpy().astype(np.float32)


def gen_slide(model, kind, out):
    model.eval()
    with torch.no_grad():
        for i, (h, w) in enumerate(S.SLIDE_SIZES):
            img = synth_image(1, (h, w), seed=S.EVAL_SEED + i)
            metas = [dict(ori_shape=(h, w), img_shape=(h, w), pad_shape=(h, w), padding_size=[0, 0, 0, 0])]
            _record_logits(out, f"{kind}::slide_{h}x{w}::", model.slide_inference(img, metas))
            print(kind, "slide", (h, w), out[f"{kind}::slide_{h}x{w}::logits_stats"])


def main():
    torch.manual_seed(0)
    M = _models()
    out = {"seeds_depth": np.array([S.HEAD_SEED, S.TRAIN_SEED, S.EVAL_SEED, S.DEPTH])}
    gen_head(M, out)
    for kind in S.KINDS:
        model = build_reference_model(M, kind)
        gen_train_step(model, kind, out)
        if kind == "lora":
            gen_slide(model, kind, out)
    path = os.path.join(GOLD, "segformer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
