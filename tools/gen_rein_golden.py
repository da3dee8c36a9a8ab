"""Writes tests/golden/rein.npz from the REFERENCE's own Rein modules (rein/models/backbones/reins.py, reins_dinov2.py, imported through
oracle/ref_shim.py): data only - slices, whole-tensor statistics, gradient norms, parameter names.  Runs where the reference tree exists
(the build container); the tests read the .npz and tests/rein_helpers.py only.

    python tools/gen_rein_golden.py

Parameters follow tests/rein_helpers.py (a recipe under which the adapter visibly moves the taps); the generator ASSERTS that, so a
re-tuned recipe cannot make the fixture blind: every tap must differ by >= 0.3 of its largest magnitude both from the adapter-less taps and from a
control whose token attention is dead (learnable_tokens_b = 0)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests.helpers import sl, stats  # noqa: E402
from tests.rein_helpers import rein_backbone_state_dict, rein_model_state_dict, rein_params, step_inputs  # noqa: E402
from vfmseg_amd import presets  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
STEP_LAYER, STEP_DEPTH = 3, 4
TAP_GRAD_SEED, TRAIN_IMG_SEED = 8, 33


def _models():
    M = ref_shim.load_all()
    ref_shim.ref_import("models.backbones.reins")
    ref_shim.ref_import("models.backbones.reins_dinov2")
    return M


def gen_step(M, out, lora):
    """One adapter step at [2048, 1024], layer 3, in float64: x', dx and every parameter gradient from forward + autograd."""
    tag = "lora" if lora else "plain"
    cfg = dict(presets.reins_cfg(depth=STEP_DEPTH))
    if not lora:
        cfg.pop("lora_dim")
        cfg["type"] = "Reins"
    mod = M.build(cfg).double()
    prm = rein_params(depth=STEP_DEPTH, lora=lora)
    missing, unexpected = mod.load_state_dict({k: v.double() for k, v in prm.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    x, g = step_inputs()
    xin = x.double()[None].requires_grad_(True)
    xo = mod.forward(xin, STEP_LAYER, batch_first=True, has_cls_token=False)
    xo.backward(g.double()[None])
    # the recipe keeps the step informative: the token term is not lost under x, the softmax neither flat nor saturated
    with torch.no_grad():
        tok = mod.get_tokens(STEP_LAYER)
        attn = torch.softmax(x.double() @ tok.t() * (x.shape[1] ** -0.5), -1)
        term = attn[:, 1:] @ mod.mlp_token2feat(tok[1:])
        ratio, top = (term.std() / x.double().std()).item(), attn.max(-1)[0].mean().item()
    assert ratio >= 0.3 and 0.1 <= top <= 0.9, (ratio, top)
    out[f"step_{tag}_token_term_ratio_top_prob"] = np.array([ratio, top])
    out[f"step_{tag}_xo_slice"], out[f"step_{tag}_xo_stats"] = sl(xo[0]), stats(xo[0])
    out[f"step_{tag}_dx_slice"], out[f"step_{tag}_dx_stats"] = sl(xin.grad[0]), stats(xin.grad[0])
    nograd = []
    for n, p in mod.named_parameters():
        if p.grad is None:
            nograd.append(n)
            continue
        gr = p.grad[STEP_LAYER] if n.startswith("learnable_tokens") else p.grad
        out[f"step_{tag}_grad_slice::{n}"] = sl(gr.reshape(1, -1) if gr.dim() < 2 else gr)
        out[f"step_{tag}_grad_norm::{n}"] = np.array([p.grad.norm().item()])
    out[f"step_{tag}_no_grad"] = np.array(sorted(nograd))
    print("step", tag, "token term / x std %.3f, mean top probability %.3f" % (ratio, top), "no grad:", nograd)


def _range_dist(a, b):
    """max |a - b| / max |a|: the measure (tests/helpers.rel_err) the tap tolerances of the tests are stated in"""
    return ((a - b).abs().max() / a.abs().max()).item()


def gen_full_depth(M, out):
    """ReinsDinoVisionTransformer at depth 24, one 512^2 image: the four taps, then backward of seeded random tap gradients."""
    cfg = presets.rein_dinov2_linear()["backbone"]
    cfg.pop("init_cfg")
    model = M.build(cfg)
    sd = rein_backbone_state_dict(24)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.train()
    x = synth_image(1, 512, seed=31)
    taps = model(x)
    with torch.no_grad():   # the two controls (same module, parameters swapped)
        keep = model.reins.scale.data.clone()
        model.reins.scale.data.zero_()
        bare = model(x)
        model.reins.scale.data.copy_(keep)
        keep_b = model.reins.learnable_tokens_b.data.clone()
        model.reins.learnable_tokens_b.data.zero_()
        dead = model(x)
        model.reins.learnable_tokens_b.data.copy_(keep_b)
    sens = np.array([[_range_dist(t, b), _range_dist(t, d)] for t, b, d in zip(taps, bare, dead)])
    assert (sens >= 0.3).all(), sens
    out["full_tap_sensitivity"] = sens     # [tap, (vs adapter-less, vs dead token attention)] in units of the tap's max |x|
    gen = torch.Generator().manual_seed(TAP_GRAD_SEED)
    loss = 0
    for i, t in enumerate(taps):
        out[f"full_tap{i}_stats"], out[f"full_tap{i}_slice"] = stats(t), sl(t)
        loss = loss + (t * torch.randn(t.shape, generator=gen)).sum()
    loss.backward()
    nograd, trainable = [], []
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.grad is None:
            nograd.append(n)
            continue
        trainable.append(n)
        gr = p.grad
        out[f"full_grad_slice::{n}"] = sl(gr.reshape(1, -1) if gr.dim() < 2 else gr)
        out[f"full_grad_norm::{n}"] = np.array([gr.double().norm().item()])
    out["full_live_params"], out["full_no_grad_params"] = np.array(sorted(trainable)), np.array(sorted(nograd))
    print("full depth: sensitivities", sens.round(2).tolist(), "no grad:", nograd)


def gen_train_step(M, out):
    """EncoderDecoder(ReinsDinoVisionTransformer, LinearHead) at depth 4, batch 2, 512^2, dropout 0: loss, acc_seg, gradient slices."""
    depth = 4
    cfg = presets.rein_dinov2_linear(depth=depth)
    cfg["backbone"].pop("init_cfg")
    cfg["backbone"]["out_indices"] = [0, 1, 2, 3]
    cfg["decode_head"]["dropout_ratio"] = 0.0
    cfg.pop("type")
    model = ref_shim.EncoderDecoder(**cfg)
    missing, unexpected = model.load_state_dict(rein_model_state_dict(depth), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.train()   # (nn.Module.train of the shim's segmentor: the backbone applies its own rule, the head is in train mode - batch-stat BN)
    img, lab = synth_image(2, 512, seed=TRAIN_IMG_SEED), synth_label(2, 512, seed=TRAIN_IMG_SEED)
    losses = model.decode_head.loss(list(model.extract_feat(img)), lab)
    losses["loss_ce"].backward()
    out["train_loss_acc"] = np.array([losses["loss_ce"].item(), losses["acc_seg"].item()])
    for n, p in model.named_parameters():
        if p.grad is not None and (n.startswith("backbone.reins.") or n in ("decode_head.conv_seg.weight", "decode_head.fusion_conv.conv.weight",
                                                                            "decode_head.output_upscaling.0.weight")):
            gr = p.grad
            out[f"train_grad_slice::{n}"] = sl(gr.reshape(1, -1) if gr.dim() < 2 else gr)
            out[f"train_grad_norm::{n}"] = np.array([gr.double().norm().item()])
    print("train step", out["train_loss_acc"])


def main():
    torch.manual_seed(0)
    M = _models()
    out = {}
    gen_step(M, out, lora=True)
    gen_step(M, out, lora=False)
    gen_full_depth(M, out)
    gen_train_step(M, out)
    path = os.path.join(GOLD, "rein.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
