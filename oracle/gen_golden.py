"""TEST INFRASTRUCTURE ONLY - runs in the build container, where /root/reference exists.

Imports the reference's own model files through oracle/ref_shim.py, runs them on CPU
(fp32) on deterministic synthetic weights/inputs and writes small golden vectors to
tests/golden/*.npz.  Those fixtures pin oracle/torch_ref.py (tests/test_oracle_golden.py).

    python -m oracle.gen_golden [--only NAME]

Fixtures hold inputs' seeds and expected outputs only (slices, statistics, hashes) -
never reference source text.
"""
import argparse
import hashlib
import os
import tempfile

import numpy as np
import torch
import torch.nn as nn

from oracle import ref_shim
from vfmseg_amd import presets
from vfmseg_amd.synth import synth_image, synth_label, synth_like

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def stats(t):
    t = t.detach().double()
    return np.array([t.mean().item(), t.abs().mean().item(), t.std().item(), t.abs().max().item()])


def sl(t, n=8):
    """Small deterministic slice of a tensor (first n along every dim)."""
    idx = tuple(slice(0, min(n, s)) for s in t.shape)
    return t.detach()[idx].contiguous().numpy().copy()


def mask_digest(m):
    return hashlib.sha256(np.ascontiguousarray(m.astype(np.uint8)).tobytes()).hexdigest()


def build_reference_model(depth=24, out_indices=None):
    """The reference's MsVFMEncoderDecoder with synthetic parameters."""
    M = ref_shim.load_all()
    cfg = presets.dinov2_ms_masked(depth=depth)
    if out_indices is not None:
        cfg["backbone"]["backbone"]["out_indices"] = list(out_indices)
    # LoRABackbone loads a checkpoint unconditionally (lora_backbone.py:27-35): give it one, in the
    # *un-renamed* key scheme the converters emit, so the reference's own rename path runs.
    bb = M.build(cfg["backbone"]["backbone"])
    base_sd = synth_like(bb.state_dict())
    del bb
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(base_sd, f.name)
        ck = f.name
    cfg["backbone"]["checkpoint"] = ck
    cfg["train_cfg"]["work_dir"] = tempfile.mkdtemp()
    model = M.build(cfg)
    os.unlink(ck)
    # non-base parameters (LoRA A/B, heads): key-hashed synthetic values
    sd = model.state_dict()
    new = synth_like(sd)
    for k in sd:
        if ".base_layer." in k or ("backbone." in k and "lora_" not in k):
            # keep what the reference's loader put there; must equal synth of the un-renamed key
            new[k] = sd[k]
    model.load_state_dict(new)
    model._synth_sd = {k: v.clone() for k, v in new.items()}
    model.local_iter = 1  # skip the matplotlib debug dump at iter 0 (Ms_VFM_encoder_decoder.py:197-199)
    return model


def reset(model):
    """Every fixture starts from the same synthetic state (train-mode passes move the BN running stats)."""
    model.load_state_dict(model._synth_sd)
    model.zero_grad()


def set_dropout_zero(model):
    for m in model.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d)):
            m.p = 0.0


class RandRecorder:
    """Records torch.rand outputs (the query mask, Transformer.py:265) without touching reference code."""

    def __init__(self):
        self.vals = []
        self._orig = torch.rand

    def __enter__(self):
        def rec(*a, **k):
            v = self._orig(*a, **k)
            self.vals.append(v.clone())
            return v

        torch.rand = rec
        return self

    def __exit__(self, *a):
        torch.rand = self._orig


# --------------------------------------------------------------------------------- fixtures
def gen_dinov2(model):
    reset(model)
    bb = model.backbone
    bb.eval()
    out = {}
    with torch.no_grad():
        for tag, size in (("sq", (512, 512)), ("rect", (512, 1024))):
            x = synth_image(1, size, seed=11)
            taps = bb(x)
            for i, t in enumerate(taps):
                out[f"{tag}_tap{i}_stats"] = stats(t)
                out[f"{tag}_tap{i}_slice"] = sl(t)
                out[f"{tag}_tap{i}_tail"] = t[0, -4:, -3:, -5:].numpy().copy()
    np.savez_compressed(os.path.join(GOLD, "dinov2_taps.npz"), **out)
    print("dinov2_taps", {k: v[:2] for k, v in out.items() if k.endswith("stats")})


def synth_feats(b, c=1024, hw=32, seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    return [torch.randn(b, c, hw, hw, generator=g) for _ in range(4)]


def gen_heads(model):
    reset(model)
    out = {}
    lab = synth_label(2, 512, seed=5)
    # --- LinearHead, train-mode BN (batch stats), dropout off
    model.train()
    set_dropout_zero(model)
    feats = synth_feats(2, seed=1)
    head = model.decode_head
    rm0 = head.output_upscaling[1].running_mean.clone()
    losses, logits = head.loss([f.clone().requires_grad_(True) for f in feats], lab, return_logits=True)
    out["lin_train_logits_stats"] = stats(logits)
    out["lin_train_logits_slice"] = sl(logits)
    out["lin_train_loss"] = np.array([losses["loss_ce"].item(), losses["acc_seg"].item()])
    out["lin_bn_running_mean_delta"] = stats(head.output_upscaling[1].running_mean - rm0)
    out["lin_bn_running_var"] = stats(head.output_upscaling[1].running_var)
    # --- LinearHead eval (running stats of the synthetic state)
    reset(model)
    model.eval()
    with torch.no_grad():
        lo = head(feats)
    out["lin_eval_logits_stats"] = stats(lo)
    out["lin_eval_logits_slice"] = sl(lo)
    # --- VFMHead with recorded mask, and with mask disabled
    aux = model.aux_decoder
    g = torch.Generator().manual_seed(77)
    ctx = torch.randn(2, 19, 256, 256, generator=g)
    torch.manual_seed(1234)
    with RandRecorder() as rr:
        losses, hl = aux.loss(feats, ctx, lab, return_logits=True)
    assert len(rr.vals) == 1
    out["vfm_mask_rand"] = rr.vals[0].numpy()
    out["vfm_logits_stats"] = stats(hl)
    out["vfm_logits_slice"] = sl(hl)
    out["vfm_loss"] = np.array([losses["loss_ce"].item(), losses["acc_seg"].item()])
    aux.transformer_decoder.mask_enable = False
    with torch.no_grad():
        lo = aux(feats, ctx)
    aux.transformer_decoder.mask_enable = True
    out["vfm_nomask_logits_stats"] = stats(lo)
    out["vfm_nomask_logits_slice"] = sl(lo)
    np.savez_compressed(os.path.join(GOLD, "heads.npz"), **out)
    print("heads", out["lin_train_loss"], out["vfm_loss"])


def gen_train_step(model):
    reset(model)
    """Full MsVFMEncoderDecoder.forward_train (B=2, 1024^2) + backward: losses and gradient probes."""
    out = {}
    model.train()
    set_dropout_zero(model)
    model.zero_grad()
    img = synth_image(2, 1024, seed=3)
    lab = synth_label(2, 1024, seed=3)
    samples = [ref_shim.SegDataSample(gt=lab[i]) for i in range(2)]
    np.random.seed(0)
    torch.manual_seed(4321)
    with RandRecorder() as rr:
        losses = model.loss(img, samples)
    assert len(rr.vals) == 1
    out["mask_rand"] = rr.vals[0].numpy()
    out["hr_crop_box"] = np.array(model.hr_crop_box)
    keys = ["decode_lr.loss_ce", "decode_lr.acc_seg", "decode_hr.loss_ce", "decode_hr.acc_seg"]
    out["losses"] = np.array([float(losses[k]) for k in keys])
    total = sum(v for k, v in losses.items() if "loss" in k)
    total.backward()
    named = dict(model.named_parameters())
    groups = {"lora": 0.0, "decode_head": 0.0, "aux_decoder": 0.0}
    n_train = 0
    for k, p in named.items():
        if p.grad is None:
            continue
        n_train += p.numel()
        g2 = p.grad.double().pow(2).sum().item()
        if "lora_" in k:
            groups["lora"] += g2
        elif k.startswith("decode_head"):
            groups["decode_head"] += g2
        elif k.startswith("aux_decoder"):
            groups["aux_decoder"] += g2
    out["grad_norms"] = np.sqrt(np.array([groups["lora"], groups["decode_head"], groups["aux_decoder"]]))
    out["n_trainable"] = np.array([n_train])
    pre = "backbone.model.base_model.model.blocks."
    probes = [
        pre + "0.attn.qkv.lora_A.default.weight",
        pre + "0.attn.qkv.lora_B.default.weight",
        pre + "23.attn.qkv.lora_A.default.weight",
        pre + "23.attn.qkv.lora_B.default.weight",
        "decode_head.conv_seg.weight",
        "decode_head.conv_seg.bias",
        "decode_head.fusion_conv.conv.weight",
        "decode_head.output_upscaling.0.weight",
        "decode_head.output_upscaling.1.weight",
        "aux_decoder.conv_seg.weight",
        "aux_decoder.transformer_decoder.mask_token",
        "aux_decoder.transformer_decoder.transformer_blocks.0.attn2.to_k.weight",
        "aux_decoder.transformer_decoder.transformer_blocks.2.ff.net.0.proj.weight",
        "aux_decoder.seg_logits_embed.0.weight",
        "aux_decoder.fuse_conv.0.weight",
    ]
    for k in probes:
        g = named[k].grad
        out["grad_stats::" + k] = stats(g)
        out["grad_slice::" + k] = sl(g.reshape(g.shape[0], -1) if g.dim() > 1 else g)
    np.savez_compressed(os.path.join(GOLD, "train_step.npz"), **out)
    print("train_step", out["losses"], out["grad_norms"], out["hr_crop_box"], n_train)


def gen_ms_inference(model):
    reset(model)
    """MsVFMEncoderDecoder.inference('ms_slide_inference') on one 1024^2 image; argmax mask digest."""
    out = {}
    model.eval()
    img = synth_image(1, 1024, seed=9)
    # thresholds chosen so that both branches of the confidence gate are taken with random weights
    thr, conf = out_thr = (0.3, 0.341)
    model.test_cfg["threadshod"], model.test_cfg["conf"] = thr, conf
    refined = []
    orig = model.enc_dec

    def spy(inputs, context=None):
        if context is not None:
            refined.append(tuple(int(v) for v in model.hr_crop_box))
        return orig(inputs, context)

    model.enc_dec = spy
    metas = [dict(ori_shape=(1024, 1024), img_shape=(1024, 1024), pad_shape=(1024, 1024), padding_size=[0, 0, 0, 0])]
    with torch.no_grad():
        logits = model.inference(img, metas)
    model.enc_dec = orig
    assert 0 < len(refined) < 9, "thresholds no longer exercise both gate branches"
    pred = logits.argmax(dim=1)[0].numpy().astype(np.uint8)
    out["test_cfg"] = np.array(out_thr)
    out["refined_boxes"] = np.array(refined).reshape(-1, 4)
    out["logits_stats"] = stats(logits)
    out["logits_slice"] = sl(logits)
    out["logits_center"] = logits[0, :, 500:504, 636:644].numpy().copy()
    out["pred_sub4"] = pred[::4, ::4].copy()
    out["pred_sha256"] = np.array(mask_digest(pred))
    out["pred_hist"] = np.bincount(pred.reshape(-1), minlength=19)
    np.savez_compressed(os.path.join(GOLD, "ms_inference.npz"), **out)
    print("ms_inference refined", len(refined), "of 9;", out["pred_sha256"], out["pred_hist"])


def gen_slide_modes(model):
    """The other three test modes of MsVFMEncoderDecoder.inference (Ms_VFM_encoder_decoder.py:278-332) on one 1024^2 image, run by the
    reference's own code: lr_slide_inference (the class default), hr_slide_inference, msfull_slide_inference.  msfull draws a query mask
    per refined window (torch.rand in MaskTransformerDecoder.forward, Transformer.py:265): recorded, so that the oracle and the HIP
    path can inject the same masks."""
    out = {}
    img = synth_image(1, 1024, seed=11)
    metas = [dict(ori_shape=(1024, 1024), img_shape=(1024, 1024), pad_shape=(1024, 1024), padding_size=[0, 0, 0, 0])]
    out["test_cfg_stride_crop"] = np.array(list(model.test_cfg["stride"]) + list(model.test_cfg["crop_size"]))
    for mode in ("lr_slide_inference", "hr_slide_inference", "msfull_slide_inference"):
        reset(model)
        model.eval()
        model.test_cfg["mode"] = mode
        torch.manual_seed(1000 + len(mode))   # msfull draws nine torch.rand query masks: seeded, so the fixture regenerates byte for byte
        with RandRecorder() as rr, torch.no_grad():
            logits = model.inference(img, metas)
        if mode == "msfull_slide_inference":
            assert len(rr.vals) == 9 and tuple(rr.vals[0].shape) == (1, 1, 32, 32), [tuple(v.shape) for v in rr.vals]
            out["msfull_mask_rand"] = torch.stack(rr.vals).reshape(9, 32, 32).numpy().astype(np.float32)
        else:
            assert len(rr.vals) == 0, "lr / hr slide run the LinearHead only: no query mask"
        assert tuple(logits.shape) == (1, 19, 1024, 1024)
        pred = logits.argmax(dim=1)[0].numpy().astype(np.uint8)
        out[mode + "::logits_stats"] = stats(logits)
        out[mode + "::logits_slice"] = sl(logits)
        out[mode + "::logits_center"] = logits[0, :, 500:504, 636:644].numpy().copy()
        out[mode + "::pred_sub4"] = pred[::4, ::4].copy()
        out[mode + "::pred_sha256"] = np.array(mask_digest(pred))
        out[mode + "::pred_hist"] = np.bincount(pred.reshape(-1), minlength=19)
        print(mode, out[mode + "::logits_stats"], out[mode + "::pred_sha256"])
    model.test_cfg["mode"] = "ms_slide_inference"
    np.savez_compressed(os.path.join(GOLD, "slide_modes.npz"), **out)


# The reference's DG evaluation sizes (test pipelines' keep-ratio resizes): Cityscapes 1024 x 2048 (3 x 6 windows), ACDC 1080 x 1920
# (3 x 6, ragged last row / column), BDD100k 720 x 1280 (2 x 4, ragged last row), a Mapillary photo 1024 x 1365 (3 x 4, odd width).
EVAL_SIZES = ((1024, 2048), (1080, 1920), (720, 1280), (1024, 1365))
EVAL_SIZES_DEPTH = 4      # window / resize / gate code does not depend on depth; full-depth parity is pinned at 1024^2


def eval_sizes_seed(h, w):
    return 500 + (h * 7 + w) % 97


def eval_sizes_probes(h, w, boxes):
    """(name, (y0, y1, x0, x1)) logit windows stored per size: a corner, the centre, a seam between the first two window columns
    (where an overlap band starts), and the bottom-right edge (the ragged last window row / column)."""
    seam_x = boxes[1][2] if len(boxes) > 1 and boxes[1][2] > 0 else w // 2
    return (("corner", (0, 8, 0, 8)), ("centre", (h // 2 - 2, h // 2 + 2, w // 2 - 4, w // 2 + 4)),
            ("seam", (h // 3, h // 3 + 4, seam_x - 4, seam_x + 4)), ("edge", (h - 4, h, w - 8, w)))


def eval_sizes_gate(seg, boxes, thrs=(0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5)):
    """(thr, conf) for which some windows of `boxes` are refined and some are not, with conf in the middle of the widest gap between
    the windows' gate fractions (so that rounding of the coarse logits cannot move a window across it)."""
    best = None
    for thr in thrs:
        conf_map = (seg.softmax(dim=1).max(dim=1)[0] > thr).double()
        fr = sorted(conf_map[:, y1:y2, x1:x2].mean().item() for (y1, y2, x1, x2) in boxes)
        for k in range(len(fr) - 1):
            gap = fr[k + 1] - fr[k]
            if best is None or gap > best[0]:
                best = (gap, thr, round((fr[k] + fr[k + 1]) / 2, 4))
    assert best is not None and best[0] > 0.008, ("no threshold separates the windows", best)
    return best[1], best[2]


def gen_eval_sizes(_model=None):
    """MsVFMEncoderDecoder.inference of the reference at its DG evaluation sizes (EVAL_SIZES; depth 4, out_indices 0-3): ms_slide_inference
    everywhere (gate thresholds per size chosen so that some windows are refined and some are not; the refined boxes recorded), and
    lr_slide_inference where the half-size image is at least one crop tall.  Pins the oracle (tests/test_oracle_golden.py) and the HIP
    path (tests/test_eval_sizes_gpu.py) where the window grid has more than 16 windows, ragged rows / columns, non-integer resize factors,
    context windows off the coarse grid, and an odd width."""
    model = build_reference_model(depth=EVAL_SIZES_DEPTH, out_indices=range(EVAL_SIZES_DEPTH))
    out = {"sizes": np.array(EVAL_SIZES), "test_cfg_stride_crop": np.array(list(model.test_cfg["stride"]) + list(model.test_cfg["crop_size"]))}
    orig = model.enc_dec
    refined = []

    def spy(inputs, context=None):
        if context is not None:
            refined.append(tuple(int(v) for v in model.hr_crop_box))
        return orig(inputs, context)

    def run(img, mode):
        reset(model)
        model.eval()
        model.test_cfg["mode"] = mode
        h, w = img.shape[2:]
        metas = [dict(ori_shape=(h, w), img_shape=(h, w), pad_shape=(h, w), padding_size=[0, 0, 0, 0])]
        refined.clear()
        with torch.no_grad():
            return model.inference(img, metas)

    model.enc_dec = spy
    for (h, w) in EVAL_SIZES:
        img = synth_image(1, (h, w), seed=eval_sizes_seed(h, w))
        boxes = [tuple(b) for b in ref_shim_grid(h, w, model)]
        # the coarse map alone: a gate that refines nothing leaves every window's coarse logits (merge of equal values)
        model.test_cfg["threadshod"], model.test_cfg["conf"] = 0.5, -1.0
        seg = run(img, "ms_slide_inference")
        assert not refined
        thr, conf = eval_sizes_gate(seg, boxes)
        model.test_cfg["threadshod"], model.test_cfg["conf"] = thr, conf
        modes = ["ms_slide_inference"] + (["lr_slide_inference"] if h // 2 >= model.test_cfg["crop_size"][0] else [])
        for mode in modes:
            logits = run(img, mode)
            key = f"{h}x{w}/{mode}::"
            if mode == "ms_slide_inference":
                assert 0 < len(refined) < len(boxes), (h, w, len(refined), len(boxes))
                out[key + "test_cfg"] = np.array([thr, conf])
                out[key + "refined_boxes"] = np.array(refined).reshape(-1, 4)
            else:
                assert not refined
            oh, ow = logits.shape[2:]
            assert (oh, ow) == ((h, w) if mode == "ms_slide_inference" else (h // 2 * 2, w // 2 * 2)), logits.shape
            pred = logits.argmax(dim=1)[0].numpy().astype(np.uint8)
            out[key + "logits_stats"] = stats(logits)
            for name, (y0, y1, x0, x1) in eval_sizes_probes(oh, ow, boxes):
                out[key + "logits_" + name] = logits[0, :, y0:y1, x0:x1].numpy().copy()
            out[key + "pred_sub8"] = pred[::8, ::8].copy()
            out[key + "pred_sha256"] = np.array(mask_digest(pred))
            out[key + "pred_hist"] = np.bincount(pred.reshape(-1), minlength=19)
            print(f"eval_sizes {h}x{w} {mode}: windows {len(boxes)}, refined {len(refined)} (thr {thr}, conf {conf}),",
                  out[key + "logits_stats"], out[key + "pred_sha256"][()][:12])
    model.enc_dec = orig
    np.savez_compressed(os.path.join(GOLD, "eval_sizes.npz"), **out)


def ref_shim_grid(h, w, model):
    """The window grid of the reference's slide loops (Ms_VFM_encoder_decoder.py:428-443) for the model's test_cfg."""
    (hs, ws), (hc, wc) = model.test_cfg["stride"], model.test_cfg["crop_size"]
    boxes = []
    for hi in range(max(h - hc + hs - 1, 0) // hs + 1):
        for wi in range(max(w - wc + ws - 1, 0) // ws + 1):
            y2, x2 = min(hi * hs + hc, h), min(wi * ws + wc, w)
            boxes.append((max(y2 - hc, 0), y2, max(x2 - wc, 0), x2))
    return boxes


def gen_eva02(_model=None):
    """EVA02-L + LoRA (q/k/v/attn.proj targets; only attn.proj is live): taps and LoRA gradients."""
    M = ref_shim.load_eva02()
    depth = 24
    bcfg = presets.eva02_backbone(depth=depth)
    bb = M.build(bcfg)
    base_sd = {k: v for k, v in synth_like(bb.state_dict()).items() if "rope." not in k}  # keep the real cos/sin tables
    out_rope = {"rope_cos": bb.rope.freqs_cos.numpy().copy(), "rope_sin": bb.rope.freqs_sin.numpy().copy()}
    del bb
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(base_sd, f.name)
        ck = f.name
    model = M.build(dict(type="LoRABackbone", backbone=bcfg, checkpoint=ck, Lora_config=presets.eva02_lora_cfg(dropout=0.0)))
    os.unlink(ck)
    sd = model.state_dict()
    new = synth_like(sd)
    for k in sd:
        if "lora_" not in k:
            new[k] = sd[k]
    model.load_state_dict(new)
    model.train()
    x = synth_image(1, 512, seed=31)
    taps = model(x)
    out = {"rope_cos_slice": out_rope["rope_cos"][::97, ::5].copy(), "rope_sin_slice": out_rope["rope_sin"][::97, ::5].copy()}
    gen = torch.Generator().manual_seed(6)
    loss = 0
    for i, t in enumerate(taps):
        out[f"tap{i}_stats"] = stats(t)
        out[f"tap{i}_slice"] = sl(t)
        loss = loss + (t * torch.randn(t.shape, generator=gen)).sum()
    loss.backward()
    named = dict(model.named_parameters())
    pre = "model.base_model.model.blocks."
    live, inert = 0.0, 0
    for k, p in named.items():
        if "lora_" in k:
            if p.grad is None or float(p.grad.abs().max()) == 0.0:
                inert += 1
            else:
                live += p.grad.double().pow(2).sum().item()
    out["lora_live_grad_norm"] = np.array([live ** 0.5])
    out["lora_inert_count"] = np.array([inert])
    for k in (pre + "0.attn.proj.lora_A.default.weight", pre + "0.attn.proj.lora_B.default.weight",
              pre + "23.attn.proj.lora_A.default.weight", pre + "23.attn.proj.lora_B.default.weight"):
        out["grad_slice::" + k] = sl(named[k].grad)
    np.savez_compressed(os.path.join(GOLD, "eva02.npz"), **out)
    print("eva02", {k: v[:2] for k, v in out.items() if k.endswith("stats")}, out["lora_live_grad_norm"], out["lora_inert_count"])


def gen_clip(_model=None):
    """CLIP ViT-L/16 + LoRA (out_proj / mlp.c_fc / mlp.c_proj targets; out_proj is consumed by weight inside
    nn.MultiheadAttention and stays inert): taps and LoRA gradients."""
    M = ref_shim.load_clip()
    bcfg = presets.clip_backbone()
    bb = M.build(bcfg)
    base_sd = synth_like(bb.state_dict())
    del bb
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(base_sd, f.name)
        ck = f.name
    model = M.build(dict(type="LoRABackbone", backbone=bcfg, checkpoint=ck, Lora_config=presets.clip_lora_cfg(dropout=0.0)))
    os.unlink(ck)
    sd = model.state_dict()
    new = synth_like(sd)
    for k in sd:
        if "lora_" not in k:
            new[k] = sd[k]
    model.load_state_dict(new)
    model.train()
    x = synth_image(1, 512, seed=51)
    taps = model(x)
    out = {}
    gen = torch.Generator().manual_seed(7)
    loss = 0
    for i, t in enumerate(taps):
        out[f"tap{i}_stats"] = stats(t)
        out[f"tap{i}_slice"] = sl(t)
        loss = loss + (t * torch.randn(t.shape, generator=gen)).sum()
    loss.backward()
    named = dict(model.named_parameters())
    pre = "model.base_model.model.transformer.resblocks."
    live, inert = 0.0, 0
    for k, p in named.items():
        if "lora_" in k:
            if p.grad is None or float(p.grad.abs().max()) == 0.0:
                inert += 1
            else:
                live += p.grad.double().pow(2).sum().item()
    out["lora_live_grad_norm"] = np.array([live ** 0.5])
    out["lora_inert_count"] = np.array([inert])
    for blk in (0, 23):
        for nm in ("mlp.c_fc", "mlp.c_proj"):
            for ab in ("lora_A", "lora_B"):
                k = f"{pre}{blk}.{nm}.{ab}.default.weight"
                out["grad_slice::" + k] = sl(named[k].grad)
    np.savez_compressed(os.path.join(GOLD, "clip.npz"), **out)
    print("clip", {k: v[:2] for k, v in out.items() if k.endswith("stats")}, out["lora_live_grad_norm"], out["lora_inert_count"])


def gen_sam(_model=None):
    """SAM-ViT-H + LoRA(qkv): taps of one 512^2 crop (28 windowed + 4 global blocks, decomposed rel-pos with non-zero tables)."""
    M = ref_shim.load_sam()
    bcfg = presets.sam_backbone()
    bb = M.build(bcfg)
    base_sd = synth_like(bb.state_dict())
    del bb
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(base_sd, f.name)
        ck = f.name
    model = M.build(dict(type="LoRABackbone", backbone=bcfg, checkpoint=ck, Lora_config=presets.lora_cfg(dropout=0.0)))
    os.unlink(ck)
    sd = model.state_dict()
    new = synth_like(sd)
    for k in sd:
        if "lora_" not in k:
            new[k] = sd[k]
    model.load_state_dict(new)
    model.train()                  # LoRABackbone.train(): base stays in eval, lora_dropout = 0 here
    x = synth_image(1, 512, seed=41)
    taps = model(x)
    out = {}
    gen = torch.Generator().manual_seed(9)
    loss = 0
    for i, t in enumerate(taps):
        out[f"tap{i}_stats"] = stats(t.detach())
        out[f"tap{i}_slice"] = sl(t.detach())
        out[f"tap{i}_tail"] = t.detach()[0, -4:, -3:, -5:].numpy().copy()
        loss = loss + (t * torch.randn(t.shape, generator=gen)).sum()
    loss.backward()
    named = dict(model.named_parameters())
    pre = "model.base_model.model.blocks."
    tot = 0.0
    for k, p_ in named.items():
        if "lora_" in k:
            tot += p_.grad.double().pow(2).sum().item()
    out["lora_grad_norm"] = np.array([tot ** 0.5])
    for blk in (0, 7, 30, 31):      # windowed (0, 30) and global (7, 31) blocks
        for ab in ("lora_A", "lora_B"):
            k = f"{pre}{blk}.attn.qkv.{ab}.default.weight"
            out["grad_slice::" + k] = sl(named[k].grad)
    np.savez_compressed(os.path.join(GOLD, "sam.npz"), **out)
    print("sam", {k: v[:2] for k, v in out.items() if k.endswith("stats")})


def gen_sam_slide(_model=None):
    """BASELINE configs[4] WHOLE: configs/_base_/models/lora_sam_linear.py (EncoderDecoder, LoRA SAM-ViT-H at depth 32, LinearHead,
    test_cfg mode 'slide', crop 512, stride 320) on one 1024^2 image: the reference's SAMViT / LoRABackbone / LinearHead bodies under the
    restated mmseg EncoderDecoder.slide_inference (3 x 3 windows, overlap-averaged).  Round-3 verdict, Weak #3: the composite that
    bench.py times had only been checked in parts (one 512^2 crop at depth 32; the slide composite at depth 8)."""
    M = ref_shim.load_sam()
    cfg = presets.sam_linear()
    bb = M.build(cfg["backbone"]["backbone"])
    base_sd = synth_like(bb.state_dict())
    del bb
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(base_sd, f.name)
        ck = f.name
    cfg["backbone"]["checkpoint"] = ck
    kw = {k: v for k, v in cfg.items() if k != "type"}
    model = ref_shim.EncoderDecoder(**kw)      # mmseg's class is third-party (absent offline): the shim's restatement of it
    os.unlink(ck)
    sd = model.state_dict()
    new = synth_like(sd)
    for k in sd:
        if k.startswith("backbone.") and "lora_" not in k:
            new[k] = sd[k]
        elif k.startswith("backbone."):   # LoRA factors: the values of the bare LoRABackbone of gen_sam (tests/helpers.py:sam_state_dict)
            kk = k[len("backbone."):]
            new[k] = synth_like({kk: sd[k]})[kk]
    model.load_state_dict(new)
    model.eval()
    img = synth_image(1, 1024, seed=47)
    metas = [dict(ori_shape=(1024, 1024), img_shape=(1024, 1024), pad_shape=(1024, 1024), padding_size=[0, 0, 0, 0])]
    with torch.no_grad():
        logits = model.slide_inference(img, metas)
    assert tuple(logits.shape) == (1, 19, 1024, 1024)
    pred = logits.argmax(dim=1)[0].numpy().astype(np.uint8)
    out = {"logits_stats": stats(logits), "logits_slice": sl(logits), "logits_center": logits[0, :, 500:504, 636:644].numpy().copy(),
           "logits_sub16": logits[0, :, ::16, ::16].numpy().copy(),      # every 16th pixel: all nine windows and every overlap band
           "pred_sub4": pred[::4, ::4].copy(), "pred_sha256": np.array(mask_digest(pred)), "pred_hist": np.bincount(pred.reshape(-1), minlength=19),
           "test_cfg_stride_crop": np.array(list(cfg["test_cfg"]["stride"]) + list(cfg["test_cfg"]["crop_size"]))}
    np.savez_compressed(os.path.join(GOLD, "sam_slide.npz"), **out)
    print("sam_slide", out["logits_stats"], out["pred_sha256"], out["pred_hist"])


def gen_rcs(_model=None):
    """Rare class sampling (rein/datasets/uda_dataset.py:16-37 get_rcs_class_probs, :44-103 DGDataset): the reference's OWN class run on
    a toy source (tests/rcs_toy.py) - class order, probabilities, per-class file lists and the first 32 draws under np.random.seed(0),
    with every source access (index, crop offset) the ten-re-draw loop made."""
    import sys
    import types as _types
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD)))
    import rcs_toy
    ref_shim.install()
    reg = ref_shim._Registry()
    reg.register_module(name="ToySource", module=rcs_toy.ToySource)
    ref_shim._mod("mmseg.datasets", CityscapesDataset=object)
    sys.modules["mmseg.registry"].DATASETS = reg
    pk = ref_shim._mod(ref_shim.PKG + ".datasets")
    pk.__path__ = [os.path.join(ref_shim.REF_ROOT, "rein", "datasets")]
    U = ref_shim.importlib.import_module(ref_shim.PKG + ".datasets.uda_dataset")
    root = tempfile.mkdtemp()
    os.makedirs(os.path.join(root, "labels"))
    rcs_toy.write_stats(root, rcs_toy.label_maps())
    ds = U.DGDataset(dict(type="ToySource", data_root=root), rare_class_sampling=dict(rcs_toy.RCS))
    out = dict(classes=np.array(ds.rcs_classes), classprob=np.asarray(ds.rcs_classprob, dtype=np.float64))
    for c in ds.rcs_classes:
        out[f"files_{c}"] = np.array([int(f.split("_")[0]) for f in ds.samples_with_class[c]])
    np.random.seed(0)
    draws, calls, ncalls = [], [], []
    for _ in range(32):
        n0 = len(ds.source.calls)
        s = ds[0]
        draws.append((s["index"],) + tuple(s["offset"]))
        ncalls.append(len(ds.source.calls) - n0)
    out["draws"] = np.array(draws)
    out["ncalls"] = np.array(ncalls)
    out["calls"] = np.array(ds.source.calls)
    out["rng_after"] = np.random.randint(0, 1 << 30, size=4)     # the global stream stands where the reference left it
    np.savez_compressed(os.path.join(GOLD, "rcs.npz"), **out)
    print("rcs classes", out["classes"], "prob", out["classprob"], "calls per draw", out["ncalls"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(os.cpu_count())
    steps = dict(dinov2=gen_dinov2, heads=gen_heads, train_step=gen_train_step, ms_inference=gen_ms_inference, slide_modes=gen_slide_modes)
    model = build_reference_model() if a.only in (None,) + tuple(steps) else None  # noqa: E501
    for name, fn in steps.items():
        if a.only in (None, name):
            fn(model)
    if a.only in (None, "eva02"):
        gen_eva02()
    if a.only in (None, "sam"):
        gen_sam()
    if a.only in (None, "clip"):
        gen_clip()
    if a.only in (None, "rcs"):
        gen_rcs()
    if a.only in (None, "sam_slide"):
        gen_sam_slide()
    if a.only in (None, "eval_sizes"):
        gen_eval_sizes()


if __name__ == "__main__":
    main()
