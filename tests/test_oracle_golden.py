"""Pins oracle/torch_ref.py against outputs of the reference's own code (tests/golden/*.npz, made by
oracle/gen_golden.py in the build container).  CPU only; does not need /root/reference."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from tests.helpers import cached_full_state_dict, rel_err, sl, stats
from vfmseg_amd.synth import synth_image, synth_label

TOL = 2e-4  # fp32 CPU vs fp32 CPU, different op order only


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _feats(b, seed):
    g = torch.Generator().manual_seed(3000 + seed)
    return [torch.randn(b, 1024, 32, 32, generator=g) for _ in range(4)]


@pytest.mark.slow
def test_dinov2_taps(golden_dir):
    G = _g(golden_dir, "dinov2_taps.npz")
    sd = cached_full_state_dict()
    with torch.no_grad():
        for tag, size in (("sq", (512, 512)), ("rect", (512, 1024))):
            taps = R.dinov2_forward(sd, synth_image(1, size, seed=11))
            for i, t in enumerate(taps):
                assert rel_err(sl(t), G[f"{tag}_tap{i}_slice"]) < TOL
                assert rel_err(t[0, -4:, -3:, -5:], G[f"{tag}_tap{i}_tail"]) < TOL
                np.testing.assert_allclose(stats(t), G[f"{tag}_tap{i}_stats"], rtol=1e-3, atol=1e-5)


def test_heads(golden_dir):
    G = _g(golden_dir, "heads.npz")
    sd = cached_full_state_dict()
    lab = synth_label(2, 512, seed=5)
    feats = _feats(2, 1)
    bn = {}
    with torch.no_grad():
        lg = R.linear_head_forward(sd, feats, training=True, bn_out=bn)
        loss, acc, up = R.head_loss(lg, lab)
        assert rel_err(sl(up), G["lin_train_logits_slice"]) < TOL
        np.testing.assert_allclose([loss.item(), acc.item()], G["lin_train_loss"], rtol=1e-4)
        np.testing.assert_allclose(stats(bn["running_mean"] - sd["decode_head.output_upscaling.1.running_mean"]),
                                   G["lin_bn_running_mean_delta"], rtol=1e-3, atol=1e-6)
        np.testing.assert_allclose(stats(bn["running_var"]), G["lin_bn_running_var"], rtol=1e-3)
        le = R.linear_head_forward(sd, feats, training=False)
        assert rel_err(sl(le), G["lin_eval_logits_slice"]) < TOL
        np.testing.assert_allclose(stats(le), G["lin_eval_logits_stats"], rtol=1e-3, atol=1e-5)
        ctx = torch.randn(2, 19, 256, 256, generator=torch.Generator().manual_seed(77))
        keep = torch.from_numpy(G["vfm_mask_rand"]) > 0.2
        hl = R.vfm_head_forward(sd, feats, ctx, keep)
        loss, acc, up = R.head_loss(hl, lab)
        assert rel_err(sl(up), G["vfm_logits_slice"]) < TOL
        np.testing.assert_allclose([loss.item(), acc.item()], G["vfm_loss"], rtol=1e-4)
        ln = R.vfm_head_forward(sd, feats, ctx, None)
        assert rel_err(sl(ln), G["vfm_nomask_logits_slice"]) < TOL
        np.testing.assert_allclose(stats(ln), G["vfm_nomask_logits_stats"], rtol=1e-3, atol=1e-5)


@pytest.mark.slow
def test_train_step_losses_and_grads(golden_dir):
    G = _g(golden_dir, "train_step.npz")
    sd = dict(cached_full_state_dict())
    tk = R.trainable_keys(sd)
    assert sum(sd[k].numel() for k in tk) == int(G["n_trainable"][0])
    for k in tk:
        sd[k] = sd[k].clone().requires_grad_(True)
    img, lab = synth_image(2, 1024, seed=3), synth_label(2, 1024, seed=3)
    np.random.seed(0)
    box = R.get_crop_bbox(1024, 1024, (512, 512), 32)
    assert tuple(box) == tuple(G["hr_crop_box"])
    keep = torch.from_numpy(G["mask_rand"]) > 0.2
    losses = R.forward_train(sd, img, lab, box, keep)
    keys = ["decode_lr.loss_ce", "decode_lr.acc_seg", "decode_hr.loss_ce", "decode_hr.acc_seg"]
    np.testing.assert_allclose([losses[k].item() for k in keys], G["losses"], rtol=2e-4)
    grads = dict(zip(tk, torch.autograd.grad(R.total_loss(losses), [sd[k] for k in tk])))
    norms = [0.0, 0.0, 0.0]
    for k, g in grads.items():
        j = 0 if "lora_" in k else (1 if k.startswith("decode_head") else 2)
        norms[j] += g.double().pow(2).sum().item()
    np.testing.assert_allclose(np.sqrt(norms), G["grad_norms"], rtol=1e-3)
    for name in G.files:
        if name.startswith("grad_slice::"):
            k = name.split("::", 1)[1]
            g = grads[k]
            g2 = g.reshape(g.shape[0], -1) if g.dim() > 1 else g
            assert rel_err(sl(g2), G[name]) < 2e-3, k


@pytest.mark.slow
def test_ms_inference_mask(golden_dir):
    G = _g(golden_dir, "ms_inference.npz")
    sd = cached_full_state_dict()
    thr, conf = G["test_cfg"]
    trace = []
    with torch.no_grad():
        logits = R.ms_inference(sd, synth_image(1, 1024, seed=9), thr=float(thr), conf=float(conf), trace=trace)
    assert np.array_equal(np.array(trace).reshape(-1, 4), G["refined_boxes"])
    assert rel_err(sl(logits), G["logits_slice"]) < TOL
    assert rel_err(logits[0, :, 500:504, 636:644], G["logits_center"]) < TOL
    pred = logits.argmax(1)[0].numpy().astype(np.uint8)
    mism = (pred[::4, ::4] != G["pred_sub4"]).mean()
    assert mism < 1e-4, mism  # near-tie pixels may flip between two fp32 evaluation orders
    if hashlib.sha256(pred.tobytes()).hexdigest() != str(G["pred_sha256"]):
        hist = np.bincount(pred.reshape(-1), minlength=19)
        assert np.abs(hist - G["pred_hist"]).sum() < 64


@pytest.mark.parametrize("mode", ["lr_slide_inference", "hr_slide_inference", "msfull_slide_inference"])
def test_other_slide_modes(golden_dir, mode):
    """The oracle's lr / hr / msfull sliding inference against the reference's OWN MsVFMEncoderDecoder.inference in those modes
    (tests/golden/slide_modes.npz, written by oracle.gen_golden --only slide_modes; Ms_VFM_encoder_decoder.py:278-332), msfull with the
    recorded torch.rand query masks.  Round 2 checked these restatements only against themselves."""
    G = np.load(os.path.join(golden_dir, "slide_modes.npz"))
    sd = cached_full_state_dict()
    stride, crop = tuple(int(v) for v in G["test_cfg_stride_crop"][:2]), tuple(int(v) for v in G["test_cfg_stride_crop"][2:])
    img = synth_image(1, 1024, seed=11)
    with torch.no_grad():
        if mode == "lr_slide_inference":
            lg = R.lr_slide_inference(sd, img, crop, stride)
        elif mode == "hr_slide_inference":
            lg = R.slide_inference(sd, img, crop, stride)
        else:
            keeps = [torch.from_numpy(G["msfull_mask_rand"][j]).reshape(1, 1, 32, 32) > 0.2 for j in range(9)]
            lg = R.msfull_slide_inference(sd, img, mask_keeps=keeps, crop=crop, stride=stride)
    assert rel_err(sl(lg), G[mode + "::logits_slice"]) < 1e-4
    assert rel_err(lg[0, :, 500:504, 636:644], G[mode + "::logits_center"]) < 1e-4
    np.testing.assert_allclose(stats(lg), G[mode + "::logits_stats"], rtol=1e-4)
    pred = lg.argmax(dim=1)[0].numpy().astype(np.uint8)
    assert (pred[::4, ::4] != G[mode + "::pred_sub4"]).mean() < 2e-4
    assert np.abs(np.bincount(pred.reshape(-1), minlength=19) - G[mode + "::pred_hist"]).sum() < 200


@pytest.mark.slow
def test_eva02_taps_and_lora_grads(golden_dir):
    from tests.helpers import eva02_state_dict
    G = _g(golden_dir, "eva02.npz")
    sd = dict(eva02_state_dict())
    cos, sin = R.eva_rope_tables(32, 16, 32)
    assert rel_err(cos[::97, ::5], G["rope_cos_slice"]) < 1e-6 and rel_err(sin[::97, ::5], G["rope_sin_slice"]) < 1e-6
    tk = [k for k in sd if "lora_" in k]
    for k in tk:
        sd[k] = sd[k].clone().requires_grad_(True)
    taps = R.eva02_forward(sd, synth_image(1, 512, seed=31))
    gen = torch.Generator().manual_seed(6)
    loss = 0
    for i, t in enumerate(taps):
        assert rel_err(sl(t), G[f"tap{i}_slice"]) < TOL
        np.testing.assert_allclose(stats(t), G[f"tap{i}_stats"], rtol=1e-3, atol=1e-5)
        loss = loss + (t * torch.randn(t.shape, generator=gen)).sum()
    grads = dict(zip(tk, torch.autograd.grad(loss, [sd[k] for k in tk], allow_unused=True)))
    inert = sum(1 for g in grads.values() if g is None or float(g.abs().max()) == 0.0)
    assert inert == int(G["lora_inert_count"][0])          # q/k/v LoRA never enters the graph
    live = sum(g.double().pow(2).sum().item() for g in grads.values() if g is not None) ** 0.5
    np.testing.assert_allclose(live, G["lora_live_grad_norm"][0], rtol=1e-3)
    for name in G.files:
        if name.startswith("grad_slice::"):
            k = "backbone." + name.split("::", 1)[1]
            assert rel_err(sl(grads[k]), G[name]) < 2e-3, k


def test_clip_taps_and_lora_grads(golden_dir):
    from tests.helpers import clip_state_dict
    G = _g(golden_dir, "clip.npz")
    sd = dict(clip_state_dict())
    tk = [k for k in sd if "lora_" in k]
    for k in tk:
        sd[k] = sd[k].clone().requires_grad_(True)
    taps = R.clip_forward(sd, synth_image(1, 512, seed=51))
    gen = torch.Generator().manual_seed(7)
    loss = 0
    for i, t in enumerate(taps):
        assert rel_err(sl(t), G[f"tap{i}_slice"]) < TOL
        np.testing.assert_allclose(stats(t), G[f"tap{i}_stats"], rtol=1e-3, atol=1e-5)
        loss = loss + (t * torch.randn(t.shape, generator=gen)).sum()
    grads = dict(zip(tk, torch.autograd.grad(loss, [sd[k] for k in tk], allow_unused=True)))
    inert = sum(1 for g in grads.values() if g is None or float(g.abs().max()) == 0.0)
    assert inert == int(G["lora_inert_count"][0])          # the out_proj adapter never enters the graph
    live = sum(g.double().pow(2).sum().item() for g in grads.values() if g is not None) ** 0.5
    np.testing.assert_allclose(live, G["lora_live_grad_norm"][0], rtol=1e-3)
    for name in G.files:
        if name.startswith("grad_slice::"):
            k = "backbone." + name.split("::", 1)[1]
            assert rel_err(sl(grads[k]), G[name]) < 2e-3, k


@pytest.mark.slow
def test_sam_taps_and_lora_grads(golden_dir):
    from tests.helpers import sam_state_dict
    G = _g(golden_dir, "sam.npz")
    sd = dict(sam_state_dict())
    tk = [k for k in sd if "lora_" in k]
    for k in tk:
        sd[k] = sd[k].clone().requires_grad_(True)
    taps = R.sam_forward(sd, synth_image(1, 512, seed=41))
    gen = torch.Generator().manual_seed(9)
    loss = 0
    for i, t in enumerate(taps):
        assert rel_err(sl(t.detach()), G[f"tap{i}_slice"]) < TOL
        assert rel_err(t.detach()[0, -4:, -3:, -5:], G[f"tap{i}_tail"]) < TOL
        np.testing.assert_allclose(stats(t.detach()), G[f"tap{i}_stats"], rtol=1e-3, atol=1e-5)
        loss = loss + (t * torch.randn(t.shape, generator=gen)).sum()
    grads = dict(zip(tk, torch.autograd.grad(loss, [sd[k] for k in tk])))
    tot = sum(g.double().pow(2).sum().item() for g in grads.values()) ** 0.5
    np.testing.assert_allclose(tot, G["lora_grad_norm"][0], rtol=1e-3)
    for name in G.files:
        if name.startswith("grad_slice::"):
            k = "backbone." + name.split("::", 1)[1]
            assert rel_err(sl(grads[k]), G[name]) < 2e-3, k


@pytest.mark.slow
def test_sam_slide_full_depth(golden_dir):
    """BASELINE configs[4] whole (SAM-ViT-H depth 32 + LoRA + LinearHead, `slide` 3 x 3 windows on a 1024^2 image): the oracle against the
    reference's own SAMViT / LoRABackbone / LinearHead run under the restated EncoderDecoder.slide_inference (sam_slide.npz,
    oracle.gen_golden --only sam_slide; sam_vit.py:127-148, configs/_base_/models/lora_sam_linear.py:50-54).  CPU budget: ONE of the nine
    crops - the pixels below row / column 320 (stride 320, crop 512) belong to the first window alone, so the composite there IS that
    window's prediction; the overlap averaging is the same `R.slide_inference` the DINOv2 hr_slide golden pins, and the HIP path is
    compared with the whole composite on the GPU (tests/test_fulldepth_gpu.py)."""
    from tests.helpers import sam_state_dict
    from vfmseg_amd import presets
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.synth import synth_state_dict
    import vfmseg_amd.sam  # noqa: F401
    G = _g(golden_dir, "sam_slide.npz")
    sd = sam_state_dict()
    model = MODELS.build(presets.sam_linear())
    head = {k: tuple(v.shape) if v.dtype != torch.int64 else ((), torch.int64) for k, v in model.state_dict().items() if k.startswith("decode_head.")}
    del model
    sd.update(synth_state_dict(head))
    stride, crop = tuple(int(v) for v in G["test_cfg_stride_crop"][:2]), tuple(int(v) for v in G["test_cfg_stride_crop"][2:])
    assert stride == (320, 320) and crop == (512, 512)
    img = synth_image(1, 1024, seed=47)
    with torch.no_grad():
        lg = R.whole_inference(sd, img[:, :, :512, :512], (512, 512), backbone="sam")      # window (0, 0)
    own = lg[0, :, :320, :320]                                                              # the part no other window touches
    assert rel_err(sl(lg), G["logits_slice"]) < 1e-4
    assert rel_err(own[:, ::16, ::16], G["logits_sub16"][:, :20, :20]) < 1e-4
    pred = own.argmax(dim=0).numpy().astype(np.uint8)
    assert (pred[::4, ::4] != G["pred_sub4"][:80, :80]).mean() < 2e-4


def test_optimizer_rules():
    ck = {"norm": dict(decay_mult=0.0), "query_embed": dict(lr_mult=1.0, decay_mult=0.0)}
    assert R.param_group_options("aux_decoder.transformer_decoder.norm.weight", True, custom_keys=ck) == (1e-4, 0.0)
    assert R.param_group_options("decode_head.fusion_conv.gn.weight", True, custom_keys=ck) == (1e-4, 0.0)
    assert R.param_group_options("decode_head.conv_seg.bias", False, custom_keys=ck) == (1e-4, 0.05)
    assert abs(R.poly_lr(1e-4, 20000) - 1e-4 * 0.5 ** 0.9) < 1e-12
    # AdamW restatement == torch.optim.AdamW
    p = torch.randn(64, generator=torch.Generator().manual_seed(0))
    g = torch.randn(64, generator=torch.Generator().manual_seed(1))
    q = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=1e-3, weight_decay=0.05)
    m = torch.zeros(64)
    v = torch.zeros(64)
    pp = p.clone()
    for step in (1, 2, 3):
        q.grad = g.clone()
        opt.step()
        pp, m, v = R.adamw_step(pp, g, m, v, step, 1e-3, 0.05)
    assert torch.allclose(pp, q.detach(), atol=1e-6)


def test_amp_emulation_follows_the_cuda_autocast_policy():
    """oracle/amp_emul.py (the CPU restatement of torch.autocast(cuda, float16) the fp16 `--amp` tests compare with): dtypes and
    rounding points of the ops the oracle calls, gradient dtypes, and restoration of the patched functions."""
    import torch.nn.functional as F
    from oracle.amp_emul import cuda_autocast
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 16, generator=g, requires_grad=True)
    w = torch.randn(8, 16, generator=g, requires_grad=True)
    b = torch.randn(8, generator=g)
    lin0, mm0, sm0 = F.linear, torch.Tensor.__matmul__, torch.Tensor.softmax
    with cuda_autocast():
        y = F.linear(x, w, b)
        assert y.dtype == torch.float16
        want = (torch.mm(x.half().float(), w.half().float().t()) + b.half().float()).half()   # (torch.mm: `@` is patched in here)
        assert torch.equal(y, want.detach())                            # fp16 operands, fp32 accumulate, ONE rounding of the result
        ln = F.layer_norm(y, (8,))
        assert ln.dtype == torch.float32                                 # fp32 list
        a = y @ y.t()
        assert a.dtype == torch.float16 and a.softmax(dim=-1).dtype == torch.float32
        z = (a.softmax(dim=-1) @ y)                                      # fp32 probabilities are cast down for the product
        assert z.dtype == torch.float16
        res = x[:, :8] + 0.5 * z                                         # fp32 residual + fp16 branch -> fp32
        assert res.dtype == torch.float32
        assert F.gelu(y).dtype == torch.float16 and F.group_norm(y[None].permute(0, 2, 1), 2).dtype == torch.float32
        loss = F.cross_entropy(res, torch.tensor([0, 1, 2, 3, 4])) * 1024.0
        loss.backward()
    assert F.linear is lin0 and torch.Tensor.__matmul__ is mm0 and torch.Tensor.softmax is sm0
    assert x.grad.dtype == torch.float32 and w.grad.dtype == torch.float32
    # the weight gradient went through an fp16 tensor (w.half()): every value is fp16-representable; x.grad has an fp32 residual part
    assert torch.equal(w.grad, w.grad.half().float()) and not torch.equal(x.grad, x.grad.half().float())


@pytest.mark.slow
def test_amp_emulation_of_forward_train_is_an_fp16_sized_perturbation():
    from oracle.amp_emul import cuda_autocast
    from tests.helpers import full_state_dict
    from vfmseg_amd.synth import synth_image, synth_label
    depth = 4
    sd = full_state_dict(depth=depth)
    keep = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(3)) > 0.2
    img, lab = synth_image(1, 1024, seed=60), synth_label(1, 1024, seed=60)
    kw = dict(depth=depth, out_indices=(0, 1, 2, 3))
    with torch.no_grad():
        l32 = R.forward_train(sd, img, lab, (256, 768, 128, 640), keep, **kw)
        with cuda_autocast():
            l16 = R.forward_train(sd, img, lab, (256, 768, 128, 640), keep, **kw)
    for k in ("decode_lr.loss_ce", "decode_hr.loss_ce"):
        e = abs(float(l16[k]) - float(l32[k])) / abs(float(l32[k]))
        assert 0 < e < 2e-3, (k, e)


def _eval_sizes_checks(G, key, lg, tol, mism_tol):
    """The eval_sizes.npz probes of one (size, mode) against logits lg [1, 19, h, w] (shared with tests/test_eval_sizes_gpu.py)."""
    from oracle.gen_golden import eval_sizes_probes
    h, w = lg.shape[2:]
    boxes = R.grid_boxes(h, w)
    for name, (y0, y1, x0, x1) in eval_sizes_probes(h, w, boxes):
        assert rel_err(lg[0, :, y0:y1, x0:x1], G[key + "logits_" + name]) < tol, (key, name)
    pred = lg.argmax(dim=1)[0].cpu().numpy().astype(np.uint8)
    assert pred[::8, ::8].shape == G[key + "pred_sub8"].shape
    assert (pred[::8, ::8] != G[key + "pred_sub8"]).mean() < mism_tol, key
    return pred


@pytest.mark.slow
def test_eval_sizes_inference(golden_dir):
    """The oracle's ms_inference / lr_slide_inference at the reference's DG evaluation sizes (1024x2048, 1080x1920, 720x1280, 1024x1365;
    tests/golden/eval_sizes.npz, written by oracle.gen_golden --only eval_sizes from the reference's own MsVFMEncoderDecoder.inference,
    depth 4): which windows the gate refines, and the logits at a corner, the centre, a window seam and the ragged edge."""
    from tests.helpers import full_state_dict
    G = _g(golden_dir, "eval_sizes.npz")
    from oracle.gen_golden import eval_sizes_seed
    sd = full_state_dict(depth=4)
    kw = dict(depth=4, out_indices=(0, 1, 2, 3))
    stride, crop = tuple(int(v) for v in G["test_cfg_stride_crop"][:2]), tuple(int(v) for v in G["test_cfg_stride_crop"][2:])
    seen = 0
    for h, w in G["sizes"].tolist():
        img = synth_image(1, (h, w), seed=eval_sizes_seed(h, w))
        for mode in ("ms_slide_inference", "lr_slide_inference"):
            key = f"{h}x{w}/{mode}::"
            if key + "logits_stats" not in G.files:
                continue
            seen += 1
            with torch.no_grad():
                if mode == "ms_slide_inference":
                    thr, conf = G[key + "test_cfg"]
                    trace = []
                    lg = R.ms_inference(sd, img, thr=float(thr), conf=float(conf), crop=crop, stride=stride, trace=trace, **kw)
                    assert np.array_equal(np.array(trace).reshape(-1, 4), G[key + "refined_boxes"]), key
                else:
                    lg = R.lr_slide_inference(sd, img, crop, stride, **kw)
            assert tuple(lg.shape[2:]) == ((h, w) if mode == "ms_slide_inference" else (h // 2 * 2, w // 2 * 2))
            _eval_sizes_checks(G, key, lg, 1e-4, 2e-4)
            np.testing.assert_allclose(stats(lg), G[key + "logits_stats"], rtol=1e-4, atol=1e-6)
            assert np.abs(np.bincount(lg.argmax(dim=1).reshape(-1).numpy(), minlength=19) - G[key + "pred_hist"]).sum() < 200
    assert seen == 7
