"""Writes tests/golden/hrda.npz from the REFERENCE's own HRDA modules (rein/models/heads/hrda.py, attention_head.py, linear_head.py,
rein/models/segmentors/hrda_encoder_decoder.py, imported through oracle/ref_shim.py): data only - slices, statistics, losses, gradient
norms, crop boxes and parameter names.  Runs where the reference tree exists; the tests read the .npz and tests/hrda_helpers.py only.

    python tools/gen_hrda_golden.py

Three names the shim lacks are added to its modules at run time, before the reference files are imported.  The generator ASSERTS that
the fixture can see the feature: fused logits far from both up2(lr) and the inserted HR logits, attention neither flat nor saturated,
the masked crop border inside the sampled slices."""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests.helpers import sl, stats  # noqa: E402
from tests import hrda_helpers as H  # noqa: E402
from vfmseg_amd import presets  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label, synth_like  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
DEPTH, TRAIN_SEED, EVAL_SEED = 4, H.TRAIN_SEED, H.EVAL_SEED


def _crop(img, box):
    y1, y2, x1, x2 = box
    return img[..., y1:y2, x1:x2]


def _models():
    ref_shim.install()

    class DepthwiseSeparableConvModule(nn.Module):   # imported by the reference's head utilities, never built here
        pass

    sys.modules["mmcv.cnn"].DepthwiseSeparableConvModule = DepthwiseSeparableConvModule
    sys.modules[ref_shim.PKG + ".utils"].crop = _crop
    sys.modules["mmseg.models"].build_head = lambda cfg: ref_shim.MODELS.build(cfg)

    def _decode_head_forward_train(self, inputs, data_samples):   # mmseg 1.2.2 EncoderDecoder, restated
        return ref_shim.add_prefix(self.decode_head.loss(inputs, data_samples, self.train_cfg), "decode")

    ref_shim.EncoderDecoder._decode_head_forward_train = _decode_head_forward_train
    ref_shim.EncoderDecoder.with_auxiliary_head = False
    M = ref_shim.load_all()
    ref_shim.ref_import("models.heads.attention_head")
    ref_shim.ref_import("models.heads.hrda")
    ref_shim.ref_import("models.segmentors.hrda_encoder_decoder")
    return M


def _zero_dropout(m):
    for mod in m.modules():
        if isinstance(mod, (nn.Dropout, nn.Dropout2d)):
            mod.p = 0.0


def _range_dist(a, b):
    return ((a - b).abs().max() / a.abs().max()).item()


# ------------------------------------------------------------------------------------------------ fusion arithmetic, small
class _Replay(nn.Module):
    """stands in for a sub-head: returns the given tensors in call order"""

    def __init__(self, outs):
        super().__init__()
        self.outs, self.i = outs, 0

    def forward(self, inp):
        o = self.outs[self.i % len(self.outs)]
        self.i += 1
        return o


def gen_fuse_small(M, out):
    """HRDAHead.forward of the reference on given LR / attention / HR logits (its sub-heads replaced by tensors), float64: the fusion
    arithmetic alone, with every gradient.  Pins tests/hrda_helpers.fuse_ref."""
    cfg = dict(presets.dinov2_hrda()["decode_head"], scales=[0.5, 1], enable_hr_crop=True)
    head = M.build(cfg).double()
    head.debug = False
    cases = {"inner": (2, 3, 2, 2, 8, 8, (8, 40, 16, 48)), "corner": (2, 3, 2, 2, 8, 8, (32, 64, 32, 64)), "nocrop": (2, 3, 2, 2, 8, 8, None),
             "wide": (1, 3, 2, 6, 8, 24, (0, 32, 64, 128))}
    for i, (name, (B, C, ha, wa, h, w, box)) in enumerate(cases.items()):
        hc, wc = ((box[1] - box[0]) // 4, (box[3] - box[2]) // 4) if box else (2 * h, 2 * w)
        lr, a, hr, dF = H.fuse_inputs(B, C, ha, wa, h, w, hc, wc, seed=900 + i)
        t = [v.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for v in (lr, a, hr)]
        head.head, head.scale_attention = _Replay([t[0], t[2]]), _Replay([t[1]])
        head.set_hr_crop_box(box)
        fused, lrs, _ = head.forward([[t[0]], [t[2]]])
        fused.backward(dF.double().permute(0, 3, 1, 2))
        head.reset_crop()
        k = f"fuse_{name}::"
        out[k + "shape"] = np.array([B, C, ha, wa, h, w, hc, wc, 900 + i] + list(box or (-1, -1, -1, -1)))
        nhwc = lambda v: v.detach().permute(0, 2, 3, 1).contiguous().numpy().astype(np.float32)   # float64 arithmetic, stored in fp32
        out[k + "fused"], out[k + "lr_scaled"] = nhwc(fused), nhwc(lrs)
        out[k + "d_lr"], out[k + "d_a"], out[k + "d_hr"] = nhwc(t[0].grad), nhwc(t[1].grad), nhwc(t[2].grad)
    print("fuse_small:", list(cases))


# ------------------------------------------------------------------------------------------------ head level
def gen_heads(M, out):
    cfg = dict(presets.dinov2_hrda()["decode_head"], scales=[0.5, 1], enable_hr_crop=True)
    head = M.build(cfg)
    head.debug = False
    sd = H.hrda_head_state_dict(prefix="")
    out["head_param_names"] = np.array(sorted(head.state_dict()))
    assert sorted(sd) == sorted(head.state_dict()), set(sd) ^ set(head.state_dict())
    lab = synth_label(2, 1024, seed=H.HEAD_SEED)
    for name, box in H.HEAD_BOXES.items():
        head.load_state_dict(sd)
        head.zero_grad()
        head.train()
        _zero_dropout(head)
        lr_f, hr_f = H.head_feats()
        lr_f, hr_f = [t.requires_grad_(True) for t in lr_f], [t.requires_grad_(True) for t in hr_f]
        head.set_hr_crop_box(box)
        fused, lrs, hr = head.forward([lr_f, hr_f])
        losses = head.losses((fused, lrs, hr), lab)
        (losses["loss_seg"] + losses["hr.loss_seg"]).backward()
        k = f"head_{name}::"
        Y0, Y1, X0, X1 = H.scale_box(box, 4)
        with torch.no_grad():
            a_log = head.scale_attention(lr_f)
            s = torch.sigmoid(a_log)
        # what the fixture must be able to see
        att_mean, att_std = s.mean().item(), s.std().item()
        assert att_std >= 0.1 and 0.2 < att_mean < 0.8, (att_mean, att_std)
        up_lr = F.interpolate(lrs, scale_factor=2, mode="bilinear", align_corners=False)
        ins = torch.zeros_like(fused)
        ins[:, :, Y0:Y1, X0:X1] = hr
        d_lr, d_hr = _range_dist(fused[:, :, Y0:Y1, X0:X1], up_lr[:, :, Y0:Y1, X0:X1]), _range_dist(fused[:, :, Y0:Y1, X0:X1], hr)
        assert d_lr >= 0.3 and d_hr >= 0.3, (d_lr, d_hr)
        out[k + "att_mean_std"] = np.array([att_mean, att_std])
        out[k + "fused_vs_uplr_vs_hr"] = np.array([d_lr, d_hr])
        out[k + "box"] = np.array(box)
        # slices: the crop's top-left border (mask decays across it) and its bottom-right corner
        ys, xs = slice(max(Y0 - 4, 0), max(Y0 - 4, 0) + 8), slice(max(X0 - 4, 0), max(X0 - 4, 0) + 8)
        ye, xe = slice(min(Y1 + 4, 256) - 8, min(Y1 + 4, 256)), slice(min(X1 + 4, 256) - 8, min(X1 + 4, 256))
        assert ys.start < Y0 < ys.stop or Y0 == 0, "the masked border must lie inside the slice"
        out[k + "fused_tl"], out[k + "fused_br"] = fused[:, :, ys, xs].detach().numpy(), fused[:, :, ye, xe].detach().numpy()
        out[k + "fused_stats"], out[k + "lr_stats"], out[k + "hr_stats"] = stats(fused), stats(lrs), stats(hr)
        out[k + "lr_slice"] = lrs[:, :, Y0 // 2 - 4:Y0 // 2 + 4, X0 // 2 - 4:X0 // 2 + 4].detach().numpy()
        out[k + "hr_slice"] = sl(hr)
        out[k + "att_logits_slice"] = sl(a_log)
        out[k + "losses"] = np.array([losses[n].item() for n in ("loss_seg", "acc_seg", "hr.loss_seg", "hr.acc_seg")])
        nograd = []
        for n, p in head.named_parameters():
            if p.grad is None:
                nograd.append(n)
                continue
            g = p.grad
            out[k + f"grad_slice::{n}"] = sl(g.reshape(g.shape[0], -1) if g.dim() > 1 else g)
            out[k + f"grad_norm::{n}"] = np.array([g.double().norm().item()])
        out[k + "no_grad"] = np.array(sorted(nograd))
        for i, t in enumerate(lr_f + hr_f):
            out[k + f"tap_grad_norm::{i}"] = np.array([t.grad.double().norm().item()])
            if i % 4 == 0:   # one LR and one HR tap
                out[k + f"tap_grad_slice::{i}"] = sl(t.grad[:, :, 8:, 8:])
        bn = head.head.output_upscaling[1]
        out[k + "bn_running_mean_slice"], out[k + "bn_running_var_slice"] = sl(bn.running_mean).copy(), sl(bn.running_var).copy()
        out[k + "bn_num_batches_tracked"] = np.array([int(bn.num_batches_tracked)])
        print("head", name, "att mean / std %.3f %.3f" % (att_mean, att_std), "fused vs up2(lr) / hr %.2f %.2f" % (d_lr, d_hr),
              "losses", out[k + "losses"], "no grad:", nograd, "bn tracked", int(bn.num_batches_tracked))


# ------------------------------------------------------------------------------------------------ segmentor
def build_reference_model(M):
    cfg = presets.dinov2_hrda(depth=DEPTH)
    cfg["backbone"]["backbone"]["out_indices"] = list(range(DEPTH))
    cfg["backbone"]["Lora_config"]["lora_dropout"] = 0.0
    bb = M.build(cfg["backbone"]["backbone"])
    base_sd = synth_like(bb.state_dict())
    del bb
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(base_sd, f.name)
        ck = f.name
    cfg["backbone"]["checkpoint"] = ck
    model = M.build(cfg)
    os.unlink(ck)
    model.debug = model.decode_head.debug = False
    sd = model.state_dict()
    want = H.hrda_model_state_dict(DEPTH)
    assert sorted(sd) == sorted(want), sorted(set(sd) ^ set(want))[:8]
    for k in sd:   # the base weights went through the reference's own loader: they must equal the recipe's
        if ".base_layer." in k or ("backbone." in k and "lora_" not in k):
            assert torch.equal(sd[k], want[k]), k
    model.load_state_dict(want)
    model._synth_sd = {k: v.clone() for k, v in want.items()}
    return model


def gen_train_step(model, out):
    model.load_state_dict(model._synth_sd)
    model.zero_grad()
    model.train()
    _zero_dropout(model)
    img, lab = synth_image(2, 1024, seed=TRAIN_SEED), synth_label(2, 1024, seed=TRAIN_SEED)
    samples = [ref_shim.SegDataSample(gt=lab[i]) for i in range(2)]
    np.random.seed(H.NP_SEED)
    boxes = []
    orig = model.decode_head.set_hr_crop_box
    model.decode_head.set_hr_crop_box = lambda b: (boxes.append(tuple(int(v) for v in b)), orig(b))[1]
    losses = model.loss(img, samples)
    model.decode_head.set_hr_crop_box = orig
    keys = ["decode.loss_seg", "decode.acc_seg", "decode.hr.loss_seg", "decode.hr.acc_seg"]
    assert sorted(losses) == sorted(keys), sorted(losses)
    (losses[keys[0]] + losses[keys[2]]).backward()
    out["train_np_seed"], out["train_box"] = np.array([H.NP_SEED]), np.array(boxes[0])
    np.random.seed(H.NP_SEED)
    out["train_boxes_stream"] = np.array(H.np_boxes(H.NP_SEED, 6))   # the same stream, six draws (resume tests)
    assert tuple(out["train_boxes_stream"][0]) == boxes[0]
    out["train_losses"] = np.array([losses[k].item() for k in keys])
    out["train_loss_keys"] = np.array(keys)
    norms, n_train, nograd = {"lora": 0.0, "head": 0.0}, 0, []
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.grad is None:
            nograd.append(n)
            continue
        n_train += p.numel()
        norms["lora" if "lora_" in n else "head"] += p.grad.double().pow(2).sum().item()
        if "blocks.0." in n or f"blocks.{DEPTH - 1}." in n or n.startswith("decode_head"):
            g = p.grad
            out[f"train_grad_slice::{n}"] = sl(g.reshape(g.shape[0], -1) if g.dim() > 1 else g)
    out["train_grad_norms"] = np.sqrt(np.array([norms["lora"], norms["head"]]))
    out["train_n_trainable"], out["train_no_grad"] = np.array([n_train]), np.array(sorted(nograd))
    bn = model.decode_head.head.output_upscaling[1]
    # copies: sl() of a 1-D buffer is a view of it, and gen_inference reloads the initial state into the same buffers
    out["train_bn_running_mean_slice"], out["train_bn_running_var_slice"] = sl(bn.running_mean).copy(), sl(bn.running_var).copy()
    for n, v in (("running_mean", out["train_bn_running_mean_slice"]), ("running_var", out["train_bn_running_var_slice"])):
        start = sl(model._synth_sd["decode_head.head.output_upscaling.1." + n])
        assert np.abs(v - start).max() > 1e-2 * np.abs(start).max(), "the BatchNorm statistics must have moved from their initial values"
    out["train_bn_num_batches_tracked"] = np.array([int(bn.num_batches_tracked)])
    out["model_param_names"] = np.array(sorted(model.state_dict()))
    print("train step: box", boxes[0], "losses", out["train_losses"], "grad norms", out["train_grad_norms"], "no grad:", nograd,
          "bn tracked", int(bn.num_batches_tracked))


def _record_logits(out, key, logits):
    top2 = logits.topk(2, dim=1)[0]
    margin = ((top2[:, 0] - top2[:, 1]) / (logits.max() - logits.min()))[0]
    out[key + "logits_stats"] = stats(logits)
    out[key + "logits_grid"] = logits[0, :, 5::64, 5::64].numpy().copy()
    out[key + "logits_slice"] = sl(logits[0, :, 508:, 508:])
    out[key + "pred_sub32"] = logits.argmax(1)[0, ::32, ::32].numpy().astype(np.uint8)
    out[key + "margin_sub32"] = margin[::32, ::32].numpy().astype(np.float32)


def gen_inference(model, out):
    model.load_state_dict(model._synth_sd)
    model.eval()
    with torch.no_grad():
        img = synth_image(1, 1024, seed=EVAL_SEED)
        metas = [dict(ori_shape=(1024, 1024), img_shape=(1024, 1024), pad_shape=(1024, 1024), padding_size=[0, 0, 0, 0])]
        _record_logits(out, "encdec_1024::", model.encode_decode(img, metas))
        img = synth_image(1, (1024, 1536), seed=EVAL_SEED + 1)
        metas = [dict(ori_shape=(1024, 1536), img_shape=(1024, 1536), pad_shape=(1024, 1536), padding_size=[0, 0, 0, 0])]
        _record_logits(out, "slide_1024x1536::", model.slide_inference(img, metas))
    print("inference:", out["encdec_1024::logits_stats"], out["slide_1024x1536::logits_stats"])


def main():
    torch.manual_seed(0)
    M = _models()
    out = {"seeds_depth": np.array([H.HEAD_SEED, TRAIN_SEED, EVAL_SEED, DEPTH])}
    gen_fuse_small(M, out)
    gen_heads(M, out)
    model = build_reference_model(M)
    gen_train_step(model, out)
    gen_inference(model, out)
    path = os.path.join(GOLD, "hrda.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 320 * 1024


if __name__ == "__main__":
    main()
