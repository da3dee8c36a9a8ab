"""Writes tests/golden/dacs.npz: two iterations of DACS self-training (Rein DINOv2 at tests/segformer_helpers.DEPTH + SegformerHead, B = 2,
512^2, synthetic source / target) computed by the REFERENCE's own rein/models/uda/dacs.py and dacs_transforms.py, imported through
oracle/ref_shim.py.  Data only.  Runs where the reference tree exists; the tests read the .npz and tests/dacs_helpers.py only.

    python tools/gen_dacs_golden.py

Route taken: the reference's own DACS.forward_train runs, unmodified, for two iterations (iteration 0: EMA init; iteration 1: EMA update
with a = 0.5), fp32 on the CPU.  What the shim lacks is defined HERE (oracle/ stays as it is): mmseg.models.EncoderDecoder / build_head (the
shim's restated EncoderDecoder, its registry's build), timm.models.layers.DropPath, the refrein.models.uda package path, mmengine's
parse_losses, a four-method optimiser-wrapper stub (scale_loss, backward, step, zero_grad around torch.optim.AdamW with
tests/dacs_helpers.OPTIM), and debug_img_interval = NaN (`local_iter % nan == 0` is never true: nothing is drawn, get_pred_label is
never reached).  SegformerHead is the restatement of tools/gen_segformer_golden.py.

The generator chooses pseudo_threshold (the 25th percentile of the initial teacher's float64 max-probability, four decimals) and ASSERTS that the
fixture can see the feature: 0.2 < ratio < 0.8, every image mixes a class in and leaves one out, and negating mix_weight or keeping the
ignore rows moves loss_tgt by at least 10 %."""
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import ref_shim  # noqa: E402
from tests import dacs_helpers as D  # noqa: E402
from tests import segformer_helpers as S  # noqa: E402
from tests.helpers import sl  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label  # noqa: E402
import gen_segformer_golden as GS  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def parse_losses(self, losses):
    """mmengine BaseModel.parse_losses."""
    log_vars = [(k, v.mean()) for k, v in losses.items()]
    loss = sum(v for k, v in log_vars if "loss" in k)
    log_vars.insert(0, ("loss", loss))
    return loss, dict(log_vars)


class OptimStub:
    """The four methods DACS.train_step / train_and_update call, around torch.optim.AdamW."""

    def __init__(self, params):
        oc = dict(D.OPTIM)
        oc.pop("type")
        self.opt = torch.optim.AdamW(params, **oc)

    def scale_loss(self, loss):
        return loss

    def backward(self, loss):
        loss.backward()

    def step(self):
        self.opt.step()

    def zero_grad(self):
        self.opt.zero_grad()


def load_reference():
    M = GS._models()
    import mmseg.models as mm
    mm.EncoderDecoder, mm.build_head = ref_shim.EncoderDecoder, M.build

    class DropPath(nn.Module):
        pass

    sys.modules["timm.models.layers"].DropPath = DropPath
    pkg = types.ModuleType(ref_shim.PKG + ".models.uda")
    pkg.__path__ = [os.path.join(ref_shim.REF_ROOT, "rein", "models", "uda")]
    pkg.__package__ = pkg.__name__
    sys.modules[pkg.__name__] = pkg
    dacs = ref_shim.ref_import("models.uda.dacs")
    dacs.DACS.parse_losses = parse_losses
    return M, dacs


def _sub(t):
    return t.reshape(D.BATCH, D.SIZE, D.SIZE)[:, ::D.SUB, ::D.SUB]


def main():
    torch.manual_seed(0)
    M, dacs = load_reference()
    cfg = D.dacs_config(0.5)
    cfg.update(debug_img_interval=float("nan"), work_dir=None)
    model = M.build(cfg)
    model.load_state_dict(D.dacs_state_dict(), strict=False)
    model.with_auxiliary_head = False   # (mmseg's EncoderDecoder property; the shim's restatement has with_neck only)
    model.train()
    GS._zero_dropout(model)
    model.mean, model.std = model.data_preprocessor.mean, model.data_preprocessor.std

    src, tgt = synth_image(D.BATCH, D.SIZE, seed=D.SRC_SEED), synth_image(D.BATCH, D.SIZE, seed=D.TGT_SEED)
    lab = synth_label(D.BATCH, D.SIZE, seed=D.SRC_SEED)
    meta = dict(img_shape=(D.SIZE, D.SIZE), ori_shape=(D.SIZE, D.SIZE), pad_shape=(D.SIZE, D.SIZE))
    img_dict = dict(inputs=src, data_samples=[ref_shim.SegDataSample(lab[i], dict(meta)) for i in range(D.BATCH)])
    tgt_dict = dict(inputs=tgt, data_samples=[ref_shim.SegDataSample(torch.zeros_like(lab[i]), dict(meta)) for i in range(D.BATCH)])

    # the threshold: the 25th percentile of the initial teacher's (= the student head's) max-probability, float64 softmax of its fp32 logits:
    # three pixels in four are confident, which keeps the pseudo-weighted part of loss_tgt large enough for the ignore rows to show
    with torch.no_grad():
        low0 = model.decode_head(model.extract_feat(tgt))
    p0 = D.pseudo_labels(low0.permute(0, 2, 3, 1), (D.SIZE, D.SIZE), 0.5)["prob"]
    thr = round(float(p0.flatten().quantile(0.25)), 4)
    model.pseudo_threshold = thr
    print("pseudo_threshold", thr)

    rec = {}
    real_fwd = model.ema_head.forward   # (the shim's predict calls forward directly: a forward hook would not fire)

    def ema_fwd(inputs):
        rec["ema_low"] = real_fwd(inputs).detach().clone()
        return rec["ema_low"]

    model.ema_head.forward = ema_fwd
    real_masks = dacs.get_class_masks
    dacs.get_class_masks = lambda labels: rec.setdefault("masks", []).append(real_masks(labels)) or rec["masks"][-1]
    real_ce = model.decode_head.loss_decode.forward

    def ce(cls_score, label, weight=None, ignore_index=-100, **kw):
        if weight is not None:
            rec["tgt_loss_in"] = (cls_score.detach(), label.detach(), weight.detach())
        return real_ce(cls_score, label, weight=weight, ignore_index=ignore_index, **kw)

    model.decode_head.loss_decode.forward = ce
    trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad and not n.startswith("ema_head.")]
    ow = OptimStub([p for _, p in trainable])
    out = {"pseudo_threshold": np.array([thr]), "seeds": np.array([D.SRC_SEED, D.TGT_SEED, D.PY_SEED, D.NP_SEED, S.DEPTH]),
           "trainable_names": np.array(sorted(n for n, _ in trainable))}
    random.seed(D.PY_SEED)
    np.random.seed(D.NP_SEED)
    for it in range(2):
        k = f"it{it}::"
        log = model.forward_train(img_dict, tgt_dict, ow)
        assert not any(n.startswith("ema_head.") and p.requires_grad for n, p in model.named_parameters())
        out[k + "log_vars"] = np.array([float(log[n]) for n in D.LOG_KEYS])
        # pseudo-labels as the reference formed them, and what float64 says about the same fp32 teacher logits
        ref = D.pseudo_labels(rec["ema_low"].permute(0, 2, 3, 1), (D.SIZE, D.SIZE), thr)
        sm = torch.softmax(F.interpolate(rec["ema_low"], size=(D.SIZE, D.SIZE), mode="bilinear", align_corners=False), dim=1)
        prob, ps = torch.max(sm, dim=1)
        count = int(prob.ge(thr).sum())
        total = ps.numel()
        ratio = count / total
        assert 0.2 < ratio < 0.8, ratio
        masks = torch.cat(rec["masks"][-1]).reshape(D.BATCH, D.SIZE, D.SIZE)
        for b in range(D.BATCH):
            present = torch.unique(lab[b]).tolist()
            mixed_in = torch.unique(lab[b][0][masks[b] > 0]).tolist()
            assert 0 < len(mixed_in) < len(present), (present, mixed_in)
        cls_score, mixed_lbl, mix_weight = rec["tgt_loss_in"]
        out[k + "count_total_band"] = np.array([count, total, ref["n_band"]])
        out[k + "pseudo_label_sub"] = _sub(ps).numpy().astype(np.uint8)
        out[k + "unsure_sub"] = _sub(~ref["sure_label"]).numpy()
        out[k + "n_unsure"] = np.array([int((~ref["sure_label"]).sum())])
        out[k + "mask_sub"] = _sub(masks).numpy().astype(np.uint8)
        out[k + "mask_sum"] = masks.sum((1, 2)).numpy()
        out[k + "mixed_lbl_sub"] = _sub(mixed_lbl).numpy().astype(np.uint8)
        out[k + "mix_weight_sum"] = np.array([mix_weight.double().sum().item()])
        if it == 1:
            out[k + "ema_low"] = rec["ema_low"].numpy().astype(np.float32)   # the teacher logits [B,C,h,w] the CPU test re-derives labels from
        # what the fixture must be able to see
        per = F.cross_entropy(cls_score.double(), mixed_lbl, reduction="none", ignore_index=255)
        loss_tgt = (per * mix_weight.double()).mean().item()
        assert abs(loss_tgt - out[k + "log_vars"][3]) < 1e-5 * abs(loss_tgt)
        w_rows = torch.where(masks > 0, torch.ones(()), torch.full((), ratio)).double()
        moved = [abs((per * -mix_weight.double()).mean().item() - loss_tgt) / abs(loss_tgt), abs((per * w_rows).mean().item() - loss_tgt) / abs(loss_tgt)]
        assert min(moved) >= 0.1, moved
        out[k + "sensitivity"] = np.array(moved)
        # gradients after the two backward passes
        norms = {"backbone": 0.0, "head": 0.0}
        out[k + "no_grad"] = np.array(sorted(n for n, p in trainable if p.grad is None))   # (Rein weights the configuration never uses)
        for n, p in trainable:
            if p.grad is None:
                continue
            norms["head" if n.startswith("decode_head.") else "backbone"] += p.grad.double().pow(2).sum().item()
            if n.startswith("decode_head.") or ".reins." in n:
                out[k + f"grad_slice::{n}"] = sl(GS._grad2d(p.grad) if p.grad.dim() else p.grad.reshape(1))
        out[k + "grad_norms"] = np.sqrt(np.array([norms["backbone"], norms["head"]]))
        print(f"iteration {it}: log vars {np.round(out[k + 'log_vars'], 5)}, ratio {ratio:.4f} ({count}/{total}, band {ref['n_band']}, unsure labels "
              f"{int((~ref['sure_label']).sum())}), sensitivity {np.round(moved, 3)}, grad norms {out[k + 'grad_norms']}")
        ow.step()
        ow.zero_grad()
    # the teacher after iteration 1's update (a = 0.5 of the initial weights and the once-stepped student)
    for n, p in model.ema_head.named_parameters():
        out[f"ema_slice::{n}"] = sl(GS._grad2d(p.data) if p.dim() else p.data.reshape(1))
    path = os.path.join(GOLD, "dacs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
