#!/usr/bin/env python
"""Timing of the Dice loss on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 500 python tools/dice_time.py`).

1. The loss of low-resolution logits against full-resolution labels, batch 2, 19 classes, 1024^2 labels, for the x4 head (256 x 256 logits)
   and the x16 head (64 x 64), softmax and sigmoid activation:
     fused     vfm_upsample_dice_sums + vfm_dice_finish (the forward) and with vfm_upsample_dice_bwd (forward + gradient)
     composed  ops.resize_bilinear + torch softmax / sigmoid + the sums + torch autograd, as mmseg writes it (VFMSEG_DICE_FUSED=0)
     ce        the fused cross-entropy (vfm_upsample_ce + vfm_ce_finish: loss, accuracy and gradient in one pass), for scale
   Device events bracket `--reps` repetitions after a warm-up; the forms alternate over `--rounds` rounds (median [min .. max]).  Logits
   and labels rotate through a ring larger than the 256-MB last-level cache.  The peak extra memory of one call of each form is logged too.
2. ms per train step of presets.dinov2_linear() at `--depth` (batch 2 x 512^2) with cross-entropy alone and with the CE + Dice list (fused
   and composed), alternating in one process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from segformer_time import _spread, _time  # noqa: E402

B, C, H, EPS = 2, 19, 1024, 1e-3


def loss_times(h, use_sigmoid, reps, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import dice_loss, ops
    g = torch.Generator().manual_seed(5)
    s = H // h
    nset = max(3, -(-320 * 2 ** 20 // (B * H * H * 8)))   # labels alone: 320 MB, beyond the last-level cache
    sets = []
    for _ in range(nset):
        low = torch.randint(0, C, (B, h, h), generator=g)
        lab = low.repeat_interleave(s, 1).repeat_interleave(s, 2).contiguous()
        lab[:, : H // 20] = 255
        sets.append(((torch.randn(B, h, h, C, generator=g) * 2).cuda(), lab.cuda()))
    it = [0]

    def nxt():
        it[0] += 1
        return sets[it[0] % nset]

    def composed():
        lg, lab = nxt()
        x = lg.detach().requires_grad_(True)
        loss, _ = dice_loss.composed(x, lab, use_sigmoid, False, EPS, -1, 3.0)
        loss.backward()
        return loss.detach(), x.grad

    def fused():
        lg, lab = nxt()
        loss, _, _, dl = ops.upsample_dice(lg, lab, use_sigmoid, False, EPS, -1, need_grad=True, grad_scale=3.0 / B)
        return loss * 3.0, dl

    forms = {
        "fused_forward_us": lambda: ops.upsample_dice(*nxt(), use_sigmoid, False, EPS, -1, need_grad=False),
        "fused_us": lambda: ops.upsample_dice(*nxt(), use_sigmoid, False, EPS, -1, need_grad=True),
        "composed_us": composed,
        "ce_us": lambda: ops.upsample_ce_loss_acc(*nxt(), 255, need_grad=True),
    }
    vals = {k: [] for k in forms}
    for rnd in range(rounds + 1):
        for k, fn in forms.items():
            t = _time(fn, reps)
            if rnd:
                vals[k].append(t)
    peak = {}
    for k in ("fused_us", "composed_us", "ce_us"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        forms[k]()
        torch.cuda.synchronize()
        peak[k.replace("_us", "_peak_extra_mb")] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    it[0] = 0
    (l1, g1) = fused()
    it[0] = 0
    (l0, g0) = composed()
    rec = dict(what=f"Dice loss (plain form, {'sigmoid' if use_sigmoid else 'softmax'}), us per call: batch {B}, {C} classes, {h}x{h} logits -> {H}x{H} labels (x{s})",
               ring_sets=nset, loss_fused=round(l1.item(), 7), loss_composed=round(l0.item(), 7),
               grad_rel_diff=float((g1 - g0).abs().max() / g0.abs().max()))
    rec.update({k: _spread(v) for k, v in vals.items()})
    rec.update(peak)
    print(json.dumps(rec), flush=True)


def step_times(step_reps, mode, depth, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label, synth_like
    set_compute_dtype(mode)
    cfg = presets.dinov2_linear(depth=depth)
    if depth < 24:
        cfg["backbone"]["backbone"]["out_indices"] = [min(i, depth - 1) for i in range(4)]
    model = MODELS.build(cfg)
    sd = synth_like(model.state_dict())
    sd.update(synth_like({k: p.detach() for k, p in model.named_parameters() if k not in sd}))
    model.load_state_dict(sd)
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    lab = synth_label(2, 512, seed=1)
    data = dict(inputs=synth_image(2, 512, seed=1).cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
    head = model.decode_head
    ce_alone = head.loss_decode
    both = torch.nn.ModuleList([MODELS.build(c) for c in presets.ce_dice_loss()])
    vals = {"ce": [], "ce_dice_fused": [], "ce_dice_composed": []}
    for rnd in range(rounds + 1):
        for key in vals:
            head.loss_decode = ce_alone if key == "ce" else both
            both[1].fused = key != "ce_dice_composed"
            t = _time(lambda: model.train_step(data, ow), step_reps, warm=5) / 1e3
            if rnd:
                vals[key].append(t)
    rec = dict(mode=mode, depth=depth, what="presets.dinov2_linear(): ms per train step, batch 2 x 512^2, CrossEntropyLoss alone and presets.ce_dice_loss()")
    rec.update({"train_step_ms_" + k: _spread(v, 3) for k, v in vals.items()})
    ce = rec["train_step_ms_ce"]["median"]
    rec["dice_share_of_step_pct"] = round(100.0 * (rec["train_step_ms_ce_dice_fused"]["median"] - ce) / ce, 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="reported rounds per figure (after one dropped round)")
    ap.add_argument("--mode", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dice_time.py measures on the GPU; none found")
    assert a.reps >= 100, "at least 100 repetitions per figure"
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps)), flush=True)
    for h in (256, 64):
        for use_sigmoid in (False, True):
            loss_times(h, use_sigmoid, a.reps, a.rounds)
    if not a.skip_model:
        step_times(a.step_reps, a.mode, a.depth, a.rounds)


if __name__ == "__main__":
    main()
