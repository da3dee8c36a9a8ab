#!/usr/bin/env python
"""Timing of the OHEM pixel sampler on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 500 python tools/ohem_time.py`).

1. The chain that turns low-resolution logits into the sampler's weight map, batch 2, 19 classes, thresh 0.7, min_kept 100000, at
   128 x 128 logits -> 1024^2 labels and 32 x 32 -> 512^2, on a spread input (randn * 2 logits) and a saturated one (the label's logit raised
   by 12: nearly every p rounds near 1, all lanes of a wave fall into one histogram bin):
     fused    vfm_ohem_prob, vfm_ohem_threshold (three picks, two histogram passes), vfm_label_weight - each alone and the three in a row
     composed ops.resize_bilinear + torch.softmax + gather + torch.sort + compare, as mmseg writes it (VFMSEG_OHEM_FUSED=0)
   Device events bracket `--reps` repetitions after a warm-up; the forms alternate over `--rounds` rounds (median [min .. max]).  Logits
   and labels rotate through a ring larger than the 256-MB last-level cache.  The peak extra memory of one call of each form is logged too.
2. ms per train step of presets.dinov2_linear() at `--depth` (batch 2 x 512^2) with and without the sampler, alternating in one process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from segformer_time import _spread, _time  # noqa: E402

THRESH, MIN_KEPT, B, C = 0.7, 100000, 2, 19


class _Ctx:
    ignore_index = 255


def chain_times(h, H, kind, reps, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import ops
    from vfmseg_amd.loss_options import OHEMPixelSampler, pixel_weights
    g = torch.Generator().manual_seed(5)
    s = H // h
    nset = max(3, -(-320 * 2 ** 20 // (B * H * H * 8)))   # labels alone: 320 MB, beyond the last-level cache
    sets = []
    for _ in range(nset):
        low = torch.randint(0, C, (B, h, h), generator=g)
        lab = low.repeat_interleave(s, 1).repeat_interleave(s, 2).contiguous()
        lab[:, : H // 20] = 255
        lg = torch.randn(B, h, h, C, generator=g) * 2
        if kind == "saturated":
            lg.scatter_add_(3, low.unsqueeze(3), torch.full((B, h, h, 1), 12.0))
        sets.append((lg.cuda(), lab.cuda()))
    it = [0]

    def nxt():
        it[0] += 1
        return sets[it[0] % nset]

    fused, composed = OHEMPixelSampler(_Ctx(), THRESH, MIN_KEPT), OHEMPixelSampler(_Ctx(), THRESH, MIN_KEPT)
    fused.fused, composed.fused = True, False
    lg0, lab0 = sets[0]
    p0, st0 = ops.ohem_prob(lg0, lab0, THRESH)
    ops.ohem_threshold(p0, st0, MIN_KEPT * B, THRESH)

    _, st1 = ops.ohem_prob(lg0, lab0, THRESH)

    def threshold_alone():   # on a fresh copy of the state that vfm_ohem_prob left (the 12-KB copy is part of the figure)
        ops.ohem_threshold(p0, st1.clone(), MIN_KEPT * B, THRESH)

    forms = {
        "ohem_prob_us": lambda: ops.ohem_prob(*nxt(), THRESH),
        "ohem_threshold_us": threshold_alone,
        "label_weight_us": lambda: ops.label_weight(nxt()[1], C, p0, st0, want_norm=False),
        "fused_chain_us": lambda: pixel_weights(*nxt(), 255, sampler=fused),
        "composed_chain_us": lambda: pixel_weights(*nxt(), 255, sampler=composed),
    }
    vals = {k: [] for k in forms}
    for rnd in range(rounds + 1):
        for k, fn in forms.items():
            t = _time(fn, reps)
            if rnd:
                vals[k].append(t)
    peak = {}
    for k in ("fused_chain_us", "composed_chain_us"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        forms[k]()
        torch.cuda.synchronize()
        peak[k.replace("_us", "_peak_extra_mb")] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    w1, w0 = pixel_weights(lg0, lab0, 255, sampler=fused)[0], pixel_weights(lg0, lab0, 255, sampler=composed)[0]
    st = st0.tolist()
    rec = dict(what=f"OHEM weight map, us per call: batch {B}, {C} classes, {h}x{h} logits -> {H}x{H} labels, thresh {THRESH}, min_kept {MIN_KEPT}; {kind} input",
               ring_sets=nset, n_valid=st[ops.OHEM_N], n_below_thresh=st[ops.OHEM_NLT], k=st[ops.OHEM_K], kept=int(w1.sum().item()),
               maps_differ_in=int((w1 != w0).sum().item()))
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
    cfg["decode_head"]["sampler"] = dict(type="OHEMPixelSampler", thresh=THRESH, min_kept=MIN_KEPT)
    model = MODELS.build(cfg)
    sd = synth_like(model.state_dict())
    sd.update(synth_like({k: p.detach() for k, p in model.named_parameters() if k not in sd}))
    model.load_state_dict(sd)
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    lab = synth_label(2, 512, seed=1)
    data = dict(inputs=synth_image(2, 512, seed=1).cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
    sampler = model.decode_head.sampler
    vals = {"sampler_free": [], "ohem_fused": [], "ohem_composed": []}
    for rnd in range(rounds + 1):
        for key in vals:
            model.decode_head.sampler = None if key == "sampler_free" else sampler
            sampler.fused = key != "ohem_composed"
            t = _time(lambda: model.train_step(data, ow), step_reps, warm=5) / 1e3
            if rnd:
                vals[key].append(t)
    rec = dict(mode=mode, depth=depth, what="presets.dinov2_linear(): ms per train step, batch 2 x 512^2, without a sampler and with OHEMPixelSampler(0.7, 100000)")
    rec.update({"train_step_ms_" + k: _spread(v, 3) for k, v in vals.items()})
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
        raise SystemExit("tools/ohem_time.py measures on the GPU; none found")
    assert a.reps >= 100, "at least 100 repetitions per figure"
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps)), flush=True)
    for h, H in ((128, 1024), (32, 512)):
        for kind in ("spread", "saturated"):
            chain_times(h, H, kind, a.reps, a.rounds)
    if not a.skip_model:
        step_times(a.step_reps, a.mode, a.depth, a.rounds)


if __name__ == "__main__":
    main()
