#!/usr/bin/env python
"""Timing of the DACS self-training path on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 500 python tools/dacs_time.py`).

1. The new kernels at the training shape (batch 2, 512^2, 19 classes, 32 x 32 teacher logits): vfm_pseudo_label, vfm_class_presence,
   vfm_class_mix, vfm_upsample_ce_w against vfm_upsample_ce, and the torch composition of the same glue (resize + softmax + max + ratio,
   torch.unique, the three one_mix products).  Device events bracket `--reps` repetitions after a warm-up; the forms alternate over
   `--rounds` rounds (median, min, max and every round are logged).  The image-sized operands rotate through a ring larger than the 256-MB
   last-level cache.
2. ms per DACS train step (presets.uda_rein_dinov2_segformer at `--depth`, batch 2 x 512^2) with the fused glue (VFMSEG_DACS_FUSED=1) and
   the composed glue (=0), alternating in one process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from segformer_time import _spread, _time  # noqa: E402


def kernel_times(reps, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import ops
    B, H, W, C, h, w = 2, 512, 512, 19, 32, 32
    g = torch.Generator().manual_seed(3)
    nset = 24   # x (two images + the mixed one, labels, weights) = 24 x ~23 MB: beyond the last-level cache
    sets = []
    for i in range(nset):
        src_lbl = torch.randint(0, C, (B, H // 32, W // 32), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()
        sets.append(dict(src=torch.randn(B, 3, H, W, generator=g).cuda(), tgt=torch.randn(B, 3, H, W, generator=g).cuda(), lbl=src_lbl.cuda(),
                         ps=torch.randint(0, C, (B, H, W), generator=g).cuda(), wt=torch.rand(B, H, W, generator=g).cuda()))
    lg = (torch.randn(B, h, w, C, generator=g) * 2).cuda()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    chosen = ops.class_lists_to_bits([[0, 3, 5, 7, 11], [1, 2, 4, 8, 16]], "cuda")
    total = B * H * W
    it = [0]

    def nxt():
        it[0] += 1
        return sets[it[0] % nset]

    def composed_pseudo():
        full = torch.empty(B, C, H, W, device="cuda")
        ops.resize_bilinear(lg, False, B, h, w, C, full, 1, (H, W))
        prob, lab = torch.max(torch.softmax(full, dim=1), dim=1)
        return lab, (prob.ge(0.5).sum().double() / total).float()

    def composed_mix():
        s = nxt()
        mask = torch.isin(s["lbl"], torch.tensor([0, 3, 5, 7, 11], device="cuda")).long()
        m = mask.unsqueeze(1)
        pw = 0.5 * torch.ones(B, H, W, device="cuda")
        pw[:, :15] = 0
        pw[:, -120:] = 0
        return m * s["src"] + (1 - m) * s["tgt"], mask * s["lbl"] + (1 - mask) * s["ps"], mask * torch.ones_like(pw) + (1 - mask) * pw

    def ce(weighted):
        def run():
            s = nxt()
            ops.upsample_ce_w_loss_acc(lg, s["lbl"], s["wt"] if weighted else None)
        return run

    forms = {
        "pseudo_label_us": lambda: ops.pseudo_label(lg, (H, W), 0.5, count),
        "pseudo_label_composed_us": composed_pseudo,
        "class_presence_us": lambda: ops.class_presence(nxt()["lbl"]),
        "class_presence_torch_unique_us": lambda: [torch.unique(l) for l in nxt()["lbl"]],
        "class_mix_us": lambda: (lambda s: ops.class_mix(s["src"], s["tgt"], s["lbl"], s["ps"], chosen, count, total, 15, 120))(nxt()),
        "class_mix_composed_us": composed_mix,
        "upsample_ce_us": ce(False),
        "upsample_ce_w_us": ce(True),
    }
    vals = {k: [] for k in forms}
    for rnd in range(rounds + 1):
        for k, fn in forms.items():
            t = _time(fn, reps)
            if rnd:
                vals[k].append(t)
    rec = dict(what="DACS glue kernels, us per call (batch 2, 512^2, 19 classes, 32 x 32 teacher logits; allocation of the outputs included)",
               ring_sets=nset, class_mix_bytes_min=total * (3 * 4 * 3 + 8 * 3 + 4))
    rec.update({k: _spread(v) for k, v in vals.items()})
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
    cfg = presets.uda_rein_dinov2_segformer(depth=depth)
    if depth < 24:
        cfg["backbone"]["out_indices"] = [min(i, depth - 1) for i in range(4)]
    cfg["pseudo_threshold"] = 0.5
    model = MODELS.build(cfg)
    sd = synth_like(model.state_dict())
    sd.update(synth_like({k: p.detach() for k, p in model.named_parameters() if k not in sd}))
    model.load_state_dict(sd)
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    lab = synth_label(2, 512, seed=1)
    data = dict(img=dict(inputs=synth_image(2, 512, seed=1).cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)]),
                target_img=dict(inputs=synth_image(2, 512, seed=2).cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)]))
    vals = {"fused": [], "composed": []}
    for rnd in range(rounds + 1):
        for key in vals:
            model.fused = key == "fused"
            t = _time(lambda: model.train_step(data, ow), step_reps, warm=5) / 1e3
            if rnd:
                vals[key].append(t)
    rec = dict(mode=mode, depth=depth, what="presets.uda_rein_dinov2_segformer(): ms per DACS train step, batch 2 x 512^2 (source + mixed pass, teacher pass)")
    rec.update({"train_step_ms_" + k: _spread(v, 3) for k, v in vals.items()})
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="reported rounds per figure (after one dropped round)")
    ap.add_argument("--mode", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dacs_time.py measures on the GPU; none found")
    assert a.reps >= 100, "at least 100 repetitions per figure"
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps)), flush=True)
    kernel_times(a.reps, a.rounds)
    if not a.skip_model:
        step_times(a.step_reps, a.mode, a.depth, a.rounds)


if __name__ == "__main__":
    main()
