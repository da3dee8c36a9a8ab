#!/usr/bin/env python
"""Timing of the SegFormer-head path on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 500 python tools/segformer_time.py`).

1. GroupNorm + ReLU forward and backward in its two forms - the one-launch tile kernels (vfm_groupnorm_tile_fwd / _bwd) and the three- /
   four-launch kernels (vfm_groupnorm_fwd / _bwd) - at the head's two shapes, [rows, 1024] with 128 groups (the four embeddings) and
   [rows, 256] with 32 groups (the fusion), for rows = 2048 (training, batch 2 x 512^2) and 18432 (eighteen windows of a 1024 x 2048
   slide).  The two forms alternate in one process over `--rounds` rounds (median, min, max and every round's value are logged), device
   events bracket `--reps` repetitions after a warm-up, and the operands rotate through a ring of buffer sets larger than the 256-MB
   last-level cache - one ring per direction, sized from the bytes that direction's call touches.
2. SegformerHead forward + backward (batch 2, 32 x 32 tokens, bf16) with either form forced (VFMSEG_GN_TILE) and with the default choice.
3. ms per train step (batch 2 x 512^2) of the three presets at `--depth`, with either form forced."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _time(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def _spread(vals, nd=2):
    """median, and every round's value: the spread of the measurement is min .. max of the rounds"""
    v = sorted(vals)
    return dict(median=round(v[len(v) // 2], nd), min=round(v[0], nd), max=round(v[-1], nd), rounds=[round(x, nd) for x in vals])


def groupnorm_forms(reps, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import ops
    out = []
    for B, P, C, G in ((2, 1024, 1024, 128), (2, 1024, 256, 32), (18, 1024, 1024, 128), (18, 1024, 256, 32)):
        assert ops.groupnorm_tile_ok(P, C, G)
        n = B * P * C
        # a ring per direction, sized from the bytes the timed call touches: forward x (4) + y (2), backward dy (2) + x (4) + dx (4)
        nbuf_f, nbuf_b = max(2, -(-(320 << 20) // (n * 6))), max(2, -(-(320 << 20) // (n * 10)))
        g = torch.Generator().manual_seed(C + B)
        x0, dy0 = torch.randn(B * P, C, generator=g).cuda(), torch.randn(B * P, C, generator=g).cuda().bfloat16()
        w, b = (1 + 0.1 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
        fsets = [dict(x=x0.clone(), y=torch.empty(B * P, C, dtype=torch.bfloat16, device="cuda")) for _ in range(nbuf_f)]
        bsets = [dict(x=x0.clone(), dy=dy0.clone(), dx=torch.empty(B * P, C, device="cuda")) for _ in range(nbuf_b)]
        stats = torch.empty(B, G, 2, device="cuda")
        dw, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ops.groupnorm_fwd(x0, w, b, 1e-5, G, ops.ACT_RELU, fsets[0]["y"], stats, B, P)   # valid statistics for the backward runs (same x in every set)
        it = [0]

        def f(fwd):
            def run():
                it[0] += 1
                s = fsets[it[0] % nbuf_f]
                fwd(s["x"], w, b, 1e-5, G, ops.ACT_RELU, s["y"], stats, B, P)
            return run

        def bk(bwd):
            def run():
                it[0] += 1
                s = bsets[it[0] % nbuf_b]
                bwd(s["dy"], s["x"], w, b, stats, G, ops.ACT_RELU, s["dx"], dw, db, B, P)
            return run
        rec = dict(what="GroupNorm + ReLU, us", rows=B * P, C=C, groups=G, blocks_of_the_tile_kernel=B * C // 32, ring_sets_fwd=nbuf_f,
                   ring_mb_fwd=round(nbuf_f * n * 6 / 2 ** 20), ring_sets_bwd=nbuf_b, ring_mb_bwd=round(nbuf_b * n * 10 / 2 ** 20),
                   bytes_fwd_min=n * 6, bytes_bwd_min=n * 10)
        forms = dict(fwd_us_tile=f(ops.groupnorm_tile_fwd), fwd_us_three_launch=f(ops.groupnorm_fwd), bwd_us_tile=bk(ops.groupnorm_tile_bwd),
                     bwd_us_four_launch=bk(ops.groupnorm_bwd))
        vals = {k: [] for k in forms}
        for rnd in range(rounds + 1):   # alternating; the first round is a warm-up and is dropped
            for k, fn in forms.items():
                t = _time(fn, reps)
                if rnd:
                    vals[k].append(t)
        rec.update({k: _spread(v) for k, v in vals.items()})
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del fsets, bsets
        torch.cuda.empty_cache()
    return out


def head_forms(reps, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import functional as Fh, presets
    from vfmseg_amd.heads import FeatPack
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.synth import synth_like
    set_compute_dtype("bf16")
    head = MODELS.build(presets.segformer_head())
    head.load_state_dict(synth_like(head.state_dict()))
    head = head.cuda().train()
    g = torch.Generator().manual_seed(1)
    xcat = torch.randn(2048, 4096, generator=g).cuda().bfloat16().requires_grad_(True)
    dlg = torch.randn(2, 32, 32, 19, generator=g).cuda()

    def step():
        for p in head.parameters():
            p.grad = None
        xcat.grad = None
        head.forward_tokens(FeatPack(xcat, 2, 32, 32)).backward(dlg)
        Fh.join_wgrad_stream()
    rec = dict(what="SegformerHead forward + backward, us (batch 2, 32 x 32 tokens, bf16, python dispatch included)")
    vals = {"tile": [], "three_four_launch": [], "default": []}
    for rnd in range(rounds + 1):
        for form, name in (("1", "tile"), ("0", "three_four_launch"), ("", "default")):
            os.environ["VFMSEG_GN_TILE"] = form
            t = _time(step, reps)
            if rnd:
                vals[name].append(t)
    os.environ.pop("VFMSEG_GN_TILE")
    rec.update({"fwd_bwd_us_" + k: _spread(v, 1) for k, v in vals.items()})
    print(json.dumps(rec), flush=True)
    return rec


def model_times(step_reps, mode, depth, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label, synth_like
    set_compute_dtype(mode)
    img, lab = synth_image(2, 512, seed=1).cuda(), synth_label(2, 512, seed=1)
    data = dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
    for name, preset in (("dinov2_segformer", presets.dinov2_segformer), ("rein_dinov2_segformer", presets.rein_dinov2_segformer),
                         ("frozen_dinov2_segformer", presets.frozen_dinov2_segformer)):
        cfg = preset(depth=depth)
        if depth < 24:
            cfg["backbone"]["out_indices"] = [min(i, depth - 1) for i in range(4)]
        model = MODELS.build(cfg)
        model.load_state_dict(synth_like(model.state_dict()), strict=False)
        model = model.cuda().train()
        oc = presets.optim_cfg()
        ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
        rec = dict(mode=mode, depth=depth, what=f"presets.{name}(): ms per train step, batch 2 x 512^2")
        vals = {"tile": [], "three_four_launch": [], "default": []}
        for rnd in range(rounds + 1):
            for form, key in (("1", "tile"), ("0", "three_four_launch"), ("", "default")):
                os.environ["VFMSEG_GN_TILE"] = form
                t = _time(lambda: model.train_step(data, ow), step_reps, warm=5) / 1e3
                if rnd:
                    vals[key].append(t)
        os.environ.pop("VFMSEG_GN_TILE")
        rec.update({"train_step_ms_" + k: _spread(v, 3) for k, v in vals.items()})
        print(json.dumps(rec), flush=True)
        del model, ow
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="reported rounds per figure (after one dropped round)")
    ap.add_argument("--mode", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/segformer_time.py measures on the GPU; none found")
    assert a.reps >= 100, "at least 100 repetitions per figure"
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps)), flush=True)
    groupnorm_forms(a.reps, a.rounds)
    head_forms(a.reps, a.rounds)
    if not a.skip_model:
        model_times(a.step_reps, a.mode, a.depth, a.rounds)


if __name__ == "__main__":
    main()
