#!/usr/bin/env python
"""Timing of full fine-tuning on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 560 python tools/fullft_time.py`).

1. The pieces only a trained base needs, at the flagship's shapes (DINOv2-L, batch 2 x 512^2: M = 2050 token rows, D = 1024, hidden 4096):
     wgrad     the weight-gradient GEMMs dW[N, K] += dy^T x of qkv / proj / fc1 / fc2 / patch embedding in three forms - direct (one
               GEMM_ATBT launch per weight, accumulating into the gradient: the default), split over tokens (gemm_splitk_tn + slab_reduce,
               kch 3 and 11: 33 = 3 x 11 steps of 64 tokens) and layer-batched (six layers per launch, as _lora_wgrads_batched) - with
               TF/s per shape
     branch    vfm_branch_param_grads (d gamma, d bias and the dgrad operand in one pass) against the composed passes
     refresh   vfm_pack_weights over every packed 2-D weight of the model (one launch) against rebuilding each Packed(...)
     adamw     vfm_adamw over the model's ~304 M parameters
   Device events bracket `--reps` repetitions after a warm-up; the forms alternate over `--rounds` rounds (median [min .. max]).  Operands
   rotate through a ring larger than the 256-MB last-level cache.
2. ms per train step of presets.full_dinov2_linear() against presets.dinov2_linear() (LoRA) and the frozen backbone at `--depth`
   (batch 2 x 512^2), alternating in one process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from segformer_time import _spread, _time  # noqa: E402

M, D, HID, KPE = 2050, 1024, 4096, 768
RING = 320 << 20


def _alternate(forms, reps, rounds):
    vals = {k: [] for k in forms}
    for rnd in range(rounds + 1):
        for k, fn in forms.items():
            t = _time(fn, reps)
            if rnd:
                vals[k].append(t)
    return vals


def wgrad_times(reps, rounds, cd):
    from vfmseg_amd import ops
    torch.manual_seed(3)
    for name, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", HID, D), ("fc2", D, HID), ("patch_embed", D, KPE)):
        LB = 6
        per_set = M * (N + K) * 2 + N * K * 4
        nset = max(2, -(-RING // per_set))
        rn = lambda *sh: (torch.randn(*sh, device="cuda") * 0.1).to(cd)   # noqa: E731
        sets = [(rn(M, N), rn(M, K), torch.zeros(N, K, device="cuda")) for _ in range(nset)]
        nb = max(2, -(-RING // (LB * per_set)))
        bsets = [(rn(LB, M, N), rn(LB, M, K), torch.zeros(LB, N, K, device="cuda")) for _ in range(nb)]
        slabs = {k: torch.empty(k, N, K, device="cuda") for k in (3, 11)}
        it = [0]

        def nxt(pool):
            it[0] += 1
            return pool[it[0] % len(pool)]

        def direct():
            dy, x, out = nxt(sets)
            ops.gemm_tn_batched(dy.unsqueeze(0), x.unsqueeze(0), out.unsqueeze(0), M, accumulate=True)

        def splitk(k):
            def f():
                dy, x, out = nxt(sets)
                ops.gemm_splitk_tn(dy, x, slabs[k], k)
                ops.slab_reduce(slabs[k], N, out, K, 1, accumulate=True)
            return f

        def batched():
            dy, x, out = nxt(bsets)
            ops.gemm_tn_batched(dy, x, out, M, accumulate=True)

        vals = _alternate({"direct_us": direct, "splitk3_us": splitk(3), "splitk11_us": splitk(11), "batched6_us_per_layer": batched}, reps, rounds)
        vals["batched6_us_per_layer"] = [v / LB for v in vals["batched6_us_per_layer"]]
        rec = dict(what=f"weight gradient dW[{N}, {K}] += dy^T x over {M} token rows ({name}), us per weight", tiles_128=(N // 128) * (K // 128),
                   ring_sets=nset)
        rec.update({k: _spread(v) for k, v in vals.items()})
        fl = 2.0 * N * K * M
        rec["tflops"] = {k.split("_us")[0]: round(fl / (rec[k]["median"] * 1e-6) / 1e12, 1) for k in vals}
        print(json.dumps(rec), flush=True)
        del sets, bsets, slabs


def branch_times(reps, rounds, cd):
    from vfmseg_amd import ops
    torch.manual_seed(4)
    nset = max(3, -(-RING // (M * D * 8)))
    sets = [(torch.randn(M, D, device="cuda"), torch.randn(M, D, device="cuda").to(cd), torch.empty(M, D, dtype=cd, device="cuda"))
            for _ in range(nset)]
    gamma = torch.randn(D, device="cuda")
    dg, db, tmp, prod = (torch.zeros(D, device="cuda") for _ in range(4))
    prod = torch.empty(M, D, device="cuda")
    it = [0]

    def nxt():
        it[0] += 1
        return sets[it[0] % nset]

    def fused():
        dx, u, t = nxt()
        ops.branch_param_grads(dx, u, gamma, dgamma=dg, dbias=db, t=t, accumulate=True)

    def composed():
        dx, u, t = nxt()
        ops.cast(dx, t, gamma)
        ops.colsum(dx, tmp)
        db.addcmul_(tmp, gamma)
        torch.mul(dx, u, out=prod)
        ops.colsum(prod, dg, accumulate=True)

    vals = _alternate({"fused_us": fused, "composed_us": composed}, reps, rounds)
    rec = dict(what=f"LayerScale branch gradients (d gamma, d bias, t = cd(dx gamma)) over [{M}, {D}], us per call", ring_sets=nset,
               bytes_read_fused=M * D * 6, bytes_written_fused=M * D * 2)
    rec.update({k: _spread(v) for k, v in vals.items()})
    rec["fused_gb_per_s"] = round(M * D * 8 / (rec["fused_us"]["median"] * 1e-6) / 1e9)
    print(json.dumps(rec), flush=True)


def refresh_and_adamw_times(reps, rounds, cd, depth):
    from vfmseg_amd import ops
    from vfmseg_amd.backbones import Packed
    shapes = [(D, KPE)] + [(3 * D, D), (D, D), (HID, D), (D, HID)] * depth
    n2d = sum(n * k for n, k in shapes)
    master = torch.randn(n2d, device="cuda") * 0.02
    views, o = [], 0
    for n, k in shapes:
        views.append(master[o:o + n * k].view(n, k))
        o += n * k
    packs = [Packed(v, cd) for v in views]
    table = ops.PackTable([(v, p.w, p.wt) for v, p in zip(views, packs)])

    def rebuild():
        for v, p in zip(views, packs):
            ops.cast(v, p.w)
            ops.transpose(v, p.wt[:v.shape[1]], pad_rows=v.shape[0])

    n = n2d + (13 * D + 2 * HID) * depth        # + the vectors: the whole trained base
    n = (n + 15) // 16 * 16
    p, gbuf, m, v = (torch.zeros(n, device="cuda") for _ in range(4))
    p.normal_(0, 0.02)
    gbuf.normal_(0, 1e-3)
    seg = torch.arange(0, n, max(16, (n // 300) // 16 * 16), dtype=torch.int64, device="cuda")
    lrm, wd = torch.ones(seg.numel(), device="cuda"), torch.full((seg.numel(),), 0.05, device="cuda")
    step = [0]

    def adamw():
        step[0] += 1
        ops.adamw(p, gbuf, m, v, seg, lrm, wd, 1e-4, (0.9, 0.999), 1e-8, step[0], 1.0, zero_grad=False, vec4=True)

    vals = _alternate({"refresh_table_us": table.run, "refresh_rebuild_us": rebuild, "adamw_us": adamw}, max(10, reps // 10), rounds)
    rec = dict(what=f"per-step refresh of the {len(shapes)} packed 2-D weights (depth {depth}: {n2d / 1e6:.0f} M elements, both images) and AdamW over "
                    f"{n / 1e6:.0f} M parameters, us per call", launches_table=1, launches_rebuild=2 * len(shapes))
    rec.update({k: _spread(v) for k, v in vals.items()})
    rec["refresh_table_gb_per_s"] = round(n2d * 8 / (rec["refresh_table_us"]["median"] * 1e-6) / 1e9)
    rec["adamw_gb_per_s"] = round(n * 28 / (rec["adamw_us"]["median"] * 1e-6) / 1e9)
    print(json.dumps(rec), flush=True)


def step_times(step_reps, mode, depth, rounds):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label, synth_like
    lab = synth_label(2, 512, seed=1)
    data = dict(inputs=synth_image(2, 512, seed=1).cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
    runs = {}
    for key in ("full", "lora", "frozen"):
        cfg = presets.dinov2_linear(depth=depth) if key == "lora" else presets.full_dinov2_linear(depth=depth)
        bb = cfg["backbone"]["backbone"] if key == "lora" else cfg["backbone"]
        if depth < 24:
            bb["out_indices"] = [min(i, depth - 1) for i in range(4)]
        if key == "frozen":
            cfg["type"] = "FrozenBackboneEncoderDecoder"
        model = MODELS.build(cfg)
        sd = synth_like(model.state_dict())
        sd.update(synth_like({k: p.detach() for k, p in model.named_parameters() if k not in sd}))
        model.load_state_dict(sd)
        model = model.cuda().train()
        oc = presets.optim_cfg(backbone_lr_mult=0.1 if key == "full" else None)
        ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
        runs[key] = (model, ow, sum(s for s in ow.optimizer.sizes))
    vals = {k: [] for k in runs}
    splitk = {}
    for rnd in range(rounds + 1):
        for key, (model, ow, _) in runs.items():
            t = _time(lambda: model.train_step(data, ow), step_reps, warm=3) / 1e3
            if rnd:
                vals[key].append(t)
        for k in (3, 11):     # the same full step with the weight gradients split over tokens
            os.environ["VFMSEG_FULL_WGRAD_SPLITK"] = str(k)
            model, ow, _ = runs["full"]
            t = _time(lambda: model.train_step(data, ow), step_reps, warm=3) / 1e3
            os.environ.pop("VFMSEG_FULL_WGRAD_SPLITK")
            if rnd:
                splitk.setdefault(k, []).append(t)
    rec = dict(mode=mode, depth=depth, what="ms per train step, batch 2 x 512^2, LinearHead: full fine-tuning, LoRA (presets.dinov2_linear) and the frozen backbone",
               trained_parameters={k: r[2] for k, r in runs.items()})
    rec.update({"train_step_ms_" + k: _spread(v, 3) for k, v in vals.items()})
    rec.update({f"train_step_ms_full_splitk{k}": _spread(v, 3) for k, v in splitk.items()})
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="reported rounds per figure (after one dropped round)")
    ap.add_argument("--mode", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/fullft_time.py measures on the GPU; none found")
    assert a.reps >= 100, "at least 100 repetitions per figure"
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd.precision import compute_dtype, set_compute_dtype
    set_compute_dtype(a.mode)
    cd = compute_dtype()
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps, mode=a.mode)), flush=True)
    if not a.skip_kernels:
        wgrad_times(a.reps, a.rounds, cd)
        branch_times(a.reps, a.rounds, cd)
        refresh_and_adamw_times(a.reps, a.rounds, cd, a.depth)
    if not a.skip_model:
        step_times(a.step_reps, a.mode, a.depth, a.rounds)


if __name__ == "__main__":
    main()
