#!/usr/bin/env python
"""Timing of the Rein adapter on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 300 python tools/rein_time.py`).

1. Per layer, fused kernels against the composed form (VFMSEG_REIN_FUSED=0: ops.gemm + ops.softmax_rows + ops.cast), in the same
   process, alternating, device events around `--reps` repetitions after a warm-up: the adapter forward without saved activations (prediction),
   the forward that saves what backward needs, and the backward (per-layer part), at batch 2 x 512^2 (2048 patch rows) and at the nine-window
   prediction batch (9216 rows).  Each figure is the whole adapter step of that direction, mlp_delta_f GEMM included (it is the same
   launch in both forms).
2. The whole train step of EncoderDecoder(ReinsDinoVisionTransformer, LinearHead) at depth 24, batch 2 x 512^2, against the
   EncoderDecoder(LoRABackbone(DinoVisionTransformer), LinearHead) step (presets.dinov2_linear), fused and composed.
The stream and gradient operands rotate through a ring of buffers larger than the 256-MB last-level cache, so every repetition reads them
from HBM as a train step does; the small token operands and (backward) the saved u / P / x16 of one forward are reused and stay cache-hot.
Bytes per layer and direction (from shapes) are printed with the times, so a rate can be read off."""
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


def per_layer(reps, mode):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import presets
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    set_compute_dtype(mode)
    cfg = presets.rein_dinov2_linear(depth=2)["backbone"]
    cfg["out_indices"] = [0, 1, 1, 1]
    model = MODELS.build(cfg).cuda().train()
    with torch.no_grad():   # an adapter that does something (the default scale 0.001 and tiny tokens would still cost the same time)
        model.reins.learnable_tokens_b.mul_(20.0)
    eng = model.engine()
    P = eng.packed()
    D = model.embed_dim
    out = []
    for rows in (2048, 9216):
        nimg = rows // 1024
        g = torch.Generator().manual_seed(rows)
        nbuf = -(-(320 << 20) // ((rows + nimg) * D * 4))
        streams = [(2.0 * torch.randn(rows + nimg, D, generator=g)).cuda() for _ in range(2)]
        streams += [streams[i % 2].clone() for i in range(nbuf - 2)]
        grads = [torch.randn(rows + nimg, D, generator=g).cuda()]
        grads += [grads[0].clone() for _ in range(nbuf - 1)]
        it = [0]

        def nxt(ring):
            it[0] += 1
            return ring[it[0] % nbuf]
        rec = dict(rows=rows, mode=mode, ring_buffers=nbuf)
        for fused in (True, False, True, False):   # alternating; the second pass is the one reported (the first also warms the allocator)
            os.environ["VFMSEG_REIN_FUSED"] = "1" if fused else "0"
            R = eng._rein_pack(P)
            assert R["fused"] == fused
            tag = "fused" if fused else "composed"

            def fwd_eval():     # prediction form: the stream is updated in place (scale = 0.001: the values barely move over the run)
                eng._rein_forward(R, 1, nxt(streams), rows, None)
            S = {}

            def fwd_train():
                S.clear()
                eng._rein_forward(R, 1, nxt(streams), rows, S)
            acc = eng._rein_backward_begin(R)
            keep = {}

            def bwd():
                S2 = dict(keep)
                eng._rein_backward(R, acc, 1, nxt(grads), rows, S2)
            rec[f"fwd_eval_us_{tag}"] = round(_time(fwd_eval, reps), 2)
            rec[f"fwd_train_us_{tag}"] = round(_time(fwd_train, reps), 2)
            fwd_train()
            keep.update(S)
            rec[f"bwd_us_{tag}"] = round(_time(bwd, reps), 2)
        # bytes the fused forward must move: the fp32 stream read twice and written once by the epilogue, u written and read once (16 bit)
        rec["fwd_bytes_min"] = rows * D * (4 * 3 + 2 * 2)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    os.environ.pop("VFMSEG_REIN_FUSED", None)
    return out


def train_steps(reps, mode):
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
    rec = dict(mode=mode, what="train step, depth 24, batch 2 x 512^2, ms")
    for name, cfg, env in (("lora_linear", presets.dinov2_linear(), None), ("rein_fused", presets.rein_dinov2_linear(), "1"),
                           ("rein_composed", presets.rein_dinov2_linear(), "0")):
        if env is not None:
            os.environ["VFMSEG_REIN_FUSED"] = env
        model = MODELS.build(cfg)
        sd = synth_like(model.state_dict())
        sd.update(synth_like({k: p.detach() for k, p in model.named_parameters() if k not in sd}))
        model.load_state_dict(sd)
        model = model.cuda().train()
        oc = presets.optim_cfg()
        ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
        rec[name] = round(_time(lambda: model.train_step(data, ow), reps, warm=5) / 1e3, 3)
        del model, ow
        torch.cuda.empty_cache()
    os.environ.pop("VFMSEG_REIN_FUSED", None)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--step-reps", type=int, default=30)
    ap.add_argument("--mode", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rein_time.py measures on the GPU; none found")
    assert a.reps >= 50, "at least 50 repetitions per figure"
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps)), flush=True)
    per_layer(a.reps, a.mode)
    if not a.skip_steps:
        train_steps(a.step_reps, a.mode)


if __name__ == "__main__":
    main()
