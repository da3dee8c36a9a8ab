#!/usr/bin/env python
"""Times the LoRA adapter sites of the DINOv2 engine (a measurement, not a gate):

  * ms per train step of EncoderDecoder(LoRABackbone(DINOv2-L), LinearHead) at batch 2 x 512^2, depth 24, bf16, for qkv-only (launch plan) and
    qkv-only with VFMSEG_PLAN=0 (the one-by-one path every other row runs on), qkv plus each single extra site, and all four sites with
    VFMSEG_LORA_FUSED=1 (vfm_lora_down) against =0 (dropout_mask + mul_mask + gemm);
  * vfm_lora_down against the three composed ops at K = 1024 and 4096, M = 2050 rows, p = 0.1.

    python tools/lora_sites_time.py [--steps 20] [--warmup 5] [--depth 24] [--out profiles/lora_sites_time.json]

Each figure is the median over `steps` of HIP-event times around one step (kernel rows: around one call); one JSON object on stdout."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def time_step(targets, depth, steps, warmup, env):
    from vfmseg_amd import presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label, synth_like
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        cfg = presets.dinov2_linear(depth=depth)
        cfg["backbone"]["Lora_config"] = presets.lora_cfg(target_modules=targets)
        model = MODELS.build(cfg)
        model.load_state_dict(synth_like(model.state_dict()))
        model = model.cuda().train()
        oc = presets.optim_cfg()
        ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
        img, lab = synth_image(2, 512, seed=3).cuda(), synth_label(2, 512, seed=3).cuda()
        batch = dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
        med, lo, hi = _median_ms(lambda: model.train_step(batch, ow), steps, warmup)
        planned = bool(model.backbone.vit.engine()._packed.get("plans"))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    del model, ow
    torch.cuda.empty_cache()
    return dict(targets=list(targets), env=env, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), launch_plan=planned)


def time_kernel(K, steps, warmup, M=2050, r=32, p=0.1, s=1.0):
    from vfmseg_amd import ops
    from vfmseg_amd.backbones import R_PAD
    buf = torch.randn(M, K + R_PAD, device="cuda").to(torch.bfloat16)
    x, T = buf[:, :K], buf[:, K:]
    a = torch.zeros(R_PAD, K, dtype=torch.bfloat16, device="cuda")
    a[:r] = 0.02 * torch.randn(r, K, device="cuda")
    mask, xd = torch.empty(M, K, dtype=torch.bfloat16, device="cuda"), torch.empty(M, K, dtype=torch.bfloat16, device="cuda")

    def composed():
        ops.dropout_mask(mask, p, 1, offset=0)
        ops.mul_mask(x, mask, xd)
        ops.gemm(xd, a, T, alpha=s)

    f = _median_ms(lambda: ops.lora_down(x, a, T, s, p, 1, 0, mask, xd), steps * 5, warmup * 5)
    c = _median_ms(composed, steps * 5, warmup * 5)
    return dict(K=K, M=M, p=p, fused_us=round(1e3 * f[0], 2), composed_us=round(1e3 * c[0], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd.precision import set_compute_dtype
    set_compute_dtype("bf16")
    rows = [("qkv_plan", ["qkv"], {}), ("qkv_one_by_one", ["qkv"], {"VFMSEG_PLAN": "0"}),
            ("qkv+attn.proj", ["qkv", "attn.proj"], {"VFMSEG_LORA_FUSED": "1"}), ("qkv+fc1", ["qkv", "fc1"], {}),
            ("qkv+fc2", ["qkv", "fc2"], {"VFMSEG_LORA_FUSED": "1"}),
            ("all_fused", ["qkv", "attn.proj", "fc1", "fc2"], {"VFMSEG_LORA_FUSED": "1"}),
            ("all_composed", ["qkv", "attn.proj", "fc1", "fc2"], {"VFMSEG_LORA_FUSED": "0"})]
    res = dict(device=torch.cuda.get_device_name(0), depth=a.depth, batch="2x512x512", mode="bf16", steps=a.steps, train_step={}, kernel=[])
    for name, targets, env in rows:
        res["train_step"][name] = time_step(targets, a.depth, a.steps, a.warmup, env)
        print(name, res["train_step"][name], file=sys.stderr, flush=True)
    for K in (1024, 4096):
        res["kernel"].append(time_kernel(K, a.steps, a.warmup))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
