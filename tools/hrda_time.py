#!/usr/bin/env python
"""Timing of the HRDA path on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 400 python tools/hrda_time.py`).

1. The fusion kernels (vfm_hrda_fuse_fwd / _bwd) at the training shape of presets.dinov2_hrda(): batch 2, lr 128 x 128, attention
   32 x 32, HR crop 128 x 128, fused 256 x 256, 19 classes - against the same arithmetic as plain torch device ops (sigmoid,
   F.interpolate, mask, pad, multiply-add; backward by autograd), alternating in one process, device events around `--reps`
   repetitions after a warm-up.  The operands rotate through a ring of buffer sets larger than the 256-MB last-level cache.
2. ms per train step (batch 2 x 1024^2) and ms per image of the 1024 x 2048 slide prediction of presets.dinov2_hrda() at depth 24."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


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


def _torch_fuse(lr, a, hr, offset, mask):
    """the composed form: NHWC operands viewed as NCHW (channels_last memory), torch device ops only"""
    lr_, a_, hr_ = (t.permute(0, 3, 1, 2) for t in (lr, a, hr))
    h, w = lr_.shape[2:]
    att = F.interpolate(torch.sigmoid(a_), size=(h, w), mode="bilinear", align_corners=False) * mask
    lrs = (1 - att) * lr_
    up_lr = F.interpolate(lrs, scale_factor=2, mode="bilinear", align_corners=False)
    up_att = F.interpolate(att, scale_factor=2, mode="bilinear", align_corners=False)
    ins = F.pad(hr_, (offset[1], 2 * w - offset[1] - hr_.shape[3], offset[0], 2 * h - offset[0] - hr_.shape[2]))
    return up_att * ins + up_lr


def fuse_kernels(reps):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import ops
    B, C, ha, h, hc = 2, 19, 32, 128, 128
    box = (88, 600, 216, 728)
    offset, mbox = (box[0] // 4, box[2] // 4), tuple(v // 8 for v in box)
    per_set = 4 * C * B * (2 * h * h + ha * ha + hc * hc + 4 * h * h * 2 + h * h)
    nbuf = -(-(320 << 20) // per_set)
    g = torch.Generator().manual_seed(0)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    sets = [dict(lr=mk(B, h, h, C), a=mk(B, ha, ha, C), hr=mk(B, hc, hc, C), dF=mk(B, 2 * h, 2 * h, C), fused=torch.empty(B, 2 * h, 2 * h, C, device="cuda"),
                 att=torch.empty(B, h, h, C, device="cuda")) for _ in range(2)]
    sets += [{k: v.clone() for k, v in sets[i % 2].items()} for i in range(nbuf - 2)]
    mask = torch.zeros(1, 1, h, h, device="cuda")
    mask[:, :, mbox[0]:mbox[1], mbox[2]:mbox[3]] = 1
    it = [0]

    def nxt():
        it[0] += 1
        return sets[it[0] % nbuf]

    def fwd_hip():
        s = nxt()
        ops.hrda_fuse_fwd(s["lr"], s["a"], s["hr"], offset, mbox, s["fused"], s["att"], None)
    d = dict(d_lr=torch.empty(B, h, h, C, device="cuda"), d_a=torch.empty(B, ha, ha, C, device="cuda"), d_hr=torch.empty(B, hc, hc, C, device="cuda"))
    for s in sets:   # a valid saved attention in every set
        ops.hrda_fuse_fwd(s["lr"], s["a"], s["hr"], offset, mbox, s["fused"], s["att"], None)

    def bwd_hip():
        s = nxt()
        ops.hrda_fuse_bwd(s["dF"], s["lr"], s["a"], s["hr"], s["att"], offset, mbox, d["d_lr"], d["d_a"], d["d_hr"])

    def fwd_torch():
        s = nxt()
        with torch.no_grad():
            _torch_fuse(s["lr"], s["a"], s["hr"], offset, mask)

    def fwd_bwd_torch():
        s = nxt()
        t = [s[k].detach().requires_grad_(True) for k in ("lr", "a", "hr")]
        _torch_fuse(t[0], t[1], t[2], offset, mask).backward(s["dF"].permute(0, 3, 1, 2))
    rec = dict(what="HRDA fusion, us", shape=dict(B=B, C=C, a=ha, lr=h, crop=hc, fused=2 * h), ring_buffer_sets=nbuf,
               bytes_fwd_min=4 * C * B * (h * h + ha * ha + hc * hc + 4 * h * h))
    for rnd in range(2):   # alternating; the second round is the one reported
        rec["fwd_us_hip"] = round(_time(fwd_hip, reps), 2)
        rec["fwd_us_torch"] = round(_time(fwd_torch, reps), 2)
        rec["bwd_us_hip"] = round(_time(bwd_hip, reps), 2)
        rec["fwd_plus_bwd_us_torch"] = round(_time(fwd_bwd_torch, reps), 2)
    rec["bwd_us_torch"] = round(rec["fwd_plus_bwd_us_torch"] - rec["fwd_us_torch"], 2)
    print(json.dumps(rec), flush=True)
    return rec


def model_times(step_reps, mode, depth):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label, synth_like
    set_compute_dtype(mode)
    cfg = presets.dinov2_hrda(depth=depth)
    if depth < 24:
        cfg["backbone"]["backbone"]["out_indices"] = [min(i, depth - 1) for i in range(4)]
    model = MODELS.build(cfg)
    model.load_state_dict(synth_like(model.state_dict()))
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    img, lab = synth_image(2, 1024, seed=1).cuda(), synth_label(2, 1024, seed=1)
    data = dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
    rec = dict(mode=mode, depth=depth, what="presets.dinov2_hrda()")
    rec["train_step_ms_batch2_1024"] = round(_time(lambda: model.train_step(data, ow), step_reps, warm=5) / 1e3, 3)
    model.eval()
    big = synth_image(1, (1024, 2048), seed=2).cuda()
    with torch.no_grad():
        rec["slide_ms_per_img_1024x2048"] = round(_time(lambda: model.predict(big), step_reps, warm=3) / 1e3, 3)
        model.sequential_windows = True
        rec["slide_ms_per_img_1024x2048_window_by_window"] = round(_time(lambda: model.predict(big), step_reps, warm=3) / 1e3, 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--mode", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hrda_time.py measures on the GPU; none found")
    assert a.reps >= 100, "at least 100 repetitions per figure"
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps)), flush=True)
    fuse_kernels(a.reps)
    if not a.skip_model:
        model_times(a.step_reps, a.mode, a.depth)


if __name__ == "__main__":
    main()
