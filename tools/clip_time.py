#!/usr/bin/env python
"""Timing of gradient clipping on the GPU (run in a fresh process under a time limit, e.g. `timeout -k 10 500 python tools/clip_time.py`).

1. At the real buffer size - the flat optimiser buffers of presets.dinov2_ms_masked() at `--depth` (24: 16.6 M floats, 66.5 MB each) -
   device time per call of
     adamw           today's fused AdamW launch alone (ops.adamw, zero_grad fused): the step without clipping
     grad_norm       vfm_grad_norm alone (one read pass + the finish launch)
     fused_clip      vfm_grad_norm, then the AdamW launch with the device-side coefficient: what clip_grad costs here
     torch_clip      torch.nn.utils.clip_grad_norm_ over the ~250 parameter views, then ops.adamw: the composition it replaces
     flat_norm_clip  gflat.norm(), the coefficient in torch on the device, gflat.mul_(coef), then ops.adamw (no host read either)
   Device events bracket `--reps` repetitions after a warm-up; the forms alternate over `--rounds` rounds (median [min .. max]).  The
   buffers rotate through a ring of sets larger than the 256-MB last-level cache.
2. Host time to ENQUEUE OptimWrapper.update_params (backward included) with and without clip_grad on one model, the queue drained
   before each call so that the host never waits for the device: what clipping adds on the host side.
3. ms per train step of that model (batch 2 x 1024^2) without clipping - the parent commit's step, launch for launch - and with
   clip_grad=dict(max_norm=1.0), alternating in one process."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from segformer_time import _spread, _time  # noqa: E402


def build(depth, mode):
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label, synth_like
    set_compute_dtype(mode)
    cfg = presets.dinov2_ms_masked(depth=depth)
    if depth < 24:
        cfg["backbone"]["backbone"]["out_indices"] = [depth * (i + 1) // 4 - 1 for i in range(4)]
    model = MODELS.build(cfg)
    model.load_state_dict(synth_like(model.state_dict()))
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    lab = synth_label(2, 1024, seed=100)
    data = dict(inputs=synth_image(2, 1024, seed=100).cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
    return model, ow, data


def kernel_times(opt, reps, rounds):
    from vfmseg_amd import ops
    n = opt.flat.numel()
    nset = max(2, -(-320 * 2 ** 20 // (n * 16)))   # p, g, m, v of one set: 16 B per element; the ring exceeds the last-level cache
    gen = torch.Generator().manual_seed(3)
    sets = []
    for _ in range(nset):
        s = dict(p=opt.flat.clone(), g=(torch.randn(n, generator=gen) * 1e-3).cuda(), m=torch.zeros_like(opt.flat), v=torch.zeros_like(opt.flat))
        views = []
        for a, sz, q in zip(opt.offsets[:-1], opt.sizes, opt.params):
            t = torch.nn.Parameter(s["p"][a:a + sz].view(q.shape))
            t.grad = s["g"][a:a + sz].view(q.shape)
            views.append(t)
        s["views"] = views
        sets.append(s)
    it = [0]

    def nxt():
        it[0] += 1
        return sets[it[0] % nset]

    state, ws = torch.zeros(4, device="cuda"), torch.empty(4096, dtype=torch.float64, device="cuda")
    step = [0]

    def adamw(s, **kw):
        step[0] += 1
        ops.adamw(s["p"], s["g"], s["m"], s["v"], opt.seg_start, opt.seg_lr, opt.seg_wd, 1e-4, opt.betas, opt.eps, step[0], 1.0,
                  zero_grad=False, vec4=True, **kw)   # (the gradients stay: every form sees the same ones in every round)

    def fused_clip():
        s = nxt()
        ops.grad_norm(s["g"], 2, 1.0, 1.0, None, state, None, ws)
        adamw(s, clip_coef=state[1:2])

    def torch_clip():
        s = nxt()
        torch.nn.utils.clip_grad_norm_(s["views"], 1.0)
        adamw(s)

    def flat_norm_clip():
        s = nxt()
        s["g"].mul_(torch.clamp(1.0 / (s["g"].norm() + 1e-6), max=1.0))
        adamw(s)

    forms = {"adamw_us": lambda: adamw(nxt()), "grad_norm_us": lambda: ops.grad_norm(nxt()["g"], 2, 1.0, 1.0, None, state, None, ws),
             "fused_clip_us": fused_clip, "torch_clip_us": torch_clip, "flat_norm_clip_us": flat_norm_clip}
    vals = {k: [] for k in forms}
    for rnd in range(rounds + 1):
        for k, fn in forms.items():
            t = _time(fn, reps)
            if rnd:
                vals[k].append(t)
    g0 = sets[0]["g"]
    ops.grad_norm(g0, 2, 1.0, 1.0, None, state, None, ws)
    rec = dict(what="clip_grad at the optimiser's buffer size, us per call on the device (events around the repetitions)", n=n,
               mb_per_buffer=round(n * 4 / 2 ** 20, 1), parameter_views=len(opt.params), ring_sets=nset,
               norm_kernel=state[0].item(), norm_torch=g0.double().norm().item())
    rec.update({k: _spread(v) for k, v in vals.items()})
    med = {k: rec[k]["median"] for k in vals}
    rec["clip_adds_us"] = dict(fused=round(med["fused_clip_us"] - med["adamw_us"], 2), torch_clip_grad_norm=round(med["torch_clip_us"] - med["adamw_us"], 2),
                               flat_norm=round(med["flat_norm_clip_us"] - med["adamw_us"], 2))
    rec["grad_norm_gb_per_s"] = round(n * 4 / med["grad_norm_us"] / 1e3, 1)
    print(json.dumps(rec), flush=True)


def _set_clip(ow, on):
    from vfmseg_amd.optim import parse_clip_grad
    ow.clip_grad = parse_clip_grad(dict(max_norm=1.0)) if on else None


def enqueue_times(model, ow, data, reps, rounds):
    """host seconds inside update_params with an empty queue in front of it"""
    vals = {"plain": [], "clip_grad": []}
    for rnd in range(rounds + 1):
        for key in vals:
            _set_clip(ow, key == "clip_grad")
            tot = 0.0
            for i in range(reps + 3):
                d = model.data_preprocessor(data, True)
                total, _ = model.parse_losses(model.forward(d["inputs"], d["data_samples"], mode="loss"))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ow.update_params(total)
                if i >= 3:
                    tot += time.perf_counter() - t0
            torch.cuda.synchronize()
            if rnd:
                vals[key].append(tot / reps * 1e3)
    rec = dict(what="host ms to enqueue OptimWrapper.update_params (backward + step), queue drained before each call")
    rec.update({"enqueue_ms_" + k: _spread(v, 3) for k, v in vals.items()})
    print(json.dumps(rec), flush=True)


def step_times(model, ow, data, step_reps, rounds, mode, depth):
    vals = {"plain": [], "clip_grad": []}
    for rnd in range(rounds + 1):
        for key in vals:
            _set_clip(ow, key == "clip_grad")
            t = _time(lambda: model.train_step(data, ow), step_reps, warm=5) / 1e3
            if rnd:
                vals[key].append(t)
    rec = dict(mode=mode, depth=depth, what="presets.dinov2_ms_masked(): ms per train step, batch 2 x 1024^2, without clip_grad (the parent "
               "commit's launch sequence) and with clip_grad=dict(max_norm=1.0)", grad_norm_last=ow.grad_norm())
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
        raise SystemExit("tools/clip_time.py measures on the GPU; none found")
    pr = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), arch=getattr(pr, "gcnArchName", "?"), compute_units=pr.multi_processor_count,
                          memory_gb=round(pr.total_memory / 2 ** 30), reps=a.reps)), flush=True)
    model, ow, data = build(a.depth, a.mode)
    kernel_times(ow.optimizer, a.reps, a.rounds)
    if not a.skip_model:
        enqueue_times(model, ow, data, a.step_reps, a.rounds)
        step_times(model, ow, data, a.step_reps, a.rounds, a.mode, a.depth)


if __name__ == "__main__":
    main()
