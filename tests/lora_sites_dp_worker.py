"""One rank of the data-parallel test of the LoRA adapter sites (tests/test_lora_sites_gpu.py; in the style of tests/dp_worker.py): TWO
train steps of a depth-2 EncoderDecoder(LoRABackbone with qkv, attn.proj, fc1 and fc2 adapted, LinearHead) in the f32 mode through the
product's DP plumbing (parallel.attach), dropout off; rank 0 writes the losses, the post-step parameters and the bucket launch order.

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the env (gloo: the ranks share the one GPU of the test box);  argv: OUT.pt

world 1 trains on the global batch [s0, s1]; world 2 gives sample r to rank r."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    out_path = sys.argv[1]
    os.environ["VFMSEG_DIST_BACKEND"] = "gloo"
    import vfmseg_amd  # noqa: F401
    from tests import lora_sites_helpers as H
    from tests.helpers import model_shapes
    from vfmseg_amd import lib as L, parallel, presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label, synth_state_dict
    rank, world, _ = parallel.init_from_env("gloo")
    torch.cuda.set_device(0)
    L.set_device_index(0)
    set_compute_dtype("f32")
    cfg = presets.dinov2_linear(depth=H.DEPTH)
    cfg["backbone"]["backbone"]["out_indices"] = [0, 1, 1, 1]
    cfg["backbone"]["Lora_config"] = presets.lora_cfg(r=H.RANK, alpha=H.ALPHA, target_modules=presets.ALL_LINEAR, dropout=0.0)
    model = MODELS.build(cfg)
    sd = {"backbone." + k: v for k, v in H.lora_state_dict().items()}
    sd.update(synth_state_dict({k: v for k, v in model_shapes(H.DEPTH, H.DIM).items() if k.startswith("decode_head.")}))
    if rank != 0:   # the constructor broadcast must make rank 0's weights win: start the others from different values
        sd = {k: (v + 0.01 if v.is_floating_point() and "lora_" in k else v) for k, v in sd.items()}
    model.load_state_dict(sd)
    model = model.cuda().train()
    for m in model.modules():
        if hasattr(m, "dropout_ratio"):
            m.dropout_ratio = 0.0
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    events = []
    gs = parallel.attach(model, ow)
    if gs is not None:   # record when each bucket is launched relative to backward (overlap order)
        orig = gs.ready

        def ready(i):
            if not gs.done[i]:
                events.append(gs.buckets[i][0])
            return orig(i)
        gs.ready = ready
    logs = []
    for step in range(2):
        idx = [0, 1] if world == 1 else [rank]
        imgs = torch.cat([synth_image(1, 512, seed=600 + 2 * step + j) for j in idx]).cuda()
        labs = torch.cat([synth_label(1, 512, seed=600 + 2 * step + j) for j in idx])
        log = model.train_step(dict(inputs=imgs, data_samples=[SegDataSample(gt_sem_seg=labs[k]) for k in range(len(idx))]), ow)
        rec = torch.tensor([float(log["decode.loss_ce"])], dtype=torch.float64)
        if world > 1:   # logged values are rank-local means: average them for the comparison
            torch.distributed.all_reduce(rec)
            rec /= world
        logs.append(rec)
    torch.cuda.synchronize()
    if rank == 0:
        state = {k: v.detach().float().cpu() for k, v in model.state_dict().items() if "lora_" in k or not k.startswith("backbone.")}
        torch.save(dict(state=state, logs=torch.stack(logs), events=events, world=world), out_path)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
