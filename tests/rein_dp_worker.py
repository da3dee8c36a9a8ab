"""One rank of the Rein data-parallel equivalence test (tests/test_rein_model_gpu.py): two train steps of a depth-2
EncoderDecoder(ReinsDinoVisionTransformer, LinearHead) in f32 through parallel.attach; rank 0 writes the results.

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the env (gloo: the ranks share the one GPU of the test box);  argv: OUT.pt

world 1 trains on the global batch [s0, s1]; world 2 gives sample r to rank r.  The `reins` gradients are sums over all layers and are
complete only when the backbone backward ends: their bucket must leave after it (a bucket sent with the heads' would carry zeros)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    out_path = sys.argv[1]
    os.environ["VFMSEG_DIST_BACKEND"] = "gloo"
    import vfmseg_amd  # noqa: F401
    from tests.rein_helpers import rein_model_state_dict
    from vfmseg_amd import backbones, lib as L, parallel, presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label
    rank, world, _ = parallel.init_from_env("gloo")
    torch.cuda.set_device(0)
    L.set_device_index(0)
    set_compute_dtype("f32")
    depth = 2
    cfg = presets.rein_dinov2_linear(depth=depth)
    cfg["backbone"]["out_indices"] = [0, 1, 1, 1]
    cfg["decode_head"]["dropout_ratio"] = 0.0
    model = MODELS.build(cfg)
    sd = rein_model_state_dict(depth)
    if rank != 0:   # the constructor broadcast must make rank 0's weights win
        sd = {k: (v + 0.01 if v.is_floating_point() and ".reins." in k else v) for k, v in sd.items()}
    model.load_state_dict(sd, strict=False)
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    events = []
    gs = parallel.attach(model, ow)
    if gs is not None:   # when each bucket is launched relative to the backbone backward
        orig, done = gs.ready, backbones.BACKWARD_EVENTS["backbone_done"]

        def ready(i):
            if not gs.done[i]:
                events.append(gs.buckets[i][0])
            return orig(i)

        def backbone_done():
            events.append("<backbone backward ended>")
            return done()
        gs.ready, backbones.BACKWARD_EVENTS["backbone_done"] = ready, backbone_done
    logs = []
    for step in range(2):
        idx = [0, 1] if world == 1 else [rank]
        imgs = torch.cat([synth_image(1, 512, seed=500 + 2 * step + j) for j in idx]).cuda()
        labs = torch.cat([synth_label(1, 512, seed=500 + 2 * step + j) for j in idx])
        log = model.train_step(dict(inputs=imgs, data_samples=[SegDataSample(gt_sem_seg=labs[k]) for k in range(len(idx))]), ow)
        rec = torch.tensor([float(log["decode.loss_ce"])], dtype=torch.float64)
        if world > 1:
            torch.distributed.all_reduce(rec)
            rec /= world
        logs.append(rec)
    torch.cuda.synchronize()
    if rank == 0:
        state = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
        torch.save(dict(state=state, logs=torch.stack(logs), events=events, world=world), out_path)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
