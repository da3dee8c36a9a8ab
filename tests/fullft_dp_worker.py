"""One rank of the full fine-tuning data-parallel equivalence test (tests/test_fullft_gpu.py): two train steps of the small
EncoderDecoder(DinoVisionTransformer, LinearHead) in f32 through parallel.attach; rank 0 writes the results.

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the env (gloo: the ranks share the one GPU of the test box);  argv: OUT.pt

world 1 trains on the global batch [s0, s1]; world 2 gives sample r to rank r.  The base weights' gradients are final block by block:
`backbone0` (the last blocks) must leave while the backbone backward runs, the last bucket (first blocks + embeddings) when it has ended."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    out_path = sys.argv[1]
    os.environ["VFMSEG_DIST_BACKEND"] = "gloo"
    import vfmseg_amd  # noqa: F401
    from tests.fullft_helpers import batch, build_small, small_state_dict
    from vfmseg_amd import backbones, lib as L, parallel, presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.segmentors import SegDataSample
    rank, world, _ = parallel.init_from_env("gloo")
    torch.cuda.set_device(0)
    L.set_device_index(0)
    set_compute_dtype("f32")
    sd = small_state_dict()
    if rank != 0:   # the constructor broadcast must make rank 0's weights win
        sd = {k: (v + 0.01 if v.is_floating_point() and k.startswith("backbone.blocks.") else v) for k, v in sd.items()}
    model = build_small(sd=sd).cuda().train()
    oc = presets.optim_cfg(backbone_lr_mult=0.1)
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
        pairs = [batch(1, seed=600 + 2 * step + j) for j in idx]
        imgs = torch.cat([p[0] for p in pairs]).cuda()
        labs = torch.cat([p[1] for p in pairs])
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
