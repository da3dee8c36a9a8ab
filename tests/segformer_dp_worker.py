"""One rank of the frozen-backbone data-parallel equivalence test (tests/test_segformer_model_gpu.py): two train steps of a depth-2
FrozenBackboneEncoderDecoder(DinoVisionTransformer, SegformerHead) in f32 through parallel.attach; rank 0 writes the results.

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the env (gloo: the ranks share the one GPU of the test box);  argv: OUT.pt

world 1 trains on the global batch [s0, s1]; world 2 gives sample r to rank r.  The backbone has no backward pass here, so no backward
event ever fires: the one gradient bucket (the head's) leaves in GradSync.finish()."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    out_path = sys.argv[1]
    os.environ["VFMSEG_DIST_BACKEND"] = "gloo"
    import vfmseg_amd  # noqa: F401
    from tests import segformer_helpers as S
    from vfmseg_amd import lib as L, parallel, presets
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
    model = MODELS.build(S.model_config("frozen", depth))
    sd = S.model_state_dict("frozen", depth)
    if rank != 0:   # the constructor broadcast must make rank 0's weights win
        sd = {k: (v + 0.01 if v.is_floating_point() and "decode_head.convs" in k else v) for k, v in sd.items()}
    model.load_state_dict(sd)
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    gs = parallel.attach(model, ow)
    buckets = [b[0] for b in gs.buckets] if gs is not None else [b[0] for b in ow.optimizer.bucket_slices()]
    logs = []
    for step in range(2):
        idx = [0, 1] if world == 1 else [rank]
        imgs = torch.cat([synth_image(1, 512, seed=700 + 2 * step + j) for j in idx]).cuda()
        labs = torch.cat([synth_label(1, 512, seed=700 + 2 * step + j) for j in idx])
        log = model.train_step(dict(inputs=imgs, data_samples=[SegDataSample(gt_sem_seg=labs[k]) for k in range(len(idx))]), ow)
        rec = torch.tensor([float(log["decode.loss_ce"])], dtype=torch.float64)
        if world > 1:
            torch.distributed.all_reduce(rec)
            rec /= world
        logs.append(rec)
    torch.cuda.synchronize()
    if rank == 0:
        state = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
        torch.save(dict(state=state, logs=torch.stack(logs), buckets=buckets, names=list(ow.optimizer.names), world=world), out_path)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
