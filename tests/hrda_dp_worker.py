"""One rank of the HRDA data-parallel equivalence test (tests/test_hrda_model_gpu.py): two train steps of a depth-2
HRDAEncoderDecoder in f32 through parallel.attach; rank 0 writes the results.

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the env (gloo: the ranks share the one GPU of the test box);  argv: OUT.pt

world 1 trains on the global batch [s0, s1]; world 2 gives sample r to rank r.  Every rank seeds the numpy stream alike, so all of them
crop the box the single process crops; the LinearHead inside the HRDAHead exchanges its BatchNorm moments in BOTH of its calls per step."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    out_path = sys.argv[1]
    os.environ["VFMSEG_DIST_BACKEND"] = "gloo"
    import vfmseg_amd  # noqa: F401
    from tests.hrda_helpers import hrda_model_state_dict
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
    cfg = presets.dinov2_hrda(depth=depth)
    cfg["backbone"]["backbone"]["out_indices"] = [0, 1, 1, 1]
    cfg["backbone"]["Lora_config"]["lora_dropout"] = 0.0
    cfg["decode_head"]["seg_head"]["dropout_ratio"] = 0.0
    cfg["decode_head"]["single_scale_head"]["dropout_ratio"] = 0.0
    model = MODELS.build(cfg)
    sd = hrda_model_state_dict(depth)
    if rank != 0:   # the constructor broadcast must make rank 0's weights win
        sd = {k: (v + 0.01 if v.is_floating_point() and "scale_attention" in k else v) for k, v in sd.items()}
    model.load_state_dict(sd)
    model = model.cuda().train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    parallel.attach(model, ow)
    assert world == 1 or model.decode_head.head.bn_world == world
    np.random.seed(5)
    logs, boxes = [], []
    for step in range(2):
        idx = [0, 1] if world == 1 else [rank]
        imgs = torch.cat([synth_image(1, 1024, seed=600 + 2 * step + j) for j in idx]).cuda()
        labs = torch.cat([synth_label(1, 1024, seed=600 + 2 * step + j) for j in idx])
        log = model.train_step(dict(inputs=imgs, data_samples=[SegDataSample(gt_sem_seg=labs[k]) for k in range(len(idx))]), ow)
        rec = torch.tensor([float(log["decode.loss_seg"]), float(log["decode.hr.loss_seg"])], dtype=torch.float64)
        if world > 1:
            torch.distributed.all_reduce(rec)
            rec /= world
        logs.append(rec)
        boxes.append(tuple(model.last_crop_box))
    torch.cuda.synchronize()
    if rank == 0:
        state = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
        torch.save(dict(state=state, logs=torch.stack(logs), boxes=boxes, world=world), out_path)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
