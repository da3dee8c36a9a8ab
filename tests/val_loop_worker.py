"""One rank of the multi-process tests of tests/test_val_loop_gpu.py (gloo; the ranks share the one GPU of the test box).
    python val_loop_worker.py eval DATA_ROOT N_IMAGES OUT_JSON     vfmseg_amd.evaluation.evaluate over the first N images of the tree
    python val_loop_worker.py train WORK_DIR BATCH_SIZE            three iterations with val_interval=2 through the Runner
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the environment."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def main():
    os.environ["VFMSEG_DIST_BACKEND"] = "gloo"
    os.environ["LOCAL_RANK"] = "0"       # one GPU
    import vfmseg_amd  # noqa: F401
    import val_loop_helpers as Hh
    from vfmseg_amd import lib as L, parallel
    from vfmseg_amd.precision import set_compute_dtype
    set_compute_dtype("bf16")
    mode = sys.argv[1]
    if mode == "eval":
        from vfmseg_amd.evaluation import evaluate
        from vfmseg_amd.registry import METRICS
        root, n, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
        rank, world, _ = parallel.init_from_env("gloo")
        torch.cuda.set_device(0)
        L.set_device_index(0)
        model = Hh.build_model()
        metric = METRICS.build(Hh.evaluator())
        seen = []
        res, info = evaluate(model, Hh.test_dataset(root), metric, rank, world, limit=n, on_output=lambda o, first: seen.append(first))
        with open(f"{out}.rank{rank}", "w") as f:
            json.dump(dict(metrics=dict(res), samples=info["samples"], state=info["state"][:-1].tolist(), seen=seen), f)
    elif mode == "train":
        from vfmseg_amd.runner import Runner
        work_dir, bs = sys.argv[2], int(sys.argv[3])
        set_compute_dtype("f32")    # no floating-point atomics in the backward: the only difference between the worlds is the order of the fp32 sums
        runner = Runner.from_cfg(Hh.train_cfg(work_dir, 3, val_interval=2, batch_size=bs, dropout=False, val_images=3))
        runner.train(log_interval=1, ckpt_interval=2)
        torch.cuda.synchronize()
    else:
        raise SystemExit(f"unknown mode {mode}")
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
