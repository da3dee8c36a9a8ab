"""The HRDA model through the product's surfaces: data parallelism (2 gloo ranks == 1 rank with the global batch) and
tools/train.py -> checkpoint -> tools/test.py on configs/dg_lora_dinov2_hrda.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, out):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", VFMSEG_DIST_SINGLE="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "hrda_dp_worker.py"), out], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return torch.load(out, weights_only=False)


def test_hrda_two_ranks_equal_one_rank_with_the_global_batch(tmp_path):
    one = _run(1, str(tmp_path / "w1.pt"))
    two = _run(2, str(tmp_path / "w2.pt"))
    assert one["boxes"] == two["boxes"] and len(set(one["boxes"])) == 2
    assert torch.allclose(one["logs"], two["logs"], rtol=1e-5, atol=1e-6), (one["logs"], two["logs"])
    worst, n = 0.0, 0
    for k, a in one["state"].items():
        b = two["state"][k]
        if k.startswith("decode_head.conv_seg"):
            assert torch.equal(a, b), k      # never in the graph: untouched on every rank
            continue
        if "running_" in k or "num_batches" in k or k == "decode_head.head.output_upscaling.0.bias":   # (a bias right before BatchNorm: exact gradient 0)
            continue
        if "lora_" not in k and k.startswith("backbone."):
            continue
        d = (a - b).abs().mean().item() / max(a.abs().mean().item(), 1e-12)
        worst, n = max(worst, d), n + 1
        assert d < 2e-5, (k, d)     # as tests/test_dp_equivalence_gpu.py (f32): an update is ~1e-4 of the parameter per step
    assert n >= 4 + 14
    assert int(two["state"]["decode_head.head.output_upscaling.1.num_batches_tracked"]) == 4
    print(f"[hrda dp equivalence f32] worst relative parameter difference {worst:.2e} over {n} tensors")


def test_train_py_then_test_py_on_the_hrda_config(tmp_path):
    """tools/train.py on configs/dg_lora_dinov2_hrda.py (depth cut by --cfg-options, synthetic 1024^2 stream) for two iterations, then
    tools/test.py on two synthetic images with the checkpoint it wrote."""
    opts = ["model.backbone.backbone.depth=2", "model.backbone.backbone.out_indices=[0,1,1,1]"]
    wd, out = tmp_path / "wd", tmp_path / "out"
    r = subprocess.run([sys.executable, "tools/train.py", "configs/dg_lora_dinov2_hrda.py", "--data", "synthetic", "--max-iters", "2",
                        "--work-dir", str(wd), "--cfg-options"] + opts + ["default_hooks.logger.interval=1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for key in ("decode.loss_seg", "decode.acc_seg", "decode.hr.loss_seg", "decode.hr.acc_seg"):
        assert key in r.stdout, r.stdout[-1500:]
    ck = torch.load(wd / "iter_2.pth", map_location="cpu", weights_only=False)
    keys = set(ck["state_dict"])
    assert "decode_head.conv_seg.weight" in keys and "decode_head.scale_attention.fusion_conv.conv.weight" in keys
    assert int(ck["state_dict"]["decode_head.head.output_upscaling.1.num_batches_tracked"]) == 4
    r = subprocess.run([sys.executable, "tools/test.py", "configs/dg_lora_dinov2_hrda.py", str(wd / "iter_2.pth"), "--data", "synthetic",
                        "--images", "2", "--size", "1024", "1024", "--launcher", "none", "--out", str(out), "--cfg-options"] + opts,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "'evaluated_samples': 2" in r.stdout and "mIoU" in r.stdout
    assert len(os.listdir(out)) == 2
