"""The Rein model through the product's surfaces: slide prediction, data parallelism (2 gloo ranks == 1 rank with the global batch, the
`reins` bucket sent after the backbone backward), and tools/train.py -> a rein-only checkpoint -> tools/test.py --backbone."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import vfmseg_amd  # noqa: E402,F401
from tests.rein_helpers import rein_model_state_dict  # noqa: E402
from vfmseg_amd import presets  # noqa: E402
from vfmseg_amd.precision import set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_like  # noqa: E402


def test_rein_slide_prediction_bf16_vs_f32():
    """`slide` (the Rein configs' test mode: 2 x 2 windows of 512^2, stride 320, on a 768^2 image), depth 4: the bf16 prediction
    (no saved activations, stream updated in place) against the f32 one; argmax equal except on near-ties of the logits - the margin rule
    of tests/test_model_gpu.py: every flipped pixel's top-2 margin is below the logits error bound."""
    depth = 4
    cfg = presets.rein_dinov2_linear(depth=depth)
    cfg["backbone"]["out_indices"] = [0, 1, 2, 3]
    model = MODELS.build(cfg)
    missing, unexpected = model.load_state_dict(rein_model_state_dict(depth), strict=False)
    assert not missing and not unexpected
    model = model.cuda().eval()
    assert not model.backbone.adapter_training()
    img = synth_image(1, 768, seed=21).cuda()
    outs = {}
    try:
        for mode in ("f32", "bf16"):
            set_compute_dtype(mode)
            with torch.no_grad():
                o = model.predict(img)[0]
            outs[mode] = (o.seg_logits.data.float().cpu(), o.pred_sem_seg.data[0].cpu())
    finally:
        set_compute_dtype("bf16")
    ref, got = outs["f32"][0], outs["bf16"][0]
    assert ref.shape == (19, 768, 768)
    e = ((got - ref).abs().max() / ref.abs().max()).item()
    mism = outs["bf16"][1] != outs["f32"][1]
    top2 = ref.topk(2, dim=0)[0]
    margin = (top2[0] - top2[1]) / (ref.max() - ref.min())
    worst = margin[mism].max().item() if mism.any() else 0.0
    frac = mism.float().mean().item()
    print(f"[rein slide bf16 vs f32] logits rel err {e:.2e}; argmax mismatch {frac:.2e}, largest relative top-2 margin among them {worst:.2e}")
    assert e < 3e-2 and frac < 1e-2 and worst < 3e-2


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "rein_dp_worker.py"), out], env=env, stdout=subprocess.PIPE,
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


def test_rein_two_ranks_equal_one_rank_with_the_global_batch(tmp_path):
    one = _run(1, str(tmp_path / "w1.pt"))
    two = _run(2, str(tmp_path / "w2.pt"))
    assert torch.allclose(one["logs"], two["logs"], rtol=1e-5, atol=1e-6), (one["logs"], two["logs"])
    worst, n = 0.0, 0
    for k, a in one["state"].items():
        if "running_" in k or "num_batches" in k or k == "decode_head.output_upscaling.0.bias":   # (a bias right before BatchNorm: exact gradient 0)
            continue
        if "transform" in k or "merge" in k:
            assert torch.equal(a, two["state"][k]), k   # never in the graph: untouched on every rank
            continue
        b = two["state"][k]
        d = (a - b).abs().mean().item() / max(a.abs().mean().item(), 1e-12)
        worst, n = max(worst, d), n + 1
        assert d < 2e-5, (k, d)     # as tests/test_dp_equivalence_gpu.py (f32): an update is ~1e-4 of the parameter per step
    assert n >= 7 + 8
    ev = two["events"]
    per_step = ev[:len(ev) // 2]
    assert per_step == ["decode_head", "<backbone backward ended>", "reins"], ev
    print(f"[rein dp equivalence f32] worst relative parameter difference {worst:.2e} over {n} tensors; bucket launch order {per_step}")


def test_train_py_then_test_py_with_a_rein_only_checkpoint(tmp_path):
    """tools/train.py on configs/dg_rein_dinov2_linearhead.py (depth cut by --cfg-options, synthetic stream), the frozen base named by the
    config's init_cfg as in the reference, saves a checkpoint of `reins` + head keys only; tools/test.py reloads it with the base from
    --backbone and writes the predictions an in-process model built from the SAME two files makes - and not those of a model without that base."""
    from PIL import Image
    import numpy as np
    from tests.rein_helpers import bare_dinov2_state_dict
    opts = ["model.backbone.depth=2", "model.backbone.reins_config.num_layers=2", "model.backbone.out_indices=[0,1,1,1]"]
    wd, bb, out = tmp_path / "wd", tmp_path / "base.pth", tmp_path / "out"
    torch.save(bare_dinov2_state_dict(2), bb)
    r = subprocess.run([sys.executable, "tools/train.py", "configs/dg_rein_dinov2_linearhead.py", "--data", "synthetic", "--max-iters", "3",
                        "--work-dir", str(wd), "--cfg-options"] + opts + ["default_hooks.logger.interval=1", f"model.backbone.init_cfg.checkpoint={bb}"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(wd / "iter_3.pth", map_location="cpu", weights_only=False)
    keys = set(ck["state_dict"])
    assert keys and all(k.startswith("backbone.reins.") or k.startswith("decode_head.") for k in keys), sorted(keys)[:4]
    assert "backbone.reins.scale" in keys and ck["state_dict"]["backbone.reins.scale"].dim() == 0
    cfg = presets.rein_dinov2_linear(depth=2)
    cfg["backbone"]["out_indices"] = [0, 1, 1, 1]
    sd0 = synth_like(MODELS.build(cfg).state_dict())
    assert not torch.equal(ck["state_dict"]["backbone.reins.learnable_tokens_a"], sd0["backbone.reins.learnable_tokens_a"]), "training moved nothing"
    r = subprocess.run([sys.executable, "tools/test.py", "configs/dg_rein_dinov2_linearhead.py", str(wd / "iter_3.pth"), "--backbone", str(bb),
                        "--data", "synthetic", "--images", "2", "--size", "512", "512", "--launcher", "none", "--out", str(out), "--cfg-options"] + opts,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "'evaluated_samples': 2" in r.stdout and "mIoU" in r.stdout
    pngs = sorted(os.listdir(out))
    assert len(pngs) == 2
    got = torch.from_numpy(np.asarray(Image.open(out / pngs[0])).astype(np.int64))
    # the same two files, in process: base through init_cfg, adapter + head from the checkpoint
    set_compute_dtype("bf16")
    preds = {}
    for with_base in (True, False):
        c2 = presets.rein_dinov2_linear(depth=2, checkpoint=str(bb) if with_base else None)
        c2["backbone"]["out_indices"] = [0, 1, 1, 1]
        m2 = MODELS.build(c2)
        missing, unexpected = m2.load_state_dict(ck["state_dict"], strict=False)
        assert not unexpected and all(k.startswith("backbone.") and ".reins." not in k for k in missing)
        m2 = m2.cuda().eval()
        with torch.no_grad():
            preds[with_base] = m2.predict(synth_image(1, 512, seed=500).cuda())[0].pred_sem_seg.data[0].cpu().long()
    same = (preds[True] == got).float().mean().item()
    blind = (preds[False] == got).float().mean().item()
    print(f"[rein tools round trip] pixels equal to the in-process prediction {same:.4f}; to a model WITHOUT the base {blind:.4f}")
    assert same > 0.999, same      # same kernels, same weights
    assert blind < 0.9, blind      # the comparison depends on the loaded base
