"""The SegFormer-head baselines (LoRA / Rein / frozen DINOv2 + SegformerHead) on the HIP path against tests/golden/segformer.npz (written
by the reference's own segmentors and backbones around a restated SegformerHead, tools/gen_segformer_golden.py), and through the
product's surfaces: optimiser, resume, data parallelism, tools/train.py -> tools/test.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import vfmseg_amd  # noqa: E402,F401
from tests import segformer_helpers as S  # noqa: E402
from tests.helpers import rel_err, sl  # noqa: E402
from vfmseg_amd import functional as Fh, ops, presets  # noqa: E402
from vfmseg_amd.heads import FeatPack  # noqa: E402
from vfmseg_amd.precision import compute_dtype, set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.segmentors import SegDataSample  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "segformer.npz"))


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    set_compute_dtype("bf16")


_MODELS = {}


def _model(kind, depth=S.DEPTH):
    """one model per (kind, depth) for the whole module, reloaded to the recipe's weights and shared across precision modes"""
    if (kind, depth) not in _MODELS:
        _MODELS[kind, depth] = MODELS.build(S.model_config(kind, depth)).to(DEV)
    model = _MODELS[kind, depth]
    missing, unexpected = model.load_state_dict(S.model_state_dict(kind, depth), strict=False)   # (strict=False: the Rein backbone's state_dict lists its adapter only)
    assert not missing and not unexpected, (missing, unexpected)
    for p in model.parameters():
        p.grad = None
    return model


def _pack(feats, dtype):
    B, C, h, w = feats[0].shape
    xcat = torch.cat([t.permute(0, 2, 3, 1).reshape(B * h * w, C) for t in feats], 1).to(DEV).to(dtype).contiguous()
    return FeatPack(xcat.requires_grad_(True), B, h, w)


def _tap_grad(fp, i):
    C = fp.xcat.shape[1] // 4
    return fp.xcat.grad[:, i * C:(i + 1) * C].reshape(fp.B, fp.hp, fp.wp, C).permute(0, 3, 1, 2).float()


def _grad2d(g):
    return g.reshape(g.shape[0], -1) if g.dim() > 1 else g


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("tile", ["0", "1"])
def test_head_matches_the_fixture_f32(G, tile, monkeypatch):
    """SegformerHead in f32 on the fixture's taps, with either GroupNorm form: logits (1e-5 of their range: the fixture is float64 arithmetic,
    the head three fp32 layers deep - measured 1.1e-6; a wrong eps or group boundary on one branch moves them by far more), loss_ce /
    acc_seg, every parameter gradient and the tap gradients (the f32 train-step bounds of tests/test_model_gpu.py: loss 1e-5, norms 1e-5,
    slices 1e-4), and the eval-mode logits."""
    monkeypatch.setenv("VFMSEG_GN_TILE", tile)
    set_compute_dtype("f32")
    head = MODELS.build(dict(presets.segformer_head(), dropout_ratio=0.0))
    head.load_state_dict(S.head_state_dict(prefix=""))
    head = head.to(DEV).train()
    assert Fh.gn_tile_selected(1024, 1024, 128) == (tile == "1")
    fp = _pack(S.head_feats(), torch.float32)
    lab = synth_label(2, 512, seed=S.HEAD_SEED).to(DEV)
    losses, full = head.loss(fp, lab, return_logits=True)
    losses["loss_ce"].backward()
    Fh.join_wgrad_stream()
    torch.cuda.synchronize()
    logits = head.forward(fp).detach()
    assert tuple(logits.shape) == (2, 19, 32, 32) and tuple(full.shape) == (2, 19, 512, 512)
    errs = dict(slice=rel_err(sl(logits), G["head::logits_slice"]), grid=rel_err(logits[:, :, 3::8, 5::8], G["head::logits_grid"]))
    assert max(errs.values()) < 1e-5, errs
    got = np.array([float(losses["loss_ce"].detach()), float(losses["acc_seg"].detach())])
    np.testing.assert_allclose(got[0], G["head::loss_acc"][0], rtol=1e-5)
    np.testing.assert_allclose(got[1], G["head::loss_acc"][1], atol=2e-3)
    serr, nerr = {}, {}
    for n, p in head.named_parameters():
        assert p.grad is not None, n
        serr[n] = rel_err(sl(_grad2d(p.grad)), G[f"head::grad_slice::{n}"])
        nerr[n] = abs(p.grad.double().norm().item() / G[f"head::grad_norm::{n}"][0] - 1.0)
    for i in range(4):
        t = _tap_grad(fp, i)
        serr[f"tap{i}"] = rel_err(sl(t[:, :, 8:, 8:]), G[f"head::tap_grad_slice::{i}"])
        nerr[f"tap{i}"] = abs(t.double().norm().item() / G[f"head::tap_grad_norm::{i}"][0] - 1.0)
    print(f"[parity] segformer head f32 (tile={tile}): logits {errs}, loss rel err {abs(got[0] / G['head::loss_acc'][0] - 1):.2e}, worst gradient slice "
          f"{max(serr.values()):.2e} ({max(serr, key=serr.get)}), worst gradient norm {max(nerr.values()):.2e} ({max(nerr, key=nerr.get)})")
    assert max(serr.values()) < 1e-4 and max(nerr.values()) < 1e-5, (serr, nerr)
    head.eval()
    with torch.no_grad():
        ev = head.forward(_pack(S.head_feats(), torch.float32))
    assert rel_err(sl(ev), G["head::eval_logits_slice"]) < 1e-5


def test_dropout2d_zeroes_whole_image_channels_and_redraws(monkeypatch):
    """Train mode, dropout_ratio 0.1: the mask has one multiplier per (image, channel) - 8 x 256 of them, each 0 or 1 / 0.9 - the zeroed share is
    inside five binomial standard deviations (n = 2048, p = 0.1: 205 +- 68), and two steps draw different masks."""
    set_compute_dtype("bf16")
    head = MODELS.build(presets.segformer_head()).to(DEV).train()
    masks = []
    real = ops.dropout_mask
    monkeypatch.setattr(ops, "dropout_mask", lambda out, *a, **k: (real(out, *a, **k), masks.append(out))[0])
    g = torch.Generator().manual_seed(3)
    fp = FeatPack(torch.randn(8 * 64, 4096, generator=g).to(DEV).bfloat16(), 8, 8, 8)
    a = head.forward_tokens(fp)
    b = head.forward_tokens(fp)
    assert len(masks) == 2 and all(tuple(m.shape) == (8, 256) for m in masks)
    n, p = 8 * 256, 0.1
    for m in masks:
        m = m.float()
        zero = (m == 0)
        assert bool((zero | ((m - 1 / 0.9).abs() < 1e-6)).all())
        assert abs(int(zero.sum()) - n * p) <= 5 * (n * p * (1 - p)) ** 0.5, int(zero.sum())
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(a, b)
    head.eval()
    assert torch.equal(head.forward_tokens(fp), head.forward_tokens(fp)) and len(masks) == 2


# ------------------------------------------------------------------------------------------------ train step
# (ltol, ntol, stol) = loss / gradient-group norm / gradient slice, per mode, from the existing LinearHead train-step tests:
#   bf16 - the depth-4 LinearHead step of tests/test_rein_gpu.py (1e-2, 5e-2, 1.2e-1), the one depth-4 LinearHead step that runs in bf16;
#   f32  - lora / frozen: the depth-24 step of tests/test_model_gpu.py (1e-5, 1e-5, 1e-4), tighter than both depth-4 tests (test_model_gpu's
#          LoraBackboneEncoderDecoder check: loss 2e-4, gradients 5e-3; test_rein_gpu's: 1e-4, 1e-3, 2e-4); rein: test_rein_gpu's;
#   fp16 - no depth-4 LinearHead step runs in fp16: the depth-24 step of tests/test_model_gpu.py (also the depth-4 HRDA step's).
# Measured (MI355X): f32 loss <= 9.4e-8, norms <= 6.0e-6, slices <= 7.6e-5; fp16 loss <= 1.3e-4, norms <= 2.3e-4, slices <= 9.3e-3;
# bf16 loss 1.4e-3 .. 1.5e-3, norms <= 3.5e-3, slices <= 4.6e-2.  The bf16 loss error is the format's, not the kernels': on the fixture's
# head inputs the bf16 head lands on 34.52629 where a float64 evaluation with bf16 roundings at the same points gives 34.52623 (float64:
# 34.50384) - ReLU'd GroupNorm maps are non-negative, so rounded weights shift a logit the same way at every pixel and the mean does not
# average it out.  It is above the 1e-3 that the depth-24 LinearHead + VFMHead step of tests/test_model_gpu.py allows in bf16.
BOUNDS = {"f32": (1e-5, 1e-5, 1e-4), "bf16": (1e-2, 5e-2, 1.2e-1), "fp16": (3e-4, 1e-3, 4e-2)}
REIN_BOUNDS = {"f32": (1e-4, 1e-3, 2e-4), "bf16": BOUNDS["bf16"], "fp16": BOUNDS["fp16"]}


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("kind", S.KINDS)
def test_train_step_matches_the_reference(G, kind, mode):
    """loss + backward at depth 4 (B = 2, 512^2, dropout 0) of the three models against the reference's own segmentors: loss, acc_seg, the
    norms of the gradient groups (backbone adapters, head) and every recorded gradient slice."""
    ltol, ntol, stol = (REIN_BOUNDS if kind == "rein" else BOUNDS)[mode]
    set_compute_dtype(mode)
    model = _model(kind).train()
    img, lab = synth_image(2, 512, seed=S.TRAIN_SEED), synth_label(2, 512, seed=S.TRAIN_SEED)
    losses = model.forward(img.to(DEV), [SegDataSample(gt_sem_seg=lab[i]) for i in range(2)], mode="loss")
    assert sorted(losses) == ["decode.acc_seg", "decode.loss_ce"]
    total, _ = model.parse_losses(losses)
    gscale = 65536.0 if mode == "fp16" else 1.0
    (total * gscale).backward()
    Fh.join_wgrad_stream()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    for p_ in named.values():
        if p_.grad is not None and gscale != 1.0:
            p_.grad.div_(gscale)
    k = f"{kind}::"
    ref_loss, ref_acc = G[k + "train_loss_acc"]
    loss, acc = float(losses["decode.loss_ce"]), float(losses["decode.acc_seg"])
    assert sum(p.numel() for p in named.values() if p.grad is not None) == int(G[k + "train_n_trainable"][0])
    assert all(named[n].grad is None for n in G[k + "train_no_grad"])
    norms, serr = [0.0, 0.0], {}
    for n, p in named.items():
        if p.grad is not None:
            norms[n.startswith("decode_head.")] += p.grad.double().pow(2).sum().item()
    for name in G.files:
        if name.startswith(k + "train_grad_slice::"):
            n = name.split("::", 2)[2]
            g = named[n].grad
            assert g is not None, n
            serr[n] = rel_err(sl(_grad2d(g) if g.dim() else g.reshape(1)), G[name])
    ref_norms = G[k + "train_grad_norms"]
    nerr = [abs(np.sqrt(a) / b - 1.0) if b > 0 else np.sqrt(a) for a, b in zip(norms, ref_norms)]
    print(f"[parity] segformer {kind} train_step {mode}: loss {loss:.6f} (ref {ref_loss:.6f}, rel err {abs(loss / ref_loss - 1):.2e}), acc abs err "
          f"{abs(acc - ref_acc):.2e}, grad-norm rel err (backbone, head) {nerr[0]:.2e} {nerr[1]:.2e}, worst of {len(serr)} gradient slices "
          f"{max(serr.values()):.2e} ({max(serr, key=serr.get)})")
    assert abs(loss - ref_loss) <= ltol * abs(ref_loss)
    assert abs(acc - ref_acc) <= (0.05 if mode == "bf16" else (1e-2 if mode == "fp16" else 2e-3))
    assert nerr[1] < ntol and (nerr[0] < ntol if ref_norms[0] > 0 else nerr[0] == 0.0), nerr
    for n, e in serr.items():
        assert e < stol, (n, e)
    if kind == "frozen":
        assert len(serr) == len(S.HEAD_KEYS)
    else:
        assert any(n.startswith("backbone.") for n in serr)


def test_frozen_model_trains_the_head_only():
    """No backbone parameter has a gradient or changes over two optimiser steps, the backbone is in eval mode, the taps carry no graph, and
    the optimiser holds the head's gradient group alone; every head parameter moves."""
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    set_compute_dtype("bf16")
    model = _model("frozen", 2).train()
    assert not model.backbone.training and model.decode_head.training
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    assert [b[0] for b in ow.optimizer.bucket_slices()] == ["decode_head"]
    assert sorted(ow.optimizer.names) == sorted("decode_head." + k for k in S.HEAD_KEYS)
    img, lab = synth_image(2, 512, seed=61).to(DEV), synth_label(2, 512, seed=61)
    fp = model.extract_feat(img)
    assert not fp.xcat.requires_grad and fp.xcat.grad_fn is None
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    for _ in range(2):
        log = model.train_step(dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)]), ow)
        assert np.isfinite(float(log["loss"]))
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if n.startswith("backbone."):
            assert not p.requires_grad and p.grad is None and torch.equal(p.detach(), before[n]), n
        else:
            assert not torch.equal(p.detach(), before[n]), n
    assert any(k.startswith("backbone.blocks.") for k in model.state_dict())   # the checkpoint holds the whole model


def test_rein_adapter_bucket_and_head_bucket():
    """The Rein model with the SegformerHead keeps the two gradient groups of the LinearHead model, in launch order: the head's, then `reins`
    (sent when the backbone backward ends, vfmseg_amd.parallel.attach)."""
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    set_compute_dtype("bf16")
    model = _model("rein", 2).train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    assert [b[0] for b in ow.optimizer.bucket_slices()] == ["decode_head", "reins"]


# ------------------------------------------------------------------------------------------------ predictions
def _check_logits(G, key, logits, ltol, mtol, margin_tol, tag):
    logits = logits.float().cpu()
    H, W = logits.shape[2:]
    errs = dict(grid=rel_err(logits[0, :, 5::64, 5::64], G[key + "logits_grid"]), slice=rel_err(sl(logits[0, :, H // 2 - 4:, W // 2 - 4:]), G[key + "logits_slice"]))
    diff = logits.argmax(1)[0, ::16, ::16].numpy() != G[key + "pred_sub16"]
    worst = float(G[key + "margin_sub16"][diff].max()) if diff.any() else 0.0
    print(f"[parity] segformer {tag}: logits rel err {errs}, argmax flips {diff.mean():.2e} of {diff.size} sampled pixels, largest top-2 margin among them {worst:.2e}")
    assert max(errs.values()) < ltol, errs
    assert diff.mean() < mtol and worst < margin_tol, (diff.mean(), worst)
    return diff.sum()


# logit bounds and the near-tie rule for argmax flips: those of the slide tests (tests/test_eval_gpu.py, tests/test_hrda_gpu.py)
@pytest.mark.parametrize("prec,ltol,mtol,margin_tol", [("f32", 1e-3, 2e-4, 1e-4), ("bf16", 2.6e-2, 2.5e-2, 1e-2)])
def test_slide_predictions_match_the_reference(G, prec, ltol, mtol, margin_tol):
    """The configs' 512 / 341 slide at depth 4 over 512 x 768 (two windows) and 1024 x 1024 (nine) against the reference's
    LoraBackboneEncoderDecoder.slide_inference; f32: no argmax flip at all."""
    set_compute_dtype(prec)
    model = _model("lora").eval()
    with torch.no_grad():
        for i, (h, w) in enumerate(S.SLIDE_SIZES):
            out = model.inference(synth_image(1, (h, w), seed=S.EVAL_SEED + i).to(DEV), None)
            assert tuple(out.shape) == (1, 19, h, w)
            flips = _check_logits(G, f"lora::slide_{h}x{w}::", out, ltol, mtol, margin_tol, f"slide {h}x{w} {prec}")
            assert prec != "f32" or flips == 0


# ------------------------------------------------------------------------------------------------ training runs
def _train_run(steps, resume_after=None, tmp_path=None):
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    Fh.manual_seed(4321)

    def build():
        cfg = presets.rein_dinov2_segformer(depth=2)      # dropout on
        cfg["backbone"]["out_indices"] = [0, 1, 1, 1]
        cfg["backbone"].pop("init_cfg")
        m = MODELS.build(cfg)
        m.load_state_dict(S.model_state_dict("rein", 2), strict=False)
        return m.to(DEV).train()
    model = build()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    img, lab = synth_image(2, 512, seed=9).to(DEV), synth_label(2, 512, seed=9)
    data = lambda: dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)])
    logs = []
    for step in range(steps):
        if resume_after is not None and step == resume_after:
            ck = dict(state_dict={k: v.clone() for k, v in model.state_dict().items()}, optimizer=ow.optimizer.state_dict(), wrapper=ow.state_dict(),
                      rng=dict(Fh._seed_state))
            ck["optimizer"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ck["optimizer"].items()}
            torch.save(ck, tmp_path / "ck.pt")
            del model, ow
            ck = torch.load(tmp_path / "ck.pt", weights_only=False)
            model = build()
            model.load_state_dict(ck["state_dict"], strict=False)
            ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
            ow.optimizer.load_state_dict(ck["optimizer"])
            ow.load_state_dict(ck["wrapper"])
            Fh._seed_state.update(ck["rng"])
        logs.append(float(model.train_step(data(), ow)["loss"]))
    torch.cuda.synchronize()
    return logs, {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_training_lowers_the_loss_and_resumes_bit_identically(tmp_path):
    """Three optimiser steps of the Rein model at depth 2 on a fixed batch (bf16, Dropout2d on): the loss falls, and checkpoint -> rebuild ->
    resume before the third step reproduces the uninterrupted run bit for bit."""
    set_compute_dtype("bf16")
    logs, state = _train_run(3)
    assert logs[2] < logs[0], logs
    logs2, state2 = _train_run(3, resume_after=2, tmp_path=tmp_path)
    assert logs2 == logs, (logs, logs2)
    for k in state:
        assert torch.equal(state[k], state2[k]), k


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "segformer_dp_worker.py"), out], env=env, stdout=subprocess.PIPE,
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


def test_frozen_two_ranks_equal_one_rank_with_the_global_batch(tmp_path):
    one = _run(1, str(tmp_path / "w1.pt"))
    two = _run(2, str(tmp_path / "w2.pt"))
    assert torch.allclose(one["logs"], two["logs"], rtol=1e-5, atol=1e-6), (one["logs"], two["logs"])
    assert two["buckets"] == ["decode_head"] and all(n.startswith("decode_head.") for n in two["names"])
    start = S.model_state_dict("frozen", 2)
    worst, n = 0.0, 0
    for k, a in one["state"].items():
        b = two["state"][k]
        if k.startswith("backbone."):
            assert torch.equal(a, b) and torch.equal(a, start[k]), k      # frozen: untouched on every rank
            continue
        d = (a - b).abs().mean().item() / max(a.abs().mean().item(), 1e-12)
        worst, n = max(worst, d), n + 1
        assert d < 2e-5, (k, d)     # as tests/test_dp_equivalence_gpu.py (f32): an update is ~1e-4 of the parameter per step
        assert not torch.equal(a, start[k]), k
    assert n == len(S.HEAD_KEYS)
    print(f"[segformer frozen dp equivalence f32] worst relative parameter difference {worst:.2e} over {n} tensors")


def test_train_py_then_test_py_on_the_rein_segformer_config(tmp_path):
    """tools/train.py on configs/dg_rein_dinov2_segformer.py (depth cut by --cfg-options, synthetic stream) for two iterations with the frozen
    base named by the config's init_cfg, then tools/test.py on two synthetic 512 x 768 images (two slide windows) with the checkpoint it wrote."""
    from tests.rein_helpers import bare_dinov2_state_dict
    opts = ["model.backbone.depth=2", "model.backbone.reins_config.num_layers=2", "model.backbone.out_indices=[0,1,1,1]"]
    wd, bb, out = tmp_path / "wd", tmp_path / "base.pth", tmp_path / "out"
    torch.save(bare_dinov2_state_dict(2), bb)
    r = subprocess.run([sys.executable, "tools/train.py", "configs/dg_rein_dinov2_segformer.py", "--data", "synthetic", "--max-iters", "2",
                        "--work-dir", str(wd), "--cfg-options"] + opts + ["default_hooks.logger.interval=1", f"model.backbone.init_cfg.checkpoint={bb}"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "decode.loss_ce" in r.stdout and "decode.acc_seg" in r.stdout, r.stdout[-1500:]
    ck = torch.load(wd / "iter_2.pth", map_location="cpu", weights_only=False)
    keys = set(ck["state_dict"])
    assert {"decode_head." + k for k in S.HEAD_KEYS} <= keys and "backbone.reins.scale" in keys
    assert all(k.startswith("backbone.reins.") or k.startswith("decode_head.") for k in keys), sorted(keys)[:4]
    r = subprocess.run([sys.executable, "tools/test.py", "configs/dg_rein_dinov2_segformer.py", str(wd / "iter_2.pth"), "--backbone", str(bb),
                        "--data", "synthetic", "--images", "2", "--size", "512", "768", "--launcher", "none", "--out", str(out), "--cfg-options"] + opts,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "'evaluated_samples': 2" in r.stdout and "mIoU" in r.stdout
    assert len(os.listdir(out)) == 2
