"""Inference at the reference's DG evaluation sizes (oracle/gen_golden.py EVAL_SIZES: Cityscapes 1024 x 2048, ACDC 1080 x 1920,
BDD100k 720 x 1280, a Mapillary photo 1024 x 1365), where the window grid has more than 16 windows (the per-window gate and merge),
ragged last rows / columns, non-integer resize factors, context windows off the coarse grid and an odd width.

- predictions of the HIP path (depth 4) against the reference's own MsVFMEncoderDecoder.inference (tests/golden/eval_sizes.npz);
- the resize, gate and merge kernels at exactly the shapes these predictions issue, against float64;
- every GEMM and attention launch of these predictions (recorded from the model, not listed by hand), replayed on fresh operands
  through the default dispatcher against a float64 product."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from oracle.gen_golden import eval_sizes_probes, eval_sizes_seed  # noqa: E402
from tests.helpers import full_state_dict, rel_err  # noqa: E402
from tests.launch_replay import Recorder, describe, replay_attn_fwd, replay_gemm  # noqa: E402
from vfmseg_amd import ops, presets  # noqa: E402
from vfmseg_amd.precision import set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.segmentors import EncoderDecoder, grid_boxes  # noqa: E402
from vfmseg_amd.synth import synth_image  # noqa: E402

DEV = "cuda"
DEPTH = 4


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_sizes.npz"))


def _cases(G):
    """(h, w, mode, key) of every prediction the golden holds."""
    out = []
    for h, w in G["sizes"].tolist():
        for mode in ("ms_slide_inference", "lr_slide_inference"):
            key = f"{h}x{w}/{mode}::"
            if key + "logits_stats" in G.files:
                out.append((h, w, mode, key))
    return out


_MODELS = {}


def _model(prec):
    """One depth-4 model per precision mode (built under that mode, used only under it)."""
    set_compute_dtype(prec)
    if prec not in _MODELS:
        cfg = presets.dinov2_ms_masked(depth=DEPTH)
        cfg["backbone"]["backbone"]["out_indices"] = list(range(DEPTH))
        model = MODELS.build(cfg)
        model.load_state_dict(full_state_dict(depth=DEPTH))
        _MODELS[prec] = model.cuda().eval()
    return _MODELS[prec]


def _predict(model, G, h, w, mode, key, conf=None):
    model.test_cfg["mode"] = mode
    if mode == "ms_slide_inference":
        thr, c = (float(v) for v in G[key + "test_cfg"])
        model.test_cfg["threadshod"], model.test_cfg["conf"] = thr, (c if conf is None else conf)
    img = synth_image(1, (h, w), seed=eval_sizes_seed(h, w)).to(DEV)
    with torch.no_grad():
        return model.inference(img, [{}])


# ------------------------------------------------------------------------------------------------ predictions vs the reference
# f32: north_star's tolerance (test_model_gpu.py::test_ms_inference_matches_reference_golden); bf16: the bounds of
# test_eval_gpu.py::test_slide_modes_match_reference_goldens
@pytest.mark.parametrize("prec,ltol,mtol,margin_tol", [("f32", 1e-3, 2e-4, 1e-4), ("bf16", 2.6e-2, 2.5e-2, 1e-2)])
def test_predictions_at_eval_sizes_match_reference_goldens(golden_dir, prec, ltol, mtol, margin_tol):
    G = _golden(golden_dir)
    try:
        model = _model(prec)
        for h, w, mode, key in _cases(G):
            logits = _predict(model, G, h, w, mode, key)
            oh, ow = (h, w) if mode == "ms_slide_inference" else (h // 2 * 2, w // 2 * 2)
            assert tuple(logits.shape) == (1, 19, oh, ow), (key, logits.shape)
            if mode == "ms_slide_inference":
                assert np.array_equal(np.array(model.last_refined).reshape(-1, 4), G[key + "refined_boxes"]), (key, model.last_refined)
            errs = {name: rel_err(logits[0, :, y0:y1, x0:x1], G[key + "logits_" + name])
                    for name, (y0, y1, x0, x1) in eval_sizes_probes(oh, ow, grid_boxes(oh, ow, (512, 512), (320, 320)))}
            sub = logits[0, :, ::8, ::8]
            pred = sub.argmax(0).cpu().numpy().astype(np.uint8)
            diff = pred != G[key + "pred_sub8"]
            top2 = torch.topk(sub, 2, dim=0).values
            margin = ((top2[0] - top2[1]) / (logits.max() - logits.min())).cpu().numpy()
            worst = float(margin[diff].max()) if diff.any() else 0.0
            print(f"[eval sizes] {key} {prec}: logits rel err {max(errs.values()):.2e}, argmax mismatches {diff.mean():.2e}, "
                  f"largest top-2 margin among them {worst:.2e}")
            assert max(errs.values()) < ltol, (key, errs)
            assert diff.mean() < mtol and worst < margin_tol, (key, diff.mean(), worst)
    finally:
        set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------------ resize kernels
def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


def _relerr(a, b):
    """max |a - b| / max |b| on the device, in float64"""
    b = b.double()
    return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# (input size, output size, scale_factor or None) of the bilinear resizes the predictions above issue: the coarse pass squeezes the image
# to 512 x 1024 and its logits go back to the image size; lr_slide_inference halves the image and doubles its logits
_RESIZES = [((720, 1280), (512, 1024), None), ((512, 1024), (720, 1280), None), ((1080, 1920), (512, 1024), None),
            ((512, 1024), (1080, 1920), None), ((1024, 1365), (512, 1024), None), ((512, 1024), (1024, 1365), None),
            ((1024, 1365), (512, 682), 0.5), ((512, 682), (1024, 1364), 2.0), ((1080, 1920), (540, 960), 0.5)]


@pytest.mark.parametrize("C", [3, 19])
def test_resize_at_eval_sizes_against_float64(C):
    """ops.resize_bilinear at the (in, out) sizes of the evaluation predictions, NCHW and NHWC input, NCHW / NHWC / window-crop output,
    against F.interpolate in float64 with the same size= or scale_factor= call.  An odd size under scale_factor samples at 1/s, not
    in/out: 1365 -> 682 columns with the size-ratio source scale lands up to 2 units off on unit noise."""
    for (hi, wi), (ho, wo), sf in _RESIZES:
        x = _rnd(2, C, hi, wi, seed=hi + wi + C)
        if sf is None:
            ref = F.interpolate(x.double(), size=(ho, wo), mode="bilinear", align_corners=False)
        else:
            ref = F.interpolate(x.double(), scale_factor=sf, mode="bilinear", align_corners=False)
        assert tuple(ref.shape[2:]) == (ho, wo)
        # fp32 source coordinates (as ATen's fp32 kernels compute them) against float64: ~1e-4 pixel at these sizes
        tol = 2e-3 * ref.abs().max().item()
        xh = x.permute(0, 2, 3, 1).contiguous()
        for src, nchw in ((x, True), (xh, False)):
            out = torch.full((2, C, ho, wo), float("nan"), device=DEV)
            ops.resize_bilinear(src, nchw, 2, hi, wi, C, out, 1, (ho, wo), scale_factor=sf)
            assert (out.double() - ref).abs().max().item() < tol, ((hi, wi), (ho, wo), sf, nchw, "NCHW out")
            outh = torch.full((2, ho, wo, C), float("nan"), device=DEV)
            ops.resize_bilinear(src, nchw, 2, hi, wi, C, outh, 0, (ho, wo), scale_factor=sf)
            assert (outh.permute(0, 3, 1, 2).double() - ref).abs().max().item() < tol, ((hi, wi), (ho, wo), sf, nchw, "NHWC out")
        # a window of the virtual output: the last (ragged) window of the evaluation grid when the output is image-sized, else the
        # bottom-right corner
        y0, y1, x0, x1 = grid_boxes(ho, wo, (512, 512), (320, 320))[-1] if min(ho, wo) >= 512 else (ho - 100, ho, wo - 132, wo)
        win = torch.full((2, C, y1 - y0, x1 - x0), float("nan"), device=DEV)
        ops.resize_bilinear(x, True, 2, hi, wi, C, win, 1, (ho, wo), (y0, x0, y1 - y0, x1 - x0), scale_factor=sf)
        assert (win.double() - ref[:, :, y0:y1, x0:x1]).abs().max().item() < tol, ((hi, wi), (ho, wo), sf, "window")


def test_odd_width_scale_factor_differs_from_size_ratio():
    """The case lr_slide_inference hits at an odd width: the size-ratio sampling is measurably wrong there, so the comparison above would
    catch a resize that ignored scale_factor."""
    x = _rnd(1, 3, 1024, 1365, seed=3)
    ref = F.interpolate(x.double(), scale_factor=0.5, mode="bilinear", align_corners=False)
    out = torch.empty(1, 3, 512, 682, device=DEV)
    ops.resize_bilinear(x, True, 1, 1024, 1365, 3, out, 1, (512, 682))
    assert (out.double() - ref).abs().max().item() > 0.5


# ------------------------------------------------------------------------------------------------ gate and merge, 18 ragged windows
def test_gate_and_merge_over_eighteen_ragged_windows_against_float64():
    """ACDC's 1080 x 1920 grid: 18 windows (3 x 6; last row at y = 568, last column at x = 1408), past the 16-window tables of
    vfm_conf_gate_windows / vfm_slide_gather, so the segmentor takes the per-window paths.  Gate counts exactly equal a float64 softmax
    threshold count (logits kept away from the threshold); the merge of kept windows (NCHW, window resolution) and refined ones (NHWC
    quarter resolution, x4 bilinear) equals float64 F.interpolate + pad + count."""
    B, C, H, W, thr = 1, 19, 1080, 1920, 0.5
    boxes = grid_boxes(H, W, (512, 512), (320, 320))
    assert len(boxes) == 18 and boxes[-1] == (568, 1080, 1408, 1920)
    seg = _rnd(B, C, H, W, seed=21) * 3.0
    pmax = seg.double().softmax(1).max(1)[0]
    near = (pmax - thr).abs() < 1e-3
    seg[:, :, near[0]] = 0.0                          # uniform logits: max softmax 1/19, far below the threshold
    pmax = seg.double().softmax(1).max(1)[0]
    assert (pmax - thr).abs().min().item() > 1e-4
    want = [int((pmax[:, y1:y2, x1:x2] > thr).sum()) for (y1, y2, x1, x2) in boxes]
    cnt = torch.zeros(len(boxes), dtype=torch.int32, device=DEV)
    EncoderDecoder._gate_counts(seg, boxes, thr, cnt)
    assert cnt.tolist() == want
    assert 0 < min(want) and max(want) < B * 512 * 512
    # merge: every third window kept its coarse logits
    wins, ref = [], torch.zeros(B, C, H, W, dtype=torch.float64, device=DEV)
    count = torch.zeros(B, 1, H, W, dtype=torch.float64, device=DEV)
    for j, (y1, y2, x1, x2) in enumerate(boxes):
        if j % 3 == 1:
            t = _rnd(B, C, 512, 512, seed=400 + j)
            wins.append((t, True, (y1, x1, 512, 512)))
            up = t.double()
        else:
            t = _rnd(B, 128, 128, C, seed=400 + j)
            wins.append((t, False, (y1, x1, 512, 512)))
            up = F.interpolate(t.permute(0, 3, 1, 2).double(), size=(512, 512), mode="bilinear", align_corners=False)
        ref += F.pad(up, (x1, W - x2, y1, H - y2))
        count[:, :, y1:y2, x1:x2] += 1
    ref /= count
    assert int(count.min()) == 1 and int(count.max()) >= 4
    assert not ops.slide_gather(wins, torch.empty(B, C, H, W, device=DEV))   # the table path refuses 18 windows
    got = EncoderDecoder._merge_windows(wins, B, C, H, W, DEV)
    assert (got.double() - ref).abs().max().item() < 1e-5 * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ GEMM / attention launch replay
def _record(model, G):
    """The distinct GEMM / attention launches (operand shapes, strides, dtypes, epilogue) of the bf16 predictions at every evaluation
    size: ms_slide_inference with every window refined (the largest token batches: 18 x 1025 rows) and with the golden's gate, and
    lr_slide_inference.  Taken where ops builds the descriptors (tests/launch_replay.py: gemm_desc serves ops.gemm and the launch plans alike)."""
    with Recorder() as rec:
        for h, w, mode, key in _cases(G):
            _predict(model, G, h, w, mode, key)
            if mode == "ms_slide_inference":
                _predict(model, G, h, w, mode, key, conf=2.0)
        torch.cuda.synchronize()
    assert not any(rec.launches[k] for k in rec.launches if k not in ("gemm", "attn_fwd")), "a prediction issued a training-only launch"
    return rec.launches["gemm"], rec.launches["attn_fwd"]


def test_every_gemm_and_attention_launch_of_eval_size_predictions_against_float64(golden_dir, monkeypatch):
    """Every distinct GEMM and attention launch of the bf16 predictions at the evaluation sizes (the tile dispatcher's shape-exact rules
    choose by M: 18 windows = 18450 rows, 12 = 12300, 8 = 8200, plus the 2049-row coarse pass and the lr passes), replayed with fresh
    operands of the same shapes, strides, dtypes and epilogue through the default dispatcher, against a float64 product on the device
    (tests/launch_replay.py: operands scaled so that every epilogue term is visible, which the replay asserts from the reference alone)."""
    G = _golden(golden_dir)
    try:
        model = _model("bf16")
        monkeypatch.setenv("VFMSEG_EVAL_OVERLAP", "0")      # one stream: the recording is host-side, the launches the same
        gemms, attns = _record(model, G)
        rows = sorted({k[2][0][-2] for k in gemms})
        assert 18 * 1025 in rows and 8 * 1025 in rows and 12 * 1025 in rows and 2049 in rows, rows
        for i, key in enumerate(sorted(gemms, key=repr)):
            res = replay_gemm(key, 1000 + 16 * i)     # asserts: fp32 output 2e-5, half output 1e-2 (C and C2), the mutant distances
            print(f"{describe('gemm', key, gemms[key])}: rel err {res['c']:.1e}, mutant distances "
                  + " ".join(f"{k} {v:.2f}" for k, v in res["mutants"].items()))
        for i, key in enumerate(sorted(attns, key=repr)):
            res = replay_attn_fwd(key, 5000 + 8 * i)  # asserts: half 2e-2, fp32 2e-5
            print(f"{describe('attn_fwd', key, attns[key])}: rel err {res['o']:.1e}")
        print(f"[replay] {len(gemms)} distinct GEMM launches, {len(attns)} distinct attention launches")
    finally:
        set_compute_dtype("bf16")
