"""Every GEMM and attention launch of ONE train step (model.loss + backward with the optimiser's flat gradient buffer in place, LoRA and
head dropout at the configs' values), recorded from the model and replayed launch by launch on fresh operands through the default
dispatcher against float64 on the device (tests/launch_replay.py).

Models: the four backbone families at depth 2 (SAM: one windowed + one global block) with full widths, batch and crop of the bench
configurations (DINOv2 / EVA02 / CLIP: B = 2, 1024^2 -> LR + HR crop, 4 x 1025 = 4100 token rows; SAM: B = 1, 2 x 1024 rows); bf16 for
all four, fp16 (the `--amp` twin library) for DINOv2.  The dgrad / wgrad launches have M, N, K permuted relative to the forward ones, so
they land on other rules of the bf16 tile dispatcher than any forward launch; whatever rule a launch lands on, it must equal the float64
product of its own operands within the project's per-kernel bounds."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests.launch_replay import KINDS, Recorder, replay_all  # noqa: E402
from vfmseg_amd import ops, presets  # noqa: E402
from vfmseg_amd.precision import set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.segmentors import SegDataSample  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label, synth_state_dict  # noqa: E402

DEPTH = 2
TAPS = [0, 0, 1, 1]          # four taps for the heads from a depth-2 backbone (an index listed twice is a tap of its own)
LOSS_SCALE = 65536.0         # tests/test_amp_gpu.py: the AMP wrapper's initial scale


def _build(family):
    from tests.helpers import clip_state_dict, eva02_state_dict, full_state_dict, sam_state_dict
    if family == "dinov2":
        cfg = presets.dinov2_ms_masked(depth=DEPTH)
        cfg["backbone"]["backbone"]["out_indices"] = TAPS
        model = MODELS.build(cfg)
        model.load_state_dict(full_state_dict(depth=DEPTH))
        return model, 2
    if family in ("eva02", "clip"):
        cfg = presets.eva02_ms_masked(depth=DEPTH) if family == "eva02" else presets.clip_ms_masked(layers=DEPTH)
        cfg["backbone"]["backbone"]["out_indices"] = TAPS
        sd = {k: v for k, v in full_state_dict(depth=1).items() if not k.startswith("backbone.")}
        sd.update(eva02_state_dict(depth=DEPTH) if family == "eva02" else clip_state_dict(depth=DEPTH))
        model = MODELS.build(cfg)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and all(("rope" in k) or (".fpn" in k) for k in missing), (missing, unexpected)
        return model, 2
    assert family == "sam"
    gidx = (1,)
    cfg = presets.sam_ms_masked(depth=DEPTH, global_idx=gidx, out_indices=tuple(TAPS))
    model = MODELS.build(cfg)
    sd = sam_state_dict(depth=DEPTH, global_idx=gidx)
    heads = {k: (tuple(v.shape) if v.dtype != torch.int64 else ((), torch.int64)) for k, v in model.state_dict().items()
             if k.startswith(("decode_head.", "aux_decoder."))}
    sd.update(synth_state_dict(heads))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return model, 1


def _record_train_step(family, mode):
    """One model.loss(...) + backward of a fresh model under `mode`, as train_step runs it: parameters' .grad pre-pointed into the fused
    optimiser's flat buffer (the weight-gradient kernels accumulate straight into it), dropout on, random crop box and token mask fixed."""
    from vfmseg_amd import functional as Fh
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    Fh.manual_seed(4321)
    torch.manual_seed(0)
    model, B = _build(family)
    model = model.cuda().train()
    oc = presets.optim_cfg()
    PEFTOptimWrapperConstructor(dict(oc["optim_wrapper"], type="OptimWrapper"))(model, oc["param_scheduler"])
    model.fixed_crop_box = (256, 768, 128, 640)
    model.aux_decoder.transformer_decoder.fixed_keep = torch.rand(B, 1, 32, 32, generator=torch.Generator().manual_seed(12)) > 0.2
    img, lab = synth_image(B, 1024, seed=500).cuda(), synth_label(B, 1024, seed=500)
    with Recorder() as rec:
        losses = model.loss(img, [SegDataSample(gt_sem_seg=lab[i]) for i in range(B)])
        total, _ = model.parse_losses(losses)
        (total * LOSS_SCALE if mode == "fp16" else total).backward()
        torch.cuda.synchronize()
    assert bool(torch.isfinite(total.detach()).all()), (family, mode, float(total))
    del model
    torch.cuda.empty_cache()
    return rec.launches


def _gemms(launches, pred):
    return [k for k in launches["gemm"] if pred(k)]


def _assert_present(family, launches):
    """The launches each family's train step must have issued, derived from the code (so that a refactor cannot turn the replay into a
    no-op without this test saying so):
    every family  - heads: LinearFn.backward's dX = g @ W as a kb_rows GEMM (functional.py, `ops.gemm(g, wp, dx, trans_b=True, kb_rows=N)`),
                    its weight gradient as gemm_splitk_tn + slab_reduce into the flat buffer (functional.py _param_grads_impl), the mask
                    decoder's self / cross attention forward with lse and backward (functional.py SelfAttnFn / CrossAttnFn);
    dinov2        - the train plan (backbones.py _DinoTrainPlan): fc1 with EP_GELU_DGELU, attention forward with lse and backward with
                    the [cls] row (nq_extra = 1), GEMMs over the 4100 token rows, the LoRA weight gradients as gemm_tn_batched
                    (DinoEngine._lora_wgrads_batched);
    eva02 / clip  - attention with the [cls] row, 4100-row GEMMs, LoRA weight gradients through backbones._wgrad_small_t (65 steps of 64
                    tokens -> 13 slices: gemm_splitk_tn + slab_reduce, dB with a transposed destination); clip: c_fc with EP_QGELU;
    sam           - sam_attn_flash_fwd_train and sam_attn_flash_bwd for the windowed block (S = 14) and the global one (S = 32), fc1 with
                    EP_GELU_DGELU (sam.py), LoRA weight gradients through _wgrad_small_t over 2048 token rows (transposed dB as above)."""
    L = launches
    assert _gemms(L, lambda k: k[14] > 0), (family, "no kb_rows GEMM")
    assert L["splitk_tn"] and L["slab_reduce"], (family, "no split-K weight gradient / slab_reduce")
    assert any(k[12] for k in L["attn_fwd"]) and L["attn_bwd"], (family, "no attention forward with lse / backward")
    if family != "dinov2":      # dinov2's LoRA gradients take the batched form instead (no slabs)
        assert any(k[4] != 1 for k in L["slab_reduce"]), (family, "no slab_reduce with a transposed destination (sq != 1)")
    if family in ("dinov2", "eva02", "clip"):
        assert _gemms(L, lambda k: k[2][0][-2] == 4100), (family, "no GEMM over the 4100 token rows")
        assert any(k[12] and k[8] == 1 for k in L["attn_fwd"]) and any(k[12] == 1 for k in L["attn_bwd"]), (family, "no backbone attention")
    if family in ("dinov2", "sam"):
        assert _gemms(L, lambda k: k[9] == ops.EP_GELU_DGELU and k[11] is not None), (family, "no EP_GELU_DGELU GEMM")
    if family == "dinov2":
        assert L["tn_batched"], (family, "no gemm_tn_batched")
    if family == "clip":
        assert _gemms(L, lambda k: k[9] == ops.EP_QGELU), (family, "no EP_QGELU GEMM")
    if family == "sam":
        for kind, n in (("sam_fwd_train", 5), ("sam_bwd", 7)):
            assert {k[n] for k in L[kind]} == {14, 32}, (family, kind, "flash launches for S = 14 and the global block", L[kind].keys())
        assert _gemms(L, lambda k: k[2][0][-2] == 2048), (family, "no GEMM over the 2048 token rows")


@pytest.mark.parametrize("family,mode", [("dinov2", "bf16"), ("eva02", "bf16"), ("clip", "bf16"), ("sam", "bf16"), ("dinov2", "fp16")])
def test_every_launch_of_a_train_step_against_float64(family, mode):
    """Record one train step, assert the recording holds what that family's code path issues, replay every distinct launch once
    (tests/launch_replay.py asserts the per-launch bounds, the NaN-prefilled outputs / padding and the mutant distances), print one line per
    launch and the count and worst error per kind.

    Measured on an MI355X, worst over the five cases (bound): GEMM 16-bit output 3.5e-3 bf16 / 4.3e-4 fp16 (1e-2), fp32 output 1.2e-6
    (2e-5); gemm_splitk_tn 7.4e-7, gemm_tn_batched 8.3e-7 (2e-5); slab_reduce 4.3e-7 where the plain fp32 sum has 1.1e-7 (4 x that);
    attention forward 5.7e-3 (2e-2), lse 2.0e-7 where the plain fp32 evaluation has 1.1e-7 (4 x that), dq / dk / dv 5.5e-3 (4e-2); SAM flash
    forward 1.6e-2 (2e-2), backward 2.0e-2 (3e-2).  No launch missed its bound; every mutant distance held (smallest: the last 64 of
    K = 4160 into an fp32 output, 0.08 against 1e-4; into a 16-bit output 0.12 at K = 4096 against 5e-2)."""
    set_compute_dtype(mode)
    try:
        launches = _record_train_step(family, mode)
        counts = collections.OrderedDict((k, (len(launches[k]), sum(launches[k].values()))) for k in KINDS)
        print(f"[train launches {family} {mode}] distinct (issued): " + ", ".join(f"{k} {d} ({n})" for k, (d, n) in counts.items()))
        _assert_present(family, launches)
        worst = replay_all(launches, tag=f"[{family} {mode}] ")
        for kind, w in worst.items():
            print(f"[train launches {family} {mode}] {kind}: {counts[kind][0]} distinct, worst " + ", ".join(f"{k} {v:.1e}" for k, v in w.items()))
    finally:
        set_compute_dtype("bf16")


def _sp(shape, ld=None, dt=torch.bfloat16):
    """spec of a row-major tensor whose rows are `ld` apart"""
    st = [1] * len(shape)
    if len(shape) > 1:
        st[-2] = ld or shape[-1]
    for i in range(len(shape) - 3, -1, -1):
        st[i] = st[i + 1] * shape[i + 1]
    return (tuple(shape), tuple(st), dt)


def test_replay_of_the_launch_forms_other_step_shapes_issue():
    """The forms the replayer knows that the recorded steps above do not reach, at the shapes the code issues them with other batch
    sizes, through the same replay functions (same references, bounds, NaN padding and mutant checks):
    - backbones._wgrad_small_t with a prime number of 64-token steps (one image: 1025 tokens -> 17 steps, no split-K):
      ops.gemm(xt, y, out, alpha, trans_b=True, kb_rows=M), A zero beyond the M tokens;
    - the same weight gradient with an operand that cannot be consumed token-major: ops.gemm_splitk_bt over 4100 tokens in 13 slices,
      whose last slice clamps y's rows >= M;
    - functional._splitk_wgrad without chunks (ops.gemm(dyt, x, out, trans_b=True, kb_rows=m_rows)) at a ragged token count;
    - EP_MUL_QGELU_GRAD (CLIP's c_proj dgrad fused with the activation gradient) over the 4100 token rows;
    - batched fp32 operands with trans_a / trans_b (the f32 mode's batched weight gradients) and alpha != 1;
    - gemm_tn_batched with alpha != 1 and valid_rows < M."""
    from tests.launch_replay import replay_gemm, replay_splitk_bt, replay_tn_batched, describe
    f32 = torch.float32
    set_compute_dtype("bf16")
    gemm_keys = [
        (_sp((64, 1088)), _sp((1025, 1024)), _sp((64, 1024), dt=f32), 1.0, None, 0, None, None, False, ops.EP_NONE, None, None, False, True, 1025),
        (_sp((256, 2112)), _sp((2050, 512)), _sp((256, 512), dt=f32), 1.0, None, 0, None, None, False, ops.EP_NONE, None, None, False, True, 2050),
        (_sp((4100, 1088)), _sp((4096, 1088)), _sp((4100, 4096), 4224), 1.0, None, 0, None, None, False, ops.EP_MUL_QGELU_GRAD,
         _sp((4100, 4096), 4160), None, False, False, 0),
        (_sp((3, 300, 200), dt=f32), _sp((3, 300, 72), dt=f32), _sp((3, 200, 72), dt=f32), 0.25, _sp((72,), dt=f32), 0, None, None, False,
         ops.EP_NONE, None, None, True, True, 0),
    ]
    for i, key in enumerate(gemm_keys):
        res = replay_gemm(key, 7000 + 16 * i)
        print(f"{describe('gemm', key, 1)}: {res}")
    key = (_sp((64, 4160)), _sp((4100, 1024)), _sp((13, 64, 1024), dt=f32), 13)
    print(f"{describe('splitk_bt', key, 1)}: {replay_splitk_bt(key, 7100)}")
    key = (_sp((3, 1100, 64), 1088), _sp((3, 1100, 1024)), _sp((3, 64, 1024), dt=f32), 1025, 0.5)
    print(f"{describe('tn_batched', key, 1)}: {replay_tn_batched(key, 7200)}")
