"""HRDA on the HIP path: the fusion kernels against a float64 restatement, the heads and the segmentor against tests/golden/hrda.npz
(written by the reference's own modules, tools/gen_hrda_golden.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import hrda_helpers as H  # noqa: E402
from tests.helpers import rel_err, sl  # noqa: E402
from vfmseg_amd import functional as Fh, ops, presets  # noqa: E402
from vfmseg_amd.heads import FeatPack  # noqa: E402
from vfmseg_amd.precision import set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.segmentors import SegDataSample  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label  # noqa: E402

DEV = "cuda"
NAN = float("nan")
ZERO_GRAD_BIAS = "head.output_upscaling.0.bias"   # a bias right before BatchNorm: its exact gradient is 0, what either side holds is rounding noise

# (B, C, ha, wa, h, w, hr size, offset in the [2h, 2w] grid, mask box on the lr grid)
FUSE_CASES = {
    "crop_at_origin": (2, 19, 4, 4, 16, 16, (16, 16), (0, 0), (0, 8, 0, 8)),
    "crop_interior": (2, 19, 4, 4, 16, 16, (16, 16), (6, 10), (3, 11, 5, 13)),
    "crop_bottom_right": (2, 19, 4, 4, 16, 16, (16, 16), (16, 16), (8, 16, 8, 16)),
    "non_square": (2, 19, 2, 6, 8, 24, (8, 16), (4, 20), (2, 6, 10, 18)),
    "no_crop": (2, 19, 4, 4, 16, 16, (32, 32), (0, 0), None),
    "ratio_2": (2, 19, 8, 8, 16, 16, (16, 16), (10, 6), (5, 13, 3, 11)),
}


def _run_kernels(lr, a, hr, dF, offset, mask_box, fill=NAN):
    lr, a, hr, dF = (t.to(DEV).contiguous() for t in (lr, a, hr, dF))
    B, h, w, C = lr.shape
    fused = torch.full((B, 2 * h, 2 * w, C), fill, device=DEV)
    att, lrs = torch.full_like(lr, fill), torch.full_like(lr, fill)
    ops.hrda_fuse_fwd(lr, a, hr, offset, mask_box, fused, att, lrs)
    d_lr, d_a, d_hr = torch.full_like(lr, fill), torch.full_like(a, fill), torch.full_like(hr, fill)
    ops.hrda_fuse_bwd(dF, lr, a, hr, att, offset, mask_box, d_lr, d_a, d_hr)
    return dict(fused=fused, lr_scaled=lrs, d_lr=d_lr, d_a=d_a, d_hr=d_hr)


@pytest.mark.parametrize("case", list(FUSE_CASES))
def test_fuse_kernels_match_float64(case):
    """vfm_hrda_fuse_fwd / _bwd into NaN-prefilled buffers against the float64 restatement (tests/hrda_helpers.fuse_ref + autograd).
    Bound: 4 x the error a plain fp32 torch evaluation of the same formulas shows against float64 on the same operands (the convention of
    test_kernels_gpu.py; floor one fp32 rounding).  From the float64 reference alone: dropping the mask, the inserted HR logits, the
    (1 - att) factor or the s (1 - s) factor moves some output by at least 10 x that bound."""
    B, C, ha, wa, h, w, (hc, wc), offset, mask_box = FUSE_CASES[case]
    lr, a, hr, dF = H.fuse_inputs(B, C, ha, wa, h, w, hc, wc, seed=700 + list(FUSE_CASES).index(case))
    names = ("fused", "lr_scaled", "d_lr", "d_a", "d_hr")
    ref = dict(zip(names, H.fuse_ref_grads(lr.double(), a.double(), hr.double(), offset, mask_box, dF.double())))
    plain = dict(zip(names, H.fuse_ref_grads(lr, a, hr, offset, mask_box, dF)))
    got = _run_kernels(lr, a, hr, dF, offset, mask_box)
    bound = {}
    for n in names:
        assert torch.isfinite(got[n]).all(), (case, n, "an output element was not written")
        e, e_plain = rel_err(got[n], ref[n]), rel_err(plain[n], ref[n])
        bound[n] = 4.0 * max(e_plain, 2.0 ** -24)
        print(f"[hrda fuse {case}] {n}: rel err {e:.2e}, plain fp32 evaluation {e_plain:.2e}")
        assert e <= bound[n], (case, n, e, bound[n])
    drops = ["hr_ins", "one_minus_att", "sig_grad"] + (["mask"] if mask_box is not None else [])
    for drop in drops:
        mut = dict(zip(names, H.fuse_ref_grads(lr.double(), a.double(), hr.double(), offset, mask_box, dF.double(), drop=drop)))
        seen = max(rel_err(mut[n], ref[n]) / bound[n] for n in names)
        assert seen >= 10.0, (case, drop, seen)


def test_fuse_kernels_are_bit_reproducible():
    B, C, ha, wa, h, w, (hc, wc), offset, mask_box = FUSE_CASES["crop_interior"]
    lr, a, hr, dF = H.fuse_inputs(B, C, ha, wa, h, w, hc, wc, seed=77)
    r1 = _run_kernels(lr, a, hr, dF, offset, mask_box)
    r2 = _run_kernels(lr, a, hr, dF, offset, mask_box, fill=1e30)
    for n in r1:
        assert torch.equal(r1[n], r2[n]), n


def test_fuse_autograd_function():
    """HrdaFuseFn: forward + backward through autograd equal the float64 restatement; the second output carries no gradient."""
    B, C, ha, wa, h, w, (hc, wc), offset, mask_box = FUSE_CASES["crop_interior"]
    lr, a, hr, dF = H.fuse_inputs(B, C, ha, wa, h, w, hc, wc, seed=78)
    t = [v.to(DEV).requires_grad_(True) for v in (lr, a, hr)]
    fused, lrs = Fh.HrdaFuseFn.apply(t[0], t[1], t[2], offset, mask_box)
    assert not lrs.requires_grad
    fused.backward(dF.to(DEV))
    ref = H.fuse_ref_grads(lr.double(), a.double(), hr.double(), offset, mask_box, dF.double())
    for got, want in zip((fused, lrs, t[0].grad, t[1].grad, t[2].grad), ref):
        assert rel_err(got, want) < 1e-5


def test_fuse_refuses_a_crop_outside_the_grid():
    from vfmseg_amd.lib import HipError
    B, C, ha, wa, h, w, (hc, wc), _, mask_box = FUSE_CASES["crop_interior"]
    lr, a, hr, dF = (v.to(DEV) for v in H.fuse_inputs(B, C, ha, wa, h, w, hc, wc, seed=79))
    with pytest.raises(HipError):
        ops.hrda_fuse_fwd(lr, a, hr, (17, 0), mask_box, torch.empty(B, 2 * h, 2 * w, C, device=DEV))
    with pytest.raises(HipError):
        ops.hrda_fuse_fwd(lr, a, hr, (0, 0), (0, 17, 0, 8), torch.empty(B, 2 * h, 2 * w, C, device=DEV))


# ------------------------------------------------------------------------------------------------ heads
@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "hrda.npz"))


def _pack(feats, dtype=torch.float32, requires_grad=False):
    B = feats[0].shape[0]
    x = torch.cat([f.permute(0, 2, 3, 1).reshape(B * 1024, 1024) for f in feats], 1).to(dtype).cuda().contiguous()
    return FeatPack(x.requires_grad_(requires_grad), B, 32, 32)


def _tap_grad(fp, i):
    return fp.xcat.grad.view(fp.B, fp.hp, fp.wp, 4, -1)[:, :, :, i].permute(0, 3, 1, 2)


def _zero_dropout(m):
    for mod in m.modules():
        if hasattr(mod, "dropout_ratio"):
            mod.dropout_ratio = 0.0
    bb = getattr(m, "backbone", None)
    if bb is not None:
        for blk in bb.vit.blocks:
            blk.attn.qkv.p = 0.0


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", list(H.HEAD_BOXES))
def test_hrda_head_matches_the_reference(G, case):
    """AttentionHead + HRDAHead in f32 (train mode, dropout 0) on seeded taps against the reference's own heads: logits around the crop
    border, the four log values, every parameter gradient, the tap gradients, and the LinearHead's BatchNorm updated twice."""
    box, k = H.HEAD_BOXES[case], f"head_{case}::"
    set_compute_dtype("f32")
    try:
        head = MODELS.build(dict(presets.dinov2_hrda()["decode_head"], scales=[0.5, 1], enable_hr_crop=True)).cuda()
        head.load_state_dict(H.hrda_head_state_dict(prefix=""))
        head.train()
        _zero_dropout(head)
        assert not head.conv_seg.weight.requires_grad
        lr_f, hr_f = H.head_feats()
        lr_fp, hr_fp = _pack(lr_f, requires_grad=True), _pack(hr_f, requires_grad=True)
        lab = synth_label(2, 1024, seed=H.HEAD_SEED).cuda()
        with torch.no_grad():
            a_log = head.scale_attention.forward_tokens(lr_fp)
        assert rel_err(sl(_nchw(a_log)), G[k + "att_logits_slice"]) < 1e-3
        head.set_hr_crop_box(box)
        fused, lrs, hr = head.forward([lr_fp, hr_fp])
        assert tuple(fused.shape) == (2, 256, 256, 19) and tuple(hr.shape) == (2, 128, 128, 19)
        Y0, Y1, X0, X1 = H.scale_box(box, 4)
        ys, xs = slice(max(Y0 - 4, 0), max(Y0 - 4, 0) + 8), slice(max(X0 - 4, 0), max(X0 - 4, 0) + 8)
        ye, xe = slice(min(Y1 + 4, 256) - 8, min(Y1 + 4, 256)), slice(min(X1 + 4, 256) - 8, min(X1 + 4, 256))
        errs = dict(fused_tl=rel_err(_nchw(fused)[:, :, ys, xs], G[k + "fused_tl"]), fused_br=rel_err(_nchw(fused)[:, :, ye, xe], G[k + "fused_br"]),
                    lr=rel_err(_nchw(lrs)[:, :, Y0 // 2 - 4:Y0 // 2 + 4, X0 // 2 - 4:X0 // 2 + 4], G[k + "lr_slice"]),
                    hr=rel_err(sl(_nchw(hr)), G[k + "hr_slice"]))
        print(f"[hrda head {case}] logits rel err {errs}")
        assert max(errs.values()) < 1e-3, errs
        from tests.helpers import stats
        np.testing.assert_allclose(stats(fused), G[k + "fused_stats"], rtol=1e-3)
        losses = head.losses((fused, lrs, hr), lab)
        head.reset_crop()
        got = np.array([float(losses[n]) for n in ("loss_seg", "acc_seg", "hr.loss_seg", "hr.acc_seg")])
        print(f"[hrda head {case}] losses {got} reference {G[k + 'losses']}")
        np.testing.assert_allclose(got[[0, 2]], G[k + "losses"][[0, 2]], rtol=1e-4)
        np.testing.assert_allclose(got[[1, 3]], G[k + "losses"][[1, 3]], atol=2e-3)
        (losses["loss_seg"] + losses["hr.loss_seg"]).backward()
        Fh.join_wgrad_stream()
        named, worst = dict(head.named_parameters()), {}
        assert sorted(n for n, p in named.items() if p.grad is None) == list(G[k + "no_grad"])
        for name in G.files:
            if name.startswith(k + "grad_norm::"):
                n = name.split("::", 2)[2]
                if n == ZERO_GRAD_BIAS:
                    continue
                g = named[n].grad
                np.testing.assert_allclose(g.double().norm().item(), G[name][0], rtol=1e-4, atol=1e-7, err_msg=n)
                worst[n] = rel_err(sl(g.reshape(g.shape[0], -1) if g.dim() > 1 else g), G[k + f"grad_slice::{n}"])
        assert len(worst) == 15
        for i, fp in enumerate((lr_fp, hr_fp)):
            for j in range(4):
                np.testing.assert_allclose(_tap_grad(fp, j).double().norm().item(), G[k + f"tap_grad_norm::{4 * i + j}"][0], rtol=1e-4)
            worst[f"tap{4 * i}"] = rel_err(sl(_tap_grad(fp, 0)[:, :, 8:, 8:]), G[k + f"tap_grad_slice::{4 * i}"])
        print(f"[hrda head {case}] worst gradient slice {max(worst.values()):.2e} ({max(worst, key=worst.get)})")
        assert max(worst.values()) < 1e-3, worst
        bn = head.head.output_upscaling[1]
        assert int(bn.num_batches_tracked) == 2 == int(G[k + "bn_num_batches_tracked"][0])
        assert rel_err(sl(bn.running_mean), G[k + "bn_running_mean_slice"]) < 1e-4 and rel_err(sl(bn.running_var), G[k + "bn_running_var_slice"]) < 1e-4
    finally:
        set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------------ segmentor
def _build_model(depth=4, frozen=False):
    cfg = presets.dinov2_hrda(depth=depth)
    cfg["backbone"]["backbone"]["out_indices"] = list(range(depth)) if depth >= 4 else [0, 1, 1, 1]
    if frozen:
        cfg["type"] = "FrozenHRDAEncoderDecoder"
    model = MODELS.build(cfg).cuda()
    missing, unexpected = model.load_state_dict(H.hrda_model_state_dict(depth), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return model


# tolerances: those of the depth-24 train-step comparison against train_step.npz (tests/test_model_gpu.py) per precision mode
@pytest.mark.parametrize("mode,ltol,ntol,stol", [("f32", 1e-5, 1e-5, 1e-4), ("bf16", 1e-3, 3e-3, 1.2e-1), ("fp16", 3e-4, 1e-3, 4e-2)])
def test_hrda_train_step_matches_the_reference(G, mode, ltol, ntol, stol):
    """HRDAEncoderDecoder.loss + backward at depth 4 (B = 2, 1024^2: half-size pass + the 512^2 crop the numpy stream draws) against the
    reference's own segmentor: the drawn box, the four log values, gradient norms and slices, BatchNorm statistics updated twice."""
    set_compute_dtype(mode)
    try:
        model = _build_model().train()
        _zero_dropout(model)
        img, lab = synth_image(2, 1024, seed=H.TRAIN_SEED), synth_label(2, 1024, seed=H.TRAIN_SEED)
        samples = [SegDataSample(gt_sem_seg=lab[i]) for i in range(2)]
        np.random.seed(int(G["train_np_seed"][0]))
        losses = model.loss(img.cuda(), samples)
        assert tuple(model.last_crop_box) == tuple(G["train_box"]) and model.decode_head.hr_crop_box is None
        keys = list(G["train_loss_keys"])
        assert sorted(losses) == sorted(keys)
        got = np.array([float(losses[k]) for k in keys])
        lerr = np.abs(got[[0, 2]] / G["train_losses"][[0, 2]] - 1.0)
        total, _ = model.parse_losses(losses)
        gscale = 65536.0 if mode == "fp16" else 1.0
        (total * gscale).backward()
        Fh.join_wgrad_stream()
        named = dict(model.named_parameters())
        for p_ in named.values():
            if p_.grad is not None and gscale != 1.0:
                p_.grad.div_(gscale)
        assert sum(p.numel() for p in named.values() if p.requires_grad) == int(G["train_n_trainable"][0])
        assert all(named[n].grad is None for n in G["train_no_grad"])
        norms, serr = [0.0, 0.0], {}
        for n, p in named.items():
            if p.grad is not None:
                norms["lora_" not in n] += p.grad.double().pow(2).sum().item()
        for name in G.files:
            if name.startswith("train_grad_slice::"):
                n = name.split("::", 1)[1]
                if n == "decode_head." + ZERO_GRAD_BIAS:
                    continue
                g = named[n].grad
                serr[n] = rel_err(sl(g.reshape(g.shape[0], -1) if g.dim() > 1 else g), G[name])
        nerr = np.abs(np.sqrt(norms) / G["train_grad_norms"] - 1.0)
        print(f"[parity] hrda train_step {mode}: loss rel err {lerr.max():.2e}, acc abs err {np.abs(got[[1, 3]] - G['train_losses'][[1, 3]]).max():.2e}, "
              f"grad-norm rel err (lora, decode_head) {nerr[0]:.2e} {nerr[1]:.2e}, worst of {len(serr)} gradient slices "
              f"{max(serr.values()):.2e} ({max(serr, key=serr.get)})")
        np.testing.assert_allclose(got[[0, 2]], G["train_losses"][[0, 2]], rtol=ltol)
        np.testing.assert_allclose(got[[1, 3]], G["train_losses"][[1, 3]], atol=0.05 if mode == "bf16" else (1e-2 if mode == "fp16" else 2e-3))
        np.testing.assert_allclose(np.sqrt(norms), G["train_grad_norms"], rtol=ntol)
        for n, e in serr.items():
            assert e < stol, (n, e)
        bn = model.decode_head.head.output_upscaling[1]
        assert int(bn.num_batches_tracked) == 2
        btol = 1e-4 if mode == "f32" else 2e-2
        print(f"[parity] hrda train_step {mode}: BN running mean / var slice rel err {rel_err(sl(bn.running_mean), G['train_bn_running_mean_slice']):.2e} "
              f"{rel_err(sl(bn.running_var), G['train_bn_running_var_slice']):.2e}")
        assert rel_err(sl(bn.running_mean), G["train_bn_running_mean_slice"]) < btol and rel_err(sl(bn.running_var), G["train_bn_running_var_slice"]) < btol
    finally:
        set_compute_dtype("bf16")


def _check_logits(G, key, logits, ltol, mtol, margin_tol, tag):
    logits = logits.float().cpu()
    errs = dict(grid=rel_err(logits[0, :, 5::64, 5::64], G[key + "logits_grid"]), slice=rel_err(sl(logits[0, :, 508:, 508:]), G[key + "logits_slice"]))
    diff = logits.argmax(1)[0, ::32, ::32].numpy() != G[key + "pred_sub32"]
    worst = float(G[key + "margin_sub32"][diff].max()) if diff.any() else 0.0
    print(f"[parity] hrda {tag}: logits rel err {errs}, argmax flips {diff.mean():.2e} of {diff.size} sampled pixels, largest top-2 margin among them {worst:.2e}")
    assert max(errs.values()) < ltol, errs
    assert diff.mean() < mtol and worst < margin_tol, (diff.mean(), worst)


# logit bounds and the near-tie rule for argmax flips: those of tests/test_eval_sizes_gpu.py
@pytest.mark.parametrize("prec,ltol,mtol,margin_tol", [("f32", 1e-3, 2e-4, 1e-4), ("bf16", 2.6e-2, 2.5e-2, 1e-2)])
def test_hrda_predictions_match_the_reference(G, prec, ltol, mtol, margin_tol):
    """encode_decode of one 1024^2 image (half-size pass + nine overlapping 512^2 crops in one backbone call, merged at os 4, fused) and
    the 1024 / 682 slide over a 1024 x 1536 image (two windows) against the reference's own segmentor at depth 4."""
    set_compute_dtype(prec)
    try:
        model = _build_model().eval()
        with torch.no_grad():
            img = synth_image(1, 1024, seed=H.EVAL_SEED).cuda()
            out = model.encode_decode(img, None)
            assert tuple(out.shape) == (1, 19, 1024, 1024)
            _check_logits(G, "encdec_1024::", out, ltol, mtol, margin_tol, f"encode_decode 1024^2 {prec}")
            img = synth_image(1, (1024, 1536), seed=H.EVAL_SEED + 1).cuda()
            out = model.inference(img, None)
            assert tuple(out.shape) == (1, 19, 1024, 1536)
            _check_logits(G, "slide_1024x1536::", out, ltol, mtol, margin_tol, f"slide 1024x1536 {prec}")
            if prec == "f32":   # one backbone call for all outer windows against one per window: the same sums
                model.sequential_windows = True
                seq = model.inference(img, None)
                assert rel_err(out, seq) < 1e-3
                pred = model.predict(img)[0].pred_sem_seg.data
                assert tuple(pred.shape[-2:]) == (1024, 1536)
    finally:
        set_compute_dtype("bf16")


def test_frozen_variant_trains_the_head_only():
    set_compute_dtype("bf16")
    model = _build_model(depth=2, frozen=True).train()
    assert not model.backbone.training
    img, lab = synth_image(1, 1024, seed=5), synth_label(1, 1024, seed=5)
    losses = model.loss(img.cuda(), [SegDataSample(gt_sem_seg=lab[0])])
    total, _ = model.parse_losses(losses)
    total.backward()
    Fh.join_wgrad_stream()
    named = dict(model.named_parameters())
    assert all(p.grad is None and not p.requires_grad for n, p in named.items() if n.startswith("backbone."))
    assert named["decode_head.scale_attention.conv_seg.weight"].grad.abs().max() > 0
    assert named["decode_head.head.conv_seg.weight"].grad.abs().max() > 0


# ------------------------------------------------------------------------------------------------ training runs
def _train_run(steps, resume_after=None, tmp_path=None):
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    Fh.manual_seed(1234)
    np.random.seed(77)
    model = _build_model(depth=2).train()
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    img, lab = synth_image(1, 1024, seed=9).cuda(), synth_label(1, 1024, seed=9)
    data = lambda: dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[0])])
    logs, boxes = [], []
    for step in range(steps):
        if resume_after is not None and step == resume_after:
            ck = dict(state_dict={k: v.clone() for k, v in model.state_dict().items()}, optimizer=ow.optimizer.state_dict(), wrapper=ow.state_dict(),
                      np_state=np.random.get_state(), rng=dict(Fh._seed_state))
            ck["optimizer"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ck["optimizer"].items()}
            torch.save(ck, tmp_path / "ck.pt")
            del model, ow
            ck = torch.load(tmp_path / "ck.pt", weights_only=False)
            model = _build_model(depth=2).train()
            model.load_state_dict(ck["state_dict"])
            ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
            ow.optimizer.load_state_dict(ck["optimizer"])
            ow.load_state_dict(ck["wrapper"])
            np.random.set_state(ck["np_state"])
            Fh._seed_state.update(ck["rng"])
        log = model.train_step(data(), ow)
        logs.append(float(log["loss"]))
        boxes.append(model.last_crop_box)
    torch.cuda.synchronize()
    return logs, boxes, {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_hrda_training_lowers_the_loss_and_resumes_bit_identically(tmp_path):
    """Three optimiser steps at depth 2 on a fixed batch (bf16, dropout on, the numpy stream drawing the crop box): two
    optimiser steps lower the loss, and checkpoint -> rebuild -> resume before the third step reproduces the uninterrupted run bit for bit."""
    set_compute_dtype("bf16")
    logs, boxes, state = _train_run(3)
    assert logs[2] < logs[0], logs   # two optimiser steps
    assert len(set(boxes)) > 1, "the crop box should move between steps"
    logs2, boxes2, state2 = _train_run(3, resume_after=2, tmp_path=tmp_path)
    assert boxes2 == boxes and logs2 == logs, (logs, logs2)
    for k in state:
        assert torch.equal(state[k], state2[k]), k
    inert = state["decode_head.conv_seg.weight"]
    assert torch.equal(inert.cpu(), H.hrda_model_state_dict(2)["decode_head.conv_seg.weight"]), "the unused conv_seg must not move (no gradient in the reference)"
