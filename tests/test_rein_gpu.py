"""Rein adapters on the GPU: the fused kernels (vfm_rein_mix_fwd / _bwd) and the whole adapter step against the reference-made one-step
fixture (tests/golden/rein.npz) and the float64 restatement of tests/rein_helpers.py (pinned to that fixture by tests/test_rein_cpu.py);
fused == composed; the full-depth backbone and a train step against the fixture; optimiser steps.

Error bounds of the 16-bit modes come from the number formats, not from what the kernels give.  eps = half an ulp of the 16-bit type
(bf16 2^-9, fp16 2^-12).  Forward values pass five roundings (x, T, P, V, u) with fp32 accumulation between them, and the softmax turns an
absolute score error d into a relative probability error d with |c x T^T| of order 8 here: 16 eps on the largest element.  Gradients pass
those and as many again (g, du, P, dS, x): 32 eps.  All comparisons are max-norm relative (tests/helpers.rel_err)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests.helpers import rel_err, sl, stats  # noqa: E402
from tests.rein_helpers import (rein_backbone_state_dict, rein_model_state_dict, rein_params, rein_step_f64,  # noqa: E402
                                step_inputs)
from vfmseg_amd import ops, presets  # noqa: E402
from vfmseg_amd.precision import compute_dtype, set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.segmentors import SegDataSample  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label  # noqa: E402

EPS = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}
D = 1024


def _fwd_tol(mode):
    return 16 * EPS[mode]


def _bwd_tol(mode):
    return 32 * EPS[mode]


_STEP_MODELS = {}


def _step_model(lora):
    """A depth-4 Rein backbone whose `reins` parameters are the one-step fixture's (shared by every precision mode)."""
    if lora not in _STEP_MODELS:
        cfg = presets.rein_dinov2_linear(depth=4)["backbone"]
        cfg["out_indices"] = [0, 1, 2, 3]
        if not lora:
            cfg["reins_config"] = dict(type="Reins", token_length=100, embed_dims=D, num_layers=4, patch_size=16, link_token_to_query=False)
        m = MODELS.build(cfg)
        missing, unexpected = m.reins.load_state_dict(rein_params(depth=4, lora=lora), strict=True)
        _STEP_MODELS[lora] = m.cuda().train()
    return _STEP_MODELS[lora]


def _pack_operands(prm, layer, m, dt):
    """t, v [128, D], their transposes [D, 128] in dtype dt (zero pad rows, zero row 0 of v) from float64 parameters."""
    _, _, _, aux = rein_step_f64(torch.zeros(1, D, dtype=torch.float64, device="cuda"), torch.zeros(1, D, dtype=torch.float64, device="cuda"), prm, layer)
    T, V = aux["T"][:m], aux["V"][:m - 1]
    t = torch.zeros(128, D, dtype=dt, device="cuda")
    v = torch.zeros(128, D, dtype=dt, device="cuda")
    t[:m], v[1:m] = T.to(dt), V.to(dt)
    return t, v, t.t().contiguous(), v.t().contiguous()


CASES = [  # rows, rows of the stream buffer (the extra ones stand for the class rows: never read, never written), ld, token_length, LoRA tokens
    (1024, 1024, D, 100, True),
    (2 * 2049 - 1, 2 * 2049 + 2, D, 100, False),     # a last tile with one live row
    (9216, 9216, D + 64, 64, True),              # nine-window prediction batch, padded leading dimension, 64 tokens
]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("rows,buf_rows,ld,m,lora", CASES)
def test_rein_mix_kernels_vs_f64(mode, rows, buf_rows, ld, m, lora):
    set_compute_dtype(mode)
    try:
        dt = compute_dtype()
        prm = {k: v.cuda() for k, v in rein_params(depth=2, m=m, lora=lora).items()}
        x, g = step_inputs(buf_rows, D, seed=rows % 97)
        xbuf = torch.full((buf_rows, ld), 7.0, device="cuda")
        xbuf[:, :D] = x.cuda()
        xv = xbuf[:rows, :D]
        xo, dx_ref, grads, aux = rein_step_f64(xv, g[:rows].cuda(), prm, 1)
        t, v, tt, vt = _pack_operands(prm, 1, m, dt)
        u = torch.full((buf_rows, D), 5.0, dtype=dt, device="cuda")
        p = torch.full((buf_rows, 128), 5.0, dtype=dt, device="cuda")
        x16 = torch.full((buf_rows, D), 5.0, dtype=dt, device="cuda")
        ops.rein_mix_fwd(xv, t, vt, u[:rows], m, D ** -0.5, p=p[:rows], x16=x16[:rows])
        torch.cuda.synchronize()
        assert bool((p[:rows, m:] == 0).all()), "pad columns must carry exactly zero probability"
        assert bool((u[rows:] == 5.0).all()) and bool((p[rows:] == 5.0).all()) and bool((x16[rows:] == 5.0).all()), "rows past the end were written"
        assert torch.equal(x16[:rows], xv.to(dt))
        ep, eu = rel_err(p[:rows, :m], aux["P"]), rel_err(u[:rows], aux["u"])
        # inference form (no saved outputs) gives the same u
        u2 = torch.empty(rows, D, dtype=dt, device="cuda")
        ops.rein_mix_fwd(xv, t, vt, u2, m, D ** -0.5)
        assert torch.equal(u2, u[:rows])
        # backward from the float64 du and P rounded to 16 bits
        du = aux["du"].to(dt)
        pin = torch.zeros(rows, 128, dtype=dt, device="cuda")
        pin[:, :m] = aux["P"].to(dt)
        ds = torch.full((buf_rows, 128), 5.0, dtype=dt, device="cuda")
        dxb = torch.full((buf_rows, ld), 3.0, device="cuda")
        g32 = g[:rows].cuda()
        dxb[:rows, :D] = g32
        ops.rein_mix_bwd(du, pin, v, tt, ds[:rows], dxb[:rows, :D], m, D ** -0.5)
        torch.cuda.synchronize()
        assert bool((ds[:rows, m:] == 0).all()) and bool((ds[rows:] == 5.0).all())
        assert bool((dxb[rows:] == 3.0).all()) and bool((dxb[:, D:] == 3.0).all()), "gradient stream written outside its rows / columns"
        eds, edx = rel_err(ds[:rows, :m], aux["dS"]), rel_err(dxb[:rows, :D], dx_ref)
        print(f"[rein kernels {mode} rows {rows} m {m}] P {ep:.2e} u {eu:.2e} dS {eds:.2e} dx {edx:.2e}")
        assert ep < _fwd_tol(mode) and eu < _fwd_tol(mode), (ep, eu)
        assert eds < _bwd_tol(mode) and edx < _bwd_tol(mode), (eds, edx)
    finally:
        set_compute_dtype("bf16")


def _engine_step(model, x, g, fused):
    """The whole adapter step of layer 3 through DinoEngine's own methods: x', dx and the gradients of the live parameters."""
    eng = model.engine()
    os.environ["VFMSEG_REIN_FUSED"] = "1" if fused else "0"
    try:
        for p_ in model.parameters():
            p_.grad = None
        P = eng.packed()
        R = eng._rein_pack(P)
        assert R["fused"] == (fused and compute_dtype() != torch.float32)
        rows = x.shape[0]
        stream = torch.cat([x, torch.full((2, x.shape[1]), 9.0)]).cuda()     # two class rows after the patch rows
        S = {}
        xn = eng._rein_forward(R, 3, stream, rows, S)
        assert torch.equal(xn[rows:], stream[rows:]) and torch.equal(stream[:rows], x.cuda()), "class rows pass through; x is not updated in training"
        dx = torch.cat([g, torch.full((2, x.shape[1]), 4.0)]).cuda()
        acc = eng._rein_backward_begin(R)
        eng._rein_backward(R, acc, 3, dx, rows, S)
        grads = eng._rein_backward_end(R, acc)
        assert bool((dx[rows:] == 4.0).all())
        order = {id(p_): n for n, p_ in model.reins.named_parameters()}
        return xn[:rows], dx[:rows], {order[id(p_)]: g_ for p_, g_ in zip(model.reins.live_params(), grads)}
    finally:
        os.environ.pop("VFMSEG_REIN_FUSED", None)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16", "fp16"])
@pytest.mark.parametrize("lora", [True, False])
def test_adapter_step_vs_fixture_and_f64(golden_dir, mode, lora):
    """[2048, 1024], layer 3: the reference's LoRAReins / Reins forward + autograd (fixture slices and norms) and the float64 restatement
    (whole tensors).  f32 meets 1e-4 (exact-fp32 products), bf16x3 ten times that; the 16-bit modes the format bounds, fused AND composed."""
    G = np.load(os.path.join(golden_dir, "rein.npz"))
    tag = "lora" if lora else "plain"
    x, g = step_inputs()
    prm = {k: v.cuda() for k, v in rein_params(depth=4, lora=lora).items()}
    xo_ref, dx_ref, gref, _ = rein_step_f64(x.cuda(), g.cuda(), prm, 3)
    set_compute_dtype(mode)
    try:
        model = _step_model(lora)
        ftol, btol = {"f32": (1e-4, 2e-4), "bf16x3": (1e-3, 2e-3)}.get(mode) or (_fwd_tol(mode), _bwd_tol(mode))
        outs = {}
        for fused in ((True, False) if mode in EPS else (False,)):
            xo, dx, grads = _engine_step(model, x, g, fused)
            outs[fused] = (xo, dx, grads)
            rep = {"xo": rel_err(xo, xo_ref), "dx": rel_err(dx, dx_ref)}
            assert rel_err(sl(xo), G[f"step_{tag}_xo_slice"]) < ftol and rel_err(sl(dx), G[f"step_{tag}_dx_slice"]) < btol
            for n, gr in grads.items():
                rep[n] = rel_err(gr, gref[n])
                np.testing.assert_allclose(gr.double().norm().item(), G[f"step_{tag}_grad_norm::{n}"][0], rtol=btol)
            print(f"[rein step {mode} {tag} {'fused' if fused else 'composed'}]", {k: f"{v:.1e}" for k, v in rep.items()})
            assert rep["xo"] < ftol, rep
            assert all(v < btol for k, v in rep.items() if k != "xo"), rep
            assert set(grads) == set(gref)
        if len(outs) == 2:   # fused == composed within the same bounds
            assert rel_err(outs[True][0], outs[False][0]) < ftol and rel_err(outs[True][1], outs[False][1]) < btol
            for n in outs[True][2]:
                assert rel_err(outs[True][2][n], outs[False][2][n]) < btol, n
    finally:
        set_compute_dtype("bf16")


def test_backbone_fused_equals_composed():
    """Depth-4 backbone, bf16, batch 2: taps and every Rein parameter gradient of the fused kernels against the composed form."""
    set_compute_dtype("bf16")
    model = _step_model(True)
    img = synth_image(2, 512, seed=83).cuda()
    res = {}
    try:
        for flag in ("1", "0"):
            os.environ["VFMSEG_REIN_FUSED"] = flag
            for p_ in model.parameters():
                p_.grad = None
            xcat, _ = model.forward_tokens([(img, None)], training=True)
            assert model.engine()._packed["rein"]["fused"] == (flag == "1")
            dx = torch.randn(xcat.shape, generator=torch.Generator().manual_seed(5)).to(xcat.dtype).cuda()
            xcat.backward(dx)
            res[flag] = (xcat.detach().float(), {n: p_.grad.clone() for n, p_ in model.reins.named_parameters() if p_.grad is not None})
    finally:
        os.environ.pop("VFMSEG_REIN_FUSED", None)
    assert len(res["1"][1]) == 7 and set(res["1"][1]) == set(res["0"][1])
    e = rel_err(res["1"][0], res["0"][0])
    eg = {n: rel_err(res["1"][1][n], res["0"][1][n]) for n in res["1"][1]}
    print("[rein backbone fused vs composed] taps", f"{e:.2e}", {k: f"{v:.1e}" for k, v in eg.items()})
    assert e < _fwd_tol("bf16") and all(v < _bwd_tol("bf16") for v in eg.values()), (e, eg)
    assert all(p_.grad is None for n, p_ in model.named_parameters() if "reins" not in n), "the frozen base must get no gradient"


# ---------------------------------------------------------------- full depth vs the reference-made fixture
_FULL = {}
# (tap slice, tensor stats, grad slice, grad norm): the rows tests/test_fulldepth_gpu.py holds the LoRA backbones to
MODES = [("f32", 1e-4, 1e-3, 2e-4, 1e-3), ("bf16", 4e-2, 2e-2, 1.2e-1, 5e-2), ("fp16", 6e-3, 3e-3, 2e-2, 8e-3)]


FORMS = [(m_ + (f_,)) for m_ in MODES for f_ in ((False, True) if m_[0] in EPS else (False,))]


@pytest.mark.parametrize("mode,tol,stol,gtol,ntol,fused", FORMS)
def test_rein_full_depth_vs_reference_golden(golden_dir, mode, tol, stol, gtol, ntol, fused):
    """reins_dinov2.py:17-34 at depth 24 (one 512^2 image): the four taps, then the gradient of every live Rein parameter.  The 16-bit
    modes are held to the same numbers in both forms of the token attention (composed = the default, fused kernels)."""
    G = np.load(os.path.join(golden_dir, "rein.npz"))
    set_compute_dtype(mode)
    os.environ["VFMSEG_REIN_FUSED"] = "1" if fused else "0"
    try:
        if "m" not in _FULL:
            cfg = presets.rein_dinov2_linear()["backbone"]
            m = MODELS.build(cfg)
            missing, unexpected = m.load_state_dict(rein_backbone_state_dict(24), strict=False)
            assert not missing and not unexpected, (missing, unexpected)
            _FULL["m"] = m.cuda().train()
        m = _FULL["m"]
        for p_ in m.parameters():
            p_.grad = None
        img = synth_image(1, 512, seed=31)
        xcat, (hp, wp) = m.forward_tokens([(img.cuda(), None)], training=True)
        assert (hp, wp) == (32, 32)
        v = xcat.float().view(1, 32, 32, 4, D)
        gen = torch.Generator().manual_seed(8)
        dts, report = [], {}
        for i in range(4):
            t = v[:, :, :, i].permute(0, 3, 1, 2).cpu()
            report[f"tap{i}"] = rel_err(sl(t), G[f"full_tap{i}_slice"])
            dts.append(torch.randn(t.shape, generator=gen))
            report[f"tap{i}_stats"] = float(np.abs(stats(t)[1:3] / G[f"full_tap{i}_stats"][1:3] - 1).max())
        dx = torch.stack([d_.permute(0, 2, 3, 1) for d_ in dts], dim=3).reshape(1024, 4 * D).to(xcat.dtype).cuda()
        xcat.backward(dx)
        named = dict(m.named_parameters())
        for n in G["full_live_params"]:
            n = str(n)
            gr = named[n].grad
            assert gr is not None, n
            gr2 = gr.reshape(1, -1) if gr.dim() < 2 else gr
            report["g:" + n[6:]] = rel_err(sl(gr2), G[f"full_grad_slice::{n}"])
            report["n:" + n[6:]] = abs(gr.double().norm().item() / G[f"full_grad_norm::{n}"][0] - 1)
        for n in G["full_no_grad_params"]:
            assert named[str(n)].grad is None and not named[str(n)].requires_grad, n
        assert m.engine()._packed["rein"]["fused"] == fused
        print(f"[rein fulldepth {mode} {'fused' if fused else 'composed'}]", {k: f"{v_:.2e}" for k, v_ in report.items()})
        for k, e in report.items():
            bound = stol if k.endswith("_stats") else tol if k.startswith("tap") else gtol if k.startswith("g:") else ntol
            assert e < bound, (mode, k, e, bound)
    finally:
        os.environ.pop("VFMSEG_REIN_FUSED", None)
        set_compute_dtype("bf16")


# ---------------------------------------------------------------- train step and optimiser
def _train_model(depth=4):
    cfg = presets.rein_dinov2_linear(depth=depth)
    cfg["backbone"]["out_indices"] = [min(i, depth - 1) for i in range(4)]   # (a tap past the last block would never be written)
    cfg["decode_head"]["dropout_ratio"] = 0.0
    model = MODELS.build(cfg)
    sd = rein_model_state_dict(depth)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return model.cuda().train(), sd


@pytest.mark.parametrize("mode,ltol,gtol,ntol", [("f32", 1e-4, 2e-4, 1e-3), ("bf16x3", 1e-3, 2e-3, 1e-2), ("bf16", 1e-2, 1.2e-1, 5e-2)])
def test_rein_train_step_vs_reference_golden(golden_dir, mode, ltol, gtol, ntol):
    """EncoderDecoder(ReinsDinoVisionTransformer, LinearHead), depth 4, batch 2, 512^2, dropout 0, against the reference's modules: loss,
    acc_seg, gradients of the Rein and head parameters (f32 / bf16 bounds of test_fulldepth_gpu.py; bf16x3 = f32 x 10)."""
    G = np.load(os.path.join(golden_dir, "rein.npz"))
    set_compute_dtype(mode)
    try:
        model, _ = _train_model()
        img, lab = synth_image(2, 512, seed=33), synth_label(2, 512, seed=33)
        losses = model.forward(img.cuda(), [SegDataSample(gt_sem_seg=lab[i]) for i in range(2)], mode="loss")
        total, log = model.parse_losses(losses)
        total.backward()
        from vfmseg_amd.functional import join_wgrad_stream
        join_wgrad_stream()
        torch.cuda.synchronize()
        loss, acc = float(log["decode.loss_ce"].detach()), float(log["decode.acc_seg"].detach())
        named = dict(model.named_parameters())
        rep = {}
        for key in G.files:
            if key.startswith("train_grad_slice::"):
                n = key.split("::", 1)[1]
                gr = named[n].grad
                assert gr is not None, n
                gr2 = gr.reshape(1, -1) if gr.dim() < 2 else gr
                rep["g:" + n.split(".", 1)[1]] = rel_err(sl(gr2), G[key])
                rep["n:" + n.split(".", 1)[1]] = abs(gr.double().norm().item() / G[f"train_grad_norm::{n}"][0] - 1)
        print(f"[rein train step {mode}] loss {loss:.6f} (ref {G['train_loss_acc'][0]:.6f}) acc {acc:.4f} (ref {G['train_loss_acc'][1]:.4f})",
              {k: f"{v:.1e}" for k, v in rep.items()})
        assert abs(loss - G["train_loss_acc"][0]) <= ltol * max(1.0, abs(G["train_loss_acc"][0]))
        assert abs(acc - G["train_loss_acc"][1]) <= (1e-3 if mode != "bf16" else 0.5)
        for k, e in rep.items():
            assert e < (gtol if k.startswith("g:") else ntol), (k, e)
    finally:
        set_compute_dtype("bf16")


def test_three_optimiser_steps_move_every_rein_parameter():
    """PEFTOptimWrapperConstructor + FusedAdamW on the Rein model: after three steps every live Rein parameter (the 0-dim scale too) and the
    head's classifier have moved, the frozen base and transform / merge have not, and the loss is finite."""
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    set_compute_dtype("bf16")
    model, sd0 = _train_model(depth=2)
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    assert ow.optimizer.names[-7:] == sorted(n for n in ow.optimizer.names if ".reins." in n)
    assert [b[0] for b in ow.optimizer.bucket_slices()] == ["decode_head", "reins"]
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    for t in range(3):
        img, lab = synth_image(2, 512, seed=90 + t), synth_label(2, 512, seed=90 + t)
        log = model.train_step(dict(inputs=img.cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(2)]), ow)
        assert np.isfinite(float(log["loss"]))
    torch.cuda.synchronize()
    live = {"backbone.reins." + n for n in ("scale", "learnable_tokens_a", "learnable_tokens_b", "mlp_token2feat.weight", "mlp_token2feat.bias",
                                            "mlp_delta_f.weight", "mlp_delta_f.bias")}
    for n, p_ in model.named_parameters():
        moved = not torch.equal(p_.detach(), before[n])
        if n in live:
            assert moved, n
        elif not n.startswith("decode_head."):
            assert not moved, n
    assert not torch.equal(model.decode_head.conv_seg.weight.detach(), before["decode_head.conv_seg.weight"])
    assert model.backbone.reins.scale.dim() == 0
    # the rein-only checkpoint: adapter + head keys, nothing of the frozen base
    keys = set(model.state_dict())
    assert all(k.startswith("backbone.reins.") or k.startswith("decode_head.") for k in keys)
    # predictions read the MOVED parameters (the packed token operands T / V / scale vector are rebuilt when the optimiser's epoch moves): the
    # stepped model must predict what a freshly built model loaded with the stepped state dict predicts, and not what it predicted before
    img = synth_image(1, 512, seed=3).cuda()
    model.eval()
    with torch.no_grad():
        a = model.predict(img)[0].seg_logits.data.float()
    fresh, _ = _train_model(depth=2)
    stepped = {k: v.detach().clone() for k, v in model.state_dict().items()}
    missing, unexpected = fresh.load_state_dict(stepped, strict=False)
    assert not unexpected and all(k.startswith("backbone.") and ".reins." not in k for k in missing)
    old, _ = _train_model(depth=2)
    fresh.eval(), old.eval()
    with torch.no_grad():
        b = fresh.predict(img)[0].seg_logits.data.float()
        c = old.predict(img)[0].seg_logits.data.float()
    assert torch.isfinite(a).all()
    e_fresh, e_old = rel_err(a, b), rel_err(a, c)
    print(f"[rein stepped model] prediction vs fresh model with the stepped weights {e_fresh:.2e}, vs the un-stepped model {e_old:.2e}")
    assert e_fresh < 1e-5, e_fresh
    assert e_old > 1e-3, e_old
    # and so does the next TRAINING forward: taps of the stepped model == taps of the fresh one
    model.train(), fresh.train()
    ta, _ = model.backbone.forward_tokens([(img, None)], training=True)
    tb, _ = fresh.backbone.forward_tokens([(img, None)], training=True)
    assert rel_err(ta.float(), tb.float()) < 1e-5


def test_composed_form_covers_more_than_128_tokens():
    """token_length = 130 (operands padded to 192 columns): no fused kernel covers it, every mode takes the composed form; one adapter step
    through the engine against the float64 restatement (f32: exact-fp32 products; bf16: the format bounds of this file)."""
    m = 130
    cfg = presets.rein_dinov2_linear(depth=2)["backbone"]
    cfg["out_indices"] = [0, 1, 1, 1]
    cfg["reins_config"]["token_length"] = m
    model = MODELS.build(cfg)
    prm = rein_params(depth=2, m=m, lora=True)
    model.reins.load_state_dict(prm, strict=True)
    model = model.cuda().train()
    x, g = step_inputs(1024 + 3, D, seed=7)
    xo_ref, dx_ref, gref, _ = rein_step_f64(x.cuda(), g.cuda(), {k: v.cuda() for k, v in prm.items()}, 1)
    eng = model.engine()
    try:
        for mode, ftol, btol in (("f32", 1e-4, 2e-4), ("bf16", _fwd_tol("bf16"), _bwd_tol("bf16"))):
            set_compute_dtype(mode)
            os.environ["VFMSEG_REIN_FUSED"] = "1"    # asked for, not available at this shape
            R = eng._rein_pack(eng.packed())
            assert not R["fused"] and R["TP"] == 192
            rows = x.shape[0]
            stream, dx = x.cuda().clone(), g.cuda().clone()
            S = {}
            xn = eng._rein_forward(R, 1, stream, rows, S)
            acc = eng._rein_backward_begin(R)
            eng._rein_backward(R, acc, 1, dx, rows, S)
            grads = eng._rein_backward_end(R, acc)
            order = {id(p_): n for n, p_ in model.reins.named_parameters()}
            rep = {"xo": rel_err(xn, xo_ref), "dx": rel_err(dx, dx_ref)}
            rep.update({order[id(p_)]: rel_err(g_, gref[order[id(p_)]]) for p_, g_ in zip(model.reins.live_params(), grads)})
            print(f"[rein step m=130 {mode}]", {k: f"{v:.1e}" for k, v in rep.items()})
            assert rep["xo"] < ftol and all(v < btol for k, v in rep.items() if k != "xo"), rep
    finally:
        os.environ.pop("VFMSEG_REIN_FUSED", None)
        set_compute_dtype("bf16")


def test_shared_gradients_wait_for_the_last_backbone_backward():
    """A segmentor may send the backbone over two inputs in one step: the `reins` gradients are complete only after the backward of BOTH
    passes, so "backbone_done" (which releases their data-parallel bucket) fires once, after the last one."""
    from vfmseg_amd import backbones
    set_compute_dtype("bf16")
    model = _step_model(True)
    for p_ in model.parameters():
        p_.grad = None
    fired = []
    saved = dict(backbones.BACKWARD_EVENTS)
    backbones._PENDING_BACKWARD[0] = 0
    backbones.BACKWARD_EVENTS["backbone_done"] = lambda: fired.append(float(model.reins.scale.grad is not None))
    try:
        xa, _ = model.forward_tokens([(synth_image(1, 512, seed=1).cuda(), None)], training=True)
        xb, _ = model.forward_tokens([(synth_image(1, 512, seed=2).cuda(), None)], training=True)
        xa.float().sum().backward()
        assert fired == [], "released after the first of two backward passes"
        xb.float().sum().backward()
        assert len(fired) == 1 and backbones._PENDING_BACKWARD[0] == 0
    finally:
        backbones.BACKWARD_EVENTS.update(saved)
        backbones._PENDING_BACKWARD[0] = 0
