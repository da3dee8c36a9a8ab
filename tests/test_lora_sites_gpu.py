"""LoRA on any linear layer of a DINOv2 block on the HIP path (Lora_config.target_modules: qkv, attn.proj, fc1, fc2):
the vfm_lora_down kernel against the composed ops and float64; the toy model of tests/golden/lora_sites.npz (written by the reference's
own modules) in every precision mode; dropout against a float64 restatement fed with the masks the engine drew; the fused / composed
switch; the qkv-only model untouched; merged prediction; two data-parallel ranks; tools/train.py on the shipped config."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lora_sites_helpers as H  # noqa: E402
from tests.helpers import rel_err  # noqa: E402
from vfmseg_amd import lib as L, ops, presets  # noqa: E402
from vfmseg_amd.backbones import R_PAD  # noqa: E402
from vfmseg_amd.precision import set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
import vfmseg_amd.segmentors  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lora_sites.npz")
MODS = ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")
# half an ulp of the 16-bit output relative to the value: bf16 has 8 significant bits, fp16 11
HALF_ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}


def _backbone(targets=H.ALL, dropout=0.0):
    m = MODELS.build(H.lora_backbone_cfg(targets, dropout=dropout))
    missing, unexpected = m.load_state_dict(H.lora_state_dict(targets))
    assert not missing and not unexpected
    return m.cuda().train()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("K", [1024, 4096])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_lora_down_kernel(mode, K):
    """vfm_lora_down in both libraries at M in {1, 86, 130} (one partial row tile, three tiles with a partial last, five), r in {4, 64},
    p in {0, 0.1}, x a column slice of a padded [M, K + 64 + 8] buffer.  mask and xd: bit-equal to vfm_dropout_mask / vfm_mul_mask.
    T against float64 of s * xd A^T on the STORED xd, per element within
        half an ulp of the output type * |T|  +  K * 2^-23 * s * sum_k |xd_k a_k|      (fp32 accumulation of K exact products, any order)
    with |T| the float64 value; where |T| < 2^-14 in fp16 the half ulp is the subnormal step's, 2^-25, whatever |T|."""
    set_compute_dtype(mode)
    try:
        dt = L.half_dtype()
        s, seed, off = 4.0, 77, 12345
        gen = torch.Generator().manual_seed(K)
        for M in (1, 86, 130):
            buf = torch.full((M, K + R_PAD + 8), float("nan"), dtype=dt).cuda()
            x = buf[:, :K]
            x.copy_(torch.randn(M, K, generator=gen).to(dt))
            x0 = x.clone()
            for r in (4, 64):
                a = torch.zeros(R_PAD, K, dtype=dt)
                a[:r] = (0.05 * torch.randn(r, K, generator=gen)).to(dt)
                a = a.cuda()
                for p in (0.0, 0.1):
                    T = buf[:, K:K + R_PAD]
                    T.fill_(float("nan"))
                    mask = torch.full((M, K), 3.0, dtype=dt).cuda() if p > 0 else None
                    xd = torch.full((M, K), 3.0, dtype=dt).cuda() if p > 0 else None
                    ops.lora_down(x, a, T, s, p, seed, off, mask, xd)
                    if p > 0:
                        mask_c, xd_c = torch.empty(M, K, dtype=dt).cuda(), torch.empty(M, K, dtype=dt).cuda()
                        ops.dropout_mask(mask_c, p, seed, offset=off)
                        ops.mul_mask(x, mask_c, xd_c)
                        assert torch.equal(mask.view(torch.int16), mask_c.view(torch.int16)), (M, r, "mask")
                        assert torch.equal(xd.view(torch.int16), xd_c.view(torch.int16)), (M, r, "xd")
                        keep = (mask != 0).float().mean().item()
                        assert M * K < 1e4 or abs(keep - 0.9) < 0.02, keep
                    assert torch.equal(x.view(torch.int16), x0.view(torch.int16)) and torch.isnan(buf[:, K + R_PAD:]).all()   # nothing else written
                    src = (xd if p > 0 else x).double().cpu()
                    ad = a.double().cpu()
                    ref = s * src @ ad.t()
                    acc = K * 2.0 ** -23 * s * (src.abs() @ ad.abs().t())
                    half = HALF_ULP[mode] * ref.abs()
                    if mode == "fp16":
                        half = torch.where(ref.abs() < 2.0 ** -14, torch.full_like(half, 2.0 ** -25), half)
                    bound = half + acc
                    got = T.double().cpu()
                    assert torch.isfinite(got).all(), (M, r, p)            # all R_PAD columns of every row are written
                    assert (got[:, r:] == 0).all()                         # (zero rows of A)
                    err = (got - ref).abs()
                    worst = (err / bound.clamp_min(1e-300))[:, :r].max().item()
                    print(f"[lora_down {mode} K={K} M={M} r={r} p={p}] max err / bound {worst:.3f}, max |T| {ref.abs().max():.3f}")
                    assert (err <= bound).all(), (M, r, p, worst)
    finally:
        set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------------ the reference's fixture
# tolerances: tests/test_backbone_gpu.py::test_backbone_taps_and_lora_grads (f32 2e-4 / 2e-3, bf16 3e-2 / 8e-2); fp16 is held to the bf16
# bounds (the qkv test has no fp16 case; fp16 carries three more bits), bf16x3 (taps only) to the f32 tap bound times ten as everywhere
@pytest.mark.parametrize("mode,tol,gtol", [("f32", 2e-4, 2e-3), ("bf16", 3e-2, 8e-2), ("fp16", 3e-2, 8e-2), ("bf16x3", 2e-3, None)])
def test_fixture_parity(mode, tol, gtol):
    G = np.load(GOLD)
    set_compute_dtype(mode)
    try:
        m = _backbone()
        xcat, (hp, wp) = m.forward_tokens([(H.toy_image().cuda(), None)])
        assert (hp, wp) == (H.HP, H.WP) and xcat.shape == (2 * H.HP * H.WP, len(H.OUT) * H.DIM)
        for i, t in enumerate(H.taps_of(xcat)):
            amax = G[f"tap{i}_stats"][3]
            e1 = np.abs(t[:8, :8, :8, :8].numpy() - G[f"tap{i}_slice"]).max() / amax
            e2 = np.abs(t[1, -5:, -3:, -4:].numpy() - G[f"tap{i}_tail"]).max() / amax
            e3 = np.abs(H.tap_grid(t).numpy() - G[f"tap{i}_grid"]).max() / amax       # (every 32nd channel at every position)
            print(f"[fixture {mode}] tap{i} slice {e1:.2e} tail {e2:.2e} grid {e3:.2e} (tol {tol})")
            assert e1 < tol and e2 < tol and e3 < tol, (i, e1, e2, e3)
            st = np.array([t.mean().item(), t.abs().mean().item(), t.std().item(), t.abs().max().item()])
            assert np.abs(st - G[f"tap{i}_stats"]).max() < tol * amax, (i, st, G[f"tap{i}_stats"])
        if gtol is None:
            return
        xcat.backward(H.dxcat_of(H.tap_grads()).to(xcat.dtype).cuda())
        n = 0
        for name, p in m.named_parameters():
            if "lora_" not in name:
                assert p.grad is None
                continue
            g = p.grad.double().cpu()
            gmax = G[f"grad_stats::{name}"][3]
            e1 = np.abs(g[:8, :8].numpy() - G[f"grad_slice::{name}"]).max() / gmax
            e2 = np.abs(g[-3:, -6:].numpy() - G[f"grad_tail::{name}"]).max() / gmax
            e3 = abs(g.norm().item() - G[f"grad_norm::{name}"][0]) / G[f"grad_norm::{name}"][0]
            e4 = np.abs(H.grad_grid(g).numpy() - G[f"grad_grid::{name}"]).max() / gmax     # (rows / columns spread over the whole factor)
            print(f"[fixture {mode}] {name} slice {e1:.2e} tail {e2:.2e} norm {e3:.2e} grid {e4:.2e} (tol {gtol})")
            assert e1 < gtol and e2 < gtol and e3 < gtol and e4 < gtol, (name, e1, e2, e3, e4)
            n += 1
        assert n == 2 * 4 * H.DEPTH
    finally:
        set_compute_dtype("bf16")


def test_two_jobs_with_a_crop_box_in_one_call():
    """What MsVFMEncoderDecoder / HRDAEncoderDecoder ask of the backbone: several jobs in ONE call, one of them a crop box of a larger image
    (three images' tokens in one row space).  f32, all four sites, taps and every factor gradient against float64 (bounds of the fixture test)."""
    from vfmseg_amd.synth import synth_image
    set_compute_dtype("f32")
    try:
        m = _backbone()
        big, box = synth_image(1, (128, 160), seed=62), (16, 16 + H.IMG_H, 32, 32 + H.IMG_W)
        xcat, (hp, wp) = m.forward_tokens([(H.toy_image().cuda(), None), (big.cuda(), box)])
        assert (hp, wp) == (H.HP, H.WP) and xcat.shape == (3 * H.HP * H.WP, len(H.OUT) * H.DIM)
        dts = [torch.randn(3, H.DIM, H.HP, H.WP, generator=torch.Generator().manual_seed(23 + i)) for i in H.OUT]
        xcat.backward(torch.stack([d.permute(0, 2, 3, 1) for d in dts], dim=3).reshape(xcat.shape).cuda())
        sd = H.lora_state_dict()
        tk = [k for k in sd if "lora_" in k]
        for k in tk:
            sd[k] = sd[k].double().requires_grad_(True)
        taps = H.forward_f64(sd, torch.cat([H.toy_image(), big[:, :, box[0]:box[1], box[2]:box[3]]]))
        og = dict(zip(tk, torch.autograd.grad(sum((t * d.double()).sum() for t, d in zip(taps, dts)), [sd[k] for k in tk])))
        v = xcat.detach().double().cpu().view(3, H.HP, H.WP, len(H.OUT), H.DIM)
        for i, ref in enumerate(taps):
            e = rel_err(v[:, :, :, i].permute(0, 3, 1, 2), ref.detach())
            assert e < 2e-4, (i, e)
        for n, p in m.named_parameters():
            if "lora_" in n:
                e = rel_err(p.grad.cpu(), og[n])
                assert e < 2e-3, (n, e)
    finally:
        set_compute_dtype("bf16")


# ------------------------------------------------------------------------------------------------ dropout
def _masks(xcat):
    """{(layer, module): engine mask [M, in]} of the forward that produced xcat (read before backward frees them)"""
    out = {}
    for li, S in enumerate(xcat.grad_fn.c["saved"]):
        out[(li, "attn.qkv")] = S["mask"]
        for k, mod in (("proj", "attn.proj"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            out[(li, mod)] = S["lora"][k][1]
    assert all(v is not None for v in out.values())
    return out


def _step(m, seed, backward=True):
    for p in m.parameters():
        p.grad = None
    xcat, _ = m.forward_tokens([(H.toy_image().cuda(), None)], seed=seed)
    masks = {k: v.clone() for k, v in _masks(xcat).items()}
    if backward:
        xcat.backward(H.dxcat_of(H.tap_grads()).to(xcat.dtype).cuda())
    return xcat.detach(), masks, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def test_dropout_against_float64_with_the_engines_masks():
    """p = 0.1, bf16: every site's multiplier is read back and fed to the float64 restatement (peft's lora.Linear on all four linears):
    taps and factor gradients within the bf16 bounds of the qkv site; the sites draw from disjoint counter streams (different masks, each
    keeping ~90 %), two steps draw different masks, a pinned seed repeats them."""
    set_compute_dtype("bf16")
    m = _backbone(dropout=0.1)
    xcat, masks, grads = _step(m, seed=1234)
    D = H.DIM
    for li in range(H.DEPTH):
        same = [masks[(li, mod)][:, :D] for mod in MODS]
        for a in range(4):
            keep = (masks[(li, MODS[a])] != 0).float().mean().item()
            assert abs(keep - 0.9) < 0.01, (li, MODS[a], keep)
            for b in range(a + 1, 4):
                assert not torch.equal(same[a], same[b]), (li, MODS[a], MODS[b])
        if li:
            for mod in MODS:
                assert not torch.equal(masks[(li, mod)], masks[(0, mod)]), mod
    sd = H.lora_state_dict()
    tk = [k for k in sd if "lora_" in k]
    for k in tk:
        sd[k] = sd[k].double().requires_grad_(True)
    mk = {k: H.token_mask_to_bnc(v, v.shape[1]) for k, v in masks.items()}
    taps = H.forward_f64(sd, H.toy_image(), mk)
    og = dict(zip(tk, torch.autograd.grad(sum((t * d.double()).sum() for t, d in zip(taps, H.tap_grads())), [sd[k] for k in tk])))
    te = [rel_err(got, ref.detach()) for got, ref in zip(H.taps_of(xcat), taps)]
    ge = {n: rel_err(g.cpu(), og[n]) for n, g in grads.items()}
    print("[dropout bf16] taps", ["%.2e" % e for e in te], "gradients", {n.split("blocks.")[1]: "%.2e" % e for n, e in ge.items()})
    assert len(grads) == len(tk)
    assert all(e < 3e-2 for e in te), te
    assert all(e < 8e-2 for e in ge.values()), ge
    # the training path (seed=None) draws fresh counters every call; an explicit seed pins them
    _, m1, _ = _step(m, None, backward=False)
    _, m2, _ = _step(m, None, backward=False)
    _, m3, _ = _step(m, 1234, backward=False)
    for k in masks:
        assert not torch.equal(m1[k], m2[k]), k
        assert torch.equal(m3[k], masks[k]), k


def test_fused_and_composed_forms_agree(monkeypatch):
    """VFMSEG_LORA_FUSED=1 (vfm_lora_down) against =0 (dropout_mask + mul_mask + gemm): the same masks bit for bit, taps and gradients
    within the bf16 bounds (T's rounding differs: s is applied before or after the 16-bit store's rounding of the same fp32 sum)."""
    set_compute_dtype("bf16")
    m = _backbone(dropout=0.1)
    monkeypatch.setenv("VFMSEG_LORA_FUSED", "1")
    x1, k1, g1 = _step(m, seed=99)
    monkeypatch.setenv("VFMSEG_LORA_FUSED", "0")
    x0, k0, g0 = _step(m, seed=99)
    for k in k1:
        assert torch.equal(k1[k].view(torch.int16), k0[k].view(torch.int16)), k
    assert rel_err(x1.float(), x0.float()) < 3e-2
    for n in g1:
        assert rel_err(g1[n], g0[n]) < 8e-2, n


def test_qkv_only_model_is_untouched_by_the_switch(monkeypatch):
    """A qkv-only model never reaches vfm_lora_down: taps and gradients are bit-identical under VFMSEG_LORA_FUSED=0 and =1, and with the
    optimiser's flat gradient buffer the step still runs as the launch plan."""
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    set_compute_dtype("bf16")
    cfg = presets.dinov2_linear(depth=H.DEPTH)
    cfg["backbone"]["backbone"]["out_indices"] = list(H.OUT)
    model = MODELS.build(cfg)
    model.backbone.load_state_dict(H.lora_state_dict(["qkv"], r=32))
    model = model.cuda().train()
    opt = PEFTOptimWrapperConstructor(presets.optim_cfg()["optim_wrapper"])(model, None).optimizer
    eng = model.backbone.vit.engine()
    assert eng.sites() == ("qkv",)
    img = H.toy_image().cuda()
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("VFMSEG_LORA_FUSED", flag)
        opt.gflat.zero_()
        xcat, _ = model.backbone.forward_tokens([(img, None)], seed=5)
        assert xcat.grad_fn.c.get("plan") is not None, "the qkv-only train step must take the launch plan"
        xcat.backward(H.dxcat_of(H.tap_grads()).to(xcat.dtype).cuda())
        res[flag] = (xcat.detach().clone(), opt.gflat.clone())
    assert torch.equal(res["1"][0], res["0"][0])
    assert res["1"][1].abs().max() > 0 and torch.equal(res["1"][1], res["0"][1])


# ------------------------------------------------------------------------------------------------ prediction
def test_merged_prediction_and_rebuild_after_a_step(monkeypatch):
    """Prediction folds every site's pair into its weight (W + s B A, cached per site): equal to the unmerged path within the bf16 bound,
    rebuilt after an optimiser step (the fused AdamW kernel rewrites the factors behind torch's version counters)."""
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label
    set_compute_dtype("bf16")
    cfg = presets.dinov2_linear(depth=H.DEPTH)
    cfg["backbone"]["backbone"]["out_indices"] = [0, 1, 1, 1]     # (the LinearHead takes four taps)
    cfg["backbone"]["Lora_config"] = presets.lora_cfg(r=H.RANK, alpha=H.ALPHA, target_modules=presets.ALL_LINEAR)
    model = MODELS.build(cfg)
    model.backbone.load_state_dict(H.lora_state_dict())
    model = model.cuda()
    img = synth_image(1, 512, seed=11).cuda()

    def feats(merge):
        monkeypatch.setenv("VFMSEG_MERGE_LORA_EVAL", "1" if merge else "0")
        model.eval()
        with torch.no_grad():
            return torch.cat([f.float().flatten() for f in model.backbone(img)])

    a1, a0 = feats(True), feats(False)
    P = model.backbone.vit.engine().packed()
    assert sorted(P["merged"]) == ["fc1", "fc2", "proj", "qkv"] and all(len(v) == H.DEPTH for v in P["merged"].values())
    print(f"[merged bf16] merged vs unmerged taps {rel_err(a1, a0):.2e}")
    assert rel_err(a1, a0) < 3e-2
    oc = presets.optim_cfg()
    oc["optim_wrapper"]["optimizer"]["lr"] = 5e-3   # a visible parameter change in one step (AdamW's first step moves every factor by ~lr: a quarter of the factors' std 0.02, at scaling 4 on four sites)
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, None)
    lab = synth_label(1, 512, seed=11).cuda()
    model.train()
    model.train_step(dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[0])]), ow)
    b1, b0 = feats(True), feats(False)
    print(f"[merged bf16] after the step: merged vs unmerged {rel_err(b1, b0):.2e}, unmerged vs before {rel_err(b0, a0):.2e}")
    assert not torch.equal(b1, a1), "the merged weights were not rebuilt"
    assert rel_err(b1, b0) < 3e-2, "stale merged weights after an optimiser step"
    assert rel_err(b0, a0) > 5 * rel_err(b1, b0), "the step should have changed the taps visibly"


# ------------------------------------------------------------------------------------------------ data parallel, entry point
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_dp(world, out):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", VFMSEG_DIST_SINGLE="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lora_sites_dp_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return torch.load(out, weights_only=False)


@pytest.mark.timeout(900)
def test_two_ranks_equal_one_rank_with_the_global_batch(tmp_path):
    """f32, all four sites: 2 ranks x B=1 (gloo) give the losses and post-step parameters of 1 process x B=2 (bounds of
    tests/test_dp_equivalence_gpu.py), and the LoRA buckets leave from inside the backbone backward, after the heads'."""
    one, two = _run_dp(1, str(tmp_path / "w1.pt")), _run_dp(2, str(tmp_path / "w2.pt"))
    assert torch.allclose(one["logs"], two["logs"], rtol=1e-5, atol=1e-6), (one["logs"], two["logs"])
    n = 0
    for k, a in one["state"].items():
        if "running_" in k or "num_batches" in k or k == "decode_head.output_upscaling.0.bias":   # (a bias before BatchNorm: exact gradient 0)
            continue
        d = (a - two["state"][k]).abs().mean().item() / max(a.abs().mean().item(), 1e-12)
        assert d < 2e-5, (k, d)
        n += "lora_" in k
    assert n == 2 * 4 * H.DEPTH
    per_step = two["events"][:len(two["events"]) // 2]
    assert per_step[0] == "decode_head" and len(per_step) > 1 and all(e.startswith("lora") for e in per_step[1:]), two["events"]


@pytest.mark.timeout(900)
def test_train_py_on_the_all_linear_config_with_amp_and_resume(tmp_path):
    """tools/train.py on configs/dg_lora_dinov2_linearhead_all_linear.py (depth cut to 2 from the command line): two steps with --amp, then
    --resume to the third; the checkpoints carry all four sites' factors under peft's key names, and the factors moved."""
    wd = tmp_path / "wd"
    base = [sys.executable, "tools/train.py", "configs/dg_lora_dinov2_linearhead_all_linear.py", "--amp", "--data", "synthetic", "--work-dir", str(wd),
            "--cfg-options", "model.backbone.backbone.depth=2", "model.backbone.backbone.out_indices=[0,1,1,1]", "train_dataloader.batch_size=1",
            "default_hooks.logger.interval=1", "default_hooks.checkpoint.interval=1"]
    r = subprocess.run(base + ["--max-iters", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "precision mode fp16" in r.stdout
    r = subprocess.run(base + ["--max-iters", "3", "--resume"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    c2 = torch.load(wd / "iter_2.pth", map_location="cpu", weights_only=False)
    c3 = torch.load(wd / "iter_3.pth", map_location="cpu", weights_only=False)
    assert c3["optim_wrapper"]["iter"] == 3
    for mod in MODS:
        for ab in ("lora_A", "lora_B"):
            k = f"backbone.model.base_model.model.blocks.1.{mod}.{ab}.default.weight"
            assert torch.isfinite(c3["state_dict"][k]).all() and not torch.equal(c2["state_dict"][k], c3["state_dict"][k]), k
