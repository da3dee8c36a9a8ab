"""Full fine-tuning of the DINOv2 backbone on the GPU: the two kernels of csrc/fullft.hip against float64, the backbone gradients of the
small model (tests/fullft_helpers.py) against autograd over the float64 oracle, train steps, the stale-pack guard, determinism, resume,
data parallelism, and what is refused.

Error bounds.  f32: the bounds tests/test_rein_gpu.py uses for exact-fp32 products - 1e-4 on forward values, 2e-4 on gradients.  16-bit
modes: the bounds come from the number formats (eps = half an ulp: bf16 2^-9, fp16 2^-12), by the count of 16-bit roundings on the path of
the worst tensor, as in tests/test_rein_gpu.py:5-8; attention scores are of order 0.5 here, so the softmax does not amplify.
  forward (a tap after block 1): patch rows and patch-embedding weight (2); per block LN1 output, W_qkv, qkv, the probabilities, the
    attention output, W_proj, LN2 output, W_fc1, gelu output, W_fc2 (10 x 2 blocks); the tap's own cast (1): 23 eps.
  gradients (worst: patch_embed.proj.weight, which every rounding precedes): those 23, the incoming tap gradient (1); per block
    t = cd(dx g2), W_fc2^T, the saved gelu', dh, W_fc1^T, dn, t = cd(dx g1), W_proj^T, dao, dP and dS inside the attention backward, dqkv,
    W_qkv^T, da1 (14 x 2 blocks); the patch-token gradient (1): 53 eps.
All comparisons are max-norm relative (tests/helpers.rel_err)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests.fullft_helpers import (BB, DIM, IMG, OUT_IDX, batch, build_small, inert_backbone_keys, oracle_backbone_grads,  # noqa: E402
                                  oracle_train_steps, small_cfg, small_state_dict, trained_backbone_keys)
from tests.helpers import rel_err  # noqa: E402
from vfmseg_amd import ops, presets  # noqa: E402
from vfmseg_amd.backbones import Packed  # noqa: E402
from vfmseg_amd.optim import PEFTOptimWrapperConstructor  # noqa: E402
from vfmseg_amd.precision import compute_dtype, set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.segmentors import SegDataSample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}
FWD_TOL = {"f32": 1e-4, "bf16": 23 * EPS["bf16"], "fp16": 23 * EPS["fp16"]}
BWD_TOL = {"f32": 2e-4, "bf16": 53 * EPS["bf16"], "fp16": 53 * EPS["fp16"]}


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        set_compute_dtype(self.mode)
        return compute_dtype()

    def __exit__(self, *a):
        set_compute_dtype("bf16")


def _data(bs=2, seed=0):
    img, lab = batch(bs, seed)
    return dict(inputs=img.cuda(), data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(bs)])


def _optim(model, backbone_lr_mult=None, end=40000, amp=False):
    oc = presets.optim_cfg(backbone_lr_mult=backbone_lr_mult)
    ow_cfg = dict(oc["optim_wrapper"])
    if amp:
        ow_cfg["type"] = "AmpOptimWrapper"
    return PEFTOptimWrapperConstructor(ow_cfg)(model, [dict(oc["param_scheduler"][0], end=end)])


# ------------------------------------------------------------------------------------------------ 6. vfm_branch_param_grads
@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_branch_param_grads_vs_float64(mode):
    """d gamma = sum_m dx u, d bias = gamma sum_m dx to 1e-6 (max-norm relative: fp32 partial sums met pairwise, the blocks' rows in
    double), accumulate on and off, with and without t; gamma holds a zero, a negative and a 1e-5 entry; t is bit-identical to
    ops.cast(dx, t, gamma); two runs are bit-identical."""
    with _mode(mode) as cd:
        g = torch.Generator(device="cuda").manual_seed(5)
        worst = 0.0
        for M in (1, 34, 130, 2050):
            for D in (64, 256, 1024):
                dx = torch.randn(M, D, generator=g, device="cuda")
                u = torch.randn(M, D, generator=g, device="cuda").to(cd)
                gamma = torch.randn(D, generator=g, device="cuda")
                gamma[0], gamma[1], gamma[2] = 0.0, -0.7, 1e-5
                ref_dg = (dx.double() * u.double()).sum(0)
                ref_db = gamma.double() * dx.double().sum(0)
                t_ref = ops.cast(dx, torch.empty(M, D, dtype=cd, device="cuda"), gamma)
                for accumulate in (False, True):
                    for want_t in (False, True):
                        base = torch.randn(2, D, generator=g, device="cuda")
                        dg, db = base[0].clone(), base[1].clone()
                        t = torch.full((M, D), 3.0, dtype=cd, device="cuda") if want_t else None
                        ops.branch_param_grads(dx, u, gamma, dgamma=dg, dbias=db, t=t, accumulate=accumulate)
                        rg = ref_dg + (base[0].double() if accumulate else 0)
                        rb = ref_db + (base[1].double() if accumulate else 0)
                        e1, e2 = rel_err(dg, rg), rel_err(db, rb)
                        worst = max(worst, e1, e2)
                        assert e1 < 1e-6 and e2 < 1e-6, (M, D, accumulate, want_t, e1, e2)
                        assert db[0].item() == (base[1, 0].item() if accumulate else 0.0)     # gamma = 0: exactly no bias gradient
                        if want_t:
                            assert torch.equal(t, t_ref), (M, D)
                        dg2, db2 = base[0].clone(), base[1].clone()
                        t2 = torch.empty(M, D, dtype=cd, device="cuda") if want_t else None
                        ops.branch_param_grads(dx, u, gamma, dgamma=dg2, dbias=db2, t=t2, accumulate=accumulate)
                        assert torch.equal(dg, dg2) and torch.equal(db, db2) and (not want_t or torch.equal(t, t2))
                # only the dgrad operand / only one of the sums
                t = torch.empty(M, D, dtype=cd, device="cuda")
                ops.branch_param_grads(dx, None, gamma, t=t)
                assert torch.equal(t, t_ref)
                db = torch.zeros(D, device="cuda")
                ops.branch_param_grads(dx, None, gamma, dbias=db)
                assert rel_err(db, ref_db) < 1e-6
        print(f"[branch_param_grads {mode}] worst max-norm relative error of d gamma / d bias {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 7. pack refresh
SHAPES = [(64, 64), (192, 64), (768, 256), (1024, 768)]


def _whole(t):
    return t._base if t._base is not None else t


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_pack_refresh_is_bit_identical_to_fresh_packs(mode):
    """One vfm_pack_weights launch over a table of all four sites rewrites Packed.w (padded leading dimension) and Packed.wt from the moved
    fp32 master: the same bits as Packed(...) built afresh, pad columns included (they stay zero)."""
    with _mode(mode) as cd:
        g = torch.Generator(device="cuda").manual_seed(9)
        masters = [torch.randn(n, k, generator=g, device="cuda") for n, k in SHAPES]
        packs = [Packed(m, cd) for m in masters]
        table = ops.PackTable([(m, p.w, p.wt) for m, p in zip(masters, packs)])
        for m in masters:
            m.mul_(1.37).add_(0.011)
        assert not torch.equal(packs[0].w, Packed(masters[0], cd).w)
        table.run()
        for (n, k), m, p in zip(SHAPES, masters, packs):
            fresh = Packed(m, cd)
            assert torch.equal(p.w, fresh.w) and torch.equal(_whole(p.w), _whole(fresh.w)), (n, k)
            assert p.wt is not None and torch.equal(p.wt, fresh.wt) and torch.equal(_whole(p.wt), _whole(fresh.wt)), (n, k)
        # an image without a transpose, and an odd shape that takes the elementwise stores
        m = torch.randn(37, 50, generator=g, device="cuda")
        w = torch.zeros(37, 56, dtype=cd, device="cuda")[:, :50]
        wt = torch.zeros(50, 40, dtype=cd, device="cuda")[:, :37]
        ops.PackTable([(m, w, wt), (masters[0], torch.zeros(64, 64, dtype=cd, device="cuda"), None)]).run()
        assert torch.equal(w, m.to(cd)) and torch.equal(wt, m.t().to(cd))
        assert _whole(w)[:, 50:].abs().max().item() == 0 and _whole(wt)[:, 37:].abs().max().item() == 0


def test_f32_operands_alias_the_master():
    """f32 mode: the operand the GEMMs read IS the optimiser's master, for every trained 2-D weight and every fp32 vector."""
    with _mode("f32"):
        model = build_small().cuda().train()
        ow = _optim(model)
        model.train_step(_data(), ow)
        P = model.backbone.engine().packed()
        flat = ow.optimizer.flat
        lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
        blk = model.backbone.blocks[1]
        for pk, p in ((P["layers"][1]["qkv"], blk.attn.qkv.weight), (P["layers"][1]["fc2"], blk.mlp.fc2.weight), (P["pe"], model.backbone.patch_embed.proj.weight)):
            assert pk.w.data_ptr() == p.data_ptr() and lo <= pk.w.data_ptr() < hi and pk.wt is None
        for vec, p in ((P["layers"][0]["g1"], model.backbone.blocks[0].ls1.gamma), (P["layers"][0]["n2b"], model.backbone.blocks[0].norm2.bias),
                       (P["cls"], model.backbone.cls_token)):
            assert vec.data_ptr() == p.data_ptr() and lo <= vec.data_ptr() < hi


# ------------------------------------------------------------------------------------------------ 8. backbone gradients
@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_backbone_gradients_vs_float64_oracle(mode):
    """Every trained backbone tensor's gradient of loss = sum(taps * R) (a fixed random R) against autograd over the float64 oracle, in the
    three modes, at the bounds of the module docstring.  Measured values: DESIGN.md section 4.10."""
    ref_taps, ref_g, Rw = oracle_backbone_grads()
    with _mode(mode):
        model = build_small().cuda().train()
        vit = model.backbone
        img, _ = batch(2, 0)
        xcat, grid = vit.forward_tokens([(img.cuda(), None)], training=True)
        assert tuple(grid) == (IMG // 16, IMG // 16) and xcat.shape == (2 * 16, len(OUT_IDX) * DIM)
        e_f = rel_err(xcat.float(), ref_taps)
        (xcat.float() * Rw.float().cuda()).sum().backward()
        named = dict(model.named_parameters())
        errs = {}
        for k, g in ref_g.items():
            assert named[k].grad is not None, k
            errs[k] = rel_err(named[k].grad, g)
        for k in inert_backbone_keys(model.state_dict()):
            assert named[k].grad is None, k
        worst = max(errs, key=errs.get)
        by_kind = {}
        for k, v in errs.items():
            kind = k.split("blocks.")[1].split(".", 1)[1] if "blocks." in k else k[len(BB):]
            by_kind[kind] = max(by_kind.get(kind, 0.0), v)
        print(f"[full gradients {mode}] taps rel err {e_f:.2e} (bound {FWD_TOL[mode]:.2e}); worst gradient {worst} {errs[worst]:.2e} "
              f"(bound {BWD_TOL[mode]:.2e}); per tensor kind " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(by_kind.items())))
        assert e_f < FWD_TOL[mode]
        assert len(errs) == 4 + 14 * 2
        for k, v in errs.items():
            assert v < BWD_TOL[mode], (k, v)


# ------------------------------------------------------------------------------------------------ 9. fails without the feature
@pytest.mark.parametrize("head", ["linear", "segformer"])
def test_one_train_step_moves_every_trained_backbone_tensor(head):
    """One train_step of EncoderDecoder(DinoVisionTransformer, head) on the small model: every trained backbone tensor receives a gradient and
    changes, norm.* / mask_token stay bit-identical; the same step on FrozenBackboneEncoderDecoder leaves the whole backbone bit-identical.
    Before full fine-tuning existed the first half failed: the backbone got no gradient at all (zero rows in the flat buffer: its LayerNorm
    weights, which are not decayed, stood still) while norm.* / mask_token sat in the optimiser and were weight-decayed."""
    set_compute_dtype("bf16")
    sd0 = small_state_dict(head)
    model = build_small(head, sd=sd0).cuda().train()
    ow = _optim(model)
    opt = ow.optimizer
    d = _data()
    total, _ = model.parse_losses(model.forward(d["inputs"], d["data_samples"], mode="loss"))
    total.backward()
    from vfmseg_amd.functional import join_wgrad_stream
    join_wgrad_stream()
    named = dict(model.named_parameters())
    for k in trained_backbone_keys(sd0):
        assert k in opt.names and named[k].grad.abs().max().item() > 0, k
    for k in inert_backbone_keys(sd0):
        assert k not in opt.names
    opt.zero_grad()
    log = model.train_step(_data(), ow)
    assert torch.isfinite(log["loss"])
    got = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    for k in trained_backbone_keys(sd0):
        assert not torch.equal(got[k], sd0[k]), k
    for k in inert_backbone_keys(sd0):
        assert torch.equal(got[k], sd0[k]), k
    frozen = build_small(head, "frozen", sd=sd0).cuda().train()
    owf = _optim(frozen)
    assert not any(n.startswith(BB) for n in owf.optimizer.names)
    frozen.train_step(_data(), owf)
    gotf = {k: v.detach().float().cpu() for k, v in frozen.state_dict().items()}
    for k in sd0:
        if k.startswith(BB):
            assert torch.equal(gotf[k], sd0[k]), k
    assert not torch.equal(gotf["decode_head.conv_seg.weight"], sd0["decode_head.conv_seg.weight"])


# ------------------------------------------------------------------------------------------------ 10. three optimiser steps
def test_three_train_steps_match_oracle_f32():
    """Three iterations in f32 against autograd + oracle.torch_ref.adamw_step with the full config's groups (backbone lr_mult 0.1, no decay
    on norms), a steep PolyLR: losses and the update of a fixed sample of parameters within the f32 bounds of
    tests/test_fulldepth_gpu.py::test_three_train_steps_match_oracle (loss 3e-4, bulk update error 2e-3, cosine 0.9999).
    The oracle's step applies the weight decay and stores the parameter in fp32, as torch's AdamW does on an fp32 parameter (the reasoning and
    the figures are in tests/fullft_helpers.oracle_train_steps: against an all-float64 step ls1 / ls2.gamma measured 2.2e-3 / 2.6e-3, every
    fp32 AdamW's own distance from float64 at lr_mult 0.1; with it the sampled tensors measure 0 to 2.8e-5)."""
    oc = presets.optim_cfg(backbone_lr_mult=0.1)
    ref_losses, sdo = oracle_train_steps(3, oc["optim_wrapper"], end=10)
    with _mode("f32"):
        sd0 = small_state_dict()
        model = build_small(sd=sd0).cuda().train()
        ow = _optim(model, backbone_lr_mult=0.1, end=10)
        for t in range(3):
            log = model.train_step(_data(seed=40 + t), ow)
            assert abs(float(log["decode.loss_ce"]) - ref_losses[t]) <= 3e-4 * max(1.0, abs(ref_losses[t])), (t, float(log["decode.loss_ce"]), ref_losses[t])
        got = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
        probes = ["backbone.patch_embed.proj.weight", "backbone.patch_embed.proj.bias", "backbone.cls_token", "backbone.pos_embed",
                  "backbone.blocks.0.norm1.weight", "backbone.blocks.0.attn.qkv.weight", "backbone.blocks.0.attn.qkv.bias",
                  "backbone.blocks.0.attn.proj.weight", "backbone.blocks.0.ls1.gamma", "backbone.blocks.1.norm2.bias",
                  "backbone.blocks.1.mlp.fc1.weight", "backbone.blocks.1.mlp.fc1.bias", "backbone.blocks.1.mlp.fc2.weight",
                  "backbone.blocks.1.mlp.fc2.bias", "backbone.blocks.1.ls2.gamma", "decode_head.conv_seg.weight",
                  "decode_head.fusion_conv.gn.weight"]
        bulks, coss = {}, {}
        for k in probes:
            du, dr = (got[k] - sd0[k]).double().flatten(), (sdo[k].double() - sd0[k].double()).flatten()
            if k.endswith("attn.qkv.bias"):
                # the K third of the qkv bias has an identically zero gradient (a constant added to every key shifts all scores of a row
                # alike and the softmax does not see it): what either side holds there is rounding noise, which Adam normalises to +-lr.
                # The Q and V thirds are probed.
                keep = torch.cat([torch.arange(0, DIM), torch.arange(2 * DIM, 3 * DIM)])
                du, dr = du[keep], dr[keep]
            assert dr.abs().max() > 0, k
            bulks[k] = ((du - dr).abs().mean() / dr.abs().mean()).item()
            coss[k] = (du @ dr / (du.norm() * dr.norm()).clamp_min(1e-300)).item()
        print("[full 3 train steps f32] update bulk err", {k[len(BB):] if k.startswith(BB) else k: f"{v:.1e}" for k, v in bulks.items()})
        for k in probes:
            assert bulks[k] < 2e-3, (k, bulks[k])
            assert coss[k] > 0.9999, (k, coss[k])
        for k in inert_backbone_keys(sd0):
            assert torch.equal(got[k], sd0[k]), k


# ------------------------------------------------------------------------------------------------ 11. stale packs
@pytest.mark.parametrize("mode", ["bf16", "f32", "fp16"])
def test_predict_after_a_step_equals_a_fresh_model(mode):
    """After optimiser steps the packed operands follow the master: `predict` equals, bit for bit, the prediction of a freshly built model
    loaded from the stepped model's state_dict()."""
    with _mode(mode):
        model = build_small().cuda().train()
        img = batch(2, 3)[0].cuda()
        model.eval()
        before = model.predict(img)[0].seg_logits.data.clone()     # (packs the weights before the optimiser re-points them)
        model.train()
        ow = _optim(model)
        for t in range(2):
            model.train_step(_data(seed=10 + t), ow)
        model.eval()
        out = model.predict(img)
        fresh = build_small(sd={k: v.detach().cpu() for k, v in model.state_dict().items()}).cuda().eval()
        ref = fresh.predict(img)
        assert not torch.equal(out[0].seg_logits.data, before)
        for a, b in zip(out, ref):
            assert torch.equal(a.seg_logits.data, b.seg_logits.data)
            assert torch.equal(a.pred_sem_seg.data, b.pred_sem_seg.data)


# ------------------------------------------------------------------------------------------------ 12. determinism
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_flat_gradient_buffer_is_bit_reproducible(mode):
    with _mode(mode):
        flats = []
        for _ in range(2):
            model = build_small().cuda().train()
            ow = _optim(model)
            d = _data(seed=21)
            total, _ = model.parse_losses(model.forward(d["inputs"], d["data_samples"], mode="loss"))
            ow.backward(total)
            flats.append(ow.optimizer.gflat.clone())
        assert flats[0].abs().max().item() > 0
        assert torch.equal(flats[0], flats[1])


# ------------------------------------------------------------------------------------------------ 13. resume
def test_resume_is_bit_identical(tmp_path):
    """Checkpoint after step 2 (whole backbone in the state dict, optimiser moments, wrapper iteration), resume in a fresh model, step 3:
    the parameters equal the uninterrupted run's bit for bit."""
    set_compute_dtype("bf16")
    model = build_small().cuda().train()
    ow = _optim(model, backbone_lr_mult=0.1, end=10)
    for t in range(2):
        model.train_step(_data(seed=30 + t), ow)
    path = str(tmp_path / "iter_2.pth")
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    assert all(k in sd for k in trained_backbone_keys(small_state_dict()) + inert_backbone_keys(small_state_dict()))
    torch.save(dict(state_dict=sd, optimizer=ow.optimizer.state_dict(), optim_wrapper=ow.state_dict()), path)
    model.train_step(_data(seed=32), ow)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    m2 = build_small().cuda().train()
    ow2 = _optim(m2, backbone_lr_mult=0.1, end=10)
    m2.load_state_dict(ck["state_dict"])
    ow2.optimizer.load_state_dict({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in ck["optimizer"].items()})
    ow2.load_state_dict(ck["optim_wrapper"])
    m2.train_step(_data(seed=32), ow2)
    a, b = model.state_dict(), m2.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 14. data parallelism
def _free_port():
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fullft_dp_worker.py"), out], env=env, stdout=subprocess.PIPE,
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


def test_two_ranks_equal_one_rank_with_the_global_batch(tmp_path):
    """Two gloo ranks x batch 1 against one process x batch 2 in f32, at the f32 bounds of tests/test_dp_equivalence_gpu.py (losses rtol
    1e-5, parameters 2e-5 mean-relative); the base-weight buckets leave in production order - `backbone0` (block 1) while the backward
    still runs, `backbone1` (block 0 and the embeddings) when it has ended."""
    one = _run(1, str(tmp_path / "w1.pt"))
    two = _run(2, str(tmp_path / "w2.pt"))
    assert torch.allclose(one["logs"], two["logs"], rtol=1e-5, atol=1e-6), (one["logs"], two["logs"])
    worst, n = 0.0, 0
    for k, a in one["state"].items():
        if "running_" in k or "num_batches" in k or k == "decode_head.output_upscaling.0.bias":   # (a bias right before BatchNorm: exact gradient 0)
            continue
        b = two["state"][k]
        if k in inert_backbone_keys(one["state"]):
            assert torch.equal(a, b), k
            continue
        d = (a - b).abs().mean().item() / max(a.abs().mean().item(), 1e-12)
        worst, n = max(worst, d), n + 1
        assert d < 2e-5, (k, d)
    assert n >= 4 + 14 * 2 + 7
    ev = two["events"]
    per_step = ev[:len(ev) // 2]
    assert per_step == ["decode_head", "backbone0", "<backbone backward ended>", "backbone1"], ev
    print(f"[full dp equivalence f32] worst relative parameter difference {worst:.2e} over {n} tensors; bucket launch order {per_step}")


# ------------------------------------------------------------------------------------------------ 15. --amp, and what is refused
def test_three_amp_steps_fp16():
    """`--amp` (AmpOptimWrapper: fp16 twin library, device-side dynamic loss scale) over the full model: three steps, none skipped, the scale
    stays at its initial 2^16, the loss is finite and every trained backbone tensor moves."""
    sd0 = small_state_dict()
    model = build_small(sd=sd0).cuda().train()
    ow = _optim(model, backbone_lr_mult=0.1, amp=True)
    assert ow.mode == "fp16"
    with _mode(ow.mode):
        losses = [float(model.train_step(_data(seed=50 + t), ow)["loss"]) for t in range(3)]
        assert all(torch.isfinite(torch.tensor(losses))), losses
        assert ow.skipped == 0 and ow.scale == 2.0 ** 16 and ow.optimizer.step_count == 3
        got = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    for k in trained_backbone_keys(sd0):
        assert not torch.equal(got[k], sd0[k]), k
    for k in inert_backbone_keys(sd0):
        assert torch.equal(got[k], sd0[k]), k


def test_training_grid_must_be_the_pos_embed_grid():
    set_compute_dtype("bf16")
    model = build_small().cuda().train()
    img = torch.zeros(1, 3, 128, 128, device="cuda")
    with pytest.raises(NotImplementedError, match="img_size"):
        model.backbone.forward_tokens([(img, None)], training=True)
    model.eval()
    with torch.no_grad():
        xcat, grid = model.backbone.forward_tokens([(img, None)], training=False)    # predictions interpolate the position embedding
    assert tuple(grid) == (8, 8)


def test_no_grad_calls_of_a_training_model_stay_on_the_prediction_path():
    set_compute_dtype("bf16")
    from vfmseg_amd import backbones
    model = build_small().cuda().train()
    pending = backbones._PENDING_BACKWARD[0]
    with torch.no_grad():
        model.extract_feat(batch(1, 0)[0].cuda())
    assert backbones._PENDING_BACKWARD[0] == pending     # no forward was registered as waiting for a backward
