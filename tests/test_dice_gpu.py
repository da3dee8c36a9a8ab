"""DiceLoss on the fused loss path on a real MI355X: the three kernels (vfm_upsample_dice_sums, vfm_dice_finish, vfm_upsample_dice_bwd)
against the float64 restatement of tests/dice_helpers.py, their edge cases, reproducibility and scaling, the fused form against the
composed one, the heads with a CE + Dice list and one train step.

Bounds are the project's own for this loss path (test_upsample_ce, tests/test_loss_options_gpu.py): loss within 1e-5 * max(1, |ref|); a, b
and coef to relative error 1e-5; gradient rel_err < 2e-5; hits and valid exact."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import dice_helpers as DH  # noqa: E402
from tests import loss_options_helpers as LO  # noqa: E402
from tests.helpers import rel_err  # noqa: E402
from tests.test_dacs_gpu import CE_CASES  # noqa: E402
from vfmseg_amd import functional as Fh, ops, presets  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402

DEV = "cuda"
B = 2
EPS = 1e-3
NONSQUARE, BIG = (5, 7, 33, 45, 19), (16, 16, 128, 128, 19)
# (h, w, H, W, C): the x4, x16 and generic geometries with clamped borders (CE_CASES), a non-square map whose image 1 is ignored
# altogether, and a map whose images span many rows of the sums' slab
CASES = [(h, h, H, H, C) for h, H, C in CE_CASES] + [NONSQUARE, BIG]
IDS = ["%dx%d-%dx%d-C%d" % c for c in CASES]
ODD = CASES[0]   # this case's labels also hold a class >= C that is not 255 and a negative label
# the tiled backward (x4 and x16 with 19 classes; CASES[4] and CASES[5] have border tiles only) with a tile that touches no border
INNER = [(12, 12, 48, 48, 19), (3, 3, 48, 48, 19)]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(logits, label): seeded, shared by the tests, never written to.  Every label map holds 255 (two rows, a column of image 0)."""
    h, w, H, W, C = case
    lg = DH.rnd(B, h, w, C, seed=900 + H + C, scale=2.0)
    lab = DH.labels(B, H, W, C, 800 + H + C, all_ignored_image=case == NONSQUARE)
    if case == ODD:
        lab[0, 6, 6], lab[1, 7, 7], lab[1, 8, 8] = C + 21, C, -3
    return lg, lab


@functools.lru_cache(maxsize=None)
def _ref(case, use_sigmoid, naive, drop_class=-1, loss_weight=1.0):
    lg, lab = _inputs(case)
    return DH.dice(lg, lab, use_sigmoid, naive, EPS, drop_class, loss_weight)


def _rel_each(got, ref):
    """largest elementwise relative error; where the reference is exactly 0 the value must be exactly 0"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    zero = ref == 0
    assert bool((got[zero] == 0).all()), (got, ref)
    return float(((got - ref).abs()[~zero] / ref.abs()[~zero]).max()) if bool((~zero).any()) else 0.0


def _kernels(lg, lab, use_sigmoid, naive, drop_class=-1, **kw):
    stats = {}
    loss, acc, coef, dl = ops.upsample_dice(lg.to(DEV), lab.to(DEV), use_sigmoid, naive, EPS, drop_class, need_grad=True, stats=stats, **kw)
    return loss, acc, coef, dl, stats["sums"], stats["counts"]


def _check(tag, got, ref, hits=None):
    """hits: the expected top-1 count where the float64 reference cannot say (exact ties); else the reference's"""
    hits = ref["hits"] if hits is None else hits
    loss, acc, coef, dl, sums, counts = got
    errs = dict(loss=abs(loss.item() - ref["loss"]) / max(1, abs(ref["loss"])), a=_rel_each(sums[:, 0], ref["a"]), b=_rel_each(sums[:, 1], ref["b"]),
                coef=_rel_each(coef, ref["coef"]), grad=rel_err(dl, ref["grad"]))
    print(f"[dice] {tag}: loss {loss.item():.7f} (ref {ref['loss']:.7f}) " + " ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f" hits {counts[0].item()} valid {counts[1].item()}")
    assert errs["loss"] < 1e-5 and errs["a"] < 1e-5 and errs["b"] < 1e-5 and errs["coef"] < 1e-5
    assert errs["grad"] < 2e-5
    assert torch.equal(sums[:, 2].cpu().double(), ref["c"])                      # sum t: an integer
    assert counts.tolist() == [hits, ref["valid"]]
    assert abs(acc.item() - 100.0 * hits / (ref["valid"] + LO.EPS)) < 1e-3


# ------------------------------------------------------------------------------------------------ 1. kernels against float64
@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
@pytest.mark.parametrize("case", CASES + INNER, ids=IDS + ["%dx%d-%dx%d-C%d" % c for c in INNER])
def test_kernels_match_float64(case, use_sigmoid, naive):
    lg, lab = _inputs(case)
    assert bool((lab == 255).any()) and (case != ODD or (bool((lab < 0).any()) and bool(((lab >= case[4]) & (lab != 255)).any())))
    _check(f"{case} {'sigmoid' if use_sigmoid else 'softmax'} {'naive' if naive else 'plain'}", _kernels(lg, lab, use_sigmoid, naive),
           _ref(case, use_sigmoid, naive))


# ------------------------------------------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_every_pixel_ignored(case, use_sigmoid, naive):
    lg, lab = _inputs(case)
    none = torch.full_like(lab, 255)
    loss, acc, coef, dl, sums, counts = _kernels(lg, none, use_sigmoid, naive)
    ref = DH.dice(lg, none, use_sigmoid, naive, EPS)
    assert counts.tolist() == [0, 0] and acc.item() == 0.0 and float(sums[:, 0].abs().max()) == 0.0 and float(sums[:, 2].abs().max()) == 0.0
    if naive:   # d = eps / s: d loss / d p = gamma / B on every channel
        assert abs(loss.item() - ref["loss"]) < 1e-5 and _rel_each(coef, ref["coef"]) < 1e-5 and float(ref["coef"][0, 2]) > 0
        if use_sigmoid:
            assert float(ref["grad"].abs().max()) > 0 and rel_err(dl, ref["grad"]) < 2e-5
        else:
            # a constant over the channels is in the null space of the softmax Jacobian: p_c (g - sum_k p_k g) = 0, and float64 leaves
            # 1e-23 of it.  What fp32 leaves is rounding of terms of size gamma / B, added over a footprint of (H / h)(W / w) pixels: the
            # gradient bound 2e-5 on that scale
            h, w, H, W, _ = case
            assert float(ref["grad"].abs().max()) < 1e-20
            assert float(dl.abs().max()) < 2e-5 * float(ref["coef"][0, 2]) / B * (H / h) * (W / w)
    else:
        assert loss.item() == 1.0 and float(dl.abs().max()) == 0.0


@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
@pytest.mark.parametrize("case", [CASES[3], BIG], ids=[IDS[3], IDS[-1]])
def test_no_pixel_ignored_and_constant_logits(case, use_sigmoid, naive):
    h, w, H, W, C = case
    lg = _inputs(case)[0]
    lab = torch.randint(0, C, (B, H, W), generator=torch.Generator().manual_seed(31))
    _check(f"{case} no pixel ignored", _kernels(lg, lab, use_sigmoid, naive), DH.dice(lg, lab, use_sigmoid, naive, EPS))
    const = torch.full((B, h, w, C), 0.3)
    got = _kernels(const, lab, use_sigmoid, naive)
    # every class ties at every pixel and the first maximum wins, as in vfm_pseudo_label: every pixel predicts class 0.  (The float64
    # reference interpolates the channels in vector lanes that round differently by 5e-17: its arg-max of the tie is noise.)
    _check(f"{case} constant logits", got, DH.dice(const, lab, use_sigmoid, naive, EPS), hits=int((lab == 0).sum()))
    # every p is sigmoid(0.3) or 1 / C
    p0 = 1 / (1 + torch.exp(torch.tensor(-0.3, dtype=torch.float64))) if use_sigmoid else torch.tensor(1.0 / C, dtype=torch.float64)
    want_b = float(C * H * W * (p0 if naive else p0 * p0))
    assert abs(float(got[4][0, 1]) - want_b) < 1e-5 * want_b
    assert got[5].tolist() == [int((lab == 0).sum()), B * H * W]


@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
@pytest.mark.parametrize("case,drop", [(CASES[1], 0), (CASES[4], 7), (ODD, 6), (NONSQUARE, 18)])
def test_drop_class_leaves_the_channel_out_of_all_three_sums(case, drop, use_sigmoid, naive):
    lg, lab = _inputs(case)
    got = _kernels(lg, lab, use_sigmoid, naive, drop_class=drop)
    _check(f"{case} drop_class {drop}", got, _ref(case, use_sigmoid, naive, drop))
    if use_sigmoid:
        assert float(got[3][..., drop].abs().max()) == 0.0   # a sigmoid channel that is in no sum gets no gradient


# ------------------------------------------------------------------------------------------------ 3. reproducibility and scaling
@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
@pytest.mark.parametrize("case", [CASES[1], CASES[5], BIG], ids=[IDS[1], IDS[5], IDS[-1]])
def test_two_runs_are_bitwise_equal(case, use_sigmoid, naive):
    lg, lab = _inputs(case)
    first, second = _kernels(lg, lab, use_sigmoid, naive), _kernels(lg, lab, use_sigmoid, naive)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("use_sigmoid,naive", [DH.FORMS[0], DH.FORMS[3]], ids=[DH.FORM_IDS[0], DH.FORM_IDS[3]])
@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5], NONSQUARE], ids=[IDS[1], IDS[4], IDS[5], IDS[6]])
def test_accumulate_adds_onto_a_cross_entropy_gradient(case, use_sigmoid, naive):
    lg, lab = _inputs(case)
    x, y = lg.to(DEV), lab.to(DEV)
    _, _, g_ce = ops.upsample_ce(x, y, 255, need_grad=True)
    g_dice = ops.upsample_dice(x, y, use_sigmoid, naive, EPS, -1, need_grad=True, grad_scale=3.0 / B)[3]
    both = g_ce.clone()
    out = ops.upsample_dice(x, y, use_sigmoid, naive, EPS, -1, need_grad=True, grad_scale=3.0 / B, accumulate_into=both)[3]
    assert out is both
    # one fp32 addition per element: within 1 ulp (2^-23 relative) of the larger term
    ulp = torch.maximum(g_ce.abs(), g_dice.abs()).double() * 2.0 ** -23
    assert bool(((both.double() - (g_ce.double() + g_dice.double())).abs() <= ulp).all())
    assert torch.equal(both, g_ce + g_dice)


@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
def test_a_scaled_loss_scales_the_gradient_exactly(use_sigmoid, naive):
    """(loss * 1024).backward(): the --amp loss scaler's power of two reaches the gradient on the device, exactly."""
    lg, lab = _inputs(CASES[4])
    grads = []
    for scale in (1.0, 1024.0):
        x = lg.to(DEV).requires_grad_(True)
        loss, acc = Fh.UpsampleDiceFn.apply(x, lab.to(DEV), use_sigmoid, naive, EPS, -1, 3.0)
        assert not acc.requires_grad
        (loss * scale).backward()
        grads.append(x.grad)
    assert float(grads[0].abs().max()) > 0 and torch.equal(grads[0] * 1024.0, grads[1])


# ------------------------------------------------------------------------------------------------ 4. fused against composed, the module
def _head(kind, C, loss_decode):
    cfg = dict(segformer=presets.segformer_head, linear=presets.linear_head)[kind](embed_dim=64, channels=64, num_classes=C)
    cfg["loss_decode"] = loss_decode
    return MODELS.build(cfg)


def _head_losses(head, lg, lab):
    """(losses, dlogits of their sum) of the head's loss path on low-resolution logits."""
    x = lg.to(DEV).requires_grad_(True)
    out = head.loss_by_feat(x, lab.to(DEV))
    sum(v for k, v in out.items() if "loss" in k).backward()
    return {k: v.detach() for k, v in out.items()}, x.grad


@pytest.mark.parametrize("use_sigmoid,naive", DH.FORMS, ids=DH.FORM_IDS)
@pytest.mark.parametrize("case", [CASES[1], CASES[4], NONSQUARE], ids=[IDS[1], IDS[4], IDS[6]])
def test_fused_equals_composed_through_loss_by_feat(case, use_sigmoid, naive, monkeypatch):
    lg, lab = _inputs(case)
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("VFMSEG_DICE_FUSED", fused)
        head = _head("segformer", case[4], [dict(type="DiceLoss", use_sigmoid=use_sigmoid, naive_dice=naive, loss_weight=3.0)])
        assert head.loss_decode[0].fused == (fused == "1")
        got[fused] = _head_losses(head, lg, lab)
    (l1, g1), (l0, g0) = got["1"], got["0"]
    print(f"[dice] {case} fused {l1['loss_dice'].item():.7f} composed {l0['loss_dice'].item():.7f} grad relerr {rel_err(g1, g0):.2e}")
    assert abs(l1["loss_dice"].item() - l0["loss_dice"].item()) < 1e-5 * max(1, abs(l0["loss_dice"].item()))
    assert rel_err(g1, g0) < 2e-5
    assert abs(l1["acc_seg"].item() - l0["acc_seg"].item()) < 1e-3


def test_dice_loss_module_forward_at_label_resolution():
    """DiceLoss.forward(pred NCHW at label size, target): the same kernels with h = H."""
    C, H, W = 19, 13, 17
    score, lab = DH.rnd(B, C, H, W, seed=720, scale=2.0), DH.labels(B, H, W, C, 721)
    for use_sigmoid, naive in DH.FORMS:
        mod = MODELS.build(dict(type="DiceLoss", use_sigmoid=use_sigmoid, naive_dice=naive, loss_weight=0.4, ignore_index=5))
        ref = DH.dice(score.permute(0, 2, 3, 1), lab, use_sigmoid, naive, EPS, drop_class=5, loss_weight=0.4)
        got = mod(score.to(DEV), lab.to(DEV).unsqueeze(1), ignore_index=255)
        assert abs(got.item() - ref["loss"]) < 1e-5 * max(1, abs(ref["loss"]))


# ------------------------------------------------------------------------------------------------ 5. heads
@pytest.mark.parametrize("kind", ["segformer", "linear"])
@pytest.mark.parametrize("case", [CASES[1], CASES[4], BIG], ids=[IDS[1], IDS[4], IDS[-1]])
def test_heads_with_the_ce_dice_list(kind, case):
    lg, lab = _inputs(case)
    C = case[4]
    both, g_both = _head_losses(_head(kind, C, presets.ce_dice_loss(ce=1.0, dice=3.0)), lg, lab)
    ce, g_ce = _head_losses(_head(kind, C, dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)), lg, lab)
    assert sorted(both) == ["acc_seg", "loss_ce", "loss_dice"] and sorted(ce) == ["acc_seg", "loss_ce"]
    assert torch.equal(both["loss_ce"], ce["loss_ce"]) and torch.equal(both["acc_seg"], ce["acc_seg"])
    ref = _ref(case, True, False, -1, 3.0)
    ref_ce = LO.options(lg, lab)
    want = ref["grad"] + ref_ce["grad"]
    print(f"[dice] {kind} {case}: loss_dice {both['loss_dice'].item():.7f} (ref {ref['loss']:.7f}), summed grad relerr {rel_err(g_both, want):.2e}")
    assert abs(both["loss_dice"].item() - ref["loss"]) < 1e-5 * max(1, abs(ref["loss"]))
    assert rel_err(g_both, want) < 2e-5
    assert rel_err(g_ce, ref_ce["grad"]) < 2e-5


@pytest.mark.parametrize("case", [CASES[1], CASES[5], NONSQUARE], ids=[IDS[1], IDS[5], IDS[6]])
def test_dice_alone_reports_the_accuracy_of_the_ce_kernel(case):
    lg, lab = _inputs(case)
    C = case[4]
    alone, _ = _head_losses(_head("segformer", C, [dict(type="DiceLoss", loss_weight=3.0)]), lg, lab)
    as_dict, _ = _head_losses(_head("segformer", C, dict(type="DiceLoss", loss_weight=3.0)), lg, lab)
    ce, _ = _head_losses(_head("segformer", C, dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)), lg, lab)
    assert sorted(alone) == ["acc_seg", "loss_dice"] and torch.equal(alone["acc_seg"], ce["acc_seg"])
    assert torch.equal(as_dict["loss_dice"], alone["loss_dice"]) and torch.equal(as_dict["acc_seg"], alone["acc_seg"])


def test_entries_that_share_a_loss_name_are_added():
    case = CASES[4]
    lg, lab = _inputs(case)
    two = [dict(type="DiceLoss", loss_name="loss_dice", loss_weight=1.0), dict(type="DiceLoss", loss_name="loss_dice", use_sigmoid=False, loss_weight=2.0)]
    out, g = _head_losses(_head("segformer", case[4], two), lg, lab)
    r1, r2 = _ref(case, True, False, -1, 1.0), _ref(case, False, False, -1, 2.0)
    assert sorted(out) == ["acc_seg", "loss_dice"]
    assert abs(out["loss_dice"].item() - (r1["loss"] + r2["loss"])) < 1e-5 * max(1, r1["loss"] + r2["loss"])
    assert rel_err(g, r1["grad"] + r2["grad"]) < 2e-5


def test_vfm_head_builds_with_the_list_and_runs_its_loss():
    cfg = presets.vfm_head(embed_dim=64, channels=128, num_classes=19)
    cfg["loss_decode"] = presets.ce_dice_loss()
    head = MODELS.build(cfg).to(DEV)
    lg, lab = _inputs(CASES[5])   # x16: the VFMHead geometry
    x = lg.to(DEV).requires_grad_(True)
    out = head._loss_from_lowres(x, lab.to(DEV).unsqueeze(1), False)
    assert sorted(out) == ["acc_seg", "loss_ce", "loss_dice"]
    (out["loss_ce"] + out["loss_dice"]).backward()
    ref = _ref(CASES[5], True, False, -1, 3.0)
    assert abs(out["loss_dice"].item() - ref["loss"]) < 1e-5 * max(1, abs(ref["loss"]))
    assert rel_err(x.grad, ref["grad"] + LO.options(lg, lab)["grad"]) < 2e-5


# ------------------------------------------------------------------------------------------------ 6. one train step
def _small_segformer(loss_decode):
    """presets.dinov2_segformer at depth 2, width 64 (one head of 64), dropout off so that two models of one seed see the same logits"""
    torch.manual_seed(1234)
    cfg = presets.dinov2_segformer(depth=2, embed_dim=64, num_heads=1)
    cfg["backbone"]["out_indices"] = [0, 1, 1, 1]
    cfg["Lora_config"]["lora_dropout"] = 0.0
    cfg["decode_head"] = presets.segformer_head(embed_dim=64, channels=64)
    cfg["decode_head"]["dropout_ratio"] = 0.0
    cfg["decode_head"]["loss_decode"] = loss_decode
    return MODELS.build(cfg).to(DEV).train()


def test_train_step_with_the_ce_dice_list():
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label
    img, lab = synth_image(2, 512, seed=31).to(DEV), synth_label(2, 512, seed=31)
    samples = [SegDataSample(gt_sem_seg=lab[i]) for i in range(2)]
    logs = {}
    for name, ld in (("list", presets.ce_dice_loss()), ("ce", dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))):
        model = _small_segformer(ld)
        before = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
        oc = presets.optim_cfg()
        ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
        logs[name] = model.train_step(dict(inputs=img, data_samples=samples), ow)
        Fh.join_wgrad_stream()
        torch.cuda.synchronize()
        changed = [n for n, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[n])]
        assert changed, "no parameter moved"
    log = logs["list"]
    assert {"decode.loss_ce", "decode.loss_dice", "decode.acc_seg", "loss"} <= set(log)
    ce, dice, total = float(log["decode.loss_ce"]), float(log["decode.loss_dice"]), float(log["loss"])
    print(f"[dice] train_step: loss_ce {ce:.7f} loss_dice {dice:.7f} loss {total:.7f} acc {float(log['decode.acc_seg']):.4f}")
    assert 0 < dice <= 3.0 and ce > 0 and abs(total - (ce + dice)) < 1e-6 * max(1, abs(total))
    assert torch.equal(log["decode.loss_ce"], logs["ce"]["decode.loss_ce"]) and torch.equal(log["decode.acc_seg"], logs["ce"]["decode.acc_seg"])
