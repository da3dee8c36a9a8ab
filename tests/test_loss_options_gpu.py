"""The loss options of the fused cross-entropy on a real MI355X: the OHEM pixel sampler (vfm_ohem_prob, vfm_ohem_threshold,
vfm_label_weight), class weights and avg_non_ignore, through the kernels, the heads' loss path and one train step, against torch.sort on
the GPU's own probabilities and against the float64 restatement of tests/loss_options_helpers.py.

Bounds are the project's own (tests/test_dacs_gpu.py, test_upsample_ce): p rel_err < 1e-5, loss 1e-5 * max(1, |ref|), gradient rel_err < 2e-5,
counters exact."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import loss_options_helpers as LO  # noqa: E402
from tests.helpers import rel_err  # noqa: E402
from tests.test_dacs_gpu import CE_CASES  # noqa: E402
from vfmseg_amd import functional as Fh, ops, presets  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402

DEV = "cuda"
B = 2
NONSQUARE, BIG = (5, 7, 33, 45, 19), (16, 16, 128, 128, 19)
# (h, w, H, W, C): every form of the loss kernel (CE_CASES), a non-square map (its image 1 is ignored altogether), histograms over dozens of blocks
CASES = [(h, h, H, H, C) for h, H, C in CE_CASES] + [NONSQUARE, BIG]
IDS = ["%dx%d-%dx%d-C%d" % c for c in CASES]
REGIMES = ["above", "below", "clamped"]


def _cw(C):
    return [0.5 + 0.1 * c for c in range(C)]


@functools.lru_cache(maxsize=None)
def _fixture(case):
    """(logits, label, {regime: (thresh, min_kept)}, {regime: float64 reference}) with the seed picked on the float64 side alone: no valid
    pixel other than those equal to the threshold lies within 1e-5 of it, in any regime.  Shared by the tests, never written to."""
    h, w, H, W, C = case
    lab = LO.labels(B, H, W, C, 700 + H + C, all_ignored_image=case == NONSQUARE)
    for seed in range(500, 560):
        lg = LO.rnd(B, h, w, C, seed=seed, scale=2.0)
        reg = LO.regimes(lg, lab)
        refs = {name: LO.options(lg, lab, *reg[name]) for name in REGIMES}
        if all(r["n_band"] == 0 for r in refs.values()):
            return lg, lab, reg, refs
    raise AssertionError("no seed gives a fixture with an empty band")


def _head(C, sampler=None, **loss_opts):
    cfg = presets.segformer_head(embed_dim=64, channels=64, num_classes=C)
    cfg["loss_decode"] = dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=loss_opts.pop("loss_weight", 1.0), **loss_opts)
    if sampler is not None:
        cfg["sampler"] = dict(type="OHEMPixelSampler", thresh=sampler[0], min_kept=sampler[1])
    return MODELS.build(cfg)


def _head_loss(head, lg, lab, seg_weight=None):
    """(loss, acc, dlogits) of the head's loss path on low-resolution logits."""
    x = lg.to(DEV).requires_grad_(True)
    out = head.loss_by_feat(x, lab.to(DEV), seg_weight)
    out["loss_ce"].backward()
    return out["loss_ce"].detach(), out["acc_seg"].detach(), x.grad


# ------------------------------------------------------------------------------------------------ 1. selection against torch.sort
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_selection_equals_torch_sort_on_the_gpu_probabilities(case, regime):
    lg, lab, reg, refs = _fixture(case)
    C = case[4]
    thresh, min_kept = reg[regime]
    labd = lab.to(DEV)
    cw = torch.tensor(_cw(C), dtype=torch.float32, device=DEV)
    weight, p, t, state, norm, counts = ops.ohem_weight(lg.to(DEV), labd, thresh, min_kept * B)
    weight_cw = ops.ohem_weight(lg.to(DEV), labd, thresh, min_kept * B, class_weight=cw)[0]
    valid = labd != 255
    th32 = torch.tensor([thresh], dtype=torch.float32, device=DEV)
    s = torch.sort(p[valid])[0]
    n = s.numel()
    k = min(min_kept * B, n - 1)
    t_ref = torch.maximum(s[k:k + 1], th32)
    print(f"[ohem] {case} {regime}: n {n} k {k} thresh {thresh} t {t.item():.9g} (sort {t_ref.item():.9g}), kept {int(weight.sum())}, "
          f"p rel err {rel_err(p[valid], refs[regime]['p'][lab != 255]):.2e}")
    assert torch.equal(t, t_ref)
    assert state[ops.OHEM_N].item() == n == refs[regime]["n"] and state[ops.OHEM_K].item() == k
    assert state[ops.OHEM_NLT].item() == int((p[valid] < th32).sum())
    assert bool((p[~valid] == -1).all()) and rel_err(p[valid], refs[regime]["p"][lab != 255]) < 1e-5
    mask = (p < t) & valid
    assert torch.equal(weight, mask.to(torch.float32))
    assert torch.equal(weight_cw, mask.to(torch.float32) * cw[torch.where(valid, labd, torch.zeros_like(labd))])
    if regime == "above":
        assert t.item() > th32.item() and int(mask.sum()) == int((s < s[k]).sum()) <= k   # (< k: ties with the k-th value, the clamped border pixels of the x16 case)
    elif regime == "below":
        assert torch.equal(t, th32) and int(mask.sum()) == state[ops.OHEM_NLT].item() > k
    else:
        assert k == n - 1 and torch.equal(t, s[-1:])


@pytest.mark.parametrize("case", [CASES[1], CASES[4], BIG], ids=[IDS[1], IDS[4], IDS[-1]])
def test_constant_logits_keep_nothing(case):
    """all p are equal (1 / C), so nothing lies below t = p and the weights are all zero"""
    h, w, H, W, C = case
    lab = LO.labels(B, H, W, C, 710).to(DEV)
    lg = torch.full((B, h, w, C), 0.3, device=DEV)
    weight, p, t, state, _, _ = ops.ohem_weight(lg, lab, 0.01, 5)
    valid = lab != 255
    assert bool((p[valid] == p[valid][0]).all()) and abs(p[valid][0].item() - 1.0 / C) < 1e-6
    assert t.item() == p[valid][0].item() and float(weight.abs().max()) == 0.0 and state[ops.OHEM_NLT].item() == 0


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ohem_loss_and_gradient_match_float64(case, regime):
    lg, lab, reg, refs = _fixture(case)
    ref = refs[regime]
    assert ref["n_band"] == 0
    head = _head(case[4], sampler=reg[regime])
    mask = head.sampler.sample_lowres(lg.to(DEV), lab.to(DEV))
    assert torch.equal(mask.cpu() != 0, ref["mask"])
    loss, acc, dl = _head_loss(head, lg, lab)
    print(f"[ohem] {case} {regime}: loss {loss.item():.7f} (ref {ref['loss']:.7f}), grad relerr {rel_err(dl, ref['grad']):.2e}, kept {int(mask.sum())} of {ref['n']}")
    assert abs(loss.item() - ref["loss"]) < 1e-5 * max(1, abs(ref["loss"]))
    assert rel_err(dl, ref["grad"]) < 2e-5
    assert abs(acc.item() - 100.0 * ref["hits"] / (ref["n"] + LO.EPS)) < 1e-3   # unweighted: every valid pixel counts


# ------------------------------------------------------------------------------------------------ 3. identities
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_thresh_two_is_the_sampler_free_path_bitwise(case):
    lg, lab, _, _ = _fixture(case)
    loss0, acc0, dl0 = _head_loss(_head(case[4]), lg, lab)
    every = _head(case[4], sampler=(2.0, 5))
    assert torch.equal(every.sampler.sample_lowres(lg.to(DEV), lab.to(DEV)).cpu(), (lab != 255).float())   # every valid pixel is kept
    loss1, acc1, dl1 = _head_loss(every, lg, lab)
    assert torch.equal(loss0, loss1) and torch.equal(acc0, acc1) and torch.equal(dl0, dl1)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5], NONSQUARE, BIG], ids=[IDS[1], IDS[4], IDS[5], IDS[6], IDS[7]])
def test_fused_and_composed_forms_agree(case, regime, monkeypatch):
    lg, lab, reg, refs = _fixture(case)
    ref = refs[regime]
    assert ref["n_band"] < 0.01 * ref["n"]
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("VFMSEG_OHEM_FUSED", fused)
        head = _head(case[4], sampler=reg[regime], class_weight=_cw(case[4]))
        assert head.sampler.fused == (fused == "1")
        out[fused] = (head.sampler.sample_lowres(lg.to(DEV), lab.to(DEV)),) + _head_loss(head, lg, lab)
    (w1, loss1, acc1, dl1), (w0, loss0, acc0, dl0) = out["1"], out["0"]
    outside = ((ref["p"] - ref["t"]).abs() >= LO.BAND).to(DEV)
    assert torch.equal(w1[outside], w0[outside])
    assert abs(loss1.item() - loss0.item()) < 1e-5 * max(1, abs(loss0.item())) and abs(acc1.item() - acc0.item()) < 1e-5 * max(1, abs(acc0.item()))
    assert rel_err(dl1, dl0) < 2e-5


# ------------------------------------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize("case", [CASES[4], BIG], ids=[IDS[4], IDS[-1]])
def test_two_runs_are_bitwise_equal(case):
    lg, lab, reg, _ = _fixture(case)
    runs = []
    for _ in range(2):
        head = _head(case[4], sampler=reg["above"], class_weight=_cw(case[4]), avg_non_ignore=True)
        weight, p, t, state, _, _ = ops.ohem_weight(lg.to(DEV), lab.to(DEV), reg["above"][0], reg["above"][1] * B)
        runs.append((weight, p, t.clone(), state.clone()) + _head_loss(head, lg, lab))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. class weights and avg_non_ignore
OPTION_SETS = {"cw": dict(class_weight=True), "avg": dict(avg_non_ignore=True), "cw+avg": dict(class_weight=True, avg_non_ignore=True),
               "cw+ohem": dict(class_weight=True, ohem=True), "avg+ohem": dict(avg_non_ignore=True, ohem=True),
               "cw+avg+ohem": dict(class_weight=True, avg_non_ignore=True, ohem=True)}


@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_class_weights_and_avg_non_ignore_match_float64(case, opts):
    lg, lab, reg, _ = _fixture(case)
    o = OPTION_SETS[opts]
    C = case[4]
    cw = _cw(C) if o.get("class_weight") else None
    sampler = reg["above"] if o.get("ohem") else None
    ref = LO.options(lg, lab, *(sampler or (None, None)), class_weight=cw, avg_non_ignore=o.get("avg_non_ignore", False), loss_weight=0.4)
    kw = dict(loss_weight=0.4, avg_non_ignore=o.get("avg_non_ignore", False))
    if cw is not None:
        kw["class_weight"] = cw
    loss, acc, dl = _head_loss(_head(C, sampler=sampler, **kw), lg, lab)
    print(f"[loss options] {case} {opts}: loss {loss.item():.7f} (ref {ref['loss']:.7f}), avg_factor {ref['avg_factor']:.3f}, grad relerr {rel_err(dl, ref['grad']):.2e}")
    assert abs(loss.item() - ref["loss"]) < 1e-5 * max(1, abs(ref["loss"]))
    assert rel_err(dl, ref["grad"]) < 2e-5
    assert abs(acc.item() - 100.0 * ref["hits"] / (ref["n"] + LO.EPS)) < 1e-3


def test_label_weight_counts_and_normaliser_are_exact():
    C = BIG[4]
    _, lab, _, _ = _fixture(BIG)
    cw = torch.tensor(_cw(C), dtype=torch.float32, device=DEV)
    valid = lab != 255
    per_class = torch.bincount(lab[valid], minlength=C).tolist()
    weight, norm, counts = ops.label_weight(lab.to(DEV), C, class_weight=cw)
    assert counts.tolist() == per_class + [0] * (ops.LABEL_COUNT_INTS - 1 - C) + [0]
    avg = sum(float(cw[c].double()) * per_class[c] for c in range(C))
    assert abs(norm[1].item() - avg) <= 1e-6 * avg and abs(norm[0].item() - lab.numel() / (avg + LO.EPS)) <= 1e-6 * lab.numel() / avg
    assert torch.equal(weight.cpu(), torch.where(valid, cw.cpu()[torch.where(valid, lab, torch.zeros_like(lab))], torch.zeros(())))
    weight, norm, counts = ops.label_weight(lab.to(DEV), C, avg_non_ignore=True, want_weight=False)
    assert weight is None and norm[1].item() == float(valid.sum()) and counts.tolist()[:C] == per_class


def test_cross_entropy_loss_module_honours_the_options_with_a_weight_map():
    """CrossEntropyLoss.forward (cls_score at label resolution) with class weights, avg_non_ignore and weight= against float64."""
    C, H, W = 19, 13, 17
    score, lab = LO.rnd(B, C, H, W, seed=720, scale=2.0), LO.labels(B, H, W, C, 721)
    pix = torch.rand(B, H, W, generator=torch.Generator().manual_seed(722))
    for kw in (dict(class_weight=_cw(C)), dict(avg_non_ignore=True), dict(class_weight=_cw(C), avg_non_ignore=True)):
        mod = MODELS.build(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4, **kw))
        for w_ in (pix, None):
            ref = LO.options(score.permute(0, 2, 3, 1), lab, class_weight=kw.get("class_weight"), avg_non_ignore=kw.get("avg_non_ignore", False),
                             pix_weight=w_, loss_weight=0.4)
            got = mod(score.to(DEV), lab.to(DEV), weight=None if w_ is None else w_.to(DEV), ignore_index=255)
            assert abs(got.item() - ref["loss"]) < 1e-5 * max(1, abs(ref["loss"]))


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_all_ignored_batch_gives_zero_loss_and_gradient(case):
    lg, lab, reg, _ = _fixture(case)
    none = torch.full_like(lab, 255)
    for kw in (dict(sampler=reg["above"]), dict(class_weight=_cw(case[4])), dict(avg_non_ignore=True),
               dict(sampler=reg["below"], class_weight=_cw(case[4]), avg_non_ignore=True)):
        loss, acc, dl = _head_loss(_head(case[4], **kw), lg, none)
        assert loss.item() == 0.0 and float(dl.abs().max()) == 0.0 and acc.item() == 0.0
    weight, p, t, state, _, _ = ops.ohem_weight(lg.to(DEV), none.to(DEV), 0.7, 10)
    assert t.item() == torch.tensor(0.7, dtype=torch.float32).item() and state[ops.OHEM_N].item() == 0 and float(weight.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 6. one train step
def _linear_model():
    from tests.helpers import full_state_dict
    cfg = presets.dinov2_linear(depth=2)
    cfg["backbone"]["backbone"]["out_indices"] = [0, 1, 1, 1]
    cfg["backbone"]["Lora_config"]["lora_dropout"] = 0.0
    cfg["decode_head"]["dropout_ratio"] = 0.0
    return cfg, {k: v for k, v in full_state_dict(depth=2).items() if not k.startswith("aux_decoder.")}


def _segformer_model():
    from tests import segformer_helpers as S
    return S.model_config("lora", 2), S.model_state_dict("lora", 2)


@pytest.mark.parametrize("kind", ["linear", "segformer"])
def test_train_step_with_sampler_and_class_weights(kind):
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label
    cfg, sd = (_linear_model if kind == "linear" else _segformer_model)()
    thresh, min_kept, cw = 0.7, 100000, _cw(19)
    cfg["decode_head"]["sampler"] = dict(type="OHEMPixelSampler", thresh=thresh, min_kept=min_kept)
    cfg["decode_head"]["loss_decode"].update(class_weight=cw)
    model = MODELS.build(cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(DEV).train()
    head = model.decode_head
    img, lab = synth_image(2, 512, seed=31).to(DEV), synth_label(2, 512, seed=31)
    samples = [SegDataSample(gt_sem_seg=lab[i]) for i in range(2)]
    seen = {}
    inner = head.forward_tokens

    def recording(*a, **k):
        seen["logits"] = inner(*a, **k)
        return seen["logits"]
    head.forward_tokens = recording

    def nonzero_grads():
        for p_ in model.parameters():
            p_.grad = None
        total, _ = model.parse_losses(model.loss(img, samples))
        total.backward()
        Fh.join_wgrad_stream()
        torch.cuda.synchronize()
        return {n for n, p_ in model.named_parameters() if p_.grad is not None and float(p_.grad.abs().max()) > 0}

    with_options = nonzero_grads()
    sampler, loss_decode = head.sampler, head.loss_decode
    head.sampler, head.loss_decode = None, MODELS.build(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))
    without = nonzero_grads()
    head.sampler, head.loss_decode = sampler, loss_decode
    assert without and without <= with_options, sorted(without - with_options)[:5]
    for p_ in model.parameters():
        p_.grad = None
    oc = presets.optim_cfg()
    ow = PEFTOptimWrapperConstructor(oc["optim_wrapper"])(model, oc["param_scheduler"])
    log = model.train_step(dict(inputs=img, data_samples=samples), ow)
    torch.cuda.synchronize()
    del head.forward_tokens   # (the recorder refers to the head: no reference cycle is left behind for the collector)
    ref = LO.options(seen["logits"].detach().float().cpu(), lab.reshape(2, 512, 512), thresh, min_kept, cw)
    loss, acc = float(log["decode.loss_ce"]), float(log["decode.acc_seg"])
    print(f"[loss options] {kind} train_step: loss {loss:.7f} (ref {ref['loss']:.7f}), acc {acc:.4f}, kept {int(ref['mask'].sum())} of {ref['n']}, "
          f"t {ref['t']:.6f}, band {ref['n_band']}")
    assert 0 < int(ref["mask"].sum()) < ref["n"]
    assert abs(loss - ref["loss"]) < 1e-5 * max(1, abs(ref["loss"]))
    assert abs(acc - 100.0 * ref["hits"] / (ref["n"] + LO.EPS)) < 2e-3
    assert abs(float(log["loss"]) - loss) < 1e-6 * max(1, abs(loss))
