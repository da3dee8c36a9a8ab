"""The DACS kernels (vfm_upsample_ce_w, vfm_pseudo_label, vfm_class_presence, vfm_class_mix) and the EMA update on a real MI355X against
the float64 restatements of tests/dacs_helpers.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import dacs_helpers as D  # noqa: E402
from tests.helpers import rel_err  # noqa: E402
from vfmseg_amd import ops  # noqa: E402

DEV = "cuda"


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _labels(B, H, W, C, seed):
    lab = torch.randint(0, C, (B, H, W), generator=torch.Generator().manual_seed(seed))
    lab[:, 2:4] = 255
    lab[0, :, 1] = 255
    return lab


def _weights(B, H, W, seed):
    """zeros, ones and fractions, a third each"""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 3, (B, H, W), generator=g)
    frac = torch.rand(B, H, W, generator=g)
    return torch.where(kind == 0, torch.zeros(()), torch.where(kind == 1, torch.ones(()), frac)).contiguous()


# (h, H, C): generic WPP 1 (5 -> 13), generic WPP 4 (3 -> 25: 625 >= 64 * 9), the <4,4,19,20> tile (8 -> 32, 19 classes) and the x16 tile (2 -> 32)
CE_CASES = [(5, 13, 7), (5, 13, 19), (3, 25, 7), (3, 25, 19), (8, 32, 19), (2, 32, 19)]


@pytest.mark.parametrize("h,H,C", CE_CASES)
def test_upsample_ce_w_matches_float64(h, H, C):
    """Bounds of test_upsample_ce: loss 1e-5, gradient relerr 2e-5, counters exact - and unweighted: a weight-0 pixel with a valid label counts."""
    B = 2
    lg, lab, wt = _rnd(B, h, h, C, seed=300 + h, scale=2.0), _labels(B, H, H, C, 301 + H), _weights(B, H, H, 302 + C)
    assert int(((wt == 0) & (lab != 255)).sum()) > 0 and int((wt == 1).sum()) > 0 and int(((wt > 0) & (wt < 1)).sum()) > 0
    loss_ref, grad_ref, counts_ref = D.upsample_ce_w(lg, lab, wt)
    loss, counts, dl = ops.upsample_ce_w(lg.to(DEV), lab.to(DEV), wt.to(DEV))
    print(f"[dacs] upsample_ce_w {h}->{H} C={C}: loss {loss.item():.7f} (ref {loss_ref:.7f}), grad relerr {rel_err(dl, grad_ref):.2e}, counts {counts.tolist()}")
    assert abs(loss.item() - loss_ref) < 1e-5 * max(1, abs(loss_ref))
    assert counts.tolist() == counts_ref
    assert rel_err(dl, grad_ref) < 2e-5
    loss2, acc2, dl2 = ops.upsample_ce_w_loss_acc(lg.to(DEV), lab.to(DEV), wt.to(DEV))   # the training form
    assert torch.equal(loss2, loss) and torch.equal(dl2, dl)
    assert abs(acc2.item() - 100.0 * counts_ref[0] / (counts_ref[1] + torch.finfo(torch.float32).eps)) < 1e-3


@pytest.mark.parametrize("h,H,C", CE_CASES)
def test_upsample_ce_w_null_and_ones_are_upsample_ce_bitwise(h, H, C):
    B = 2
    lg, lab = _rnd(B, h, h, C, seed=310 + h, scale=2.0).to(DEV), _labels(B, H, H, C, 311 + H).to(DEV)
    loss0, counts0, dl0 = ops.upsample_ce(lg, lab)
    p_null, p_ones = (torch.empty(B * h * h, device=DEV) for _ in range(2))
    loss1, counts1, dl1 = ops.upsample_ce_w(lg, lab, None, parts_out=p_null)
    loss2, counts2, dl2 = ops.upsample_ce_w(lg, lab, torch.ones(B, H, H, device=DEV), parts_out=p_ones)
    for loss, counts, dl in ((loss1, counts1, dl1), (loss2, counts2, dl2)):
        assert torch.equal(loss, loss0) and torch.equal(counts, counts0) and torch.equal(dl, dl0)
    assert torch.equal(p_null, p_ones)


@pytest.mark.parametrize("h,H,C", CE_CASES)
def test_upsample_ce_w_all_zero_weight_or_ignored(h, H, C):
    B = 2
    lg, lab, wt = _rnd(B, h, h, C, seed=320 + h, scale=2.0), _labels(B, H, H, C, 321 + H), _weights(B, H, H, 322 + C)
    wt[lab != 255] = 0.0   # every pixel is weight-0 or ignored (the ignored ones keep non-zero weights)
    loss, counts, dl = ops.upsample_ce_w(lg.to(DEV), lab.to(DEV), wt.to(DEV))
    assert loss.item() == 0.0 and float(dl.abs().max()) == 0.0
    assert counts[1].item() == int((lab != 255).sum())


def test_cross_entropy_loss_module_takes_a_weight_map():
    """CrossEntropyLoss.forward(cls_score NCHW at label resolution, label, weight=...) (the API-parity path) against the float64 restatement,
    with and without the map, and with loss_weight."""
    from vfmseg_amd.registry import MODELS
    B, C, H, W = 2, 19, 13, 17
    score, lab, wt = _rnd(B, C, H, W, seed=330, scale=2.0), _labels(B, H, W, C, 331), _weights(B, H, W, 332)
    mod = MODELS.build(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4))
    for w_ in (wt, None):
        ref, _, _ = D.upsample_ce_w(score.permute(0, 2, 3, 1), lab, w_)
        got = mod(score.to(DEV), lab.to(DEV), weight=None if w_ is None else w_.to(DEV), ignore_index=255)
        assert abs(got.item() - 0.4 * ref) < 1e-5 * max(1, abs(ref))


def _teacher_logits(h, C, thr, H):
    """randn * 4 logits whose float64 pseudo-labels leave under 1 % of the pixels undecided (top-2 margin / distance to thr below 1e-5) and
    whose max-prob straddles thr; the seed is picked here, on the float64 side alone."""
    for seed in range(400, 420):
        lg = _rnd(2, h, h, C, seed=seed, scale=4.0)
        ref = D.pseudo_labels(lg, (H, H), thr)
        n = ref["label"].numel()
        if int((~ref["sure_label"]).sum()) < 0.01 * n and ref["n_band"] < 0.01 * n and 0.1 * n < ref["count"] < 0.9 * n:
            return lg, ref
    raise AssertionError("no seed gives a decidable fixture")


@pytest.mark.parametrize("h,H,C", [(8, 32, 19), (5, 13, 7), (8, 32, 7), (5, 13, 19)])
@pytest.mark.parametrize("want_prob", [False, True])
def test_pseudo_label_matches_float64(h, H, C, want_prob):
    thr = 0.8
    lg, ref = _teacher_logits(h, C, thr, H)
    n = ref["label"].numel()
    assert int((~ref["sure_label"]).sum()) < 0.01 * n and ref["n_band"] < 0.01 * n
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    lab, prob = ops.pseudo_label(lg.to(DEV), (H, H), thr, count, want_prob=want_prob)
    sure = ref["sure_label"]
    print(f"[dacs] pseudo_label {h}->{H} C={C}: count {count.item()} (ref {ref['count']}, band {ref['n_band']}), unsure labels {int((~sure).sum())}")
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (2, H, H)
    assert torch.equal(lab.cpu()[sure], ref["label"][sure])
    assert abs(count.item() - ref["count"]) <= ref["n_band"]
    if want_prob:
        assert rel_err(prob, ref["prob"]) < 1e-5
    else:
        assert prob is None
    ops.pseudo_label(lg.to(DEV), (H, H), thr, count)   # the counter accumulates: integer add, the caller resets it
    assert abs(count.item() - 2 * ref["count"]) <= 2 * ref["n_band"]


@pytest.mark.parametrize("h,H", [(8, 32), (5, 13)])
def test_pseudo_label_first_maximum_wins(h, H):
    """classes 2 and 5 are bit-identical copies of class 1 and lie above the rest everywhere: every pixel is an exact three-way tie and
    torch.max returns the first of them."""
    lg = _rnd(2, h, h, 7, seed=430)
    lg[..., 1] = lg[..., 1] + 20.0
    lg[..., 2] = lg[..., 1]
    lg[..., 5] = lg[..., 1]
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    lab, prob = ops.pseudo_label(lg.to(DEV), (H, H), 0.5, count, want_prob=True)
    assert bool((lab == 1).all())
    assert rel_err(prob, torch.full((2, H, H), 1.0 / 3.0)) < 1e-5 and count.item() == 0


def test_class_presence_equals_torch_unique():
    g = torch.Generator().manual_seed(440)
    vals = torch.tensor([0, 3, 18, 255])
    for Hh, Ww in ((13, 17), (16, 32)):   # odd pixel count: scalar loads; even: 16-byte loads
        lab = torch.stack([vals[torch.randint(0, 4, (Hh, Ww), generator=g)], torch.full((Hh, Ww), 18), vals[1:][torch.randint(0, 3, (Hh, Ww), generator=g)],
                           torch.full((Hh, Ww), 255)]).contiguous()
        lab[2][lab[2] == 18] = 3
        bits = ops.class_presence(lab.to(DEV))
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (4, 8)
        got = ops.class_bits_to_lists(bits)
        assert got == D.class_sets(lab), (got, D.class_sets(lab))
        assert got[1] == [18] and got[3] == [255] and got[0] == [0, 3, 18, 255]
        assert torch.equal(ops.class_lists_to_bits(got, DEV), bits)


@pytest.mark.parametrize("Hh,Ww", [(13, 17), (16, 32)])
@pytest.mark.parametrize("top,bottom", [(2, 3), (0, 0), (13, 0)])
@pytest.mark.parametrize("count_kind", ["zero", "total", "between"])
def test_class_mix_equals_the_torch_composition(Hh, Ww, top, bottom, count_kind):
    B = 2
    g = torch.Generator().manual_seed(450 + Hh)
    src, tgt = torch.randn(B, 3, Hh, Ww, generator=g), torch.randn(B, 3, Hh, Ww, generator=g)
    vals = torch.tensor([0, 3, 18, 255])
    src_lbl = vals[torch.randint(0, 4, (B, Hh, Ww), generator=g)].contiguous()
    ps_lbl = torch.randint(0, 19, (B, Hh, Ww), generator=g)
    chosen = [[255, 3], [0]]
    total = B * Hh * Ww
    cnt = {"zero": 0, "total": total, "between": (total * 2) // 7}[count_kind]
    mask_ref = D.class_masks(src_lbl, chosen)
    assert 0 < int(mask_ref.sum()) < total
    img_ref, lbl_ref, w_ref = D.class_mix(src, tgt, src_lbl, ps_lbl, mask_ref, cnt, total, top, bottom)
    count = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    for want_mask in (True, False):
        img, lbl, wgt, mask = ops.class_mix(src.to(DEV), tgt.to(DEV), src_lbl.to(DEV), ps_lbl.to(DEV), ops.class_lists_to_bits(chosen, DEV), count,
                                            total, top, bottom, want_mask=want_mask)
        assert torch.equal(img.cpu(), img_ref) and torch.equal(lbl.cpu(), lbl_ref) and torch.equal(wgt.cpu(), w_ref)
        assert lbl.dtype == torch.int64 and wgt.dtype == torch.float32
        if want_mask:
            assert mask.dtype == torch.uint8 and torch.equal(mask.cpu().long(), mask_ref)
        else:
            assert mask is None
    assert count.item() == cnt   # read, never written


@pytest.mark.parametrize("it", [1, 2, 5000])
def test_ema_update_matches_float64(it):
    """teacher = a * teacher + (1 - a) * student over an odd-sized flat buffer, a = min(1 - 1 / (it + 1), 0.999): one vfm_axpby."""
    n, alpha = 100003, 0.999
    student, teacher = _rnd(n, seed=460), _rnd(n, seed=461)
    ref = D.ema(teacher, student, it, alpha)
    a = min(1 - 1 / (it + 1), alpha)
    t = teacher.to(DEV)
    ops.axpby(student.to(DEV), 1 - a, t, a)
    assert rel_err(t, ref) < 1e-6
