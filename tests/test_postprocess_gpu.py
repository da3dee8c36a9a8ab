"""vfm_postprocess_argmax (un-pad, un-flip, bilinear resize to ori_shape, argmax, confusion counts in one pass) against
 - the composition of the existing ops it replaces (strided_copy + resize_bilinear + slide_finalize + confusion_hist): the label
   map byte-identical, the counts equal;
 - float64 on the CPU (F.interpolate bilinear, align_corners=False, in double; argmax; numpy bin counts): the label map equal on
   every pixel whose float64 top-2 gap is at least 1e-4 (at most 0.2 % of a case may be closer; N(0,1) logits at these shapes
   leave at most 2.6e-4 of the pixels there), the counts equal to those recomputed from the kernel's own label map.
Every test runs against both builds of the library (bf16 and the fp16 twin): the entry point is fp32 / uint8 / int64 in both."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vfmseg_amd import lib as L, ops
from vfmseg_amd.precision import set_compute_dtype

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
# (C, (h, w) -> (oh, ow)): identity; non-integer down-scale with ow no multiple of 4 or 16; non-integer up-scale (edge clamping,
# several blocks); ow smaller than one vector store; the channel limit
CASES = [(19, (16, 32), (16, 32)), (19, (23, 37), (16, 29)), (19, (17, 19), (50, 61)), (3, (9, 7), (13, 5)), (32, (40, 24), (29, 47))]
PAD = (1, 4, 2, 3)     # left, right, top, bottom
GAP, MAX_EXCLUDED = 1e-4, 2e-3


@pytest.fixture(autouse=True, params=["bf16", "fp16"])
def _library(request):
    set_compute_dtype(request.param)
    yield
    set_compute_dtype("bf16")


def _unflip(win, flip):
    return win.flip(2) if flip == 1 else win.flip(1) if flip == 2 else win


@functools.lru_cache(maxsize=None)
def _case(C, hw, out, flip):
    """logits of the window (CPU fp32), labels (int64 with 255s and 200s), and the float64 evaluation: argmax and the mask of the
    pixels whose top-2 gap is at least GAP.  Computed once per case, shared by the layouts and the two libraries; never modified."""
    g = torch.Generator().manual_seed(C * 100003 + hw[0] * 1009 + hw[1] * 31 + out[0] * 7 + out[1] + 17 * flip)
    win = torch.randn(C, *hw, generator=g)
    ref = F.interpolate(_unflip(win, flip).double()[None], size=out, mode="bilinear", align_corners=False)[0]
    top2 = ref.topk(2, dim=0).values
    sure = (top2[0] - top2[1]) >= GAP
    label = torch.randint(0, C, out, generator=g)
    r = torch.rand(out, generator=g)
    label[r < 0.15] = 255
    label[(r >= 0.15) & (r < 0.25)] = 200
    return win, label, ref.argmax(0).to(torch.uint8), sure


def _place(win, padded):
    """(one image's [C, Hm, Wm] view on the GPU, window): the window alone, or inside batch element 1 of a NaN-filled padded map
    whose row stride is larger than w - a read outside the window shows up as NaN in the sample."""
    C, h, w = win.shape
    if not padded:
        return win.to(DEV).contiguous(), (0, 0, h, w)
    pl, pr, pt, pb = PAD
    m = torch.full((2, C, pt + h + pb, pl + w + pr), NAN, device=DEV)
    m[1, :, pt:pt + h, pl:pl + w] = win.to(DEV)
    return m[1], (pt, pl, h, w)


def _composed(img, window, flip, out, label=None, hist=None, nc=None):
    """today's chain: postprocess_result's ops, then metrics.confusion's"""
    C = img.shape[0]
    y0, x0, h, w = window
    win = img[:, y0:y0 + h, x0:x0 + w]
    cur = torch.empty(1, C, h, w, dtype=torch.float32, device=DEV)
    src, sstr = win, [win.stride(0), win.stride(1), win.stride(2)]
    if flip == 1:
        src, sstr = win[:, :, w - 1:], [win.stride(0), win.stride(1), -win.stride(2)]
    elif flip == 2:
        src, sstr = win[:, h - 1:, :], [win.stride(0), -win.stride(1), win.stride(2)]
    ops.strided_copy(src, cur, (C, h, w), sstr, (h * w, w, 1))
    if tuple(out) != (h, w):
        res = torch.empty(1, C, out[0], out[1], dtype=torch.float32, device=DEV)
        ops.resize_bilinear(cur, True, 1, h, w, C, res, 1, tuple(out))
        cur = res
    am = torch.empty(1, out[0], out[1], dtype=torch.uint8, device=DEV)
    ops.slide_finalize(cur, None, am)
    if hist is not None:
        ops.confusion_hist(am.reshape(-1), label.reshape(-1).contiguous(), hist, nc, 255)
    return am[0]


def _counts(pred, label, nc):
    """numpy bin counts of (label row, prediction) with the binning rule of vfm_confusion_hist"""
    pred, label = pred.reshape(-1).astype(np.int64), label.reshape(-1).astype(np.int64)
    keep = (label != 255) & (pred < nc)
    row = np.where((label >= 0) & (label < nc), label, nc)
    return np.bincount(row[keep] * nc + pred[keep], minlength=(nc + 1) * nc)


@pytest.mark.parametrize("flip", [0, 1, 2], ids=["noflip", "hflip", "vflip"])
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"C{c[0]}_{c[1][0]}x{c[1][1]}_to_{c[2][0]}x{c[2][1]}")
def test_label_map_and_counts(case, padded, flip):
    C, hw, out = case
    nc = C
    win, label, ref_am, sure = _case(C, hw, out, flip)
    img, window = _place(win, padded)
    want_hist = torch.zeros((nc + 1) * nc, dtype=torch.int64, device=DEV)
    lab64 = label.to(DEV)
    want = _composed(img, window, flip, out, lab64, want_hist, nc)
    for lab in (lab64, lab64.to(torch.uint8)):
        hist = torch.zeros((nc + 1) * nc, dtype=torch.int64, device=DEV)
        pred = ops.postprocess_argmax(img, window, flip, out, label=lab, hist=hist, num_classes=nc)
        assert pred.dtype == torch.uint8 and tuple(pred.shape) == tuple(out)
        assert torch.equal(pred, want), f"{(pred != want).sum().item()} pixels differ from the composed ops"
        assert torch.equal(hist, want_hist)
        p = pred.cpu()
        excluded = 1.0 - sure.double().mean().item()
        assert excluded <= MAX_EXCLUDED, excluded
        assert torch.equal(p[sure], ref_am[sure]), f"{(p[sure] != ref_am[sure]).sum().item()} sure pixels differ from float64"
        np.testing.assert_array_equal(hist.cpu().numpy(), _counts(p.numpy(), label.numpy(), nc))
        assert hist[nc * nc:].sum().item() > 0      # the labels equal to 200 landed in row nc
        # accumulation: a second call doubles the counts
        ops.postprocess_argmax(img, window, flip, out, label=lab, hist=hist, num_classes=nc)
        assert torch.equal(hist, 2 * want_hist)
        # an all-ignore map leaves the counts alone
        ops.postprocess_argmax(img, window, flip, out, label=torch.full_like(lab, 255), hist=hist, num_classes=nc)
        assert torch.equal(hist, 2 * want_hist)
    # without a histogram: the same label map
    assert torch.equal(ops.postprocess_argmax(img, window, flip, out), want)


def test_identity_passes_values_through():
    """Same size: every value passes through exactly, so an infinite neighbour cannot turn a sample into NaN and the label map is
    torch's argmax of the window."""
    C, hw, out = CASES[0]
    win = _case(C, hw, out, 0)[0].clone()
    win[3, 5, 7] = float("inf")
    win[4, 5, 9] = float("-inf")
    for padded in (False, True):
        img, window = _place(win, padded)
        pred = ops.postprocess_argmax(img, window, 0, out)
        assert torch.equal(pred.cpu(), win.argmax(0).to(torch.uint8))
        assert torch.equal(pred, _composed(img, window, 0, out))


@pytest.mark.parametrize("flip", [0, 1, 2])
def test_ties_first_index_wins(flip):
    C, (h, w) = 19, (16, 32)
    g = torch.Generator().manual_seed(5)
    win = torch.randint(0, 5, (C, h, w), generator=g).float()
    a = torch.randint(0, C - 1, (h, w), generator=g)
    b = (a + 1 + (torch.rand(h, w, generator=g) * (C - 1 - a)).long()).clamp(max=C - 1)     # a second, later channel
    win.scatter_(0, a[None], 10.0)
    win.scatter_(0, b[None], 10.0)
    assert (b > a).all() and (b < C).all()
    img, window = _place(win, True)
    pred = ops.postprocess_argmax(img, window, flip, (h, w))
    assert torch.equal(pred.cpu(), _unflip(a[None], flip)[0].to(torch.uint8))
    assert torch.equal(pred, _composed(img, window, flip, (h, w)))


def test_grid_stride_loop():
    """More output pixels than one pass of the capped grid covers (2048 blocks x 256 threads x 4 pixels)."""
    C, hw, out = 3, (17, 19), (1500, 1501)
    win, label, ref_am, sure = _case(C, hw, out, 1)
    img, window = _place(win, True)
    hist, want_hist = (torch.zeros((C + 1) * C, dtype=torch.int64, device=DEV) for _ in range(2))
    lab = label.to(DEV).to(torch.uint8)
    pred = ops.postprocess_argmax(img, window, 1, out, label=lab, hist=hist, num_classes=C)
    assert torch.equal(pred, _composed(img, window, 1, out, lab, want_hist, C)) and torch.equal(hist, want_hist)
    assert 1.0 - sure.double().mean().item() <= MAX_EXCLUDED
    assert torch.equal(pred.cpu()[sure], ref_am[sure])
    np.testing.assert_array_equal(hist.cpu().numpy(), _counts(pred.cpu().numpy(), label.numpy(), C))


def test_bad_arguments_are_errors():
    out = (8, 8)
    with pytest.raises(L.HipError, match="C=33"):
        ops.postprocess_argmax(torch.zeros(33, 8, 8, device=DEV), (0, 0, 8, 8), 0, out)
    x = torch.zeros(19, 8, 8, device=DEV)
    lab = torch.zeros(64, dtype=torch.int64, device=DEV)
    with pytest.raises(L.HipError, match="num_classes 65"):
        ops.postprocess_argmax(x, (0, 0, 8, 8), 0, out, label=lab, hist=torch.zeros(66 * 65, dtype=torch.int64, device=DEV), num_classes=65)
    with pytest.raises(L.HipError, match="aligned pred"):
        ops.postprocess_argmax(x, (0, 0, 8, 8), 0, out, pred=torch.zeros(80, dtype=torch.uint8, device=DEV)[1:65])
    with pytest.raises(L.HipError, match="aligned label"):
        ops.postprocess_argmax(x, (0, 0, 8, 8), 0, out, label=torch.zeros(80, dtype=torch.uint8, device=DEV)[1:65],
                               hist=torch.zeros(20 * 19, dtype=torch.int64, device=DEV), num_classes=19)
    with pytest.raises(L.HipError, match="without label"):
        ops.postprocess_argmax(x, (0, 0, 8, 8), 0, out, hist=torch.zeros(20 * 19, dtype=torch.int64, device=DEV), num_classes=19)
    with pytest.raises(L.HipError, match="empty window"):
        ops.postprocess_argmax(x, (0, 0, 0, 8), 0, out)
    with pytest.raises(L.HipError, match="outside"):
        ops.postprocess_argmax(x, (1, 0, 8, 8), 0, out)
