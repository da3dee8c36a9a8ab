"""DACS self-training on the HIP path against tests/golden/dacs.npz (two iterations of the reference's own DACS.forward_train,
tools/gen_dacs_golden.py) and against itself: fused vs composed glue, two backward passes + step vs one update_params."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import dacs_helpers as D  # noqa: E402
from tests import segformer_helpers as S  # noqa: E402
from tests.helpers import rel_err, sl  # noqa: E402
from tests.test_segformer_model_gpu import REIN_BOUNDS  # noqa: E402
from vfmseg_amd import functional as Fh  # noqa: E402
from vfmseg_amd.optim import PEFTOptimWrapperConstructor  # noqa: E402
from vfmseg_amd.precision import set_compute_dtype  # noqa: E402
from vfmseg_amd.registry import MODELS  # noqa: E402
from vfmseg_amd.segmentors import SegDataSample  # noqa: E402
from vfmseg_amd.synth import synth_image, synth_label  # noqa: E402
from vfmseg_amd.uda import fused_default  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "dacs.npz"))


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    set_compute_dtype("bf16")


_CACHE = {}


def _fresh(thr, optim=None):
    """The fixture's model (one per module), back at the recipe's weights with a new optimiser and a teacher yet to be initialised."""
    if "model" not in _CACHE:
        _CACHE["model"] = MODELS.build(D.dacs_config(thr)).to(DEV)
    model = _CACHE["model"]
    missing, unexpected = model.load_state_dict(D.dacs_state_dict(), strict=False)
    assert not unexpected and all(k.startswith("ema_head.") for k in missing), (missing, unexpected)
    model.pseudo_threshold, model.local_iter, model._ema_flat, model.fused, model.keep_mask = float(thr), 0, None, fused_default(), True
    ow = PEFTOptimWrapperConstructor(dict(optimizer=dict(optim or D.OPTIM)))(model)
    assert not any(n.startswith("ema_head.") for n in ow.optimizer.names)
    random.seed(D.PY_SEED)
    np.random.seed(D.NP_SEED)
    return model, ow


def _data():
    if "data" not in _CACHE:
        src, tgt = synth_image(D.BATCH, D.SIZE, seed=D.SRC_SEED).to(DEV), synth_image(D.BATCH, D.SIZE, seed=D.TGT_SEED).to(DEV)
        lab = synth_label(D.BATCH, D.SIZE, seed=D.SRC_SEED)
        _CACHE["data"] = (src, tgt, lab)
    src, tgt, lab = _CACHE["data"]
    return (dict(inputs=src, data_samples=[SegDataSample(gt_sem_seg=lab[i]) for i in range(D.BATCH)]),
            dict(inputs=tgt, data_samples=[SegDataSample(gt_sem_seg=torch.zeros_like(lab[i])) for i in range(D.BATCH)]))


def _iteration(model, ow):
    """forward_train (both backward passes), the state a test wants to see, then the step."""
    img, tgt = _data()
    log = model.forward_train(img, tgt, ow)
    Fh.join_wgrad_stream()
    torch.cuda.synchronize()
    log = {k: float(v) for k, v in log.items()}
    grads = {n: p.grad.detach().clone() for n, p in zip(ow.optimizer.names, ow.optimizer.params)}
    last = dict(model._last)
    ow.step()
    ow.zero_grad()
    return log, grads, last


def _sub(t):
    return t.reshape(D.BATCH, D.SIZE, D.SIZE)[:, ::D.SUB, ::D.SUB].cpu()


def _grad2d(g):
    return g.reshape(g.shape[0], -1) if g.dim() > 1 else g.reshape(-1)


def test_two_iterations_match_the_reference_f32(G):
    """f32 against the reference's forward_train: masks everywhere and mixed_lbl outside the recorded undecided pixels equal, the ratio within
    the recorded band / N, log vars, gradient-group norms and slices within the f32 row of REIN_BOUNDS, the teacher after iteration 1 to 1e-5."""
    ltol, ntol, stol = REIN_BOUNDS["f32"]
    set_compute_dtype("f32")
    model, ow = _fresh(float(G["pseudo_threshold"][0]))
    # the reference's Rein module also owns weights its configuration never uses (no gradient there; not parameters here)
    ours, theirs = set(ow.optimizer.names), set(G["trainable_names"].tolist())
    assert ours <= theirs and theirs - ours <= set(G["it0::no_grad"].tolist()), (sorted(ours - theirs), sorted(theirs - ours))
    for it in range(2):
        k = f"it{it}::"
        log, grads, last = _iteration(model, ow)
        assert sorted(log) == sorted(D.LOG_KEYS)
        ref_log = dict(zip(D.LOG_KEYS, G[k + "log_vars"]))
        count, total, band = (int(v) for v in G[k + "count_total_band"])
        got_count = int(last["count"].item())
        sure = ~torch.from_numpy(G[k + "unsure_sub"])
        lbl_eq = (_sub(last["mixed_lbl"]) == torch.from_numpy(G[k + "mixed_lbl_sub"]).long())
        ps_eq = (_sub(last["pseudo_label"]) == torch.from_numpy(G[k + "pseudo_label_sub"]).long())
        norms = [0.0, 0.0]
        serr = {}
        for n, g in grads.items():
            norms[n.startswith("decode_head.")] += g.double().pow(2).sum().item()
            if k + f"grad_slice::{n}" in G.files:
                serr[n] = rel_err(sl(_grad2d(g)), G[k + f"grad_slice::{n}"])
        nerr = [abs(np.sqrt(a) / b - 1.0) for a, b in zip(norms, G[k + "grad_norms"])]
        lerr = {n: abs(log[n] / ref_log[n] - 1.0) for n in D.LOG_KEYS if "loss" in n}
        aerr = {n: abs(log[n] - ref_log[n]) for n in D.LOG_KEYS if "acc" in n}
        print(f"[parity] dacs f32 iteration {it}: count {got_count} (ref {count}, band {band}, total {total}), label mismatches on decided pixels "
              f"{int((~lbl_eq & sure).sum())} / pseudo {int((~ps_eq & sure).sum())} (undecided {int((~sure).sum())}), loss rel err {lerr}, acc abs err {aerr}, "
              f"grad-norm rel err (backbone, head) {nerr[0]:.2e} {nerr[1]:.2e}, worst of {len(serr)} gradient slices {max(serr.values()):.2e} "
              f"({max(serr, key=serr.get)})")
        assert last["total"] == total
        assert all(float(grads[n].abs().max()) == 0.0 for n in G[k + "no_grad"].tolist() if n in grads)
        assert torch.equal(_sub(last["mask"]).long(), torch.from_numpy(G[k + "mask_sub"]).long())
        assert torch.equal(last["mask"].sum((1, 2)).cpu(), torch.from_numpy(G[k + "mask_sum"]))
        assert bool(lbl_eq[sure].all()) and bool(ps_eq[sure].all())
        assert abs(got_count / total - count / total) <= band / total
        assert max(lerr.values()) <= ltol and max(aerr.values()) <= 2e-3
        assert max(nerr) < ntol and len(serr) > 10
        for n, e in serr.items():
            assert e < stol, (n, e)
    eerr = {n: rel_err(sl(_grad2d(p.data)), G[f"ema_slice::{n}"]) for n, p in model.ema_head.named_parameters()}
    print(f"[parity] dacs f32 teacher after iteration 1: worst slice {max(eerr.values()):.2e} ({max(eerr, key=eerr.get)})")
    assert max(eerr.values()) < 1e-5, eerr
    assert sorted(k for k in model.state_dict() if k.startswith("ema_head.")) == sorted("ema_head." + n for n in S.HEAD_KEYS)


def test_bf16_step_is_finite_and_mixes_exactly(G):
    """bf16: every log var finite, the source branch within the bf16 row of REIN_BOUNDS, and mixed_lbl / mix_weight exactly the torch
    composition of the model's OWN pseudo-labels and counter (the mask is the fixture's: the same seeds draw the same classes)."""
    ltol, _, _ = REIN_BOUNDS["bf16"]
    set_compute_dtype("bf16")
    model, ow = _fresh(float(G["pseudo_threshold"][0]))
    log, grads, last = _iteration(model, ow)
    ref_log = dict(zip(D.LOG_KEYS, G["it0::log_vars"]))
    print(f"[parity] dacs bf16: log vars {log} (ref {ref_log}), count {int(last['count'].item())}")
    assert all(np.isfinite(v) for v in log.values()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert abs(log["decode.loss_src"] / ref_log["decode.loss_src"] - 1.0) <= ltol
    assert abs(log["decode.acc_src"] - ref_log["decode.acc_src"]) <= 0.05
    src, tgt, lab = _CACHE["data"]
    mask = last["mask"].cpu().long()
    assert torch.equal(_sub(mask), torch.from_numpy(G["it0::mask_sub"]).long())
    _, lbl_ref, w_ref = D.class_mix(src.cpu(), tgt.cpu(), lab[:, 0], last["pseudo_label"].cpu(), mask, int(last["count"].item()), last["total"],
                                    D.IGNORE_TOP, D.IGNORE_BOTTOM)
    assert torch.equal(last["mixed_lbl"].cpu(), lbl_ref) and torch.equal(last["mix_weight"].cpu(), w_ref)
    assert 0 < int(last["count"].item()) < last["total"]


def test_fused_and_composed_glue_agree_f32(G, monkeypatch):
    """VFMSEG_DACS_FUSED=0 and 1 give the same log vars to 1e-5 over two iterations in f32."""
    set_compute_dtype("f32")
    logs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("VFMSEG_DACS_FUSED", flag)
        model, ow = _fresh(float(G["pseudo_threshold"][0]))
        assert model.fused == (flag == "1")
        logs[flag] = [_iteration(model, ow)[0] for _ in range(2)]
    print(f"[parity] dacs fused {logs['1']} composed {logs['0']}")
    for a, b in zip(logs["1"], logs["0"]):
        for n in D.LOG_KEYS:
            assert abs(a[n] - b[n]) <= 1e-5 * max(1.0, abs(b[n])), (n, a[n], b[n])


def test_two_backwards_then_step_equal_update_params(G):
    """OptimWrapper.backward twice + step + zero_grad == update_params on the summed loss: parameters to 2e-5, gradients cleared.  AdamW with
    lr 1e-2 and eps 1 (an update that is smooth in the gradient and 40 times the bound, so that a lost or doubled backward pass shows)."""
    set_compute_dtype("f32")
    optim = dict(D.OPTIM, lr=1e-2)
    img, tgt = _data()
    flats = []
    for split in (True, False):
        model, ow = _fresh(float(G["pseudo_threshold"][0]), optim)
        before = ow.optimizer.flat.detach().clone()
        l1 = model.parse_losses(model.forward(img["inputs"], img["data_samples"], mode="loss"))[0]
        l2 = model.parse_losses(model.forward(tgt["inputs"], img["data_samples"], mode="loss"))[0]
        if split:
            ow.backward(ow.scale_loss(l1))
            ow.backward(ow.scale_loss(l2))
            ow.step()
            ow.zero_grad()
        else:
            ow.update_params(l1 + l2)
        assert ow.iter == 1 and ow.optimizer.step_count == 1 and float(ow.optimizer.gflat.abs().max()) == 0.0
        flats.append(ow.optimizer.flat.detach().clone())
        assert float((flats[-1] - before).abs().max()) > 1e-4   # the step moved the parameters
    err = rel_err(flats[0], flats[1])
    print(f"[parity] two backwards + step vs update_params: parameter rel err {err:.2e}")
    assert err < 2e-5
