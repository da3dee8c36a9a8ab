"""Pins the float64 restatements of tests/sam_window_helpers.py (what tests/test_sam_window_gpu.py holds the kernels to) to the
oracle: the materialised decomposition  softmax(q_aug k_aug^T) v_win -> merge  and its hand-written backward against
`window_attention_ref` (sam_vit.py:273-430 restated) and its autograd, and `bicubic_ref` (ATen) against the kernel's 4 x 4-tap formula."""
import pytest
import torch

from tests import sam_window_helpers as W
from tests.helpers import rel_err

CASES = [(14, 20, 2, 2, 8, 27), (6, 15, 1, 3, 10, 13), (7, 7, 2, 2, 16, 27)]   # S, G, nimg, H, d, L (L != 2S-1 for the last two)


def _inputs(S, G, nimg, H, d, L):
    g = torch.Generator().manual_seed(1000 * S + G)
    C = H * d
    qkv = torch.randn(nimg * G * G, 3 * C, generator=g, dtype=torch.float64) * 1.5
    bias = torch.randn(3 * C, generator=g, dtype=torch.float64) * 0.5 + 0.25             # non-zero: padded tokens are real keys
    rel_h, rel_w = torch.randn(L, d, generator=g, dtype=torch.float64) * 0.3, torch.randn(L, d, generator=g, dtype=torch.float64) * 0.3
    dout = torch.randn(nimg * G * G, C, generator=g, dtype=torch.float64)
    return qkv, bias, rel_h, rel_w, dout


@pytest.mark.parametrize("S,G,nimg,H,d,L", CASES)
def test_materialised_decomposition_equals_window_attention(S, G, nimg, H, d, L):
    qkv, bias, rel_h, rel_w, _ = _inputs(S, G, nimg, H, d, L)
    rh, rw = W.relpos_table(rel_h, S), W.relpos_table(rel_w, S)
    Dq = W.pad64(d + 2 * S)
    qa, ka, vw = W.prep_ref(qkv, bias, rh, rw, nimg, G, S, H, d, Dq, d ** -0.5)
    p = (qa @ ka.transpose(1, 2)).softmax(-1)
    got = W.merge_ref(p @ vw, nimg, G, S, H, d)
    ref = W.window_attention_ref(qkv, bias, rel_h, rel_w, nimg, G, S, H, d)
    e = rel_err(got, ref)
    print(f"[sam window cpu S={S} G={G}] decomposition vs window attention rel err {e:.2e}")
    assert e < 1e-12, e


@pytest.mark.parametrize("S,G,nimg,H,d,L", CASES)
def test_materialised_backward_equals_autograd(S, G, nimg, H, d, L):
    """dqkv through bwd_prep_ref -> dP = dO V^T -> softmax_bwd_ref -> dV^T = dO^T P, dK^T = (scale q)^T dS, dQaug = dS Kaug -> bwd_merge_ref
    (the products SamEngine.attention_bwd runs as GEMMs, padded to NP rows / dp channels) against autograd of window_attention_ref."""
    qkv, bias, rel_h, rel_w, dout = _inputs(S, G, nimg, H, d, L)
    rh, rw = W.relpos_table(rel_h, S), W.relpos_table(rel_w, S)
    S2, Dq, NP, dp, scale = S * S, W.pad64(d + 2 * S), W.pad64(S * S), W.pad64(d), d ** -0.5
    qa, ka, vw = W.prep_ref(qkv, bias, rh, rw, nimg, G, S, H, d, Dq, scale)
    nb = qa.shape[0]
    p = torch.zeros(nb, NP, NP, dtype=torch.float64)
    p[:, :S2, :S2] = (qa @ ka.transpose(1, 2)).softmax(-1)
    dow, dowT, vp, qsT = W.bwd_prep_ref(dout, qkv, bias, nimg, G, S, H, d, dp, NP, scale)
    assert torch.equal(dowT, dow.transpose(1, 2)) and torch.equal(vp[:, :S2, :d], vw) and torch.equal(qsT[:, :d, :S2].transpose(1, 2), qa[..., :d])
    dP = torch.full((nb, NP, NP), float("nan"), dtype=torch.float64)
    dP[:, :S2] = dow[:, :S2] @ vp.transpose(1, 2)
    dS = W.softmax_bwd_ref(p.view(nb * NP, NP)[:, :S2], dP.view(nb * NP, NP)[:, :S2], NP, S2)
    dS = torch.cat([dS, torch.zeros(nb * NP, NP - S2, dtype=torch.float64)], 1).view(nb, NP, NP)
    dvT, dkT = dowT @ p, qsT @ dS
    kaP = torch.zeros(nb, NP, Dq, dtype=torch.float64)
    kaP[:, :S2] = ka
    got = W.bwd_merge_ref(dS @ kaP, dkT, dvT, rh, rw, nimg, G, S, H, d, scale)
    x = qkv.clone().requires_grad_(True)
    W.window_attention_ref(x, bias, rel_h, rel_w, nimg, G, S, H, d).backward(dout)
    e = rel_err(got, x.grad)
    print(f"[sam window cpu S={S} G={G}] hand-written backward vs autograd rel err {e:.2e}")
    assert torch.isfinite(got).all() and e < 1e-12, e


def test_softmax_refs_follow_autograd_and_the_dead_row_rule():
    g = torch.Generator().manual_seed(3)
    s = torch.randn(8, 37, generator=g) * 5
    s[3] = float("nan")
    s[7] = float("nan")                                                                   # rows 3 and 7 are dead with (4, 3)
    p = W.softmax_ref(s, 4, 3)
    assert torch.equal(p[3], torch.zeros(37, dtype=torch.float64)) and torch.isfinite(p).all()
    live = [0, 1, 2, 4, 5, 6]
    x = s[live].double().requires_grad_(True)
    dp = torch.randn(8, 37, generator=g).double()
    x.softmax(-1).backward(dp[live])
    ds = W.softmax_bwd_ref(p, dp, 4, 3)
    assert rel_err(ds[live], x.grad) < 1e-12 and ds[3].abs().max() == 0 and ds[7].abs().max() == 0


@pytest.mark.parametrize("s,hp,wp", [(5, 7, 3), (6, 2, 11), (4, 4, 9), (3, 1, 1), (37, 5, 5)])
def test_bicubic_ref_is_the_kernels_formula(s, hp, wp):
    x = torch.randn(s, s, 3, generator=torch.Generator().manual_seed(s), dtype=torch.float64)
    sy, sx = s / (hp + 0.1), s / (wp + 0.1)
    ref = W.bicubic_ref(x, sy, sx)
    taps, mag = W.bicubic_taps(x, hp, wp, sy, sx)
    assert ref.shape == (hp, wp, 3)
    e = (ref - taps).abs().max().item()
    print(f"[bicubic cpu {s}->{hp}x{wp}] ATen float64 vs 4x4 taps max diff {e:.1e}")
    assert e < 1e-13 and (mag >= taps.abs() - 1e-15).all()
