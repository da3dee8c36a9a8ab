"""Plain-torch restatements (CPU, any float dtype: float64 for references, float32 where a test needs the exact value a kernel
must store) of what csrc/sam.hip computes, of the row softmax pair and of the bicubic resize in csrc/vision.hip.

The materialised SAM attention is   softmax(q_aug @ k_aug^T) @ v_win   per (image, window, head) batch, then `merge_ref`;
tests/test_sam_window_cpu.py pins that decomposition (and its backward through bwd_prep_ref / softmax_bwd_ref / bwd_merge_ref)
to `window_attention_ref`, the restatement of sam_vit.py:273-430 the flash tests already use.

Batch order everywhere: bz = (img * nws * nws + window) * H + head, windows row-major over the grid padded to a multiple of S,
tokens row-major inside a window (tok = iy * S + ix)."""
import math

import torch
import torch.nn.functional as F

from oracle import torch_ref as R


def pad64(n):
    return (n + 63) // 64 * 64


def window_attention_ref(qkv, bias, rel_h, rel_w, nimg, G, S, H, d, dtype=torch.float64):
    """fp64 (or `dtype`): [nimg*G*G, 3*H*d] -> [nimg*G*G, H*d]  (bias None = zero-valued padded tokens)"""
    C = H * d
    x = (qkv if qkv.dtype == dtype else qkv.to(dtype)).view(nimg, G, G, 3 * C)
    if S < G:
        pad = (S - G % S) % S
        Gp = G + pad
        fill = bias.to(dtype) if bias is not None else torch.zeros(3 * C, dtype=dtype)
        xp = fill.view(1, 1, 1, 3 * C).expand(nimg, Gp, Gp, 3 * C).clone()              # padded tokens: qkv = bias
        xp[:, :G, :G] = x
        w = xp.view(nimg, Gp // S, S, Gp // S, S, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, S * S, 3, H, d)
    else:
        Gp = G
        w = x.reshape(nimg, S * S, 3, H, d)
    q, k, v = w.permute(2, 0, 3, 1, 4).unbind(0)                                         # [nb, H, S*S, d]
    attn = (q * d ** -0.5) @ k.transpose(-2, -1)
    rh, rw = R.sam_rel_pos(S, S, rel_h.to(dtype)), R.sam_rel_pos(S, S, rel_w.to(dtype))
    rq = q.reshape(q.shape[0], H, S, S, d)
    attn = attn.view(-1, H, S, S, S, S) + torch.einsum("bnhwc,hkc->bnhwk", rq, rh)[..., None] + torch.einsum("bnhwc,wkc->bnhwk", rq, rw)[..., None, :]
    o = attn.view(-1, H, S * S, S * S).softmax(-1) @ v                                    # [nb, H, S*S, d]
    o = o.permute(0, 2, 1, 3).reshape(-1, S, S, C)
    if S < G:
        o = o.view(nimg, Gp // S, Gp // S, S, S, C).permute(0, 1, 3, 2, 4, 5).reshape(nimg, Gp, Gp, C)[:, :G, :G]
    return o.reshape(nimg * G * G, C)


def relpos_table(rel, S):
    """[L, d] parameter -> [S, S, d] table[i, j] = (re-interpolated) rel[i - j + S - 1], in rel's dtype."""
    return R.sam_rel_pos(S, S, rel)


def _partition(x, fill, nimg, G, S):
    """[nimg*G*G, F] token-major -> ([nimg*nws*nws, S*S, F] windows of the padded grid, padded tokens = fill (None: 0),
    [nws*nws, S*S] bool mask of the tokens inside the G x G grid)"""
    Fd = x.shape[1]
    nws = (G + S - 1) // S
    Gp = nws * S
    f = fill.to(x.dtype) if fill is not None else torch.zeros(Fd, dtype=x.dtype)
    xp = f.view(1, 1, 1, Fd).expand(nimg, Gp, Gp, Fd).clone()
    xp[:, :G, :G] = x.reshape(nimg, G, G, Fd)
    w = xp.view(nimg, nws, S, nws, S, Fd).permute(0, 1, 3, 2, 4, 5).reshape(nimg * nws * nws, S * S, Fd)
    m = torch.zeros(Gp, Gp, dtype=torch.bool)
    m[:G, :G] = True
    inside = m.view(nws, S, nws, S).permute(0, 2, 1, 3).reshape(nws * nws, S * S)
    return w, inside


def window_qkv(qkv, bias, nimg, G, S, H, d):
    """-> q, k, v [nb, S*S, d] (copies: exact in any dtype) and inside [nb, S*S]"""
    C = H * d
    w, inside = _partition(qkv[:, :3 * C], bias, nimg, G, S)
    nw = w.shape[0]
    w = w.view(nw, S * S, 3, H, d).permute(2, 0, 3, 1, 4).reshape(3, nw * H, S * S, d)
    inside = inside.repeat(nimg, 1)[:, None, :].expand(nw, H, S * S).reshape(nw * H, S * S)
    return w[0], w[1], w[2], inside


def prep_ref(qkv, bias, rh, rw, nimg, G, S, H, d, Dq, scale):
    """-> q_aug [nb, S*S, Dq] = [scale q | q.Rh[iy, kh, :] | q.Rw[ix, kw, :] | 0], k_aug = [k | onehot(iy) | onehot(ix) | 0],
    v_win [nb, S*S, d]; rh / rw are the [S, S, d] tables."""
    q, k, v, _ = window_qkv(qkv, bias, nimg, G, S, H, d)
    nb, S2 = q.shape[0], S * S
    dt = q.dtype
    q4 = q.view(nb, S, S, d)
    qa = torch.zeros(nb, S2, Dq, dtype=dt)
    ka = torch.zeros(nb, S2, Dq, dtype=dt)
    qa[..., :d] = q * torch.as_tensor(scale, dtype=dt)
    qa[..., d:d + S] = torch.einsum("bywc,ykc->bywk", q4, rh.to(dt)).reshape(nb, S2, S)
    qa[..., d + S:d + 2 * S] = torch.einsum("bywc,wkc->bywk", q4, rw.to(dt)).reshape(nb, S2, S)
    ka[..., :d] = k
    eye = torch.eye(S, dtype=dt)
    ka[..., d:d + S] = eye[:, None, :].expand(S, S, S).reshape(S2, S)                     # onehot(iy)
    ka[..., d + S:d + 2 * S] = eye[None, :, :].expand(S, S, S).reshape(S2, S)             # onehot(ix)
    return qa, ka, v


def prep_bias_magnitude(qkv, bias, rh, rw, nimg, G, S, H, d):
    """sum_c |q_c| |r_c| of every bias column of q_aug: [nb, S*S, 2S]"""
    qa, _, _ = prep_ref(qkv.abs(), None if bias is None else bias.abs(), rh.abs(), rw.abs(), nimg, G, S, H, d, d + 2 * S, 1.0)
    return qa[..., d:]


def merge_ref(o_win, nimg, G, S, H, d):
    """[nb, >= S*S, d] -> token-major [nimg*G*G, H*d] (window_unpartition + head merge, padded tokens dropped)"""
    nws = (G + S - 1) // S
    o = o_win[:, :S * S].reshape(nimg, nws, nws, H, S, S, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(nimg, nws * S, nws * S, H * d)
    return o[:, :G, :G].reshape(nimg * G * G, H * d)


def bwd_prep_ref(dao, qkv, bias, nimg, G, S, H, d, dp, NP, scale):
    """-> dow [nb, NP, dp], dowT [nb, dp, NP], vp [nb, NP, dp], qsT [nb, dp, NP]: window-partitioned d(out) (0 at padded tokens),
    v and scale*q (bias-valued at padded tokens), zero in the d..dp and S*S..NP pads."""
    C = H * d
    q, _, v, _ = window_qkv(qkv, bias, nimg, G, S, H, d)
    g3 = torch.cat([dao[:, :C]] * 3, 1)
    g, _, _, _ = window_qkv(g3, None, nimg, G, S, H, d)
    nb, S2, dt = q.shape[0], S * S, q.dtype
    dow = torch.zeros(nb, NP, dp, dtype=dt)
    vp = torch.zeros(nb, NP, dp, dtype=dt)
    qs = torch.zeros(nb, NP, dp, dtype=dt)
    dow[:, :S2, :d] = g
    vp[:, :S2, :d] = v
    qs[:, :S2, :d] = q * torch.as_tensor(scale, dtype=dt)
    return dow, dow.transpose(1, 2).contiguous(), vp, qs.transpose(1, 2).contiguous()


def bwd_merge_ref(dqa, dkT, dvT, rh, rw, nimg, G, S, H, d, scale):
    """dQaug [nb, NP, Dq], dkT / dvT [nb, dp, NP] -> token-major dqkv [nimg*G*G, 3*H*d]:
    dq = scale dQaug[:d] + sum_k dQaug[d+k] Rh[iy,k] + sum_k dQaug[d+S+k] Rw[ix,k]; dk / dv read from the transposed operands."""
    nb, S2, dt = dqa.shape[0], S * S, dqa.dtype
    a = dqa[:, :S2]
    a4 = a.view(nb, S, S, -1)
    dq = a[..., :d] * torch.as_tensor(scale, dtype=dt)
    dq = dq + torch.einsum("bywk,ykc->bywc", a4[..., d:d + S], rh.to(dt)).reshape(nb, S2, d)
    dq = dq + torch.einsum("bywk,wkc->bywc", a4[..., d + S:d + 2 * S], rw.to(dt)).reshape(nb, S2, d)
    dk = dkT[:, :d, :S2].transpose(1, 2)
    dv = dvT[:, :d, :S2].transpose(1, 2)
    return torch.cat([merge_ref(t, nimg, G, S, H, d) for t in (dq, dk, dv)], 1)


def _live_rows(rows, rows_per_batch, valid_rows):
    return (torch.arange(rows) % rows_per_batch) < valid_rows


def softmax_ref(scores, rows_per_batch=1, valid_rows=1):
    """float64 softmax of the rows of scores [rows, n]; rows with (row % rows_per_batch) >= valid_rows come out 0 whatever they hold."""
    live = _live_rows(scores.shape[0], rows_per_batch, valid_rows)
    p = torch.zeros(scores.shape, dtype=torch.float64)
    p[live] = scores[live].double().softmax(-1)
    return p


def softmax_bwd_ref(p, dp, rows_per_batch=1, valid_rows=1):
    """float64 p o (dp - sum_j p_j dp_j) with the same dead-row rule (dead rows of p / dp are not read)."""
    live = _live_rows(p.shape[0], rows_per_batch, valid_rows)
    ds = torch.zeros(p.shape, dtype=torch.float64)
    pl, dl = p[live].double(), dp[live].double()
    ds[live] = pl * (dl - (pl * dl).sum(-1, keepdim=True))
    return ds


def bicubic_ref(x, sy, sx):
    """x [Hi, Wi, C] -> float64 [floor(Hi / sy), floor(Wi / sx), C]: ATen's bicubic with source scales (sy, sx)"""
    y = F.interpolate(x.double().permute(2, 0, 1)[None], scale_factor=(1.0 / sy, 1.0 / sx), mode="bicubic", align_corners=False)
    return y[0].permute(1, 2, 0).contiguous()


def _cubic(t):
    A = -0.75
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    return [((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * x1 - (A + 3)) * x1 * x1 + 1,
            ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A]


def bicubic_taps(x, Ho, Wo, sy, sx):
    """The kernel's formula, tap by tap, in float64: src = scale * (dst + 0.5) - 0.5 (not clamped), 4 x 4 taps with border-clamped
    indices, A = -0.75.  -> (out [Ho, Wo, C], sum |w_y| |w_x| |x| [Ho, Wo, C])"""
    Hi, Wi, C = x.shape
    xd = x.double()
    out = torch.zeros(Ho, Wo, C, dtype=torch.float64)
    mag = torch.zeros(Ho, Wo, C, dtype=torch.float64)
    for y in range(Ho):
        fy = sy * (y + 0.5) - 0.5
        iy = math.floor(fy)
        wy = _cubic(fy - iy)
        for xo in range(Wo):
            fx = sx * (xo + 0.5) - 0.5
            ix = math.floor(fx)
            wx = _cubic(fx - ix)
            for a in range(4):
                yy = min(max(iy - 1 + a, 0), Hi - 1)
                for b in range(4):
                    xx = min(max(ix - 1 + b, 0), Wi - 1)
                    out[y, xo] += wy[a] * wx[b] * xd[yy, xx]
                    mag[y, xo] += abs(wy[a] * wx[b]) * xd[yy, xx].abs()
    return out, mag
