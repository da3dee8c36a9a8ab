"""Per-kernel numerics on a real MI355X: every C-ABI entry point against a plain PyTorch fp32 CPU reference."""
import math

import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from vfmseg_amd import ops  # noqa: E402

DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def test_cast_transpose_strided():
    x = rnd(37, 70, seed=1)
    cs = rnd(70, seed=2)
    y = torch.empty(37, 70, dtype=torch.bfloat16, device=DEV)
    ops.cast(x.to(DEV), y, cs.to(DEV))
    assert relerr(y.float(), (x * cs).bfloat16().float()) < 1e-6
    # column-slice destination
    big = torch.zeros(37, 128, dtype=torch.float32, device=DEV)
    ops.cast(x.to(DEV), big[:, 16:86])
    assert torch.equal(big[:, 16:86].cpu(), x) and big[:, :16].abs().sum() == 0
    t = torch.full((70, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.transpose(x.to(DEV), t, pad_rows=64)
    assert torch.equal(t[:, :37].float().cpu(), x.t().bfloat16().float()) and t[:, 37:].abs().sum() == 0
    w = rnd(6, 5, 2, 2, seed=3)
    out = torch.empty(2, 2, 5, 6, dtype=torch.float32, device=DEV)
    ops.permute_copy(w.to(DEV), (2, 3, 1, 0), out)
    assert torch.equal(out.cpu(), w.permute(2, 3, 1, 0).contiguous())


def test_colsum_axpby_masks():
    x = rnd(1000, 130, seed=4)
    out = torch.ones(130, device=DEV)
    ops.colsum(x.to(DEV), out, accumulate=True)
    assert relerr(out, x.sum(0) + 1) < 1e-5
    y = rnd(999, seed=5).to(DEV)
    x2 = rnd(999, seed=6).to(DEV)
    ref = 2.0 * x2 + 0.5 * y
    ops.axpby(x2, 2.0, y, 0.5)
    assert relerr(y, ref) < 1e-6
    m = torch.empty(1 << 20, dtype=torch.float32, device=DEV)
    ops.dropout_mask(m, 0.1, seed=123)
    keep = (m > 0).float().mean().item()
    assert abs(keep - 0.9) < 3e-3 and abs(m.max().item() - 1 / 0.9) < 1e-6
    m2 = torch.empty(1 << 20, dtype=torch.float32, device=DEV)
    ops.dropout_mask(m2, 0.1, seed=123)
    assert torch.equal(m, m2)  # counter-based: reproducible
    src = rnd(64, 48, seed=7)
    msk = (rnd(4, 48, seed=8) > 0).float() * 2
    dst = torch.empty(64, 48, dtype=torch.float32, device=DEV)
    ops.mul_mask(src.to(DEV), msk.to(DEV), dst, rows_per_group=16)
    assert relerr(dst, src * msk.repeat_interleave(16, 0)) < 1e-6


def test_geglu_masktoken():
    h = rnd(50, 96, seed=9)
    out = torch.empty(50, 48, device=DEV)
    ops.geglu_fwd(h.to(DEV), out)
    a, g = h.chunk(2, -1)
    assert relerr(out, a * F.gelu(g)) < 1e-5
    hh = h.clone().requires_grad_(True)
    a, g = hh.chunk(2, -1)
    do = rnd(50, 48, seed=10)
    (a * F.gelu(g)).backward(do)
    dh = torch.empty(50, 96, device=DEV)
    ops.geglu_bwd(h.to(DEV), do.to(DEV), dh)
    assert relerr(dh, hh.grad) < 1e-5
    x = rnd(40, 64, seed=11)
    keep = (rnd(40, seed=12) > -0.5)
    tok = rnd(64, seed=13)
    o = torch.empty(40, 64, device=DEV)
    ops.mask_token_fwd(x.to(DEV), keep.to(torch.uint8).to(DEV), tok.to(DEV), o)
    assert torch.equal(o.cpu(), torch.where(keep[:, None], x, tok[None]))
    dx = torch.empty(40, 64, device=DEV)
    dt = torch.empty(64, device=DEV)
    ops.mask_token_bwd(x.to(DEV), keep.to(torch.uint8).to(DEV), dx, dt)
    assert relerr(dx, x * keep[:, None]) < 1e-6 and relerr(dt, (x * (~keep)[:, None]).sum(0)) < 1e-5


def test_vector_forms_of_mul_mask_and_geglu_equal_the_scalar_kernels():
    """The eight-columns-per-thread forms (any mix of the 16-bit type and fp32 for mul_mask; 16-bit GEGLU forward / backward) against the
    element-per-thread kernels, which an unaligned leading dimension still selects: same arithmetic, so the same bits."""
    rows, C = 300, 512
    bf = torch.bfloat16
    for sdt, mdt, ddt in ((bf, torch.float32, bf), (torch.float32, torch.float32, torch.float32), (torch.float32, bf, torch.float32),
                          (bf, torch.float32, torch.float32), (torch.float32, torch.float32, bf), (torch.float32, bf, bf), (bf, bf, torch.float32)):
        for rpg in (1, 20):
            src = rnd(rows, C, seed=160).to(sdt).to(DEV)
            msk = ((rnd((rows + rpg - 1) // rpg, C, seed=161) > 0).float() * 1.25).to(mdt).to(DEV)
            fast = torch.empty(rows, C, dtype=ddt, device=DEV)
            ops.mul_mask(src, msk, fast, rows_per_group=rpg)
            wide = torch.empty(rows, C + 4, dtype=ddt, device=DEV)          # ld % 8 != 0: the scalar kernel
            ops.mul_mask(src, msk, wide[:, :C], rows_per_group=rpg)
            assert torch.equal(fast, wide[:, :C]), (sdt, mdt, ddt, rpg)
            ref = src.float() * msk.float().repeat_interleave(rpg, 0)[:rows]
            assert torch.equal(fast.float(), ref.to(ddt).float())
    h = rnd(rows, 2 * C, seed=162).to(bf).to(DEV)
    do = rnd(rows, C, seed=163).to(bf).to(DEV)
    out, dh = torch.empty(rows, C, dtype=bf, device=DEV), torch.empty(rows, 2 * C, dtype=bf, device=DEV)
    ops.geglu_fwd(h, out)
    ops.geglu_bwd(h, do, dh)
    out_s, dh_s = torch.empty(rows, C + 4, dtype=bf, device=DEV), torch.empty(rows, 2 * C + 4, dtype=bf, device=DEV)
    ops.geglu_fwd(h, out_s[:, :C])
    ops.geglu_bwd(h, do, dh_s[:, :2 * C])
    assert torch.equal(out, out_s[:, :C]) and torch.equal(dh, dh_s[:, :2 * C])
    a, g = h.float().chunk(2, -1)
    assert relerr(out.float(), a * F.gelu(g)) < 1e-2


@pytest.mark.parametrize("C", [256, 1024])
def test_layernorm(C):
    rows = 77
    x = rnd(rows, C, seed=14, scale=2.0) + 0.5
    w, b = rnd(C, seed=15) * 0.1 + 1, rnd(C, seed=16) * 0.1
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), wr, br, 1e-6)
    dy = rnd(rows, C, seed=17)
    ref.backward(dy)
    y = torch.empty(rows, C, device=DEV)
    stats = torch.empty(rows, 2, device=DEV)
    ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, y, stats)
    assert relerr(y, ref) < 1e-5
    yb = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, yb, None)
    assert relerr(yb.float(), ref) < 1e-2
    dx = torch.ones(rows, C, device=DEV)
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ops.layernorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), stats, dx, accumulate_dx=True, dw=dw, db=db)
    assert relerr(dx - 1, xr.grad) < 2e-5
    assert relerr(dw, wr.grad) < 2e-5 and relerr(db, br.grad) < 2e-5


def test_elementwise_bf16_vector_paths():
    """The 8-elements-per-lane bf16 forms of dropout mask / mask multiply / activation-gradient multiply / SwiGLU (aligned rows
    inside wider buffers) against the scalar forms on a one-element-shifted (misaligned) copy of the same data and against torch."""
    rows, C, ld = 37, 256, 264
    def wide(t, shift=0):  # bf16 [rows, C] view inside a [rows, ld] buffer; shift=1 misaligns it -> scalar kernels
        buf = torch.zeros(rows * ld + 8, dtype=torch.bfloat16, device=DEV)
        v = buf[shift:shift + rows * ld].view(rows, ld)[:, :C]
        v.copy_(t)
        return v
    x, y = rnd(rows, C, seed=90).bfloat16().to(DEV), rnd(rows, C, seed=91).bfloat16().to(DEV)
    # dropout mask: identical counter-based values from both forms
    m8, m1 = torch.empty(rows * C, dtype=torch.bfloat16, device=DEV), torch.empty(rows * C + 1, dtype=torch.bfloat16, device=DEV)
    ops.dropout_mask(m8, 0.3, 1234, offset=77)
    ops.dropout_mask(m1[1:], 0.3, 1234, offset=77)
    assert torch.equal(m8, m1[1:]) and 0.6 < (m8 > 0).float().mean() < 0.8
    mask = m8.view(rows, C)
    for shift in (0, 1):
        out = wide(torch.zeros(rows, C), shift)
        ops.mul_mask(wide(x, shift), wide(mask, shift), out)
        assert relerr(out.float(), x.float() * mask.float()) < 1e-2
        for act, fn in ((ops.ACT_GELU, lambda t: 0.5 * (1 + torch.erf(t / 2 ** 0.5)) + t * torch.exp(-0.5 * t * t) / (2 * 3.141592653589793) ** 0.5),
                        (ops.ACT_RELU, lambda t: (t > 0).double()), (ops.ACT_QGELU, lambda t: torch.sigmoid(1.702 * t) * (1 + 1.702 * t * (1 - torch.sigmoid(1.702 * t))))):
            ops.act_grad_mul(wide(x, shift), wide(y, shift), out, act)
            assert relerr(out.float(), x.double().cpu() * fn(y.double().cpu())) < 1.2e-2, (shift, act)
    # SwiGLU: h = [a | g] bf16, fp32 product (EVA02) and bf16 product; backward with fp32 dout
    h = rnd(rows, 2 * C, seed=92).bfloat16().to(DEV)
    a, g = h[:, :C].double().cpu(), h[:, C:].double().cpu()
    ref = a * torch.sigmoid(a) * g
    of, ob = torch.empty(rows, C, device=DEV), torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    ops.swiglu_fwd(h, of, C)
    ops.swiglu_fwd(h, ob, C)
    assert relerr(of, ref) < 1e-5 and relerr(ob.float(), ref) < 1e-2
    dout = rnd(rows, C, seed=93).to(DEV)
    dh = torch.empty(rows, 2 * C, dtype=torch.bfloat16, device=DEV)
    ops.swiglu_bwd(h, dout, dh, C)
    sg = torch.sigmoid(a)
    d = dout.double().cpu()
    assert relerr(dh[:, :C].float(), d * g * sg * (1 + a * (1 - sg))) < 1e-2 and relerr(dh[:, C:].float(), d * a * sg) < 1e-2


def test_rope_vector_path():
    """EVA02 RoPE (eva_02.py:119-160): the 8-columns-per-lane bf16 form against the scalar form (same data, misaligned by one
    element) and against the rotation written out in torch; inverse = transpose."""
    rows, np_, H, d = 3 * 16, 16, 4, 64
    ncols = H * d
    x = rnd(rows, ncols, seed=95).bfloat16()
    ang = rnd(np_, d // 2, seed=96)
    cos_t = torch.cos(ang).repeat_interleave(2, dim=1).contiguous().to(DEV)
    sin_t = torch.sin(ang).repeat_interleave(2, dim=1).contiguous().to(DEV)
    xv = x.float().view(rows, H, d // 2, 2)
    t = torch.arange(rows) % np_
    c, s_ = torch.cos(ang)[t][:, None, :], torch.sin(ang)[t][:, None, :]
    ref = torch.stack([xv[..., 0] * c - xv[..., 1] * s_, xv[..., 1] * c + xv[..., 0] * s_], dim=-1).view(rows, ncols)
    buf = torch.zeros(rows * ncols + 8, dtype=torch.bfloat16, device=DEV)
    outs = []
    for shift in (0, 1):
        v = buf[shift:shift + rows * ncols].view(rows, ncols)
        v.copy_(x)
        ops.rope(v, rows, np_, ncols, d, cos_t, sin_t)
        outs.append(v.clone())
        assert relerr(v.float(), ref) < 1e-2
        ops.rope(v, rows, np_, ncols, d, cos_t, sin_t, inverse=True)
        assert relerr(v.float(), x.float()) < 2e-2
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("C,ld", [(2730, 2752), (1366, 1366), (2731, 2752)])
def test_layernorm_wide_ragged(C, ld):
    """EVA02's SwiGLU sub-LN.  By the dispatchers of csrc/norm.hip: at (2730, 2752) and the odd (2731, 2752) the calls whose operands all
    sit in the 2752-wide buffers (the 16-bit forward, both backwards) take the padded-pitch kernels k_ln_fwd_v4t / k_ln_bwd_v4t (the pitch
    is a multiple of 4 and covers the partly valid last piece); the float32 forward writes a contiguous y of pitch C and so takes the
    pair-vectorised k_ln_fwd_v2 at C = 2730 and the scalar k_ln_fwd<float, 48> at C = 2731.  (1366, 1366), whose pitch is only even,
    takes k_ln_fwd_v2 / k_ln_bwd_v2 throughout.  No backward here reaches the scalar kernel (tests/test_norm_gpu.py does)."""
    rows = 70
    x = rnd(rows, C, seed=24, scale=1.5) + 0.3
    w, b = rnd(C, seed=25) * 0.1 + 1, rnd(C, seed=26) * 0.1
    xr = x.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), w, b, 1e-5)
    dy = rnd(rows, C, seed=27)
    ref.backward(dy)
    xw = torch.zeros(rows, ld, device=DEV)
    xw[:, :C] = x.to(DEV)
    yw = torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(rows, 2, device=DEV)
    ops.layernorm_fwd(xw[:, :C], w.to(DEV), b.to(DEV), 1e-5, yw[:, :C], stats)
    assert relerr(yw[:, :C].float(), ref) < 1e-2 and (yw[:, C:] == 7.0).all()
    yf = torch.empty(rows, C, device=DEV)
    ops.layernorm_fwd(xw[:, :C], w.to(DEV), b.to(DEV), 1e-5, yf, None)
    assert relerr(yf, ref) < 1e-5
    for dt in (torch.float32, torch.bfloat16):
        dyw = torch.zeros(rows, ld, dtype=dt, device=DEV)
        dyw[:, :C] = dy.to(DEV).to(dt)
        dxw = torch.full((rows, ld), 3.0, device=DEV)
        ops.layernorm_bwd(dyw[:, :C], xw[:, :C], w.to(DEV), stats, dxw[:, :C], accumulate_dx=False)
        xr2 = x.clone().requires_grad_(True)
        F.layer_norm(xr2, (C,), w, b, 1e-5).backward(dyw[:, :C].float().cpu())
        assert relerr(dxw[:, :C], xr2.grad) < 3e-5 and (dxw[:, C:] == 3.0).all()
        ops.layernorm_bwd(dyw[:, :C], xw[:, :C], w.to(DEV), stats, dxw[:, :C], accumulate_dx=True)
        assert relerr(dxw[:, :C], 2 * xr2.grad) < 3e-5


@pytest.mark.parametrize("C", [1024, 1280])
def test_layernorm_fused_variants(C):
    """LN forward + LoRA dropout and LN backward + scaled bf16 copy: bit-identical to the separate kernels they replace."""
    rows = 133
    x = (rnd(rows, C, seed=70, scale=2.0) + 0.5).to(DEV)
    w, b = (rnd(C, seed=71) * 0.1 + 1).to(DEV), (rnd(C, seed=72) * 0.1).to(DEV)
    y0 = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    st0 = torch.empty(rows, 2, device=DEV)
    ops.layernorm_fwd(x, w, b, 1e-6, y0, st0)
    m0 = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    ops.dropout_mask(m0, 0.1, 1234, offset=5 * rows * C)
    d0 = torch.empty_like(y0)
    ops.mul_mask(y0, m0, d0)
    big = torch.zeros(rows, C + 64, dtype=torch.bfloat16, device=DEV)   # y lands in a strided view, as in the engine
    st1 = torch.empty(rows, 2, device=DEV)
    m1, d1 = torch.empty_like(m0), torch.empty_like(d0)
    ops.layernorm_dropout_fwd(x, w, b, 1e-6, big[:, :C], st1, d1, m1, 0.1, 1234, offset=5 * rows * C)
    assert torch.equal(big[:, :C], y0) and torch.allclose(st1, st0, rtol=1e-6, atol=1e-7) and torch.equal(m1, m0)
    assert torch.equal(d1.view(torch.int16), d0.view(torch.int16))
    assert 0.05 < (m1 == 0).float().mean().item() < 0.15
    dy = rnd(rows, C, seed=73).to(DEV).bfloat16()
    g = (rnd(C, seed=74) * 0.3 + 1).to(DEV)
    dx0 = torch.ones(rows, C, device=DEV)
    ops.layernorm_bwd(dy, x, w, st0, dx0, accumulate_dx=True)
    t0 = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    ops.cast(dx0, t0, g)
    dx1 = torch.ones(rows, C, device=DEV)
    t1 = torch.empty_like(t0)
    ops.layernorm_bwd_scaled(dy, x, w, st0, dx1, t1, g, accumulate_dx=True)
    assert torch.allclose(dx1, dx0, rtol=1e-6, atol=1e-7) and relerr(t1.float(), t0.float()) < 1e-2


@pytest.mark.parametrize("C,G,act", [(1024, 32, 2), (256, 32, 1), (64, 32, 1), (128, 32, 0)])
def test_groupnorm(C, G, act):
    B, P = 2, 32 * 32
    x = rnd(B, P, C, seed=18, scale=1.5) + 0.3
    w, b = rnd(C, seed=19) * 0.1 + 1, rnd(C, seed=20) * 0.1
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.group_norm(xr.permute(0, 2, 1), G, wr, br, 1e-5).permute(0, 2, 1)
    ref = F.gelu(ref) if act == 1 else (F.relu(ref) if act == 2 else ref)
    dy = rnd(B, P, C, seed=21)
    ref.backward(dy)
    y = torch.empty(B * P, C, device=DEV)
    stats = torch.empty(B, G, 2, device=DEV)
    xd = x.reshape(B * P, C).to(DEV)
    ops.groupnorm_fwd(xd, w.to(DEV), b.to(DEV), 1e-5, G, act, y, stats, B, P)
    assert relerr(y, ref.reshape(B * P, C)) < 2e-5
    dx = torch.empty(B * P, C, device=DEV)
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ops.groupnorm_bwd(dy.reshape(B * P, C).to(DEV), xd, w.to(DEV), b.to(DEV), stats, G, act, dx, dw, db, B, P)
    assert relerr(dx, xr.grad.reshape(B * P, C)) < 5e-5
    assert relerr(dw, wr.grad) < 5e-5 and relerr(db, br.grad) < 5e-5


def test_batchnorm():
    rows, C = 4096, 512
    x = rnd(rows, C, seed=22, scale=1.3) + 0.2
    w, b = rnd(C, seed=23) * 0.1 + 1, rnd(C, seed=24) * 0.1
    rm, rv = rnd(C, seed=25) * 0.1, rnd(C, seed=26).abs() * 0.1 + 1
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rm_ref, rv_ref = rm.clone(), rv.clone()
    ref = F.gelu(F.batch_norm(xr, rm_ref, rv_ref, wr, br, True, 0.1, 1e-5))
    dy = rnd(rows, C, seed=27)
    ref.backward(dy)
    xd = x.to(DEV)
    sums = torch.empty(2, C, device=DEV)
    mv = torch.empty(2, C, device=DEV)
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    ops.bn_moments(xd, sums)
    ops.bn_finalize(sums, rows, mv, rmd, rvd, 0.1)
    y = torch.empty(rows, C, device=DEV)
    ops.bn_apply(xd, mv, w.to(DEV), b.to(DEV), 1e-5, 1, y)
    assert relerr(y, ref) < 2e-5
    assert relerr(rmd, rm_ref) < 1e-5 and relerr(rvd, rv_ref) < 1e-5
    sd = torch.empty(2, C, device=DEV)
    ops.bn_bwd_reduce(dy.to(DEV), xd, mv, w.to(DEV), b.to(DEV), 1e-5, 1, sd)
    assert relerr(sd[0], br.grad) < 5e-5 and relerr(sd[1], wr.grad) < 5e-5
    dx = torch.empty(rows, C, device=DEV)
    ops.bn_bwd_apply(dy.to(DEV), xd, mv, w.to(DEV), b.to(DEV), 1e-5, 1, sd, rows, dx)
    assert relerr(dx, xr.grad) < 5e-5


def _gemm_ref(a, b, bias=None, colscale=None, residual=None, ep=0, aux=None, alpha=1.0):
    v = alpha * (a.double() @ b.double().t())
    if bias is not None:
        v = v + bias.double()
    pre = v.clone()
    if ep == 1:
        v = F.gelu(v)
    elif ep == 2:
        v = F.relu(v)
    elif ep == 3:
        ad = aux.double().requires_grad_(True)
        F.gelu(ad).sum().backward()
        v = v * ad.grad
    elif ep == 4:
        v = v * aux.double()
    if colscale is not None:
        v = v * colscale.double()
    if residual is not None:
        v = v + residual.double()
    return v, pre


@pytest.mark.parametrize("M,N,K", [(100, 70, 50), (257, 130, 64), (64, 19, 256)])
def test_gemm_f32(M, N, K):
    a, b = rnd(M, K, seed=28), rnd(N, K, seed=29)
    bias, cs, res, aux = rnd(N, seed=30), rnd(N, seed=31), rnd(M, N, seed=32), rnd(M, N, seed=33)
    for ep in (0, 1, 2, 3, 4):
        c = torch.empty(M, N, device=DEV)
        c2 = torch.empty(M, N, device=DEV)
        ops.gemm(a.to(DEV), b.to(DEV), c, alpha=0.5, bias=bias.to(DEV), colscale=cs.to(DEV), residual=res.to(DEV), ep_mode=ep,
                 aux=aux.to(DEV), c2=c2)
        ref, pre = _gemm_ref(a, b, bias, cs, res, ep, aux, 0.5)
        assert relerr(c, ref) < 1e-5, ep
        assert relerr(c2, pre) < 1e-5
    # GELU forward that saves gelu'(pre-activation) in the second output
    c, c2 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    ops.gemm(a.to(DEV), b.to(DEV), c, bias=bias.to(DEV), ep_mode=ops.EP_GELU_DGELU, c2=c2)
    pre = (a.double() @ b.double().t() + bias.double()).requires_grad_(True)
    gl = F.gelu(pre)
    gl.sum().backward()
    assert relerr(c, gl.detach()) < 1e-5 and relerr(c2, pre.grad) < 1e-5
    # transposed operands via strides + in-place accumulate
    c = res.clone().to(DEV)
    ops.gemm(a.t().contiguous().to(DEV), b.t().contiguous().to(DEV), c, residual=c, trans_a=True, trans_b=True)
    assert relerr(c, a.double() @ b.double().t() + res.double()) < 1e-5
    # batched
    ab, bb = rnd(3, M, K, seed=34), rnd(3, N, K, seed=35)
    cb = torch.empty(3, M, N, device=DEV)
    ops.gemm(ab.to(DEV), bb.to(DEV), cb)
    assert relerr(cb, ab.double() @ bb.double().transpose(1, 2)) < 1e-5


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 200, 192), (4100, 1024, 1024), (2048, 19, 256), (513, 64, 1088)])
def test_gemm_bf16(M, N, K):
    a, b = rnd(M, K, seed=36).bfloat16(), rnd(N, K, seed=37).bfloat16()
    bias, cs, res, aux = rnd(N, seed=38), rnd(N, seed=39), rnd(M, N, seed=40), rnd(M, N, seed=41).bfloat16()
    for ep in (0, 1, 3):
        c = torch.empty(M, N, device=DEV)
        c2 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        ops.gemm(a.to(DEV), b.to(DEV), c, bias=bias.to(DEV), colscale=cs.to(DEV), residual=res.to(DEV), ep_mode=ep,
                 aux=aux.to(DEV), c2=c2)
        ref, pre = _gemm_ref(a.float(), b.float(), bias, cs, res, ep, aux.float())
        assert relerr(c, ref) < 2e-5, (ep, relerr(c, ref))  # bf16 inputs are exact in fp32; only accumulation order differs
        assert relerr(c2.float(), pre) < 1e-2
    cb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(a.to(DEV), b.to(DEV), cb)
    assert relerr(cb.float(), (a.double() @ b.double().t())) < 1e-2
    # strided (column-slice) operands: A view inside a wider buffer, C into a column slice
    wide = torch.zeros(M, K + 64, dtype=torch.bfloat16, device=DEV)
    wide[:, :K] = a.to(DEV)
    cw = torch.zeros(M, N + 8, device=DEV)
    ops.gemm(wide[:, :K], b.to(DEV), cw[:, :N])
    assert relerr(cw[:, :N], a.double() @ b.double().t()) < 2e-5 and cw[:, N:].abs().sum() == 0


@pytest.mark.parametrize("cfg", [17, 16, 30, 31, 32, 33, 34, 35, 36, 39, 40, 50, 51, 52, 10])
@pytest.mark.parametrize("M,N,K", [(4100, 1024, 1024), (300, 520, 320), (1024, 2048, 448), (256, 256, 4096), (512, 512, 128)])
def test_gemm_bf16_configs_fast_epilogues(cfg, M, N, K):
    """Every tile configuration incl. the ping-pong kernels (30: 256x256, 31: 128x128) and the 64-wide-K-tile 256x256 kernels
    (32: 4 waves / AGPR accumulator, 33: 8 waves; K = 128 is their shortest pipeline) x the specialised epilogue instances the
    backbones use; repeated launches double as a race screen for the LDS-DMA rings."""
    if cfg in (31, 35, 36) and K < 256:
        pytest.skip("the 128x128 ping-pong and deep-ring kernels need K >= 256 (the dispatcher rejects shorter K)")
    if cfg == 50 and os.environ.get("VFMSEG_EXPERIMENTAL", "0") != "1":
        pytest.skip("gemm_v5.hip (config 50) is built only with VFMSEG_EXPERIMENTAL=1")
    if cfg == 51 and (K % 128 or K < 512):
        pytest.skip("the split-K ring kernel halves K into whole K-tiles: K % 128 == 0, K >= 512")
    a, b = rnd(M, K, seed=80).bfloat16().to(DEV), rnd(N, K, seed=81).bfloat16().to(DEV)
    bias, cs, res = rnd(N, seed=82).to(DEV), (rnd(N, seed=83) * 0.2 + 1).to(DEV), rnd(M, N, seed=84).to(DEV)
    aux = rnd(M, N, seed=85).bfloat16().to(DEV)
    acc = a.double() @ b.double().t()
    bd, cd, rd, ad = bias.double(), cs.double(), res.double(), aux.double()
    gelu = lambda t: 0.5 * t * (1 + torch.erf(t / 2 ** 0.5))
    gelu_grad = lambda t: 0.5 * (1 + torch.erf(t / 2 ** 0.5)) + t * torch.exp(-0.5 * t * t) / (2 * 3.141592653589793) ** 0.5
    ops.tune("gemm_cfg", cfg)
    try:
        for rep in range(3):
            c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            ops.gemm(a, b, c, bias=bias)
            assert relerr(c.float(), acc + bd) < 1e-2
            c = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(a, b, c, alpha=0.5)
            assert relerr(c, 0.5 * acc) < 2e-5
            c = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(a, b, c, bias=bias, colscale=cs, residual=res)
            assert relerr(c, (acc + bd) * cd + rd) < 2e-5
            c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            c2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            ops.gemm(a, b, c, bias=bias, ep_mode=ops.EP_GELU, c2=c2)
            assert relerr(c.float(), gelu(acc + bd)) < 1e-2 and relerr(c2.float(), acc + bd) < 1e-2
            c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            ops.gemm(a, b, c, ep_mode=ops.EP_MUL_GELU_GRAD, aux=aux)
            assert relerr(c.float(), acc * gelu_grad(ad)) < 1e-2
            # forward that saves the activation's derivative + the backward that only multiplies (what the backbones use)
            c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            c2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            ops.gemm(a, b, c, bias=bias, ep_mode=ops.EP_GELU_DGELU, c2=c2)
            assert relerr(c.float(), gelu(acc + bd)) < 1e-2 and relerr(c2.float(), gelu_grad(acc + bd)) < 1e-2
            c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            ops.gemm(a, b, c, ep_mode=ops.EP_MUL, aux=aux)
            assert relerr(c.float(), acc * ad) < 1e-2
            c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
            ops.gemm(a, b, c, bias=bias, ep_mode=ops.EP_GELU)
            assert relerr(c.float(), gelu(acc + bd)) < 1e-2
    finally:
        ops.tune("gemm_cfg", -1)


@pytest.mark.parametrize("M,N,K,ta,tb", [(4100, 1024, 1024, False, False), (300, 200, 192, True, False), (513, 64, 100, False, True), (64, 19, 27, True, True)])
def test_gemm_split_bf16x3(M, N, K, ta, tb):
    """The bf16 x 3 form of an fp32 GEMM (vfm_split3 + one bf16 MFMA GEMM over K' = 3 ceil64(K)): hi / lo halves are exact bf16
    roundings, and the product agrees with float64 to ~2^-16 - 100x closer than a plain bf16 GEMM, 100x inside the 1e-3 budget."""
    from vfmseg_amd.precision import set_compute_dtype
    a, b = rnd(M, K, seed=70), rnd(N, K, seed=71)
    bias, res = rnd(N, seed=72), rnd(M, N, seed=73)
    ref = a.double() @ b.double().t() + bias.double() + res.double()
    ad = (a.t().contiguous() if ta else a).to(DEV)
    bd = (b.t().contiguous() if tb else b).to(DEV)
    x3 = ops.split3(ad, 0, trans=ta)
    kp = (K + 63) // 64 * 64
    hi = x3[:, :kp].float().cpu()[:, :K]
    lo = x3[:, 2 * kp:].float().cpu()[:, :K]
    assert torch.equal(hi, a.bfloat16().float()) and torch.equal(x3[:, kp:2 * kp].float().cpu()[:, :K], hi)
    assert torch.equal(lo, (a - hi).bfloat16().float())
    assert x3[:, K:kp].abs().sum() == 0
    set_compute_dtype("bf16x3")
    try:
        c = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm(ad, bd, c, bias=bias.to(DEV), residual=res.to(DEV), trans_a=ta, trans_b=tb)
        e3 = relerr(c, ref)
    finally:
        set_compute_dtype("bf16")
    c16 = torch.empty(M, N, device=DEV)
    kpad = (-K) % 64
    a16 = F.pad(a, (0, kpad)).bfloat16().to(DEV)
    b16 = F.pad(b, (0, kpad)).bfloat16().to(DEV)
    ops.gemm(a16, b16, c16, bias=bias.to(DEV), residual=res.to(DEV))
    e1 = relerr(c16, ref)
    print(f"[parity] split-bf16 GEMM {M}x{N}x{K}: rel err {e3:.2e} (plain bf16 operands: {e1:.2e})")
    assert e3 < 3e-5 and e3 < e1 / 50


def test_bf16x3_weight_cache_follows_in_place_weight_edits():
    """bf16x3 mode: functional.linear packs its weights into a persistent buffer and ops.split3 caches the split image ON that buffer.
    An in-place edit of the parameter (load_state_dict, p.copy_, a non-fused optimiser) re-packs the buffer behind torch's version
    counter; the split image must be rebuilt then (round-3 advisor finding: it was not)."""
    from vfmseg_amd import functional as Fh
    from vfmseg_amd.precision import set_compute_dtype
    x = rnd(130, 256, seed=90).to(DEV)
    w = torch.nn.Parameter(rnd(64, 256, seed=91).to(DEV), requires_grad=False)
    w2 = rnd(64, 256, seed=92).to(DEV)
    set_compute_dtype("bf16x3")
    try:
        y0 = Fh.linear(x, w, "linear", out_dtype=torch.float32)
        assert relerr(y0, x.double() @ w.double().t()) < 1e-4
        with torch.no_grad():
            w.copy_(w2)
        y1 = Fh.linear(x, w, "linear", out_dtype=torch.float32)
        assert relerr(y1, x.double() @ w2.double().t()) < 1e-4
    finally:
        set_compute_dtype("bf16")



@pytest.mark.skipif(os.environ.get("VFMSEG_EXPERIMENTAL", "0") != "1", reason="gemm_ps.hip is built only with VFMSEG_EXPERIMENTAL=1")
@pytest.mark.parametrize("cfg", [37, 38])
@pytest.mark.parametrize("M,N,K", [(4100, 4096, 1024), (512, 256, 640), (1024, 2048, 1088), (256, 256, 4096), (4356, 768, 576)])
def test_gemm_bf16_persistent_two_accumulators(cfg, M, N, K):
    """gemm_ps.hip (config 37: two 256 x 128 sub-tiles per block, the first one's epilogue under the second one's K loop; 38: one
    sub-tile per block) on its four epilogue kinds, with and without [cls] tail rows, against float64; three launches each as a race
    screen for the hand-counted LDS-DMA ring (every output element is checked, NaN-prefilled)."""
    if cfg == 37 and N % 256:
        pytest.skip("config 37 walks 256-column regions")
    a, b = rnd(M, K, seed=90).bfloat16().to(DEV), rnd(N, K, seed=91).bfloat16().to(DEV)
    bias = rnd(N, seed=92).to(DEV)
    aux = rnd(M, N, seed=93).bfloat16().to(DEV)
    acc = a.double() @ b.double().t()
    bd, ad = bias.double(), aux.double()
    gelu = lambda t: 0.5 * t * (1 + torch.erf(t / 2 ** 0.5))
    gelu_grad = lambda t: 0.5 * (1 + torch.erf(t / 2 ** 0.5)) + t * torch.exp(-0.5 * t * t) / (2 * 3.141592653589793) ** 0.5
    nan = lambda: torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.tune("gemm_cfg", cfg)
    try:
        for rep in range(3):
            c = nan()
            ops.gemm(a, b, c, bias=bias, alpha=0.5)
            assert relerr(c.float(), 0.5 * acc + bd) < 1e-2
            c, c2 = nan(), nan()
            ops.gemm(a, b, c, bias=bias, ep_mode=ops.EP_GELU_DGELU, c2=c2)
            assert relerr(c.float(), gelu(acc + bd)) < 1e-2 and relerr(c2.float(), gelu_grad(acc + bd)) < 1e-2
            c = nan()
            ops.gemm(a, b, c, ep_mode=ops.EP_MUL, aux=aux)
            assert relerr(c.float(), acc * ad) < 1e-2
            c = nan()
            ops.gemm(a, b, c, bias=bias, ep_mode=ops.EP_GELU)
            assert relerr(c.float(), gelu(acc + bd)) < 1e-2
    finally:
        ops.tune("gemm_cfg", -1)
    # with the knob on, the dispatcher itself picks config 37 for whole rounds of 256 x 256 regions: same numbers as the default path
    if (M, N, K) == (4100, 4096, 1024):
        c1, c2 = nan(), nan()
        ops.gemm(a, b, c1, bias=bias, ep_mode=ops.EP_GELU)
        ops.tune("gemm_use_ps", 1)
        try:
            ops.gemm(a, b, c2, bias=bias, ep_mode=ops.EP_GELU)
        finally:
            ops.tune("gemm_use_ps", 0)
        assert relerr(c1.float(), c2.float().double()) < 1e-2


@pytest.mark.parametrize("cfg", [-1, 17, 32, 33, 34, 39, 40])  # (35 / 36 need K >= 256)
def test_gemm_bf16_batched_ragged(cfg):
    """Batched bf16 GEMMs (SAM's per-window products) with ragged M / N, a batch stride wider than the matrix, a bf16 residual
    and the scalar (N % 4 != 0) epilogue, through the default dispatch and the ring kernels; K = 128 and 192 are the shortest
    pipelines of the five-chunk ring (two and three K-tiles)."""
    ops.tune("gemm_cfg", cfg)
    try:
        for (Bt, M, N, K) in [(3, 200, 328, 192), (5, 196, 196, 128), (2, 130, 19, 256), (4, 257, 260, 1088)]:
            a, b = rnd(Bt, M, K, seed=70).bfloat16().to(DEV), rnd(Bt, N, K, seed=71).bfloat16().to(DEV)
            ref = a.double() @ b.double().transpose(1, 2)
            for rep in range(2):
                wide = torch.full((Bt, M + 3, N), float("nan"), dtype=torch.bfloat16, device=DEV)  # batch stride > M * N
                c = wide[:, :M]
                ops.gemm(a, b, c, alpha=0.25)
                assert relerr(c.float(), 0.25 * ref) < 1e-2 and torch.isnan(wide[:, M:].float()).all()
                cf = torch.full((Bt, M, N), float("nan"), device=DEV)
                ops.gemm(a, b, cf)
                assert relerr(cf, ref) < 2e-5
                if N % 4 == 0:
                    res = rnd(Bt, M, N, seed=72).bfloat16().to(DEV)
                    cr = torch.full((Bt, M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
                    ops.gemm(a, b, cr, residual=res)
                    assert relerr(cr.float(), ref + res.double()) < 1e-2
    finally:
        ops.tune("gemm_cfg", -1)


@pytest.mark.parametrize("cfg", [-1, 10, 18, 17, 34, 35])
@pytest.mark.parametrize("M,N", [(516, 200), (516, 198), (544, 200), (544, 198), (20, 64)])
def test_gemm_bf16_tail_modes(cfg, M, N):
    """The ways the tail rows of M (4 or 32 past a 128-row boundary) can run, at the smallest shapes that reach them (gemm_select.h GemmTail;
    which plan each case gets is pinned by test_gemm_dispatch_cpu.py): a skinny launch of their own (the rules at this size, configs 10 and
    18), skinny blocks of the tile launch (17, 34, and 35 with 32 tail rows), inside the regular blocks of the deep ring (35 with 4 tail
    rows); N = 198 takes the scalar epilogue.  [20 x 64] runs whole on the skinny kernel whatever the config.  Every output element is
    checked against float64 (NaN-prefilled)."""
    K = 128 if M == 20 else 256
    a, b = rnd(M, K, seed=160).bfloat16().to(DEV), rnd(N, K, seed=161).bfloat16().to(DEV)
    bias = rnd(N, seed=162).to(DEV)
    ref = a.double() @ b.double().t() + bias.double()
    ops.tune("gemm_cfg", cfg)
    try:
        c = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm(a, b, c, bias=bias)
        assert relerr(c, ref) < 2e-5
        ch = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.gemm(a, b, ch, bias=bias)
        assert relerr(ch.float(), ref) < 1e-2
    finally:
        ops.tune("gemm_cfg", -1)


@pytest.mark.parametrize("P,M,Q", [(64, 4100, 3072), (64, 4100, 1024), (1024, 2048, 4096), (19, 1000, 256), (200, 333, 128)])
def test_gemm_bf16_transposed_b(P, M, Q):
    """Weight-gradient form: out[P,Q] = xs^T[P,M] @ y[M,Q], y consumed in place ([K,N] operand), tokens zero-padded."""
    xs, y = rnd(M, P, seed=60).bfloat16(), rnd(M, Q, seed=61).bfloat16()
    mp = (M + 63) // 64 * 64
    xt = torch.zeros(P, mp, dtype=torch.bfloat16, device=DEV)
    ops.transpose(xs.to(DEV), xt, pad_rows=mp)
    out = torch.empty(P, Q, device=DEV)
    ops.gemm(xt, y.to(DEV), out, trans_b=True, kb_rows=M)
    ref = xs.double().t() @ y.double()
    assert relerr(out, ref) < 2e-5, relerr(out, ref)
    # y as a column slice of a wider buffer + split-K batching
    if M % 128 == 0 or M == 2048:
        wide = torch.zeros(M, Q + 64, dtype=torch.bfloat16, device=DEV)
        wide[:, :Q] = y.to(DEV)
        kch = 4
        slabs = torch.empty(kch, P, Q, device=DEV)
        ops.gemm_splitk_bt(xt, wide[:, :Q], slabs, kch)
        assert relerr(slabs.sum(0), ref) < 2e-5
    if M == 4100:   # ragged token count: 65 steps of 64 -> 13 slices, the last one clamps rows >= M
        slabs = torch.empty(13, P, Q, device=DEV)
        ops.gemm_splitk_bt(xt, y.to(DEV), slabs, 13)
        assert relerr(slabs.sum(0), ref) < 2e-5


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nq_extra,nk_extra,nq,nk,B1024", [(1, 1, 200, 200, 0), (0, 0, 256, 256, 0), (0, 0, 130, 70, 0), (1, 1, 1024, 1024, 6),
                                                            (1, 1, 128, 384, 0), (0, 0, 512, 512, 0), (1, 1, 1024, 1024, 5)])
def test_attention(dt, nq_extra, nk_extra, nq, nk, B1024):
    # (B, H) = (2, 3): short grids -> the 2-wave-per-block kernels; the 1024-token case runs with 48 (image, head) pairs and the
    # 512-token case with 96 (192 blocks of 256 queries) so that the 64-queries-per-wave forward, the 4-wave backward kernels and
    # their single-row [cls] blocks (last linear block ids) are exercised as in the backbones; with 40 pairs the 1024-token case
    # stays on the 32-queries-per-wave forward
    B, H, d = (2, 3, 64) if nq < 512 else ((12, 8, 64) if nq == 512 else (B1024, 8, 64))
    hd = H * d
    tol = 2e-5 if dt == torch.float32 else 2e-2
    # token-major buffers: main tokens first, then the per-image extra (cls) rows
    q = rnd(B * nq + B * nq_extra, hd, seed=42).to(dt)
    k = rnd(B * nk + B * nk_extra, hd, seed=43).to(dt)
    if nk >= 256:  # keys of the later tiles score much higher: forces the lazy-rescale branch of the online softmax mid-stream
        k = k.float()
        k[B * nk // 2: B * nk // 2 + 7] *= 4.0
        k[B * nk - 5: B * nk] *= 6.0
        k = k.to(dt)
    v = rnd(B * nk + B * nk_extra, hd, seed=44).to(dt)
    do = rnd(B * nq + B * nq_extra, hd, seed=45).to(dt)

    def gather(t, n, ne):  # -> [B, H, n+ne, d] float
        main = t[: B * n].reshape(B, n, H, d)
        if ne:
            main = torch.cat([main, t[B * n:].reshape(B, 1, H, d)], 1)
        return main.permute(0, 2, 1, 3).float()

    qq, kk, vv = (gather(q, nq, nq_extra).requires_grad_(True), gather(k, nk, nk_extra).requires_grad_(True),
                  gather(v, nk, nk_extra).requires_grad_(True))
    scale = d ** -0.5
    ref = ((qq @ kk.transpose(-1, -2)) * scale).softmax(-1) @ vv
    ref.backward(gather(do, nq, nq_extra))

    def scatter(g, n, ne):  # [B,H,n+ne,d] -> token-major
        g = g.permute(0, 2, 1, 3)
        main = g[:, :n].reshape(B * n, hd)
        return torch.cat([main, g[:, n:].reshape(B * ne, hd)], 0) if ne else main

    o = torch.empty(q.shape, dtype=dt, device=DEV)
    lse = torch.empty(B, H, nq + nq_extra, device=DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ops.attn_fwd(qd, kd, vd, o, lse, B, H, d, nq, nq_extra, nk, nk_extra, scale)
    assert relerr(o.float(), scatter(ref, nq, nq_extra)) < tol
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    ops.attn_bwd(qd, kd, vd, o, lse, do.to(DEV), dq, dk, dv, B, H, d, nq, nq_extra, nk, nk_extra, scale)
    assert relerr(dq.float(), scatter(qq.grad, nq, nq_extra)) < tol * 2
    assert relerr(dk.float(), scatter(kk.grad, nk, nk_extra)) < tol * 2
    assert relerr(dv.float(), scatter(vv.grad, nk, nk_extra)) < tol * 2


@pytest.mark.parametrize("nq_extra,nk_extra,nq,nk,B,H", [(1, 1, 200, 200, 2, 3), (0, 0, 130, 70, 2, 3), (1, 1, 1024, 1024, 3, 8), (0, 0, 256, 320, 1, 16)])
def test_attention_split_bf16x3_forward(nq_extra, nk_extra, nq, nk, B, H):
    """vfm_attn_fwd_x3 (bf16x3 mode: fp32 in / out, every product as hi*hi + hi*lo + lo*hi on the bf16 MFMA) against float64 softmax
    attention: ~1e-5, where the plain bf16 kernel sits at ~1e-2; lse too (the exact-fp32 backward consumes it); a spike in the later
    keys forces the lazy-rescale branch."""
    from vfmseg_amd.precision import set_compute_dtype
    d, hd = 64, H * 64
    q = rnd(B * nq + B * nq_extra, hd, seed=42)
    k = rnd(B * nk + B * nk_extra, hd, seed=43)
    k[B * nk // 2: B * nk // 2 + 7] *= 4.0
    k[B * nk - 5: B * nk] *= 6.0
    v = rnd(B * nk + B * nk_extra, hd, seed=44)

    def gather(t, n, ne):
        main = t[: B * n].reshape(B, n, H, d)
        if ne:
            main = torch.cat([main, t[B * n:].reshape(B, 1, H, d)], 1)
        return main.permute(0, 2, 1, 3).double()

    qq, kk, vv = gather(q, nq, nq_extra), gather(k, nk, nk_extra), gather(v, nk, nk_extra)
    sc = (qq @ kk.transpose(-1, -2)) * d ** -0.5
    ref = sc.softmax(-1) @ vv
    ref_lse = torch.logsumexp(sc, -1)
    g = ref.permute(0, 2, 1, 3)
    ref_tok = torch.cat([g[:, :nq].reshape(B * nq, hd), g[:, nq:].reshape(B * nq_extra, hd)], 0) if nq_extra else g.reshape(B * nq, hd)
    # K and V as column slices of a packed [rows, 3 hd] buffer, as the backbones pass them
    packed = torch.cat([q if nq == nk and nq_extra == nk_extra else torch.zeros(k.shape[0], hd), k, v], 1).to(DEV)
    o = torch.full(q.shape, float("nan"), device=DEV)
    lse = torch.empty(B, H, nq + nq_extra, device=DEV)
    set_compute_dtype("bf16x3")
    try:
        ops.attn_fwd(q.to(DEV), packed[:, hd:2 * hd], packed[:, 2 * hd:], o, lse, B, H, d, nq, nq_extra, nk, nk_extra, d ** -0.5)
    finally:
        set_compute_dtype("bf16")
    e = relerr(o, ref_tok)
    el = (lse.double().cpu() - ref_lse).abs().max().item()
    print(f"[parity] split-bf16 attention fwd nq {nq}+{nq_extra} nk {nk}+{nk_extra}: out rel err {e:.2e}, lse abs err {el:.2e}")
    assert e < 5e-5 and el < 2e-5 * max(1.0, ref_lse.abs().max().item()) + 1e-4   # (spiked keys: |lse| ~ 30)


@pytest.mark.parametrize("nq_extra,nk_extra,nq,nk,B,H", [(1, 1, 200, 200, 2, 3), (0, 0, 130, 70, 2, 3), (1, 1, 1024, 1024, 2, 4), (0, 0, 256, 320, 1, 8)])
def test_attention_split_bf16x3_backward(nq_extra, nk_extra, nq, nk, B, H):
    """vfm_attn_bwd_x3 (bf16x3 mode: fp32 q / k / v / o / dout -> fp32 dq / dk / dv, the five products as hi*hi + hi*lo + lo*hi on the bf16
    MFMA) against float64 autograd of softmax attention: ~1e-5 (the plain bf16 backward sits at ~1e-2).  q, k, v as column slices of one
    packed buffer (as the backbones pass them), gradients written into column slices of a packed gradient buffer; ragged tails, the extra
    token as the last row of every sequence."""
    from vfmseg_amd.precision import set_compute_dtype
    d, hd = 64, H * 64
    same = nq == nk and nq_extra == nk_extra
    q = rnd(B * nq + B * nq_extra, hd, seed=52)
    k = rnd(B * nk + B * nk_extra, hd, seed=53)
    k[B * nk // 2: B * nk // 2 + 5] *= 3.0
    v = rnd(B * nk + B * nk_extra, hd, seed=54)
    do = rnd(B * nq + B * nq_extra, hd, seed=55)

    def gather(t, n, ne):
        main = t[: B * n].reshape(B, n, H, d)
        if ne:
            main = torch.cat([main, t[B * n:].reshape(B, 1, H, d)], 1)
        return main.permute(0, 2, 1, 3).double()

    def scatter(g, n, ne):   # [B, H, n + ne, d] -> token-major [rows, hd] in the cls-last order
        g = g.permute(0, 2, 1, 3)
        return torch.cat([g[:, :n].reshape(B * n, hd), g[:, n:].reshape(B * ne, hd)], 0) if ne else g.reshape(B * n, hd)

    qq, kk, vv = (gather(t, n, ne).requires_grad_(True) for t, n, ne in ((q, nq, nq_extra), (k, nk, nk_extra), (v, nk, nk_extra)))
    sc = (qq @ kk.transpose(-1, -2)) * d ** -0.5
    out = sc.softmax(-1) @ vv
    out.backward(gather(do, nq, nq_extra))
    ref = [scatter(qq.grad, nq, nq_extra), scatter(kk.grad, nk, nk_extra), scatter(vv.grad, nk, nk_extra)]
    o_tok = scatter(out.detach(), nq, nq_extra).float().to(DEV)
    lse = torch.logsumexp(sc.detach(), -1).float().to(DEV).contiguous()
    if same:
        packed = torch.cat([q, k, v], 1).to(DEV)
        qd, kd, vd = packed[:, :hd], packed[:, hd:2 * hd], packed[:, 2 * hd:]
        grads = torch.full(packed.shape, float("nan"), device=DEV)
        dq, dk, dv = grads[:, :hd], grads[:, hd:2 * hd], grads[:, 2 * hd:]
    else:
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        dq, dk, dv = (torch.full(t.shape, float("nan"), device=DEV) for t in (q, k, v))
    set_compute_dtype("bf16x3")
    try:
        ops.attn_bwd(qd, kd, vd, o_tok, lse, do.to(DEV), dq, dk, dv, B, H, d, nq, nq_extra, nk, nk_extra, d ** -0.5)
    finally:
        set_compute_dtype("bf16")
    errs = [relerr(a, b) for a, b in zip((dq, dk, dv), ref)]
    print(f"[parity] split-bf16 attention bwd nq {nq}+{nq_extra} nk {nk}+{nk_extra}: dq / dk / dv rel err {errs[0]:.2e} / {errs[1]:.2e} / {errs[2]:.2e}")
    assert max(errs) < 1e-4


def test_bf16x3_producers_write_the_split_operand_image():
    """bf16x3 predictions: LayerNorm and the split-bf16 attention forward hand their output to the consuming GEMM as the split image
    [hi | hi | lo] (vfm_layernorm_fwd_split3, vfm_attn_fwd_x3_split) - bit for bit what vfm_split3 makes of the fp32 output, found by
    ops.split3 on the tensor object; with split_out / o_split = "only" the fp32 copy is not written at all."""
    from vfmseg_amd.precision import set_compute_dtype
    set_compute_dtype("bf16x3")
    try:
        x = rnd(300, 1024, seed=130).to(DEV) * 3
        w, b = (rnd(1024, seed=131) * 0.1 + 1).to(DEV), rnd(1024, seed=132).to(DEV)
        y_ref, st_ref = torch.empty(300, 1024, device=DEV), torch.empty(300, 2, device=DEV)
        ops.layernorm_fwd(x, w, b, 1e-6, y_ref, st_ref)
        img_ref = ops.split3(y_ref, 0)
        for mode in ("also", "only"):
            y = torch.full((300, 1024), float("nan"), device=DEV)
            st = torch.empty(300, 2, device=DEV)
            ops.layernorm_fwd(x, w, b, 1e-6, y, st, split_out=mode)
            got = ops.split3(y, 0)                     # the registered image, not a new pass
            assert got.data_ptr() == y._vfm_split3_out[1].data_ptr()
            assert torch.equal(got.view(torch.int16), img_ref.view(torch.int16)) and torch.equal(st, st_ref)
            assert torch.equal(y, y_ref) if mode == "also" else bool(torch.isnan(y).all())
        # attention: B 2, H 3, 200 + 1 tokens
        B, H, n, d, hd = 2, 3, 200, 64, 192
        qkv = rnd(B * n + B, 3 * hd, seed=133).to(DEV)
        o_ref, lse_ref = torch.empty(B * n + B, hd, device=DEV), torch.empty(B, H, n + 1, device=DEV)
        ops.attn_fwd(qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:], o_ref, lse_ref, B, H, d, n, 1, n, 1, d ** -0.5)
        o_img = ops.split3(o_ref, 0)
        for mode in ("also", "only"):
            o = torch.full((B * n + B, hd), float("nan"), device=DEV)
            lse = torch.empty(B, H, n + 1, device=DEV)
            ops.attn_fwd(qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:], o, lse, B, H, d, n, 1, n, 1, d ** -0.5, o_split=mode)
            assert torch.equal(ops.split3(o, 0).view(torch.int16), o_img.view(torch.int16)) and torch.equal(lse, lse_ref)
            assert torch.equal(o, o_ref) if mode == "also" else bool(torch.isnan(o).all())
        # the consumer: a GEMM on the fp32 tensor object picks the image up (the fp32 values are NaN here: a fresh split would poison c)
        wgt = rnd(64, 1024, seed=134).to(DEV)
        c = torch.empty(300, 64, device=DEV)
        ops.gemm(y, wgt, c)
        assert relerr(c, y_ref.double() @ wgt.double().t()) < 3e-5
        # a GEMM as the producer (vfm_gemm c_dt VFM_SPLIT3): fc1 + GELU of the backbone shape, a ragged M, and the plain epilogue
        for (m, n_, k, ep) in ((1370, 4096, 1024, ops.EP_GELU), (333, 512, 256, ops.EP_NONE), (130, 64, 128, ops.EP_GELU)):
            a, wt, bias = rnd(m, k, seed=135).to(DEV), (rnd(n_, k, seed=136) * 0.05).to(DEV), rnd(n_, seed=137).to(DEV)
            g_ref = torch.empty(m, n_, device=DEV)
            ops.gemm(a, wt, g_ref, bias=bias, ep_mode=ep)
            g = torch.full((m, n_), float("nan"), device=DEV)
            ops.gemm(a, wt, g, bias=bias, ep_mode=ep, c_split="only")
            assert bool(torch.isnan(g).all())
            img = ops.split3(g, 0)
            assert img.data_ptr() == g._vfm_split3_out[1].data_ptr() and img.shape == (m, 3 * n_)
            hi, hi2, lo = img[:, :n_].float(), img[:, n_:2 * n_].float(), img[:, 2 * n_:].float()
            assert torch.equal(hi, hi2)
            # hi + lo carries the fp32 result to 2^-16 relative (the vector epilogue's GELU is the 1.5e-7 erf polynomial)
            assert float(((hi + lo) - g_ref).abs().max()) <= 2e-5 * float(g_ref.abs().max()) + 1e-6
            out_ref, out = torch.empty(m, 64, device=DEV), torch.empty(m, 64, device=DEV)
            w2 = rnd(64, n_, seed=138).to(DEV) * 0.05
            ops.gemm(g_ref, w2, out_ref)
            ops.gemm(g, w2, out)
            assert relerr(out, out_ref) < 2e-5
    finally:
        set_compute_dtype("bf16")


@pytest.mark.parametrize("mode,dt", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
def test_gemm_tile_configurations_agree_bit_for_bit(mode, dt):
    """The ring-kernel forms (34: 128^2 / 8 waves, 52: 128^2 / 4 waves - what the dispatcher uses from K = 1024 on -, 33: 256^2 / 8 waves) and
    the two-stage kernel (17) accumulate every output element over K in the same order, and the [cls] tail rows of M (skinny blocks) always
    split K eight ways whatever the block's wave count: the same bits from every configuration, so a dispatch rule can change without moving
    any parity number (the fp16 logits bound sits at 9.5e-4 of 1e-3)."""
    from vfmseg_amd.precision import set_compute_dtype
    set_compute_dtype(mode)
    try:
        for (M, N, K) in ((4100, 1024, 1024), (2049, 1024, 4096), (1300, 384, 1088)):
            a, b = rnd(M, K, seed=150).to(dt).to(DEV), (rnd(N, K, seed=151) * 0.05).to(dt).to(DEV)
            bias, res = rnd(N, seed=152).to(DEV), rnd(M, N, seed=153).to(DEV)
            outs = []
            for cfg in (34, 52, 33, 17):
                ops.tune("gemm_cfg", cfg)
                c = torch.empty(M, N, device=DEV)
                ops.gemm(a, b, c, bias=bias, residual=res)
                ch = torch.empty(M, N, dtype=dt, device=DEV)
                ops.gemm(a, b, ch, bias=bias, ep_mode=ops.EP_GELU)
                outs.append((c, ch))
            for c, ch in outs[1:]:
                assert torch.equal(c, outs[0][0]) and torch.equal(ch, outs[0][1]), (mode, M, N, K)
    finally:
        ops.tune("gemm_cfg", -1)
        set_compute_dtype("bf16")


def test_gemm_split_k_form_is_order_independent_and_stream_safe():
    """Config 51 (gemm_w4.hip SPLITK): two blocks per tile, one per half of K; the first to finish leaves its partial sums in the stream's
    workspace, the second adds them and runs the epilogue.  own + partner is one fp32 addition whichever block finishes last, so repeated
    launches are bit-identical; the counter / flag words are left zero (the next launch works); two streams have separate workspaces."""
    M, N, K = 2049, 1024, 4096          # the coarse prediction pass' fc2: 128 tiles + one [cls] row as skinny blocks
    a, b = rnd(M, K, seed=140).bfloat16().to(DEV), (rnd(N, K, seed=141) * 0.05).bfloat16().to(DEV)
    bias, cs, res = rnd(N, seed=142).to(DEV), (rnd(N, seed=143) * 0.2 + 1).to(DEV), rnd(M, N, seed=144).to(DEV)
    ref = (a.double() @ b.double().t() + bias.double()) * cs.double() + res.double()
    ops.tune("gemm_cfg", 51)
    try:
        outs = []
        for _ in range(4):
            c = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(a, b, c, bias=bias, colscale=cs, residual=res)
            outs.append(c)
        assert relerr(outs[0], ref) < 2e-5 and all(torch.equal(outs[0], o) for o in outs[1:])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        c_main, c_side = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
        for _ in range(3):
            with torch.cuda.stream(side):
                ops.gemm(a, b, c_side, bias=bias, colscale=cs, residual=res)
            ops.gemm(a, b, c_main, bias=bias, colscale=cs, residual=res)
        torch.cuda.synchronize()
        assert torch.equal(c_main, outs[0]) and torch.equal(c_side, outs[0])
    finally:
        ops.tune("gemm_cfg", -1)


@pytest.mark.skipif(os.environ.get("VFMSEG_EXPERIMENTAL", "0") != "1", reason="attention_fwd64.hip is built only with VFMSEG_EXPERIMENTAL=1")
def test_attention_fwd64_experimental():
    # the 64-queries-per-wave forward (vfm_tune attn_fwd64, off by default) against the regular kernel on the backbone shape
    from vfmseg_amd import lib as L
    B, H, d, n = 4, 16, 64, 1024
    lib = L.load()
    for ex in (1, 0):
        q, k, v = [rnd(B * n + B * ex, H * d, seed=60 + i).to(torch.bfloat16).to(DEV) for i in range(3)]
        outs = []
        for mode in (0, 1):
            assert lib.vfm_tune(b"attn_fwd64", mode) == 0
            o = torch.empty_like(q)
            lse = torch.empty(B, H, n + ex, device=DEV)
            ops.attn_fwd(q, k, v, o, lse, B, H, d, n, ex, n, ex, d ** -0.5)
            outs.append((o.float(), lse.clone()))
        lib.vfm_tune(b"attn_fwd64", 0)
        assert relerr(outs[1][0], outs[0][0]) < 1e-2
        assert (outs[1][1] - outs[0][1]).abs().max().item() < 2e-3


def test_patchify_tokens():
    B, P = 2, 16
    img = rnd(B, 3, 96, 128, seed=46)
    w = rnd(32, 3, P, P, seed=47)
    ref = F.conv2d(img[:, :, 32:96, 16:112], w, stride=P).flatten(2).transpose(1, 2)  # [B, 24, 32]
    a = torch.empty(B * 4 * 6, 3 * P * P, device=DEV)
    ops.patchify(img.to(DEV), a, box=(32, 96, 16, 112))
    got = a.cpu() @ w.reshape(32, -1).t()
    assert relerr(got, ref.reshape(B * 24, 32)) < 1e-5
    ptok, cls, pos = rnd(B * 24, 32, seed=48), rnd(32, seed=49), rnd(25, 32, seed=50)
    x = torch.empty(B * 24 + B, 32, device=DEV)
    ops.assemble_tokens(ptok.to(DEV), cls.to(DEV), pos.to(DEV), x, B, 24, 32)
    exp_main = ptok.reshape(B, 24, 32) + pos[1:][None]
    assert relerr(x[: B * 24], exp_main.reshape(B * 24, 32)) < 1e-6
    assert relerr(x[B * 24:], (cls + pos[0])[None].expand(B, -1)) < 1e-6


def test_resize_and_labels():
    B, C = 2, 19
    x = rnd(B, C, 32, 48, seed=51)
    ref = F.interpolate(x, size=(128, 192), mode="bilinear", align_corners=False)
    out = torch.empty(B, C, 128, 192, device=DEV)
    ops.resize_bilinear(x.to(DEV), True, B, 32, 48, C, out, 1, (128, 192))
    assert relerr(out, ref) < 1e-6
    # NHWC in, cropped NHWC out
    xn = x.permute(0, 2, 3, 1).contiguous()
    o2 = torch.empty(B, 40, 64, C, device=DEV)
    ops.resize_bilinear(xn.to(DEV), False, B, 32, 48, C, o2, 0, (128, 192), window=(8, 16, 40, 64))
    assert relerr(o2.permute(0, 3, 1, 2), ref[:, :, 8:48, 16:80]) < 1e-6
    # down-scaling by 0.5 (no antialias) and blocked output
    d = F.interpolate(ref, scale_factor=0.5, mode="bilinear", align_corners=False)  # [B,C,64,96]
    o3 = torch.zeros(B * 32 * 48, 128, device=DEV)
    ops.resize_bilinear(ref.to(DEV), True, B, 128, 192, C, o3, 2, (64, 96), out_ld=128)
    # rows ordered (b, y/4, x/4, (y/2)%2, (x/2)%2); inside a row k = ((y%2)*2 + x%2)*C + c
    exp = d.reshape(B, C, 16, 2, 2, 24, 2, 2).permute(0, 2, 5, 3, 6, 4, 7, 1).reshape(B * 16 * 24 * 4, 4 * C)
    assert relerr(o3[:, : 4 * C], exp) < 1e-6 and o3[:, 4 * C:].abs().sum() == 0
    lab = torch.randint(0, 19, (B, 64, 64), generator=torch.Generator().manual_seed(52))
    lr = F.interpolate(lab[:, None].float(), scale_factor=0.5, mode="nearest").long()[:, 0]
    o4 = torch.empty(B, 32, 32, dtype=torch.int64, device=DEV)
    ops.label_resize(lab.to(DEV), o4, (32, 32))
    assert torch.equal(o4.cpu(), lr)
    o5 = torch.empty(B, 16, 24, dtype=torch.int64, device=DEV)
    ops.label_resize(lab.to(DEV), o5, (64, 64), window=(8, 4, 16, 24))
    assert torch.equal(o5.cpu(), lab[:, 8:24, 4:28])
    # unblock round trip
    z = rnd(B, 16 * 16, 5, seed=53)
    u = torch.empty(B, 16, 16, 5, device=DEV)
    ops.unblock(z.to(DEV), u, B, 16, 16, 5, 2)
    zb = torch.empty(B, 256, 5, device=DEV)
    ops.unblock(u, zb, B, 16, 16, 5, 2, inverse=True)
    assert torch.equal(zb.cpu(), z)
    e = z.reshape(B, 4, 4, 2, 2, 2, 2, 5).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B, 16, 16, 5)
    assert torch.equal(u.cpu(), e)


@pytest.mark.parametrize("h,H", [(32, 128), (8, 128), (16, 16), (12, 48), (128, 512), (3, 5), (32, 512), (7, 100)])
def test_upsample_ce(h, H):
    B, C = 2, 19
    lg = rnd(B, h, h, C, seed=54, scale=2.0)
    lab = torch.randint(0, C, (B, H, H), generator=torch.Generator().manual_seed(55))
    lab[:, 5:9] = 255
    lr = lg.clone().requires_grad_(True)
    up = F.interpolate(lr.permute(0, 3, 1, 2), size=(H, H), mode="bilinear", align_corners=False)
    loss_ref = F.cross_entropy(up, lab, reduction="none", ignore_index=255).mean()
    loss_ref.backward()
    valid = lab != 255
    hits_ref = ((up.argmax(1) == lab) & valid).sum().item()
    loss, counts, dl = ops.upsample_ce(lg.to(DEV), lab.to(DEV))
    assert abs(loss.item() - loss_ref.item()) < 1e-5 * max(1, abs(loss_ref.item()))
    assert counts.tolist() == [hits_ref, int(valid.sum())]
    assert relerr(dl, lr.grad) < 2e-5


@pytest.mark.parametrize("h,H,C,mode", [(32, 128, 19, "all_ignored"), (32, 512, 19, "all_ignored"), (16, 64, 19, "none_ignored"), (16, 256, 19, "none_ignored"),
                                        (32, 128, 7, "band"), (16, 256, 21, "band")])
def test_upsample_ce_edge_cases(h, H, C, mode):
    # every pixel ignored (loss 0, zero gradient, accuracy denominators empty), none ignored, and class counts other than 19
    # (the tiled kernels are instantiated for 19 classes; anything else takes the generic kernels) at the x4 / x16 scale factors
    B = 2
    lg = rnd(B, h, h, C, seed=154, scale=2.0)
    lab = torch.randint(0, C, (B, H, H), generator=torch.Generator().manual_seed(155))
    if mode == "all_ignored":
        lab[:] = 255
    elif mode == "band":
        lab[:, 3:11] = 255
    lr = lg.clone().requires_grad_(True)
    up = F.interpolate(lr.permute(0, 3, 1, 2), size=(H, H), mode="bilinear", align_corners=False)
    loss_ref = F.cross_entropy(up, lab, reduction="none", ignore_index=255).mean()
    loss_ref.backward()
    valid = lab != 255
    hits_ref = ((up.argmax(1) == lab) & valid).sum().item()
    loss, counts, dl = ops.upsample_ce(lg.to(DEV), lab.to(DEV))
    assert abs(loss.item() - loss_ref.item()) < 1e-5 * max(1, abs(loss_ref.item()))
    assert counts.tolist() == [hits_ref, int(valid.sum())]
    if mode == "all_ignored":
        assert float(dl.abs().max()) == 0.0 and loss.item() == 0.0
    else:
        assert relerr(dl, lr.grad) < 2e-5
    loss2, acc2, _ = ops.upsample_ce_loss_acc(lg.to(DEV), lab.to(DEV))   # the training form: accuracy = 100 * hits / (valid + eps)
    assert abs(loss2.item() - loss_ref.item()) < 1e-5 * max(1, abs(loss_ref.item()))
    eps = torch.finfo(torch.float32).eps
    assert abs(acc2.item() - 100.0 * hits_ref / (int(valid.sum()) + eps)) < 1e-3


def test_copy_batch_sums_partials():
    # one launch, several jobs: plain strided copy into bf16, accumulate into fp32, and a job whose value is the sum of four source
    # slices (the token-range partials of a reduction; jobs of a table run concurrently, so partials must not be separate jobs)
    g = torch.Generator().manual_seed(70)
    a = torch.randn(6, 10, generator=g).to(DEV)
    d1 = torch.zeros(10, 6, dtype=torch.bfloat16, device=DEV)
    parts = torch.randn(4, 5, 7, generator=g).to(DEV)
    d2 = torch.ones(5, 7, device=DEV)
    b = torch.randn(3, 4, generator=g).to(DEV)
    d3 = torch.full((3, 4), 2.0, device=DEV)
    tab = ops.CopyBatch([(a, d1, (6, 10), (10, 1), (1, 6)),                       # transpose into bf16
                         (parts[0], d2, (5, 7), (7, 1), (7, 1), True, 4, 35),      # d2 += parts.sum(0)
                         (b, d3, (3, 4), (4, 1), (4, 1), True)])                   # d3 += b
    tab.run()
    assert torch.equal(d1.float().cpu(), a.t().bfloat16().float().cpu())
    assert relerr(d2, 1.0 + parts.sum(0)) < 1e-6
    assert relerr(d3, 2.0 + b) < 1e-7
    tab.run()                                                                     # tables are reusable: accumulates again
    assert relerr(d2, 1.0 + 2 * parts.sum(0)) < 1e-6


def test_inference_helpers():
    B, C, H, W = 1, 19, 96, 128
    lg = rnd(B, C, H, W, seed=56, scale=2.0)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.conf_gate_count(lg.to(DEV), (16, 32, 64, 64), 0.3, cnt)
    ref = (lg[:, :, 16:80, 32:96].softmax(1).max(1)[0] > 0.3).sum().item()
    assert cnt.item() == ref
    preds = torch.zeros(B, C, H, W, device=DEV)
    count = torch.zeros(B, 1, H, W, device=DEV)
    crop = rnd(B, 8, 8, C, seed=57)
    pr, cr = torch.zeros(B, C, H, W), torch.zeros(B, 1, H, W)
    for (y0, x0) in ((0, 0), (32, 64), (16, 32)):
        ops.slide_accumulate(crop.to(DEV), False, B, 8, 8, C, preds, count, (y0, x0, 64, 64))
        pr[:, :, y0:y0 + 64, x0:x0 + 64] += F.interpolate(crop.permute(0, 3, 1, 2), size=(64, 64), mode="bilinear", align_corners=False)
        cr[:, :, y0:y0 + 64, x0:x0 + 64] += 1
    cr = cr.clamp_min(1)
    count.clamp_(min=1)
    am = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
    ops.slide_finalize(preds, count, am)
    assert relerr(preds, pr / cr) < 1e-6
    assert torch.equal(am.cpu().long(), (pr / cr).argmax(1))


def test_slide_gather_and_gate_windows_equal_the_per_window_ops():
    """vfm_slide_gather (one gather pass over the output map) against vfm_slide_accumulate per window + vfm_slide_finalize, and
    vfm_conf_gate_windows (all gates in one pass) against vfm_conf_gate per window: mixed low-res NHWC / full-res NCHW windows,
    overlapping 3 x 3 grid as in the 1024^2 predictions, B = 2."""
    B, C, H, W, hc, wc = 2, 19, 320, 448, 160, 192
    boxes = [(y0, x0, hc, wc) for y0 in (0, 96, 160) for x0 in (0, 128, 256)]
    wins = []
    for j, bx in enumerate(boxes):
        if j % 3 == 1:   # a window that kept its coarse logits: NCHW at window resolution
            wins.append((rnd(B, C, hc, wc, seed=300 + j).to(DEV), True, bx))
        else:            # refined window: NHWC low-res logits, upsampled x4
            wins.append((rnd(B, hc // 4, wc // 4, C, seed=300 + j).to(DEV), False, bx))
    preds0 = torch.zeros(B, C, H, W, device=DEV)
    count = torch.zeros(B, 1, H, W, device=DEV)
    for t, nchw, bx in wins:
        h, w = (t.shape[2], t.shape[3]) if nchw else (t.shape[1], t.shape[2])
        ops.slide_accumulate(t, nchw, B, h, w, C, preds0, count, bx)
    ops.slide_finalize(preds0, count)
    preds1 = torch.full((B, C, H, W), float("nan"), device=DEV)
    assert ops.slide_gather(wins, preds1)
    assert torch.isfinite(preds1).all() and (preds1 - preds0).abs().max().item() <= 1e-6 * preds0.abs().max().item()
    assert not ops.slide_gather(wins * 2, preds1)   # 18 windows: the caller falls back to the per-window path
    seg = (rnd(B, C, H, W, seed=333) * 3).to(DEV)
    c0 = torch.zeros(len(boxes), dtype=torch.int32, device=DEV)
    for j, bx in enumerate(boxes):
        ops.conf_gate_count(seg, bx, 0.5, c0[j:j + 1])
    c1 = torch.zeros(len(boxes), dtype=torch.int32, device=DEV)
    ops.conf_gate_windows(seg, boxes, 0.5, c1)
    assert torch.equal(c0, c1) and 0 < int(c0.min()) and int(c0.max()) < B * hc * wc


@pytest.mark.parametrize("vec4,zero", [(False, False), (True, True)])
def test_adamw(vec4, zero):
    """vs torch.optim.AdamW with two parameter groups (different lr multipliers and decays), scalar and float4 forms; the
    fused zero_grad clears the gradient buffer in the same pass."""
    n = 10000 + (0 if vec4 else 3)
    cut = 6000
    p, g = rnd(n, seed=58), rnd(n, seed=59)
    q1, q2 = p[:cut].clone().requires_grad_(True), p[cut:].clone().requires_grad_(True)
    opt = torch.optim.AdamW([dict(params=[q1], weight_decay=0.05, lr=1e-3), dict(params=[q2], weight_decay=0.0, lr=2e-3)])
    pd, m, v = p.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    seg = torch.tensor([0, cut], dtype=torch.int64, device=DEV)
    lrm = torch.tensor([1.0, 2.0], device=DEV)
    wd = torch.tensor([0.05, 0.0], device=DEV)
    for step in (1, 2, 3):
        q1.grad, q2.grad = g[:cut].clone() * step, g[cut:].clone() * step
        opt.step()
        gd = (g * step * 4.0).to(DEV)
        ops.adamw(pd, gd, m, v, seg, lrm, wd, 1e-3, (0.9, 0.999), 1e-8, step, grad_scale=0.25, zero_grad=zero, vec4=vec4)
        assert (gd.abs().sum().item() == 0) == zero
    assert relerr(pd, torch.cat([q1, q2]).detach()) < 1e-5


def test_launch_plan_replays_the_same_launches_and_samples_them():
    """ops.Plan / vfm_run_plan: a recorded GEMM -> LayerNorm -> cast -> accumulate-copy sequence gives bit-identical results to the same calls
    issued one by one, twice in a row; a partial replay (start / count) runs just those entries; an unknown entry kind fails with its index;
    the library's event sampler (vfm_prof_config / vfm_prof_read) times the sampled GEMM entries."""
    from vfmseg_amd import lib as L
    a, b = rnd(300, 256, seed=120).bfloat16().to(DEV), rnd(192, 256, seed=121).bfloat16().to(DEV)
    bias, w, g = rnd(192, seed=122).to(DEV), (rnd(192, seed=123) * 0.1 + 1).to(DEV), rnd(192, seed=124).to(DEV)

    def bufs():
        return dict(c=torch.full((300, 192), float("nan"), device=DEV), y=torch.empty(300, 192, dtype=torch.bfloat16, device=DEV),
                    st=torch.empty(300, 2, device=DEV), z=torch.empty(300, 192, device=DEV), acc=torch.ones(300, 192, device=DEV))
    r = bufs()
    ops.gemm(a, b, r["c"], bias=bias)
    ops.layernorm_fwd(r["c"], w, g, 1e-6, r["y"], r["st"])
    ops.cast(r["y"], r["z"], w)
    ops.strided_copy(r["z"], r["acc"], (300, 192), (192, 1), (192, 1), accumulate=True)
    p = bufs()
    pl = ops.Plan()
    pl.gemm(a, b, p["c"], bias=bias)
    pl.layernorm_fwd(p["c"], w, g, 1e-6, p["y"], p["st"])
    i_cast = pl.cast(p["y"], p["z"], w)
    pl.strided_copy(p["z"], p["acc"], (300, 192), (192, 1), (192, 1), accumulate=True)
    assert len(pl) == 4
    ops.prof_config(1)
    try:
        pl.run()
        recs = ops.prof_read()
    finally:
        ops.prof_config(0)
    assert [k for k, _, _ in recs] == ["gemm"] and recs[0][1] == 2.0 * 300 * 192 * 256 and recs[0][2] > 0
    for k in ("c", "y", "st", "z", "acc"):
        assert torch.equal(p[k], r[k]), k
    pl.run(start=i_cast, count=1)                       # only the cast again: nothing else moves
    assert torch.equal(p["acc"], r["acc"]) and torch.equal(p["z"], r["z"])
    pl.run()                                            # a second full replay accumulates once more
    assert torch.equal(p["acc"], r["acc"] + r["z"])
    bad = ops.Plan()
    bad.cast(p["y"], p["z"])
    bad.entry(0).kind = 99
    with pytest.raises(L.HipError, match="entry 0"):
        bad.run()


def test_checkpoint_converters():
    """vfmseg_amd.convert (HIP resize kernels) vs the F.interpolate calls of the reference's tools/convert_models/*."""
    from vfmseg_amd import convert
    g = torch.Generator().manual_seed(90)
    D = 64
    sd = {"patch_embed.proj.weight": torch.randn(D, 3, 14, 14, generator=g), "pos_embed": torch.randn(1, 1 + 37 * 37, D, generator=g),
          "blocks.0.attn.rope.freqs_cos": torch.zeros(4)}
    ref_k = F.interpolate(sd["patch_embed.proj.weight"], size=(16, 16), mode="bicubic", align_corners=False)
    ref_p = F.interpolate(sd["pos_embed"][:, 1:].reshape(1, 37, 37, D).permute(0, 3, 1, 2), size=(32, 32), mode="bicubic",
                          align_corners=False).permute(0, 2, 3, 1).reshape(1, 1024, D)
    out = convert.convert_dinov2(sd)
    assert relerr(out["patch_embed.proj.weight"], ref_k) < 1e-5
    assert relerr(out["pos_embed"][:, 1:], ref_p) < 1e-5 and torch.equal(out["pos_embed"][:, :1], sd["pos_embed"][:, :1])
    out = convert.convert_eva02(dict(model=sd))
    assert "blocks.0.attn.rope.freqs_cos" not in out and relerr(out["pos_embed"][:, 1:], ref_p) < 1e-5
    sam = {"image_encoder.patch_embed.proj.weight": sd["patch_embed.proj.weight"], "image_encoder.pos_embed": torch.randn(1, 64, 64, D, generator=g),
           "mask_decoder.x": torch.zeros(1)}
    out = convert.convert_sam(sam)
    ref_s = F.interpolate(sam["image_encoder.pos_embed"].permute(0, 3, 1, 2), size=(32, 32), mode="bicubic", align_corners=False).permute(0, 2, 3, 1)
    assert set(out) == {"patch_embed.proj.weight", "pos_embed"} and relerr(out["pos_embed"], ref_s) < 1e-5
    clip = {"visual.conv1.weight": sd["patch_embed.proj.weight"], "visual.positional_embedding": torch.randn(1 + 16 * 16, D, generator=g),
            "transformer.x": torch.zeros(1)}
    out = convert.convert_clip(clip, 512, 16, D)
    ref_c = F.interpolate(clip["visual.positional_embedding"][1:].reshape(1, 16, 16, D).permute(0, 3, 1, 2), size=(32, 32),
                          mode="bilinear").reshape(D, 1024).permute(1, 0)
    assert relerr(out["positional_embedding"][1:], ref_c) < 1e-5 and relerr(out["conv1.weight"], ref_k) < 1e-5


def test_seg_data_preprocessor_uint8():
    """uint8 BGR CHW samples of different sizes -> RGB, normalised, padded to `size` (mmseg SegDataPreProcessor + stack_batch)."""
    from vfmseg_amd.segmentors import SegDataPreProcessor, SegDataSample
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    pp = SegDataPreProcessor(mean=mean, std=std, size=(64, 96), bgr_to_rgb=True, pad_val=0, seg_pad_val=255)
    g = torch.Generator().manual_seed(91)
    imgs = [torch.randint(0, 256, (3, 64, 96), generator=g, dtype=torch.uint8), torch.randint(0, 256, (3, 50, 70), generator=g, dtype=torch.uint8)]
    labs = [torch.randint(0, 19, (1, 64, 96), generator=g), torch.randint(0, 19, (1, 50, 70), generator=g)]
    out = pp(dict(inputs=imgs, data_samples=[SegDataSample(gt_sem_seg=l) for l in labs]), training=True)
    x = out["inputs"].cpu()
    assert x.shape == (2, 3, 64, 96)
    for i, im in enumerate(imgs):
        ref = (im[[2, 1, 0]].float() - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
        h, w = im.shape[-2:]
        assert torch.allclose(x[i, :, :h, :w], ref, rtol=1e-6, atol=1e-6)
        assert (x[i, :, h:, :] == 0).all() and (x[i, :, :, w:] == 0).all()
        lab = out["data_samples"][i].gt_sem_seg.data
        assert lab.shape == (1, 64, 96) and torch.equal(lab[:, :h, :w], labs[i]) and (lab[:, h:, :] == 255).all() and (lab[:, :, w:] == 255).all()
        assert out["data_samples"][i].metainfo["padding_size"] == (0, 96 - w, 0, 64 - h)


@pytest.mark.parametrize("P,M,Q,ld", [(64, 4100, 3072, 1088), (64, 4100, 1024, 64), (32, 700, 256, 40)])
def test_gemm_bf16_tn_splitk(P, M, Q, ld):
    """Weight-gradient form with BOTH operands token-major (no transposed copies): slabs.sum(0) = xs^T @ y; xs is a column
    slice of a wider buffer, rows past M count as zeros."""
    wide = rnd(M, ld, seed=62).bfloat16().to(DEV)
    xs = wide[:, ld - P:] if ld - P >= 0 and (ld - P) % 8 == 0 else wide[:, :P]
    y = rnd(M, Q, seed=63).bfloat16().to(DEV)
    mp = (M + 63) // 64 * 64
    steps = mp // 64
    kch = max(d for d in range(1, 17) if steps % d == 0)
    slabs = torch.full((kch, P, Q), float("nan"), device=DEV)
    ops.gemm_splitk_tn(xs, y, slabs, kch)
    ref = xs.double().t() @ y.double()
    assert relerr(slabs.sum(0), ref) < 2e-5


@pytest.mark.parametrize("L,M,valid,P,Q,ld,alpha", [(1, 4100, 4100, 64, 3072, 1088, 1.0), (3, 1100, 1025, 64, 1024, 1088, 0.5),
                                                   (3, 300, 200, 32, 256, 40, 1.0), (1, 130, 70, 8, 64, 8, 2.0)])
def test_gemm_bf16_tn_batched(L, M, valid, P, Q, ld, alpha):
    """ops.gemm_tn_batched (one weight gradient per layer in one launch) against float64: out[l] = alpha * xs[l, :valid]^T @ y[l, :valid].
    xs is a column slice of a wider buffer (P = 64 at ld 1088: the LoRA wgrad's T columns behind the 1024 activations); valid_rows
    smaller than M and not a multiple of 64; the token rows past valid_rows hold NaN (the kernel reads them as zeros, by row index: the
    64-row steps of problem l reach into them); alpha != 1."""
    wide = rnd(L, M, ld, seed=71, scale=valid ** -0.25).bfloat16().to(DEV)
    xs = wide[:, :, ld - P:]
    y = rnd(L, M, Q, seed=72, scale=valid ** -0.25).bfloat16().to(DEV)
    wide[:, valid:] = float("nan")
    y[:, valid:] = float("nan")
    out = torch.full((L, P, Q), float("nan"), device=DEV)
    for rep in range(2):
        ops.gemm_tn_batched(xs, y, out, valid, alpha=alpha)
    assert torch.isfinite(out).all()
    ref = alpha * torch.matmul(xs[:, :valid].double().transpose(1, 2), y[:, :valid].double())
    assert relerr(out, ref) < 2e-5
    assert alpha == 1.0 or relerr(ref / alpha, ref) > 1e-1     # a dropped alpha is visible


@pytest.mark.parametrize("kch,P,Q,rows_used,sp,sq,alpha,accumulate", [
    (13, 64, 1024, 32, 1024, 1, 1.0, True),      # LoRA dA [r, in] inside the flat buffer: rows_used < P
    (13, 64, 3072, 32, 1, 32, 1.0, True),        # LoRA dB [out, r]: transposed destination (sp = 1, sq = r)
    (16, 64, 1280, 32, 1280, 1, 0.25, True),     # alpha != 1
    (4, 19, 256, 19, 256, 1, 1.0, False),        # overwrite
    (2, 24, 100, 17, 1, 24, -1.5, False)])       # transposed, rows_used < P, row stride larger than rows_used: gaps stay untouched
def test_slab_reduce(kch, P, Q, rows_used, sp, sq, alpha, accumulate):
    """ops.slab_reduce (the split-K combine that adds straight into a parameter's slot of the flat gradient buffer) against float64:
    dst[p*sp + q*sq] (+)= alpha * sum_k slabs[k, p, q] for p < rows_used; every other destination element bit-identical afterwards."""
    slabs = rnd(kch, P, Q, seed=81).to(DEV)
    n = (rows_used - 1) * sp + (Q - 1) * sq + 1 + 37
    dst = rnd(n, seed=82).to(DEV)
    before = dst.clone()
    idx = (torch.arange(rows_used, device=DEV)[:, None] * sp + torch.arange(Q, device=DEV)[None, :] * sq).reshape(-1)
    ops.slab_reduce(slabs, rows_used, dst, sp, sq, alpha=alpha, accumulate=accumulate)
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    touched[idx] = True
    assert torch.equal(dst[~touched], before[~touched])
    ref = alpha * slabs.double().sum(0)[:rows_used].reshape(-1) + (before.double()[idx] if accumulate else 0.0)
    plain = alpha * slabs.sum(0)[:rows_used].reshape(-1) + (before[idx] if accumulate else 0.0)
    # bound: 4 x the error of the plain fp32 torch evaluation of the same sum against float64 on the same operands (summation order is the
    # only freedom a correct kernel has); measured on these cases 5.7e-8 .. 1.1e-7, so the bound is 2.4e-7 .. 4.5e-7
    # (floor: one fp32 rounding, 2^-24); the kernel itself 5.7e-8 .. 1.6e-7
    e, e_plain = relerr(dst[idx], ref), relerr(plain, ref)
    print(f"[slab_reduce kch {kch} P {P} Q {Q}] rel err {e:.2e}, plain fp32 evaluation {e_plain:.2e}")
    assert e <= 4.0 * max(e_plain, 2.0 ** -24)
