"""Recorder / replayer of the GEMM and attention launches a model issues (a plain helper module; imports without a GPU).

`Recorder` hooks the places where `vfmseg_amd.ops` builds a launch descriptor and keeps, per kind, the DISTINCT launches: operand
shapes, strides and dtypes, epilogue, scalar arguments, aliasing of residual and C.  `REPLAY[kind](key, seed)` then issues the same call
through the default dispatcher on fresh operands and compares it with a float64 evaluation of the documented formula on the device.

Operand contracts (include/vfmseg_hip.h, the `ops` docstrings):
- every element of an operand's storage OUTSIDE the recorded view (ld padding, the columns of a packed buffer the view leaves out) is NaN;
- where the kernel masks (token rows >= valid_rows / >= M of gemm_tn_batched / gemm_splitk_tn "read as zeros", B rows >= kb_rows of
  gemm_splitk_bt "clamped") the storage is grown to the padded row count and those rows are NaN: a kernel that reads them shows;
- where the duty is the caller's ("A must be zero beyond" kb_rows) the replay zeroes them;
- every output is NaN-prefilled; the view must come back finite and everything outside it must still be NaN (or unchanged).

Operand scaling: A and B of a GEMM are N(0, 1) * (K |alpha|) ** -0.25, so alpha * accumulator has unit variance like every epilogue operand
(bias, residual, aux, colscale are N(0, 1)); `_check_mutants` asserts, from the float64 reference alone, that leaving out any present
term moves the reference by >= 10 x the launch's tolerance (5 x for the last 64 of K): a condition on the inputs, not on the kernel.

Tolerances (metric max |a - b| / max |b|) are the project's: fp32 output 2e-5, half output 1e-2 (tests/test_kernels_gpu.py), attention
half 2e-2 forward and 2 x that for dq / dk / dv, fp32 attention 2e-5; SAM flash 2e-2 forward, 3e-2 backward (tests/test_sam_flash_gpu.py).
lse and slab_reduce have no bound in the project: 4 x the error of a plain fp32 torch evaluation of the same formula on the same
operands against float64 (summation order is the only freedom a correct kernel has)."""
import torch
import torch.nn.functional as F

from vfmseg_amd import ops

DEV = "cuda"
NAN = float("nan")
KINDS = ("gemm", "splitk_bt", "splitk_tn", "tn_batched", "slab_reduce", "attn_fwd", "attn_bwd", "sam_fwd_train", "sam_bwd")


def spec(t):
    return None if t is None else (tuple(t.shape), tuple(t.stride()), t.dtype)


def _same_storage(a, b):
    return a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.stride() == b.stride()


def relerr(a, b):
    """max |a - b| / max |b| on the device, in float64"""
    b = b.double()
    return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def out_tol(dt):
    return 2e-5 if dt == torch.float32 else 1e-2


# ---------------------------------------------------------------------------------------------------------------- recording
class Recorder:
    """with Recorder() as rec: <run the model>  ->  rec.launches[kind] = {key: count}."""

    def __init__(self):
        self.launches = {k: {} for k in KINDS}
        self._in_bwd = 0
        self._saved = []

    def _add(self, kind, key):
        d = self.launches[kind]
        d[key] = d.get(key, 0) + 1

    def _patch(self, obj, name, new):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)

    def __enter__(self):
        rec = self
        o_gd, o_ad = ops.gemm_desc, ops._attn_desc
        o_bt, o_tn, o_tb, o_sr = ops.gemm_splitk_bt, ops.gemm_splitk_tn, ops.gemm_tn_batched, ops.slab_reduce
        o_ab, o_pab = ops.attn_bwd, ops.Plan.attn_bwd
        o_sf, o_sb = ops.sam_attn_flash_fwd_train, ops.sam_attn_flash_bwd

        def gemm_desc(a, b, c, *, alpha=1.0, bias=None, bias_mod=0, colscale=None, residual=None, ep_mode=ops.EP_NONE, aux=None, c2=None,
                      trans_a=False, trans_b=False, kb_rows=0, d=None):
            rec._add("gemm", (spec(a), spec(b), spec(c), float(alpha), spec(bias), int(bias_mod), spec(colscale), spec(residual),
                              _same_storage(residual, c), int(ep_mode), spec(aux), spec(c2), bool(trans_a), bool(trans_b), int(kb_rows)))
            return o_gd(a, b, c, alpha=alpha, bias=bias, bias_mod=bias_mod, colscale=colscale, residual=residual, ep_mode=ep_mode, aux=aux,
                        c2=c2, trans_a=trans_a, trans_b=trans_b, kb_rows=kb_rows, d=d)

        def attn_desc(q, k, v, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse):
            if not rec._in_bwd:   # _attn_desc alone cannot tell forward from backward: the backward callers raise the flag
                rec._add("attn_fwd", (spec(q), spec(k), spec(v), spec(o), B, H, d, nq_main, nq_extra, nk_main, nk_extra, float(scale),
                                      lse is not None))
            return o_ad(q, k, v, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse)

        def _bwd_key(q, k, v, o, lse, dout, dq, dk, dv, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale):
            return (spec(q), spec(k), spec(v), spec(o), spec(dout), spec(dq), spec(dk), spec(dv), B, H, d, nq_main, nq_extra, nk_main,
                    nk_extra, float(scale))

        def attn_bwd(*a):
            rec._add("attn_bwd", _bwd_key(*a))
            rec._in_bwd += 1
            try:
                return o_ab(*a)
            finally:
                rec._in_bwd -= 1

        def plan_attn_bwd(self_, *a):
            rec._add("attn_bwd", _bwd_key(*a))
            rec._in_bwd += 1
            try:
                return o_pab(self_, *a)
            finally:
                rec._in_bwd -= 1

        def splitk_bt(at, y, slabs, kch):
            rec._add("splitk_bt", (spec(at), spec(y), spec(slabs), int(kch)))
            return o_bt(at, y, slabs, kch)

        def splitk_tn(xs, y, slabs, kch):
            rec._add("splitk_tn", (spec(xs), spec(y), spec(slabs), int(kch)))
            return o_tn(xs, y, slabs, kch)

        def tn_batched(xs, y, out, valid_rows, alpha=1.0):
            rec._add("tn_batched", (spec(xs), spec(y), spec(out), int(valid_rows), float(alpha)))
            return o_tb(xs, y, out, valid_rows, alpha=alpha)

        def slab_reduce(slabs, rows_used, dst, sp, sq, alpha=1.0, accumulate=False):
            rec._add("slab_reduce", (spec(slabs), int(rows_used), int(dst.numel()), int(sp), int(sq), float(alpha), bool(accumulate)))
            return o_sr(slabs, rows_used, dst, sp, sq, alpha=alpha, accumulate=accumulate)

        def sam_fwd_train(qkv, bias, tbl_h, tbl_w, out, lse, qext, nimg, G, S, H, d, scale):
            rec._add("sam_fwd_train", (spec(qkv), spec(out), spec(tbl_h), nimg, G, S, H, d, float(scale)))
            return o_sf(qkv, bias, tbl_h, tbl_w, out, lse, qext, nimg, G, S, H, d, scale)

        def sam_bwd(qkv, bias, tbl_h, tbl_w, out, dout, lse, qext, dqkv, nimg, G, S, H, d, scale):
            rec._add("sam_bwd", (spec(qkv), spec(out), spec(dout), spec(dqkv), spec(tbl_h), nimg, G, S, H, d, float(scale)))
            return o_sb(qkv, bias, tbl_h, tbl_w, out, dout, lse, qext, dqkv, nimg, G, S, H, d, scale)

        for obj, name, new in ((ops, "gemm_desc", gemm_desc), (ops, "_attn_desc", attn_desc), (ops, "attn_bwd", attn_bwd),
                               (ops.Plan, "attn_bwd", plan_attn_bwd), (ops, "gemm_splitk_bt", splitk_bt), (ops, "gemm_splitk_tn", splitk_tn),
                               (ops, "gemm_tn_batched", tn_batched), (ops, "slab_reduce", slab_reduce),
                               (ops, "sam_attn_flash_fwd_train", sam_fwd_train), (ops, "sam_attn_flash_bwd", sam_bwd)):
            self._patch(obj, name, new)
        return self

    def __exit__(self, *exc):
        for obj, name, old in reversed(self._saved):
            setattr(obj, name, old)
        self._saved = []
        return False


# ---------------------------------------------------------------------------------------------------------------- operands
def _randn(shape, seed, scale, dt):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).mul_(scale).to(dt)


def fresh(sp, seed, scale=1.0, grow=None, fill=None):
    """A tensor with the recorded shape / strides / dtype: N(0, scale^2) values in the view (or `fill`), NaN everywhere else in its storage.
    grow=(dim, n): the storage is that of the same view with n entries along `dim` (the extra ones NaN): rows a masking kernel must not use."""
    shape, stride, dt = sp
    big = list(shape)
    if grow is not None:
        big[grow[0]] = max(grow[1], shape[grow[0]])
    t = torch.empty_strided(big, stride, dtype=dt, device=DEV)
    n = t.untyped_storage().nbytes() // t.element_size()
    torch.as_strided(t, (n,), (1,), 0).fill_(NAN)
    v = torch.as_strided(t, shape, stride, 0)
    if fill is None:
        v.copy_(_randn(shape, seed, scale, dt))
    else:
        v.fill_(fill)
    return v


def outside_is_nan(t):
    """Every element of t's storage outside the view t is still NaN."""
    n = t.untyped_storage().nbytes() // t.element_size()
    inside = torch.zeros(n, dtype=torch.bool, device=t.device)
    torch.as_strided(inside, t.shape, t.stride(), t.storage_offset()).fill_(True)
    flat = torch.as_strided(t, (n,), (1,), 0)
    return bool(torch.isnan(flat[~inside].float()).all())


def _gelu_grad(x):
    x = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        F.gelu(x).sum().backward()
    return x.grad


def _qgelu(x):
    return x * torch.sigmoid(1.702 * x)


def _qgelu_grad(x):
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1.0 - s)


_ACT = {ops.EP_GELU: F.gelu, ops.EP_GELU_DGELU: F.gelu, ops.EP_RELU: F.relu, ops.EP_QGELU: _qgelu}
_AUX = {ops.EP_MUL: lambda x: x, ops.EP_MUL_GELU_GRAD: _gelu_grad, ops.EP_MUL_QGELU_GRAD: _qgelu_grad}
_KNOWN_EP = (ops.EP_NONE,) + tuple(_ACT) + tuple(_AUX)


# ---------------------------------------------------------------------------------------------------------------- GEMM
def _gemm_reference(acc, alpha, bias, bias_mod, ep, aux, cs, res, drop=None, bias_rows=None):
    """include/vfmseg_hip.h epilogue order in float64; `drop` leaves one term out (the mutants of _check_mutants).  -> (C, pre-activation)"""
    v = (1.0 if drop == "alpha" else alpha) * acc
    if bias is not None and drop != "bias":
        n = v.shape[-1]
        bv = bias[torch.arange(n, device=v.device) % (bias_mod if bias_mod else n)]
        if drop == "bias_tail_rows":
            v = v.clone()
            v[..., :bias_rows, :] += bv
        else:
            v = v + bv
    pre = v
    if ep in _ACT and drop != "act":
        v = _ACT[ep](v)
    if ep in _AUX and drop != "aux":
        v = v * _AUX[ep](aux)
    if cs is not None and drop != "colscale":
        v = v * cs
    if res is not None and drop != "residual":
        v = v + res
    return v, pre


def _check_mutants(key, ref, tol, acc, acc_tail, alpha, bias, bias_mod, ep, aux, cs, res):
    """From the float64 reference alone: each present term left out in turn must move the reference by >= 10 x tol (the last 64 of K: 5 x)
    in the launch's own metric, else a kernel that dropped the term would pass.  -> {mutant: distance}"""
    M = ref.shape[-2]
    muts = []
    if bias is not None:
        muts.append(("bias", 10.0))
        if M % 128 and M > 128:
            muts.append(("bias_tail_rows", 10.0))
    if cs is not None:
        muts.append(("colscale", 10.0))
    if res is not None:
        muts.append(("residual", 10.0))
    if ep in _AUX:
        muts.append(("aux", 10.0))
    if ep in _ACT:
        muts.append(("act", 10.0))
    if alpha != 1.0:
        muts.append(("alpha", 10.0))
    dist = {}
    for name, factor in muts:
        mut, _ = _gemm_reference(acc, alpha, bias, bias_mod, ep, aux, cs, res, drop=name, bias_rows=M - M % 128)
        dist[name] = relerr(mut, ref)
        assert dist[name] >= factor * tol, (key, "the reference cannot see a missing " + name, dist[name], factor * tol)
    mut, _ = _gemm_reference(acc - acc_tail, alpha, bias, bias_mod, ep, aux, cs, res)
    dist["k_tail"] = relerr(mut, ref)
    assert dist["k_tail"] >= 5.0 * tol, (key, "the reference cannot see a missing last K chunk", dist["k_tail"], 5.0 * tol)
    return dist


def replay_gemm(key, seed):
    """ops.gemm (ops.gemm_desc) on fresh operands -> {"c": rel err[, "c2": rel err], "mutants": {...}}"""
    (sa, sb, sc, alpha, sbias, bias_mod, scs, sres, res_alias, ep, saux, sc2, ta, tb, kb) = key
    assert ep in _KNOWN_EP, f"replay has no reference for ep_mode {ep}"
    assert kb >= 0 and (not kb or (tb and len(sa[0]) == 2)), ("replay has no reference for this kb_rows launch", key)
    K = kb if kb else (sa[0][-2] if ta else sa[0][-1])
    s = (K * abs(alpha)) ** -0.25
    a, b = fresh(sa, seed, s), fresh(sb, seed + 1, s)
    if kb:
        a[:, kb:] = 0     # vfmseg_hip.h kb_rows: "A must be zero beyond" is the caller's duty (B's own rows end at kb_rows)
    bias = fresh(sbias, seed + 3) if sbias else None
    cs = fresh(scs, seed + 4) if scs else None
    if res_alias:
        c = fresh(sc, seed + 2)
        res, res_val = c, c.double().clone()
    else:
        c = fresh(sc, seed + 2, fill=NAN)
        res = fresh(sres, seed + 5) if sres else None
        res_val = None if res is None else res.double()
    aux = fresh(saux, seed + 6) if saux else None
    c2 = fresh(sc2, seed + 7, fill=NAN) if sc2 else None
    ops.gemm(a, b, c, alpha=alpha, bias=bias, bias_mod=bias_mod, colscale=cs, residual=res, ep_mode=ep, aux=aux, c2=c2,
             trans_a=ta, trans_b=tb, kb_rows=kb)
    ad = a.double().transpose(-1, -2) if ta else a.double()      # [.., M, K]
    bd = b.double() if tb else b.double().transpose(-1, -2)      # [.., K(b), N]
    kk = bd.shape[-2]
    acc = torch.matmul(ad[..., :kk], bd)
    t0 = max(ad.shape[-1] - 64, 0)                               # the last 64 of K (with kb_rows: of A's K, of which B holds the first kb)
    acc_tail = torch.matmul(ad[..., t0:kk], bd[..., t0:kk, :]) if t0 < kk else torch.zeros_like(acc)
    biasd = None if bias is None else bias.double()
    auxd = None if aux is None else aux.double()
    csd = None if cs is None else cs.double()
    ref, pre = _gemm_reference(acc, alpha, biasd, bias_mod, ep, auxd, csd, res_val)
    tol = out_tol(c.dtype)
    out = {"mutants": _check_mutants(key, ref, tol, acc, acc_tail, alpha, biasd, bias_mod, ep, auxd, csd, res_val)}
    assert bool(torch.isfinite(c.float()).all()) and outside_is_nan(c), (key, "C: unwritten elements or a write outside the view")
    out["c"] = relerr(c, ref)
    assert out["c"] < tol, (key, out["c"])
    if c2 is not None:
        want2 = _gelu_grad(pre) if ep == ops.EP_GELU_DGELU else pre
        assert bool(torch.isfinite(c2.float()).all()) and outside_is_nan(c2), (key, "C2: unwritten elements or a write outside the view")
        out["c2"] = relerr(c2, want2)
        assert out["c2"] < out_tol(c2.dtype), (key, out["c2"])
    return out


def _pad64(n):
    return (n + 63) // 64 * 64


def replay_splitk_bt(key, seed):
    """ops.gemm_splitk_bt: slabs.sum(0) = at[:, :M] @ y; `at` zero beyond M (caller), y's rows >= M clamped by the kernel (NaN here)."""
    (sat, sy, ssl, kch) = key
    M, mp = sy[0][0], sat[0][1]
    s = M ** -0.25
    at, y = fresh(sat, seed, s), fresh(sy, seed + 1, s, grow=(0, mp))
    at[:, M:] = 0
    slabs = fresh(ssl, seed + 2, fill=NAN)
    ops.gemm_splitk_bt(at, y, slabs, kch)
    assert bool(torch.isfinite(slabs).all()) and outside_is_nan(slabs), key
    err = relerr(slabs.double().sum(0), at.double()[:, :M] @ y.double())
    assert err < 2e-5, (key, err)
    return {"sum": err}


def replay_splitk_tn(key, seed):
    """ops.gemm_splitk_tn: slabs.sum(0) = xs^T @ y; token rows >= M read as zeros by the kernel (NaN here)."""
    (sxs, sy, ssl, kch) = key
    M = sxs[0][0]
    s = M ** -0.25
    xs, y = fresh(sxs, seed, s, grow=(0, _pad64(M))), fresh(sy, seed + 1, s, grow=(0, _pad64(M)))
    slabs = fresh(ssl, seed + 2, fill=NAN)
    ops.gemm_splitk_tn(xs, y, slabs, kch)
    assert bool(torch.isfinite(slabs).all()) and outside_is_nan(slabs), key
    err = relerr(slabs.double().sum(0), xs.double().t() @ y.double())
    assert err < 2e-5, (key, err)
    return {"sum": err}


def replay_tn_batched(key, seed):
    """ops.gemm_tn_batched: out[l] = alpha * xs[l, :valid]^T @ y[l, :valid]; rows >= valid_rows read as zeros by the kernel (NaN here, the rows
    the last problem's 64-row steps reach past the end of the buffer included)."""
    (sxs, sy, so, valid, alpha) = key
    M = sxs[0][1]
    s = (valid * abs(alpha)) ** -0.25
    xs, y = fresh(sxs, seed, s, grow=(1, _pad64(valid))), fresh(sy, seed + 1, s, grow=(1, _pad64(valid)))
    if valid < M:
        xs[:, valid:], y[:, valid:] = NAN, NAN
    out = fresh(so, seed + 2, fill=NAN)
    ops.gemm_tn_batched(xs, y, out, valid, alpha=alpha)
    assert bool(torch.isfinite(out).all()), key
    ref = alpha * torch.matmul(xs.double()[:, :valid].transpose(1, 2), y.double()[:, :valid])
    err = relerr(out, ref)
    assert err < 2e-5, (key, err)
    if alpha != 1.0:   # the reference can see a missing alpha
        assert relerr(ref / alpha, ref) >= 10 * 2e-5, key
    return {"out": err}


def slab_reduce_case(kch, P, Q, rows_used, dst_numel, sp, sq, alpha, accumulate, seed):
    """One ops.slab_reduce call against float64.  -> (rel err of the kernel, rel err of the plain fp32 torch evaluation, both against float64)
    Asserts that the destination elements the formula does not name are bit-identical afterwards."""
    slabs = _randn((kch, P, Q), seed, 1.0, torch.float32)
    n = max(dst_numel, (rows_used - 1) * sp + (Q - 1) * sq + 1)
    dst = _randn((n,), seed + 1, 1.0, torch.float32)
    before = dst.clone()
    idx = (torch.arange(rows_used, device=DEV)[:, None] * sp + torch.arange(Q, device=DEV)[None, :] * sq).reshape(-1)
    assert idx.unique().numel() == idx.numel(), "destination indices collide"
    ops.slab_reduce(slabs, rows_used, dst, sp, sq, alpha=alpha, accumulate=accumulate)
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    touched[idx] = True
    assert torch.equal(dst[~touched], before[~touched]), "slab_reduce wrote outside dst[p*sp + q*sq], p < rows_used"
    ref = alpha * slabs.double().sum(0)[:rows_used].reshape(-1) + (before.double()[idx] if accumulate else 0.0)
    plain = (alpha * slabs.sum(0)[:rows_used].reshape(-1) + (before[idx] if accumulate else 0.0))    # the same formula in fp32
    return relerr(dst[idx], ref), relerr(plain, ref)


def replay_slab_reduce(key, seed):
    (ssl, rows_used, dst_numel, sp, sq, alpha, accumulate) = key
    kch, P, Q = ssl[0]
    err, plain = slab_reduce_case(kch, P, Q, rows_used, dst_numel, sp, sq, alpha, accumulate, seed)
    # no bound in the project: 4 x the error of the plain fp32 evaluation (torch's sum) of the same formula on the same operands.  Measured
    # on the train steps' launches (2 .. 128 slabs of N(0, 1) values): plain evaluation 7.5e-8 .. 1.5e-7, so the bound is 3e-7 .. 6e-7; the
    # kernel (a sequential sum, fixed order) 9.4e-8 .. 4.3e-7, its worst ratio 3.9 at 128 slabs.  Floor: one fp32 rounding of the result
    # (2^-24 = 6e-8 of the largest element), since the plain evaluation can come out exact on a small case.
    bound = 4.0 * max(plain, 2.0 ** -24)
    assert err <= bound, (key, err, plain, bound)
    return {"dst": err, "fp32_eval": plain}


# ---------------------------------------------------------------------------------------------------------------- attention
def _gather(t, B, H, d, n, ne, b):
    """image b of a token-major [rows, >= H*d] view -> [H, n + ne, d]"""
    main = t[b * n:(b + 1) * n, :H * d].reshape(n, H, d)
    if ne:
        main = torch.cat([main, t[B * n + b:B * n + b + 1, :H * d].reshape(1, H, d)], 0)
    return main.permute(1, 0, 2)


def _scatter(dst, g, B, H, d, n, ne, b):
    """[H, n + ne, d] -> rows of image b of the token-major dst [rows, H*d]"""
    g = g.permute(1, 0, 2).reshape(n + ne, H * d)
    dst[b * n:(b + 1) * n] = g[:n]
    if ne:
        dst[B * n + b] = g[n]


def replay_attn_fwd(key, seed):
    """ops.attn_fwd against float64 softmax(q k^T scale) v; with lse: against float64 logsumexp of the scaled scores."""
    (sq, sk, sv, so, B, H, d, nq, nqe, nk, nke, scale, has_lse) = key
    q, k, v = fresh(sq, seed), fresh(sk, seed + 1), fresh(sv, seed + 2)
    o = fresh(so, seed + 3, fill=NAN)
    lse = torch.full((B, H, nq + nqe), NAN, device=DEV) if has_lse else None
    ops.attn_fwd(q, k, v, o, lse, B, H, d, nq, nqe, nk, nke, scale)
    tol = 2e-5 if q.dtype == torch.float32 else 2e-2
    assert bool(torch.isfinite(o.float()).all()) and outside_is_nan(o), (key, "o: unwritten elements or a write outside the view")
    out = {"o": 0.0}
    lse_ref, lse_plain = [], []
    for b in range(B):
        qq, kk, vv = (_gather(t, B, H, d, n, ne, b).double() for t, n, ne in ((q, nq, nqe), (k, nk, nke), (v, nk, nke)))
        sc = (qq @ kk.transpose(-1, -2)) * scale
        out["o"] = max(out["o"], relerr(_gather(o, B, H, d, nq, nqe, b), sc.softmax(-1) @ vv))
        if has_lse:
            lse_ref.append(torch.logsumexp(sc, -1))
            lse_plain.append(torch.logsumexp((qq.float() @ kk.float().transpose(-1, -2)) * scale, -1))
    assert out["o"] < tol, (key, out["o"])
    if has_lse:
        ref = torch.stack(lse_ref)
        out["lse"], out["lse_fp32_eval"] = relerr(lse, ref), relerr(torch.stack(lse_plain), ref)
        # no bound in the project for the 16-bit kernels' lse: 4 x the error of the plain fp32 evaluation of logsumexp(q k^T scale) on the same
        # operands.  Measured at 1024 / 1025 keys, d = 64 (max |lse| ~ 8): plain evaluation 1.0e-7 .. 1.1e-7 of max |lse|, so the bound is
        # 4.0e-7 .. 4.4e-7; the kernels 1.5e-7 .. 2.0e-7
        assert out["lse"] <= 4.0 * out["lse_fp32_eval"], (key, out["lse"], out["lse_fp32_eval"])
    return out


def replay_attn_bwd(key, seed):
    """ops.attn_bwd against float64 autograd of softmax(q k^T scale) v; o and lse handed in are the float64 forward's (rounded)."""
    (sq, sk, sv, so, sdo, sdq, sdk, sdv, B, H, d, nq, nqe, nk, nke, scale) = key
    q, k, v = fresh(sq, seed), fresh(sk, seed + 1), fresh(sv, seed + 2)
    do = fresh(sdo, seed + 3)
    o = fresh(so, seed + 4, fill=0.0)
    dq, dk, dv = fresh(sdq, seed + 5, fill=NAN), fresh(sdk, seed + 6, fill=NAN), fresh(sdv, seed + 7, fill=NAN)
    lse = torch.empty(B, H, nq + nqe, device=DEV)
    hd = H * d
    rq, rk, rv = (torch.empty(t.shape[0], hd, dtype=torch.float64, device=DEV) for t in (q, k, v))
    for b in range(B):
        qq, kk, vv = (_gather(t, B, H, d, n, ne, b).double().requires_grad_(True) for t, n, ne in ((q, nq, nqe), (k, nk, nke), (v, nk, nke)))
        with torch.enable_grad():
            sc = (qq @ kk.transpose(-1, -2)) * scale
            ref = sc.softmax(-1) @ vv
            ref.backward(_gather(do, B, H, d, nq, nqe, b).double())
        lse[b] = torch.logsumexp(sc.detach(), -1).float()
        _scatter(o[:, :hd], ref.detach().to(o.dtype), B, H, d, nq, nqe, b)
        for dst, g, n, ne in ((rq, qq.grad, nq, nqe), (rk, kk.grad, nk, nke), (rv, vv.grad, nk, nke)):
            _scatter(dst, g, B, H, d, n, ne, b)
    ops.attn_bwd(q, k, v, o, lse, do, dq, dk, dv, B, H, d, nq, nqe, nk, nke, scale)
    tol = 2.0 * (2e-5 if q.dtype == torch.float32 else 2e-2)
    out = {}
    for name, got, want in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
        assert bool(torch.isfinite(got.float()).all()) and outside_is_nan(got), (key, name + ": unwritten elements or a write outside the view")
        out[name] = relerr(got[:, :hd], want)
        assert out[name] < tol, (key, name, out[name])
    return out


# ---------------------------------------------------------------------------------------------------------------- SAM flash
def _sam_operands(sqkv, stbl, nimg, G, S, H, d, seed):
    from tests.test_sam_flash_gpu import _tables     # the reference math lives there (a float64 restatement of sam_vit.py)
    g = torch.Generator().manual_seed(seed)
    L = 27 if S == 14 else 127                       # the rel-pos parameter lengths of SAM-H (global blocks re-interpolate 127 -> 63)
    qkv = (torch.randn(nimg * G * G, 3 * H * d, generator=g) * 1.5).to(sqkv[2])
    bias = torch.randn(3 * H * d, generator=g) * 0.5
    rel_h, rel_w = torch.randn(L, d, generator=g) * 0.3, torch.randn(L, d, generator=g) * 0.3
    JP = stbl[0][0]
    th, tw = _tables(rel_h, S, JP).to(stbl[2]), _tables(rel_w, S, JP).to(stbl[2])
    qkv_d = fresh(sqkv, 0, fill=0.0)
    qkv_d.copy_(qkv)
    return qkv, qkv_d, bias, rel_h, rel_w, th, tw


def replay_sam_fwd_train(key, seed):
    from tests.helpers import rel_err
    from tests.test_sam_flash_gpu import _ref
    (sqkv, so, stbl, nimg, G, S, H, d, scale) = key
    assert abs(scale - d ** -0.5) < 1e-7, key      # the reference math scales by d ** -0.5
    qkv, qkv_d, bias, rel_h, rel_w, th, tw = _sam_operands(sqkv, stbl, nimg, G, S, H, d, seed)
    out = fresh(so, seed + 1, fill=NAN)
    lse, qext = ops.sam_attn_flash_stats(nimg, G, S, H, DEV)
    ops.sam_attn_flash_fwd_train(qkv_d, bias.to(DEV), th, tw, out, lse, qext, nimg, G, S, H, d, scale)
    assert bool(torch.isfinite(out.float()).all()) and outside_is_nan(out), key
    e = rel_err(out.float().cpu(), _ref(qkv.float(), bias, rel_h, rel_w, nimg, G, S, H, d))
    assert e < 2e-2, (key, e)      # the bound of tests/test_sam_flash_gpu.py::test_sam_flash_forward_matches_reference_math
    return {"out": e}


def replay_sam_bwd(key, seed):
    from tests.helpers import rel_err
    from tests.test_sam_flash_gpu import _ref
    (sqkv, so, sdo, sdqkv, stbl, nimg, G, S, H, d, scale) = key
    assert abs(scale - d ** -0.5) < 1e-7, key
    qkv, qkv_d, bias, rel_h, rel_w, th, tw = _sam_operands(sqkv, stbl, nimg, G, S, H, d, seed)
    out = fresh(so, seed + 1, fill=NAN)
    dout = fresh(sdo, seed + 2)
    dqkv = fresh(sdqkv, seed + 3, fill=NAN)
    lse, qext = ops.sam_attn_flash_stats(nimg, G, S, H, DEV)
    ops.sam_attn_flash_fwd_train(qkv_d, bias.to(DEV), th, tw, out, lse, qext, nimg, G, S, H, d, scale)
    ops.sam_attn_flash_bwd(qkv_d, bias.to(DEV), th, tw, out, dout, lse, qext, dqkv, nimg, G, S, H, d, scale)
    assert bool(torch.isfinite(dqkv.float()).all()) and outside_is_nan(dqkv), (key, "dqkv: every element must be written")
    x = qkv.double().requires_grad_(True)
    with torch.enable_grad():
        _ref(x, bias, rel_h, rel_w, nimg, G, S, H, d).backward(dout.double().cpu())
    C = H * d
    got, res = dqkv.float().cpu(), {}
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        res[name] = rel_err(got[:, sl], x.grad[:, sl])
        assert res[name] < 3e-2, (key, name, res[name])     # tests/test_sam_flash_gpu.py::test_sam_flash_backward_matches_autograd
    return res


# ---------------------------------------------------------------------------------------------------------------- driver
REPLAY = {"gemm": replay_gemm, "splitk_bt": replay_splitk_bt, "splitk_tn": replay_splitk_tn, "tn_batched": replay_tn_batched,
          "slab_reduce": replay_slab_reduce, "attn_fwd": replay_attn_fwd, "attn_bwd": replay_attn_bwd,
          "sam_fwd_train": replay_sam_fwd_train, "sam_bwd": replay_sam_bwd}


def _fmt(res):
    parts = [f"{k} {v:.1e}" for k, v in res.items() if k != "mutants"]
    if res.get("mutants"):
        parts.append("mutant distances " + " ".join(f"{k} {v:.2f}" for k, v in res["mutants"].items()))
    return ", ".join(parts)


def describe(kind, key, count):
    if kind == "gemm":
        return (f"[replay gemm] A{key[0][0]}{'^T' if key[12] else ''} B{key[1][0]}{'^T' if key[13] else ''} -> C{key[2][0]} {key[2][2]} "
                f"ld(a,c)=({key[0][1][-2]},{key[2][1][-2]}) ep {key[9]} alpha {key[3]:g} bias {key[4] is not None} colscale {key[6] is not None} "
                f"residual {key[7] is not None}{' (C)' if key[8] else ''} c2 {key[11] is not None} kb_rows {key[14]} x{count}")
    if kind in ("splitk_bt", "splitk_tn"):
        return f"[replay {kind}] A{key[0][0]} ld {key[0][1][0]} B{key[1][0]} ld {key[1][1][0]} -> slabs{key[2][0]} kch {key[3]} x{count}"
    if kind == "tn_batched":
        return (f"[replay tn_batched] xs{key[0][0]} strides {key[0][1]} y{key[1][0]} strides {key[1][1]} -> out{key[2][0]} valid_rows {key[3]} "
                f"alpha {key[4]:g} x{count}")
    if kind == "slab_reduce":
        return f"[replay slab_reduce] slabs{key[0][0]} rows_used {key[1]} sp {key[3]} sq {key[4]} alpha {key[5]:g} accumulate {key[6]} x{count}"
    if kind == "attn_fwd":
        return (f"[replay attn] B {key[4]} H {key[5]} d {key[6]} nq {key[7]}+{key[8]} nk {key[9]}+{key[10]} {key[0][2]} "
                f"ld {key[0][1][0]} lse {key[12]} x{count}")
    if kind == "attn_bwd":
        return (f"[replay attn_bwd] B {key[8]} H {key[9]} d {key[10]} nq {key[11]}+{key[12]} nk {key[13]}+{key[14]} {key[0][2]} "
                f"ld(q,k,do,dq) ({key[0][1][0]},{key[1][1][0]},{key[4][1][0]},{key[5][1][0]}) x{count}")
    n = 3 if kind == "sam_fwd_train" else 5
    return f"[replay {kind}] nimg {key[n]} G {key[n + 1]} S {key[n + 2]} H {key[n + 3]} d {key[n + 4]} {key[0][2]} ld {key[0][1][0]} x{count}"


def replay_all(launches, tag="", seed0=1000):
    """Replays every distinct launch once, prints one line per launch.  -> {kind: {result name: worst error}}"""
    worst = {}
    seed = seed0
    for kind in KINDS:
        for key in sorted(launches[kind], key=repr):
            res = REPLAY[kind](key, seed)
            seed += 16
            print(f"{tag}{describe(kind, key, launches[kind][key])}: {_fmt(res)}")
            w = worst.setdefault(kind, {})
            for k, v in res.items():
                if k == "mutants":
                    continue
                if kind == "gemm":      # fp32 and 16-bit outputs have bounds of their own: keep their worst cases apart
                    k += " fp32" if key[2 if k == "c" else 11][2] == torch.float32 else " half"
                w[k] = max(w.get(k, 0.0), v)
    return worst
