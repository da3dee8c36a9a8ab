"""Tensor-level wrappers over the C ABI (one Python function per entry point, no autograd here).

All tensors must live on the GPU; every call is asynchronous on torch's current HIP stream.
"""
import ctypes as C
import os

import torch

from .precision import is_half
from . import lib as L
from .lib import (ACT_GELU, ACT_NONE, ACT_QGELU, ACT_RELU, BF16, EP_GELU, EP_GELU_DGELU, EP_MUL, EP_MUL_GELU_GRAD,  # noqa: F401
                  EP_MUL_QGELU_GRAD, EP_NONE, EP_QGELU, EP_RELU, F32)

_ws_cache = {}

# Measurement hook (bench.py installs it; None in production): PROFILE(kind, flops, region) -> finish() | None is called around the
# launches of the two MFMA kernel families so that HIP events bracket exactly one kernel on the stream it is launched on.
# REGION names who is launching ("backbone" inside the ViT engines, "heads" elsewhere).
PROFILE = None
REGION = ["heads"]


class region:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        REGION.append(self.name)

    def __exit__(self, *a):
        REGION.pop()


def workspace(nfloats, device, tag="default"):
    """Grow-only fp32 scratch per (device, tag, STREAM); kernels never allocate.  Per stream: the decoder heads' weight gradients run on a
    side stream (functional.wgrad_stream) - kernels that may run concurrently must not share scratch."""
    key = (str(device), tag, L.stream())
    t = _ws_cache.get(key)
    if t is None or t.numel() < nfloats:
        t = torch.empty(max(int(nfloats), 1 << 16), dtype=torch.float32, device=device)
        _ws_cache[key] = t
    return t


def ld_pad(cols, dtype):
    """Extra columns for a row-major buffer whose rows would otherwise be a multiple of 8 KiB apart: with such a stride the
    128 rows of a GEMM tile fall on a few L2 channels and the LDS-DMA operand stream loses ~10 % (measured at K = 4096:
    ld 4096 -> 744 TF, ld 4224 -> 815 TF; 128- or 16-byte pads are worse than none)."""
    esz = torch.empty(0, dtype=dtype).element_size()
    return (256 // esz) if (cols * esz) % 8192 == 0 else 0


def empty_ld(rows, cols, dtype, device, zero=False):
    """[rows, cols] view of a buffer whose leading dimension avoids the 8-KiB stride (see ld_pad)."""
    pad = ld_pad(cols, dtype)
    make = torch.zeros if zero else torch.empty
    if pad == 0:
        return make(rows, cols, dtype=dtype, device=device)
    return make(rows, cols + pad, dtype=dtype, device=device)[:, :cols]


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major 2-D view"
    return t.stride(0)


def cast(src, dst, colscale=None):
    """dst[r,c] = src[r,c] * colscale[c]; src/dst 2-D row-major views (may be column slices)."""
    lib = L.load()
    L.check(lib.vfm_cast(L.ptr(src), L.dt_of(src), _ld(src), L.ptr(dst), L.dt_of(dst), _ld(dst), src.shape[0], src.shape[1],
                         L.ptr(colscale), L.stream()), "vfm_cast")
    return dst


def transpose(src, dst, pad_rows=None):
    """dst[c, r] = src[r, c]; dst [cols, >=pad_rows]; columns rows..pad_rows-1 zero-filled."""
    lib = L.load()
    rows, cols = src.shape
    pad_rows = rows if pad_rows is None else pad_rows
    L.check(lib.vfm_transpose(L.ptr(src), L.dt_of(src), _ld(src), L.ptr(dst), L.dt_of(dst), _ld(dst), rows, cols, pad_rows,
                              L.stream()), "vfm_transpose")
    return dst


def strided_copy(src, dst, shape, sstr, dstr, accumulate=False):
    lib = L.load()
    n = list(shape) + [1] * (4 - len(shape))
    s = list(sstr) + [0] * (4 - len(sstr))
    d = list(dstr) + [0] * (4 - len(dstr))
    # leading singleton padding must be at the FRONT so that the fastest index stays last
    k = 4 - len(shape)
    n = [1] * k + list(shape)
    s = [0] * k + list(sstr)
    d = [0] * k + list(dstr)
    L.check(lib.vfm_strided_copy(L.ptr(src), L.dt_of(src), L.ptr(dst), L.dt_of(dst), *n, *s, *d, int(accumulate), L.stream()),
            "vfm_strided_copy")
    return dst


class CopyBatch:
    """Device table for vfm_strided_copy_batch: jobs = [(src fp32 tensor, dst tensor, shape, src strides, dst strides[, accumulate
    [, nsum, sum_stride]])], each up to 4-D; run() performs all of them in one launch.  The tensors are kept alive by the table.
    Jobs of one table run concurrently: two jobs must not accumulate into the same destination - sum the partials of one
    reduction with nsum / sum_stride instead."""

    def __init__(self, jobs):
        import struct
        buf = bytearray()
        self.keep, self.max_elems, self.n = [], 0, len(jobs)
        for job in jobs:
            src, dst, shape, sstr, dstr = job[:5]
            acc = int(bool(job[5])) if len(job) > 5 else 0    # optional 6th item: accumulate into an fp32 dst
            nsum, sstride = (int(job[6]), int(job[7])) if len(job) > 7 else (1, 0)
            assert src.dtype == torch.float32 and src.is_cuda and dst.is_cuda and (not acc or dst.dtype == torch.float32)
            k = 4 - len(shape)
            n, s_, d_ = [1] * k + list(shape), [0] * k + list(sstr), [0] * k + list(dstr)
            buf += struct.pack("2Q16q", src.data_ptr(), dst.data_ptr(), L.dt_of(dst), acc, *n, *s_, *d_, nsum, sstride)
            self.keep += [src, dst]
            e = 1
            for v in shape:
                e *= v
            self.max_elems = max(self.max_elems, e)
        self.table = torch.frombuffer(buf, dtype=torch.uint8).clone().to(jobs[0][1].device) if jobs else None

    def run(self):
        if self.n:
            lib = L.load()
            L.check(lib.vfm_strided_copy_batch(L.ptr(self.table), self.n, self.max_elems, L.stream()), "vfm_strided_copy_batch")


def permute_copy(src, perm, dst):
    """dst (contiguous, any dtype) = src.permute(perm) ; src may be any strided <=4-D tensor."""
    v = src.permute(*perm)
    strided_copy(src, dst, list(v.shape), list(v.stride()), list(torch.empty(v.shape, device="meta").stride()))
    return dst


def axpby(x, a, y, b):
    lib = L.load()
    assert x.is_contiguous() and y.is_contiguous() and x.dtype == y.dtype == torch.float32 and x.numel() == y.numel()
    L.check(lib.vfm_axpby(L.ptr(x), float(a), L.ptr(y), float(b), x.numel(), L.stream()), "vfm_axpby")
    return y


def scale_by_device_scalar(y, scalar):
    lib = L.load()
    assert y.is_contiguous() and y.dtype == torch.float32
    L.check(lib.vfm_scale_by_device_scalar(L.ptr(y), L.ptr(scalar), y.numel(), L.stream()), "vfm_scale_by_device_scalar")
    return y


def colsum(x, out, accumulate=False):
    lib = L.load()
    rows, cols = x.shape
    ws = workspace(64 * cols, x.device)
    L.check(lib.vfm_colsum(L.ptr(x), L.dt_of(x), _ld(x), rows, cols, L.ptr(out), int(accumulate), L.ptr(ws), L.stream()),
            "vfm_colsum")
    return out


def dropout_mask(out, p, seed, offset=0):
    lib = L.load()
    assert out.is_contiguous()
    L.check(lib.vfm_dropout_mask(L.ptr(out), L.dt_of(out), out.numel(), float(p), int(seed), int(offset), L.stream()),
            "vfm_dropout_mask")
    return out


def mul_mask(src, mask, dst, rows_per_group=1):
    lib = L.load()
    L.check(lib.vfm_mul_mask(L.ptr(src), L.dt_of(src), _ld(src), L.ptr(mask), L.dt_of(mask), _ld(mask), rows_per_group,
                             L.ptr(dst), L.dt_of(dst), _ld(dst), src.shape[0], src.shape[1], L.stream()), "vfm_mul_mask")
    return dst


LORA_DOWN_KC = 128   # vfm_lora_down stages K in chunks of 128


def lora_down_ok(x, a):
    """Does the fused LoRA down-projection kernel cover this operand?  (16-bit, K % 128 == 0, A padded to 64 rows, 16-byte alignment)"""
    return (is_half(x.dtype) and a.dtype == x.dtype and x.shape[1] % LORA_DOWN_KC == 0 and a.shape == (64, x.shape[1]) and
            x.stride(1) == 1 and a.stride(1) == 1 and x.stride(0) % 8 == 0 and a.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0
            and a.data_ptr() % 16 == 0)


def lora_down(x, a, t, s, p=0.0, seed=0, offset=0, mask=None, xd=None):
    """One launch over x [M, K] (16 bit, may be a column slice): mask = dropout multiplier (the bits of dropout_mask on a contiguous
    [M, K] map), xd = x * mask (the bits of mul_mask), t [M, 64] = s * xd @ a^T.  p == 0: no mask, no xd, t = s * x @ a^T."""
    lib = L.load()
    M, K = x.shape
    assert lora_down_ok(x, a) and t.shape == (M, 64) and t.dtype == x.dtype and t.stride(1) == 1
    if p > 0:
        assert mask is not None and xd is not None and mask.shape == (M, K) and xd.shape == (M, K) and mask.dtype == x.dtype == xd.dtype
    else:
        mask = xd = None
    L.check(lib.vfm_lora_down(L.ptr(x), _ld(x), L.ptr(a), _ld(a), L.ptr(mask), _ld(mask) if mask is not None else 0, L.ptr(xd),
                              _ld(xd) if xd is not None else 0, L.ptr(t), _ld(t), M, K, float(s), float(p), int(seed), int(offset), L.stream()),
            "vfm_lora_down")
    return t


def geglu_fwd(h, out):
    lib = L.load()
    rows, c2 = h.shape
    L.check(lib.vfm_geglu_fwd(L.ptr(h), L.dt_of(h), _ld(h), L.ptr(out), L.dt_of(out), _ld(out), rows, c2 // 2, L.stream()),
            "vfm_geglu_fwd")
    return out


def geglu_bwd(h, dout, dh):
    lib = L.load()
    rows, c2 = h.shape
    L.check(lib.vfm_geglu_bwd(L.ptr(h), L.dt_of(h), _ld(h), L.ptr(dout), L.dt_of(dout), _ld(dout), L.ptr(dh), L.dt_of(dh),
                              _ld(dh), rows, c2 // 2, L.stream()), "vfm_geglu_bwd")
    return dh


def swiglu_fwd(h, out, C_):
    lib = L.load()
    L.check(lib.vfm_swiglu_fwd(L.ptr(h), L.dt_of(h), _ld(h), L.ptr(out), L.dt_of(out), _ld(out), h.shape[0], C_, L.stream()),
            "vfm_swiglu_fwd")
    return out


def swiglu_bwd(h, dout, dh, C_):
    lib = L.load()
    L.check(lib.vfm_swiglu_bwd(L.ptr(h), L.dt_of(h), _ld(h), L.ptr(dout), L.dt_of(dout), _ld(dout), L.ptr(dh), L.dt_of(dh),
                               _ld(dh), h.shape[0], C_, L.stream()), "vfm_swiglu_bwd")
    return dh


def rope(x, rows, np_, ncols, d, cos_t, sin_t, inverse=False):
    """In place on columns [0, ncols) of the first `rows` rows of the 2-D view x."""
    lib = L.load()
    L.check(lib.vfm_rope(L.ptr(x), L.dt_of(x), _ld(x), rows, np_, ncols, d, L.ptr(cos_t), L.ptr(sin_t), int(inverse), L.stream()),
            "vfm_rope")
    return x


def act_grad_mul(dy, pre, out, act):
    lib = L.load()
    L.check(lib.vfm_act_grad_mul(L.ptr(dy), L.dt_of(dy), _ld(dy), L.ptr(pre), L.dt_of(pre), _ld(pre), L.ptr(out),
                                 L.dt_of(out), _ld(out), dy.shape[0], dy.shape[1], act, L.stream()), "vfm_act_grad_mul")
    return out


def mask_token_fwd(x, keep, token, out):
    lib = L.load()
    L.check(lib.vfm_mask_token_fwd(L.ptr(x), L.ptr(keep), L.ptr(token), L.ptr(out), x.shape[0], x.shape[1], L.stream()),
            "vfm_mask_token_fwd")
    return out


def mask_token_bwd(dout, keep, dx, dtoken):
    lib = L.load()
    ws = workspace(64 * dout.shape[1], dout.device)
    L.check(lib.vfm_mask_token_bwd(L.ptr(dout), L.ptr(keep), L.ptr(dx), L.ptr(dtoken), L.ptr(ws), dout.shape[0], dout.shape[1],
                                   L.stream()), "vfm_mask_token_bwd")


def _split_key(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version)


def _register_split_out(t, t3):
    """t3 is the split-bf16 image (vfm_split3 pattern 0) of the fp32 tensor t, written by t's producer: the GEMM that consumes t finds it on
    the tensor OBJECT (ops.split3) instead of running vfm_split3.  When the producer skipped the fp32 copy, t holds no data at all."""
    try:
        t._vfm_split3_out = (_split_key(t), t3)
    except AttributeError:
        pass


def layernorm_fwd(x, w, b, eps, y, stats=None, split_out=None):
    """split_out (bf16x3 mode, y fp32, C % 256 == 0): "also" = y and its split-bf16 image, "only" = the image alone (y is then NOT written:
    for outputs whose one consumer is a GEMM's A operand); the image is registered on y for ops.split3."""
    lib = L.load()
    rows, c = x.shape
    if split_out and _split3_on() and y.dtype == torch.float32 and c % 256 == 0 and c // 256 in (1, 2, 4, 5, 8) and y.shape[1] == c:
        kp = (c + 63) // 64 * 64
        y3 = torch.empty(rows, 3 * kp, dtype=L.half_dtype(), device=x.device)
        L.check(lib.vfm_layernorm_fwd_split3(L.ptr(x), _ld(x), L.ptr(w), L.ptr(b), float(eps), None if split_out == "only" else L.ptr(y), _ld(y),
                                             L.ptr(y3), y3.stride(0), kp, L.ptr(stats), rows, c, L.stream()), "vfm_layernorm_fwd_split3")
        _register_split_out(y, y3)
        return y
    L.check(lib.vfm_layernorm_fwd(L.ptr(x), _ld(x), L.ptr(w), L.ptr(b), float(eps), L.ptr(y), L.dt_of(y), _ld(y),
                                  L.ptr(stats), rows, c, L.stream()), "vfm_layernorm_fwd")
    return y


def layernorm_dropout_fwd(x, w, b, eps, y, stats, y_drop, mask, p, seed, offset=0):
    """LN forward that also writes the dropout multiplier `mask` and y_drop = y * mask (bf16 outputs, C % 256 == 0)."""
    lib = L.load()
    rows, c = x.shape
    assert is_half(y.dtype) and is_half(y_drop.dtype) and is_half(mask.dtype)
    L.check(lib.vfm_layernorm_dropout_fwd(L.ptr(x), _ld(x), L.ptr(w), L.ptr(b), float(eps), L.ptr(y), _ld(y), L.ptr(stats),
                                          L.ptr(y_drop), _ld(y_drop), L.ptr(mask), _ld(mask), float(p), int(seed), int(offset),
                                          rows, c, L.stream()), "vfm_layernorm_dropout_fwd")
    return y


def layernorm_bwd_scaled(dy, x, w, stats, dx, t_out, t_scale, accumulate_dx=False):
    """LN backward into dx (fp32) that also emits t_out = bf16(dx_new * t_scale[c])."""
    lib = L.load()
    rows, c = x.shape
    assert is_half(t_out.dtype) and t_scale.dtype == torch.float32
    L.check(lib.vfm_layernorm_bwd_scaled(L.ptr(dy), L.dt_of(dy), _ld(dy), L.ptr(x), _ld(x), L.ptr(w), L.ptr(stats), L.ptr(dx),
                                         _ld(dx), int(accumulate_dx), L.ptr(t_out), _ld(t_out), L.ptr(t_scale), rows, c,
                                         L.stream()), "vfm_layernorm_bwd_scaled")
    return dx


def layernorm_bwd(dy, x, w, stats, dx, accumulate_dx=False, dw=None, db=None):
    lib = L.load()
    rows, c = x.shape
    ws = workspace(2 * 128 * c, x.device) if (dw is not None or db is not None) else None
    L.check(lib.vfm_layernorm_bwd(L.ptr(dy), L.dt_of(dy), _ld(dy), L.ptr(x), _ld(x), L.ptr(w), L.ptr(stats), L.ptr(dx),
                                  _ld(dx), int(accumulate_dx), L.ptr(dw), L.ptr(db), L.ptr(ws), rows, c, L.stream()),
            "vfm_layernorm_bwd")
    return dx


def groupnorm_fwd(x, w, b, eps, groups, act, y, stats, B, P):
    """x fp32 [B*P, C] contiguous; stats fp32 [B, G, 2]."""
    lib = L.load()
    c = x.shape[1]
    ws = workspace(B * groups * 2 + B * 64 * 2 * c, x.device)
    L.check(lib.vfm_groupnorm_fwd(L.ptr(x), L.ptr(w), L.ptr(b), float(eps), groups, act, L.ptr(y), L.dt_of(y), L.ptr(stats),
                                  L.ptr(ws), B, P, c, L.stream()), "vfm_groupnorm_fwd")
    return y


def groupnorm_bwd(dy, x, w, b, stats, groups, act, dx, dw, db, B, P):
    lib = L.load()
    c = x.shape[1]
    ws = workspace(B * groups * 2 + B * 64 * 2 * c, x.device)
    L.check(lib.vfm_groupnorm_bwd(L.ptr(dy), L.dt_of(dy), L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(stats), groups, act, L.ptr(dx),
                                  L.ptr(dw), L.ptr(db), L.ptr(ws), B, P, c, L.stream()), "vfm_groupnorm_bwd")
    return dx


def groupnorm_tile_ok(P, C, groups):
    """The coverage predicate of the one-launch GroupNorm, asked of the library itself (the C entries check the same function)."""
    return bool(L.load().vfm_groupnorm_tile_ok(int(P), int(C), int(groups)))


def groupnorm_tile_fwd(x, w, b, eps, groups, act, y, stats, B, P):
    """groupnorm_fwd's contract in one launch; raises (VFM_E_SHAPE) outside groupnorm_tile_ok."""
    lib = L.load()
    L.check(lib.vfm_groupnorm_tile_fwd(L.ptr(x), L.ptr(w), L.ptr(b), float(eps), groups, act, L.ptr(y), L.dt_of(y), L.ptr(stats),
                                       B, P, x.shape[1], L.stream()), "vfm_groupnorm_tile_fwd")
    return y


def groupnorm_tile_bwd(dy, x, w, b, stats, groups, act, dx, dw, db, B, P):
    lib = L.load()
    c = x.shape[1]
    ws = workspace(B * 2 * c, x.device)
    L.check(lib.vfm_groupnorm_tile_bwd(L.ptr(dy), L.dt_of(dy), L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(stats), groups, act, L.ptr(dx),
                                       L.ptr(dw), L.ptr(db), L.ptr(ws), B, P, c, L.stream()), "vfm_groupnorm_tile_bwd")
    return dx


def bn_moments(x, sums):
    lib = L.load()
    rows, c = x.shape
    ws = workspace(64 * 2 * c, x.device)
    L.check(lib.vfm_bn_moments(L.ptr(x), rows, c, L.ptr(sums), L.ptr(ws), L.stream()), "vfm_bn_moments")
    return sums


def bn_finalize(sums, count, mean_var, running_mean=None, running_var=None, momentum=0.1):
    lib = L.load()
    L.check(lib.vfm_bn_finalize(L.ptr(sums), float(count), L.ptr(mean_var), L.ptr(running_mean), L.ptr(running_var),
                                float(momentum), sums.shape[1], L.stream()), "vfm_bn_finalize")
    return mean_var


def bn_apply(x, mean_var, w, b, eps, act, y):
    lib = L.load()
    rows, c = x.shape
    L.check(lib.vfm_bn_apply(L.ptr(x), L.ptr(mean_var), L.ptr(w), L.ptr(b), float(eps), act, L.ptr(y), L.dt_of(y), rows, c,
                             L.stream()), "vfm_bn_apply")
    return y


def bn_bwd_reduce(dy, x, mean_var, w, b, eps, act, sums_dy):
    lib = L.load()
    rows, c = x.shape
    ws = workspace(64 * 2 * c, x.device)
    L.check(lib.vfm_bn_bwd_reduce(L.ptr(dy), L.dt_of(dy), L.ptr(x), L.ptr(mean_var), L.ptr(w), L.ptr(b), float(eps), act,
                                  L.ptr(sums_dy), L.ptr(ws), rows, c, L.stream()), "vfm_bn_bwd_reduce")
    return sums_dy


def bn_bwd_apply(dy, x, mean_var, w, b, eps, act, sums_dy, total_rows, dx):
    lib = L.load()
    rows, c = x.shape
    L.check(lib.vfm_bn_bwd_apply(L.ptr(dy), L.dt_of(dy), L.ptr(x), L.ptr(mean_var), L.ptr(w), L.ptr(b), float(eps), act,
                                 L.ptr(sums_dy), float(total_rows), L.ptr(dx), rows, c, L.stream()), "vfm_bn_bwd_apply")
    return dx


def split3(x, pattern, trans=False, cache=False):
    """fp32 operand x [rows, K] ([K, rows] if trans) -> bf16 [rows, 3 ceil64(K)] split form (vfm_split3).  cache=True keeps the result on
    the tensor OBJECT (weights packed once by the engines: same object every call) and rebuilds it when the tensor's version counter
    moves (LoRA-merged weights are re-packed in place); activations are fresh objects and never hit."""
    if pattern == 0 and not trans:   # an image its producer wrote (LayerNorm / attention / GEMM epilogue in the bf16x3 mode)
        hit = getattr(x, "_vfm_split3_out", None)
        if hit is not None and hit[0] == _split_key(x):
            return hit[1]
    if cache:
        from .optim import PARAM_EPOCH   # the fused AdamW / LoRA re-pack kernels rewrite packed operands behind torch's version counters
        key = (PARAM_EPOCH[0], x._version, x.data_ptr(), pattern, trans, tuple(x.shape), tuple(x.stride()))
        hit = getattr(x, "_vfm_split3", None)
        if hit is not None and hit[0] == key:
            return hit[1]
    rows, K = (x.shape[1], x.shape[0]) if trans else (x.shape[0], x.shape[1])
    sr, sc = (x.stride(1), x.stride(0)) if trans else (x.stride(0), x.stride(1))
    kp = (K + 63) // 64 * 64
    out = torch.empty(rows, 3 * kp, dtype=L.half_dtype(), device=x.device)
    L.check(L.load().vfm_split3(L.ptr(x), sr, sc, L.ptr(out), out.stride(0), rows, K, pattern, L.stream()), "vfm_split3")
    if cache:
        try:
            x._vfm_split3 = (key, out)
        except AttributeError:
            pass
    return out


def gemm(a, b, c, *, alpha=1.0, bias=None, bias_mod=0, colscale=None, residual=None, ep_mode=EP_NONE, aux=None, c2=None,
         trans_a=False, trans_b=False, kb_rows=0, c_split=None):
    """c[M,N] = epilogue(alpha * A @ B^T).  a: [M,K] (or [K,M] if trans_a), b: [N,K] (or [K,N] if trans_b); 2-D views
    (or 3-D batched with equal batch).  bf16 inputs require K-contiguous operands with K % 64 == 0.
    In the bf16x3 mode (precision.split3()) an fp32 x fp32 2-D product is computed by the bf16 MFMA kernels on split operands;
    c_split="only" (that mode, c fp32, N % 64 == 0, no residual / c2) makes the epilogue write the split-bf16 image of the result
    INSTEAD of c (c_dt VFM_SPLIT3) and registers it on c for ops.split3: for a result whose one consumer is the next GEMM's A operand."""
    if a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2 and not kb_rows and _split3_on():
        a3 = split3(a, 0, trans=trans_a)
        b3 = split3(b, 1, trans=trans_b, cache=not b.requires_grad)
        c3 = None
        if (c_split == "only" and c.dtype == torch.float32 and c.dim() == 2 and c.shape[1] % 64 == 0 and residual is None and c2 is None
                and ep_mode in (EP_NONE, EP_GELU)):
            c3 = torch.empty(c.shape[0], 3 * c.shape[1], dtype=L.half_dtype(), device=c.device)
        gemm(a3, b3, c, alpha=alpha, bias=bias, bias_mod=bias_mod, colscale=colscale, residual=residual, ep_mode=ep_mode, aux=aux, c2=c2, c_split=c3)
        if c3 is not None:
            _register_split_out(c, c3)
        return c
    lib = L.load()
    d = gemm_desc(a, b, c, alpha=alpha, bias=bias, bias_mod=bias_mod, colscale=colscale, residual=residual, ep_mode=ep_mode, aux=aux, c2=c2,
                  trans_a=trans_a, trans_b=trans_b, kb_rows=kb_rows)
    if torch.is_tensor(c_split):   # the image replaces c as the output
        d.C, d.c_dt, d.ldc, d.c_plane = L.ptr(c_split), L.SPLIT3, c_split.stride(0), c.shape[1]
    fin = PROFILE("gemm", 2.0 * d.M * d.N * d.K * d.batch, REGION[-1]) if (PROFILE is not None and is_half(a.dtype)) else None
    L.check(lib.vfm_gemm(C.byref(d), L.stream()), "vfm_gemm")
    if fin is not None:
        fin()
    return c


def gemm_desc(a, b, c, *, alpha=1.0, bias=None, bias_mod=0, colscale=None, residual=None, ep_mode=EP_NONE, aux=None, c2=None,
              trans_a=False, trans_b=False, kb_rows=0, d=None):
    """The vfm_gemm_desc of gemm(a, b, c, ...) (filled into `d` when given: an entry of a launch plan)."""
    d = L.GemmDesc() if d is None else d
    batched = a.dim() == 3
    a2 = a[0] if batched else a
    b2 = b[0] if batched else b
    c2d = c[0] if batched else c
    if trans_a:
        K, M = a2.shape
        d.sa_m, d.sa_k = a2.stride(1), a2.stride(0)
    else:
        M, K = a2.shape
        d.sa_m, d.sa_k = a2.stride(0), a2.stride(1)
    if trans_b:
        Kb, N = b2.shape
        d.sb_n, d.sb_k = b2.stride(1), b2.stride(0)
    else:
        N, Kb = b2.shape
        d.sb_n, d.sb_k = b2.stride(0), b2.stride(1)
    if kb_rows:
        assert trans_b and Kb == kb_rows and K >= Kb, "kb_rows: b holds the first kb_rows of the K (token) dimension"
        d.kb_rows = int(kb_rows)
    else:
        assert K == Kb, f"gemm K mismatch {K} vs {Kb}"
    assert a.dtype == b.dtype
    assert c2d.shape[0] == M and c2d.shape[1] == N and c2d.stride(1) == 1
    d.A, d.B, d.C = L.ptr(a), L.ptr(b), L.ptr(c)
    d.in_dt, d.c_dt = L.dt_of(a), L.dt_of(c)
    d.M, d.N, d.K = M, N, K
    d.ldc = c2d.stride(0)
    d.alpha = float(alpha)
    d.bias, d.bias_mod = L.ptr(bias), int(bias_mod)
    d.colscale = L.ptr(colscale)
    if residual is not None:
        r2 = residual[0] if batched else residual
        d.residual, d.r_dt, d.ldr = L.ptr(residual), L.dt_of(residual), r2.stride(0)
    d.ep_mode = ep_mode
    if aux is not None:
        d.aux, d.aux_dt, d.ld_aux = L.ptr(aux), L.dt_of(aux), aux.stride(0)
    if c2 is not None:
        d.C2, d.c2_dt, d.ldc2 = L.ptr(c2), L.dt_of(c2), c2.stride(0)
    if batched:
        d.batch, d.stride_a, d.stride_b, d.stride_c = a.shape[0], a.stride(0), b.stride(0), c.stride(0)
    else:
        d.batch = 1
    return d


class Plan:
    """A launch plan (include/vfmseg_hip.h "launch plans"): entries are appended with the same tensor arguments the one-by-one wrappers
    take, run() replays them through vfm_run_plan in ONE ctypes call.  The tensors are kept alive by the plan; their addresses must stay
    what they were when the entry was appended (persistent buffers), except for fields patched through `entry(i)` before a run."""

    def __init__(self, region="backbone"):
        self.ops, self.keep, self.arr, self.region = [], [], None, region

    def _new(self, kind, prof=L.PROF_NONE, flops=0.0, *tensors):
        op = L.PlanOp()
        op.kind, op.prof_kind, op.flops = kind, prof, float(flops)
        self.ops.append(op)
        self.keep.extend(t for t in tensors if t is not None)
        self.arr = None
        return op

    def gemm(self, a, b, c, **kw):
        op = self._new(L.OP_GEMM, L.PROF_GEMM if is_half(a.dtype) else L.PROF_NONE, 0.0, a, b, c, kw.get("bias"), kw.get("colscale"),
                       kw.get("residual"), kw.get("aux"), kw.get("c2"))
        d = gemm_desc(a, b, c, d=op.u.gemm, **kw)
        op.flops = 2.0 * d.M * d.N * d.K * d.batch
        return len(self.ops) - 1

    def layernorm_fwd(self, x, w, b, eps, y, stats):
        op = self._new(L.OP_LN_FWD, L.PROF_NONE, 0.0, x, w, b, y, stats)
        u = op.u.ln_fwd
        u.x, u.ld_x, u.w, u.b, u.eps, u.y, u.y_dt, u.ld_y, u.stats = L.ptr(x), _ld(x), L.ptr(w), L.ptr(b), float(eps), L.ptr(y), L.dt_of(y), _ld(y), L.ptr(stats)
        u.rows, u.C = x.shape
        return len(self.ops) - 1

    def layernorm_dropout_fwd(self, x, w, b, eps, y, stats, y_drop, mask, p, offset):
        """`offset` is relative to the rng_base given to run()."""
        assert is_half(y.dtype) and is_half(y_drop.dtype) and is_half(mask.dtype)
        op = self._new(L.OP_LN_DROPOUT_FWD, L.PROF_NONE, 0.0, x, w, b, y, stats, y_drop, mask)
        u = op.u.ln_drop
        u.x, u.ld_x, u.w, u.b, u.eps, u.y, u.ld_y, u.stats = L.ptr(x), _ld(x), L.ptr(w), L.ptr(b), float(eps), L.ptr(y), _ld(y), L.ptr(stats)
        u.y_drop, u.ld_yd, u.mask, u.ld_mask, u.p, u.offset = L.ptr(y_drop), _ld(y_drop), L.ptr(mask), _ld(mask), float(p), int(offset)
        u.rows, u.C = x.shape
        return len(self.ops) - 1

    def layernorm_bwd_scaled(self, dy, x, w, stats, dx, t_out, t_scale, accumulate_dx=False):
        assert is_half(t_out.dtype) and t_scale.dtype == torch.float32
        op = self._new(L.OP_LN_BWD_SCALED, L.PROF_NONE, 0.0, dy, x, w, stats, dx, t_out, t_scale)
        u = op.u.ln_bwd
        u.dy, u.dy_dt, u.ld_dy, u.x, u.ld_x, u.w, u.stats = L.ptr(dy), L.dt_of(dy), _ld(dy), L.ptr(x), _ld(x), L.ptr(w), L.ptr(stats)
        u.dx, u.ld_dx, u.accumulate_dx, u.t_out, u.ld_t, u.t_scale = L.ptr(dx), _ld(dx), int(accumulate_dx), L.ptr(t_out), _ld(t_out), L.ptr(t_scale)
        u.rows, u.C = x.shape
        return len(self.ops) - 1

    def attn_fwd(self, q, k, v, o, lse, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale):
        fl = 4.0 * B * H * (nq_main + nq_extra) * (nk_main + nk_extra) * d
        op = self._new(L.OP_ATTN_FWD, L.PROF_ATTN_FWD if is_half(q.dtype) else L.PROF_NONE, fl, q, k, v, o, lse)
        C.memmove(C.byref(op.u.attn), C.byref(_attn_desc(q, k, v, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse)), C.sizeof(L.AttnDesc))
        return len(self.ops) - 1

    def attn_bwd(self, q, k, v, o, lse, dout, dq, dk, dv, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale):
        fl = 10.0 * B * H * (nq_main + nq_extra) * (nk_main + nk_extra) * d
        delta = _attn_bwd_delta(q, B, H, nq_main + nq_extra)
        op = self._new(L.OP_ATTN_BWD, L.PROF_ATTN_BWD if is_half(q.dtype) else L.PROF_NONE, fl, q, k, v, o, lse, dout, dq, dk, dv, delta)
        a = _attn_desc(q, k, v, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse)
        a.dout, a.ld_do = L.ptr(dout), dout.stride(0)
        a.dq, a.dk, a.dv = L.ptr(dq), L.ptr(dk), L.ptr(dv)
        a.ld_dq, a.ld_dk, a.ld_dv = dq.stride(0), dk.stride(0), dv.stride(0)
        a.delta = L.ptr(delta)
        C.memmove(C.byref(op.u.attn), C.byref(a), C.sizeof(L.AttnDesc))
        return len(self.ops) - 1

    def cast(self, src, dst, colscale=None):
        op = self._new(L.OP_CAST, L.PROF_NONE, 0.0, src, dst, colscale)
        u = op.u.cast
        u.src, u.src_dt, u.ld_src, u.dst, u.dst_dt, u.ld_dst = L.ptr(src), L.dt_of(src), _ld(src), L.ptr(dst), L.dt_of(dst), _ld(dst)
        u.rows, u.cols = src.shape
        u.colscale = L.ptr(colscale)
        return len(self.ops) - 1

    def strided_copy(self, src, dst, shape, sstr, dstr, accumulate=False):
        op = self._new(L.OP_STRIDED_COPY, L.PROF_NONE, 0.0, src, dst)
        u = op.u.copy
        k = 4 - len(shape)
        u.src, u.src_dt, u.dst, u.dst_dt = L.ptr(src), L.dt_of(src), L.ptr(dst), L.dt_of(dst)
        for i, (n, s_, d_) in enumerate(zip([1] * k + list(shape), [0] * k + list(sstr), [0] * k + list(dstr))):
            u.n[i], u.ss[i], u.ds[i] = n, s_, d_
        u.accumulate = int(accumulate)
        return len(self.ops) - 1

    def _array(self):
        if self.arr is None:
            self.arr = (L.PlanOp * len(self.ops))()
            for i, op in enumerate(self.ops):
                C.memmove(C.byref(self.arr[i]), C.byref(op), C.sizeof(L.PlanOp))
        return self.arr

    def entry(self, i):
        """The i-th entry of the array run() hands to the library (for per-run patches of pointer fields)."""
        return self._array()[i]

    def run(self, seed=0, rng_base=0, start=0, count=None):
        arr = self._array()
        n = len(self.ops) - start if count is None else count
        first = C.cast(C.byref(arr, start * C.sizeof(L.PlanOp)), C.POINTER(L.PlanOp))
        L.check(L.load().vfm_run_plan(first, n, int(seed), int(rng_base), L.stream()), "vfm_run_plan")

    def __len__(self):
        return len(self.ops)


def prof_config(every):
    L.check(L.load().vfm_prof_config(int(every)), "vfm_prof_config")


def prof_read(cap=65536):
    """[(kind name, flops, ms)] of the launches the plan sampler timed since the last read (waits for their events)."""
    buf = (C.c_double * (3 * cap))()
    n = L.load().vfm_prof_read(buf, cap)
    if n < 0:
        L.check(n, "vfm_prof_read")
    return [(L.PROF_NAMES.get(int(buf[3 * i]), "other"), buf[3 * i + 1], buf[3 * i + 2]) for i in range(n)]


class LoraPackTable:
    """Device-resident table for vfm_lora_pack: one entry per adapter site (A, B fp32 parameters and the packed operands they
    feed).  Built once per packing (pointers are stable: parameters live in the optimiser's flat buffer, operands in the
    engine's packed dict); `run()` re-packs every site with one launch."""

    def __init__(self, sites, dt_tensor):
        import struct
        buf = bytearray()
        self.max_elems = 0
        self.keep = []
        for (A, B, a, at, w, wt, r, K, N, Kw) in sites:
            assert A.dtype == torch.float32 and B.dtype == torch.float32 and A.is_contiguous() and B.is_contiguous()
            self.keep += [A, B, a, at, w, wt]
            buf += struct.pack("6Q8q", A.data_ptr(), B.data_ptr(), a.data_ptr(), at.data_ptr(), w.data_ptr(),
                               wt.data_ptr() if wt is not None else 0, r, K, N, Kw, a.stride(0), at.stride(0), w.stride(0),
                               wt.stride(0) if wt is not None else 0)
            self.max_elems = max(self.max_elems, r * (K + N))
        self.n = len(sites)
        self.dt = L.dt_of(dt_tensor)
        dev = sites[0][2].device
        self.table = torch.frombuffer(buf, dtype=torch.uint8).clone().to(dev)
        self.ptrs = [s_[0].data_ptr() for s_ in sites] + [s_[1].data_ptr() for s_ in sites]

    def valid_for(self, sites):
        return self.n == len(sites) and self.ptrs == [s_[0].data_ptr() for s_ in sites] + [s_[1].data_ptr() for s_ in sites]

    def run(self):
        lib = L.load()
        L.check(lib.vfm_lora_pack(L.ptr(self.table), self.n, self.max_elems, self.dt, L.stream()), "vfm_lora_pack")


BRANCH_WS_PARTS = 128   # VFM_BRANCH_WS_PARTS


def branch_param_grads(dx, u, gamma, dgamma=None, dbias=None, t=None, accumulate=False):
    """Residual branch x_out = x_in + gamma * (y W^T + b), one read pass over dx (fp32 [M, D]) and the saved pre-scale output u
    (fp32 | half [M, D]):  dgamma[c] (+)= sum_m dx u,  dbias[c] (+)= gamma[c] sum_m dx,  t = cast(dx * gamma) - the dgrad operand, the
    bits ops.cast(dx, t, gamma) writes.  Each output may be None (u may be None when dgamma is).  Deterministic, no atomics."""
    lib = L.load()
    M, D = dx.shape
    assert dx.dtype == torch.float32 and gamma.dtype == torch.float32 and gamma.is_contiguous() and gamma.numel() == D
    for o in (dgamma, dbias):
        assert o is None or (o.dtype == torch.float32 and o.is_contiguous() and o.numel() == D)
    assert u is None or tuple(u.shape) == (M, D)
    assert t is None or tuple(t.shape) == (M, D)
    ws = workspace(2 * BRANCH_WS_PARTS * D, dx.device, "branch")
    L.check(lib.vfm_branch_param_grads(L.ptr(dx), _ld(dx), L.ptr(u), L.dt_of(u) if u is not None else 0, _ld(u) if u is not None else 0,
                                       L.ptr(gamma), M, D, L.ptr(dgamma), L.ptr(dbias), int(accumulate), L.ptr(t),
                                       L.dt_of(t) if t is not None else 0, _ld(t) if t is not None else 0, L.ptr(ws), L.stream()),
            "vfm_branch_param_grads")
    return t


class PackTable:
    """Device-resident table for vfm_pack_weights: sites = [(src fp32 [N, K] contiguous, w [N, >=K], wt [K, >=N] or None)] - the fp32
    master of a trained 2-D weight and the packed GEMM operands it feeds.  Built once per packing (the master lives in the optimiser's
    flat buffer, the images in the engine's packed dict: stable pointers); run() rewrites every image with one launch."""

    def __init__(self, sites):
        import struct
        buf = bytearray()
        self.keep, self.max_tiles, self.n = [], 0, len(sites)
        self.dt = None
        for src, w, wt in sites:
            n, k = src.shape
            assert src.dtype == torch.float32 and src.is_contiguous() and src.is_cuda and w.shape[0] == n and w.shape[1] >= k and w.stride(1) == 1
            assert wt is None or (wt.dtype == w.dtype and wt.shape[0] >= k and wt.shape[1] >= n and wt.stride(1) == 1)
            assert self.dt in (None, w.dtype), "one table packs into one dtype"
            self.dt = w.dtype
            buf += struct.pack("3Q4q", src.data_ptr(), w.data_ptr(), wt.data_ptr() if wt is not None else 0, n, k, w.stride(0),
                               wt.stride(0) if wt is not None else 0)
            self.keep += [src, w, wt]
            self.max_tiles = max(self.max_tiles, ((n + 63) // 64) * ((k + 63) // 64))
        self.ptrs = [s_[0].data_ptr() for s_ in sites]
        self.table = torch.frombuffer(buf, dtype=torch.uint8).clone().to(sites[0][0].device) if sites else None

    def valid_for(self, srcs):
        return self.ptrs == [s_.data_ptr() for s_ in srcs]

    def run(self):
        if self.n:
            lib = L.load()
            L.check(lib.vfm_pack_weights(L.ptr(self.table), self.n, self.max_tiles, L.dt_of(self.keep[1]), L.stream()),
                    "vfm_pack_weights")


def slab_reduce(slabs, rows_used, dst, sp, sq, alpha=1.0, accumulate=False):
    """dst[p*sp + q*sq] (+)= alpha * sum_k slabs[k, p, q] for p < rows_used (slabs fp32 [kch, P, Q], dst fp32)."""
    lib = L.load()
    kch, P, Q = slabs.shape
    assert slabs.is_contiguous() and slabs.dtype == torch.float32 and dst.dtype == torch.float32
    L.check(lib.vfm_slab_reduce(L.ptr(slabs), kch, P, Q, int(rows_used), float(alpha), L.ptr(dst), int(sp), int(sq), int(accumulate),
                                L.stream()), "vfm_slab_reduce")
    return dst


def gemm_splitk_bt(at, y, slabs, kch):
    """Split-K weight gradient: slabs[z] = at[:, z*ck:(z+1)*ck] @ y[z*ck:(z+1)*ck, :]  (z < kch, ck = at.shape[1] / kch).
    at [P, Mp] bf16 (tokens zero-padded to Mp), y [M, Q] bf16 consumed in place as the [K, N] operand (rows >= M are
    clamped in the kernel - `at` is zero there), slabs fp32 [kch, P, Q]."""
    lib = L.load()
    d = L.GemmDesc()
    P, mp = at.shape
    M, Q = y.shape
    ck = mp // kch
    assert ck * kch == mp and ck % 64 == 0 and slabs.shape == (kch, P, Q)
    d.A, d.B, d.C = L.ptr(at), L.ptr(y), L.ptr(slabs)
    d.in_dt, d.c_dt = L.dt_of(at), L.dt_of(slabs)
    d.M, d.N, d.K = P, Q, ck
    d.sa_m, d.sa_k = at.stride(0), 1
    d.sb_n, d.sb_k = 1, y.stride(0)
    d.ldc = slabs.stride(1)
    d.alpha = 1.0
    d.batch, d.stride_a, d.stride_b, d.stride_c = kch, ck, ck * y.stride(0), slabs.stride(0)
    d.kb_rows = int(M)
    fin = PROFILE("gemm_tn", 2.0 * P * Q * mp, REGION[-1]) if PROFILE is not None else None
    L.check(lib.vfm_gemm(C.byref(d), L.stream()), "vfm_gemm")
    if fin is not None:
        fin()
    return slabs


def gemm_splitk_tn(xs, y, slabs, kch):
    """Split-K weight gradient with BOTH operands token-major: slabs[z] = xs[z*ck:(z+1)*ck, :]^T @ y[z*ck:(z+1)*ck, :]
    (xs [M, P], y [M, Q] bf16 views consumed in place, P % 8 == 0; token rows >= M read as zeros), slabs fp32 [kch, P, Q],
    ck = ceil64(M) / kch."""
    lib = L.load()
    d = L.GemmDesc()
    M, P = xs.shape
    M2, Q = y.shape
    assert M == M2 and xs.stride(1) == 1 and y.stride(1) == 1
    mp = (M + 63) // 64 * 64
    ck = mp // kch
    assert ck * kch == mp and ck % 64 == 0 and slabs.shape == (kch, P, Q)
    d.A, d.B, d.C = L.ptr(xs), L.ptr(y), L.ptr(slabs)
    d.in_dt, d.c_dt = L.dt_of(xs), L.dt_of(slabs)
    d.M, d.N, d.K = P, Q, ck
    d.sa_m, d.sa_k = 1, xs.stride(0)
    d.sb_n, d.sb_k = 1, y.stride(0)
    d.ldc = slabs.stride(1)
    d.alpha = 1.0
    d.batch, d.stride_a, d.stride_b, d.stride_c = kch, ck * xs.stride(0), ck * y.stride(0), slabs.stride(0)
    d.kb_rows = int(M)
    fin = PROFILE("gemm_tn", 2.0 * P * Q * mp, REGION[-1]) if PROFILE is not None else None
    L.check(lib.vfm_gemm(C.byref(d), L.stream()), "vfm_gemm")
    if fin is not None:
        fin()
    return slabs


def gemm_tn_batched(xs, y, out, valid_rows, alpha=1.0, accumulate=False):
    """out[l] = alpha * xs[l]^T @ y[l] for independent problems l (one weight gradient per layer in ONE launch): xs [L, M, P],
    y [L, M, Q] bf16 views (unit column stride, P % 8 == 0, Q % 8 == 0), out fp32 [L, P, Q]; token rows >= valid_rows read as zeros.
    accumulate: out[l] += ... (the epilogue's residual is its own destination)."""
    lib = L.load()
    d = L.GemmDesc()
    Lb, M, P = xs.shape
    _, M2, Q = y.shape
    assert M == M2 and xs.stride(2) == 1 and y.stride(2) == 1 and out.shape == (Lb, P, Q) and out.is_contiguous()
    d.A, d.B, d.C = L.ptr(xs), L.ptr(y), L.ptr(out)
    d.in_dt, d.c_dt = L.dt_of(xs), L.dt_of(out)
    d.M, d.N, d.K = P, Q, (valid_rows + 63) // 64 * 64
    d.sa_m, d.sa_k = 1, xs.stride(1)
    d.sb_n, d.sb_k = 1, y.stride(1)
    d.ldc = Q
    d.alpha = float(alpha)
    d.batch, d.stride_a, d.stride_b, d.stride_c = Lb, xs.stride(0), y.stride(0), P * Q
    d.kb_rows = -int(valid_rows)
    if accumulate:
        d.residual, d.r_dt, d.ldr = L.ptr(out), L.dt_of(out), Q
    fin = PROFILE("gemm_tn", 2.0 * P * Q * valid_rows * Lb, REGION[-1]) if PROFILE is not None else None
    L.check(lib.vfm_gemm(C.byref(d), L.stream()), "vfm_gemm")
    if fin is not None:
        fin()
    return out


def _split3_on():
    from .precision import split3 as _s3
    return _s3()


def tune(key, value):
    lib = L.load()
    L.check(lib.vfm_tune(key.encode(), int(value)), "vfm_tune")


def _attn_desc(q, k, v, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse):
    a = L.AttnDesc()
    a.q, a.k, a.v, a.o = L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(o)
    a.dt = L.dt_of(q)
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    a.B, a.H, a.d = B, H, d
    a.nq_main, a.nq_extra, a.nk_main, a.nk_extra = nq_main, nq_extra, nk_main, nk_extra
    a.scale = float(scale)
    a.lse = L.ptr(lse)
    return a


def _qkv_split3(q, k, v, hd):
    """q, k, v fp32 [rows, hd] that are the three column thirds of ONE packed [rows, 3 hd] buffer (self-attention: the QKV projection's
    output) -> the vfm_split3(pattern 1) image of the whole buffer, bf16 [rows, 9 hd]: hi of q / k / v at columns 0 / hd / 2 hd, lo at
    3 hd + the same.  Kept on the buffer object (views share their base) so that the backward reuses the forward's split; None when the
    operands are not laid out that way."""
    base = q._base if q._base is not None else None
    if (base is None or k._base is not base or v._base is not base or q.stride(1) != 1 or q.stride(0) != 3 * hd or k.stride(0) != 3 * hd
            or v.stride(0) != 3 * hd or k.storage_offset() - q.storage_offset() != hd or v.storage_offset() - q.storage_offset() != 2 * hd
            or q.storage_offset() % (3 * hd) != 0):
        return None
    rows = q.shape[0]
    hit = getattr(base, "_vfm_qkv3", None)
    key = (base._version, q.storage_offset(), rows)
    if hit is not None and hit[0] == key:
        return hit[1]
    whole = q.as_strided((rows, 3 * hd), (3 * hd, 1), q.storage_offset())
    full = split3(whole, 1)
    try:
        base._vfm_qkv3 = (key, full)
    except AttributeError:
        pass
    return full


_attn_bwd_ws = {}


def _attn_bwd_delta(q, B, H, nq):
    """delta[B, H, nq] + the zero-on-entry scratch of the extra-token rows (the kernels leave it zeroed): one buffer per shape"""
    key = (str(q.device), B, H, nq)
    delta = _attn_bwd_ws.get(key)
    if delta is None:
        delta = _attn_bwd_ws[key] = torch.zeros(B * H * nq + B * H * 192, dtype=torch.float32, device=q.device)
    return delta


def attn_fwd(q, k, v, o, lse, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, keep_split=False, o_split=None):
    """q,k,v,o: 2-D row-major views [rows, >=H*d] (column slices of a packed qkv buffer are fine).  keep_split (bf16x3 mode): a backward
    pass will follow - split the whole packed qkv buffer once and keep the image for it (a prediction splits only k and v)."""
    lib = L.load()
    if q.dtype == torch.float32 and d == 64 and _split3_on() and k.shape[1] == H * d and v.shape[1] == H * d:
        # bf16x3 mode: K and V as split bf16 operands ([hi | lo | hi] per row), Q split in the kernel, fp32 softmax and output
        full = _qkv_split3(q, k, v, H * d) if keep_split else None
        if full is not None:
            k3, v3, lo = full[:, H * d:], full[:, 2 * H * d:], 3 * H * d
        else:
            k3, v3, lo = split3(k, 1), split3(v, 1), H * d
        a = _attn_desc(q, k3, v3, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse)
        a.dt = L.dt_of(q)
        if o_split and o.shape[1] == H * d and o.stride(1) == 1:
            # the output as the split operand of the projection GEMM that consumes it (o_split "only": no fp32 copy at all)
            o3 = torch.empty(o.shape[0], 3 * H * d, dtype=L.half_dtype(), device=o.device)
            if o_split == "only":
                a.o = None
            L.check(lib.vfm_attn_fwd_x3_split(C.byref(a), lo, L.ptr(o3), o3.stride(0), H * d, L.stream()), "vfm_attn_fwd_x3_split")
            _register_split_out(o, o3)
            return o
        L.check(lib.vfm_attn_fwd_x3(C.byref(a), lo, L.stream()), "vfm_attn_fwd_x3")
        return o
    a = _attn_desc(q, k, v, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse)
    fin = None
    if PROFILE is not None and is_half(q.dtype):   # QK^T + PV: 4 B H Nq Nk d
        fin = PROFILE("attn_fwd", 4.0 * B * H * (nq_main + nq_extra) * (nk_main + nk_extra) * d, REGION[-1])
    L.check(lib.vfm_attn_fwd(C.byref(a), L.stream()), "vfm_attn_fwd")
    if fin is not None:
        fin()
    return o


def attn_bwd(q, k, v, o, lse, dout, dq, dk, dv, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale):
    lib = L.load()
    a = _attn_desc(q, k, v, o, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale, lse)
    a.dout, a.ld_do = L.ptr(dout), dout.stride(0)
    a.dq, a.dk, a.dv = L.ptr(dq), L.ptr(dk), L.ptr(dv)
    a.ld_dq, a.ld_dk, a.ld_dv = dq.stride(0), dk.stride(0), dv.stride(0)
    a.delta = L.ptr(_attn_bwd_delta(q, B, H, nq_main + nq_extra))
    if (q.dtype == torch.float32 and d == 64 and _split3_on() and q.shape[1] == H * d and k.shape[1] == H * d and v.shape[1] == H * d
            and dout.shape[1] == H * d and dq.dtype == torch.float32):
        # bf16x3 mode: the five products on split-bf16 operands (streamed operands arrive split; stationary rows, P and dS are split in the kernels)
        g3 = split3(dout, 1)
        full = _qkv_split3(q, k, v, H * d)
        if full is not None:       # q / k / v are the column thirds of one packed buffer: ONE split (kept from the forward) serves all three
            q3, k3, v3, lo = full[:, :H * d], full[:, H * d:], full[:, 2 * H * d:], 3 * H * d
        else:
            q3, k3, v3, lo = split3(q, 1), split3(k, 1), split3(v, 1), H * d
            assert q3.stride(0) == k3.stride(0) == v3.stride(0)
        L.check(lib.vfm_attn_bwd_x3(C.byref(a), L.ptr(q3), L.ptr(k3), L.ptr(v3), q3.stride(0), lo, L.ptr(g3), g3.stride(0), H * d, L.stream()),
                "vfm_attn_bwd_x3")
        return
    fin = None
    if PROFILE is not None and is_half(q.dtype):   # algorithmic: S, dP, dV, dK, dQ = five products = 10 B H Nq Nk d
        fin = PROFILE("attn_bwd", 10.0 * B * H * (nq_main + nq_extra) * (nk_main + nk_extra) * d, REGION[-1])
    L.check(lib.vfm_attn_bwd(C.byref(a), L.stream()), "vfm_attn_bwd")
    if fin is not None:
        fin()


def sam_relpos_table(rel_pos, S, out):
    lib = L.load()
    L.check(lib.vfm_sam_relpos_table(L.ptr(rel_pos), rel_pos.shape[0], rel_pos.shape[1], S, L.ptr(out), L.stream()),
            "vfm_sam_relpos_table")
    return out


def sam_attn_flash_fwd(qkv, bias, tbl_h, tbl_w, out, nimg, G, S, H, d, scale):
    """One-launch SAM attention forward (inference): qkv [M, 3*H*d] bf16 -> out [M, H*d] bf16."""
    lib = L.load()
    assert is_half(qkv.dtype) and is_half(out.dtype) and is_half(tbl_h.dtype) and tbl_h.is_contiguous()
    fin = None
    if PROFILE is not None:   # algorithmic FLOPs: q.k and p.v over the S*S keys of every window token (bias products not counted)
        nws = 1 if S == 32 else (G + S - 1) // S
        fin = PROFILE("attn_fwd", 4.0 * nimg * nws * nws * H * (S * S) ** 2 * d, REGION[-1])
    L.check(lib.vfm_sam_attn_flash_fwd(L.ptr(qkv), _ld(qkv), L.ptr(bias), L.ptr(tbl_h), L.ptr(tbl_w), L.ptr(out), _ld(out), nimg, G, S, H, d,
                                       float(scale), L.stream()), "vfm_sam_attn_flash_fwd")
    if fin is not None:
        fin()
    return out


def sam_attn_flash_stats(nimg, G, S, H, dev):
    """Buffers the training forward leaves for the backward: lse [rows] fp32, qext [rows, 2*SP] bf16 (rows = window-heads x 256 / 1024)."""
    nws = 1 if S == 32 else (G + S - 1) // S
    rows = nimg * nws * nws * H * (256 if S == 14 else 1024)
    return (torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, 2 * (16 if S == 14 else 32), dtype=L.half_dtype(), device=dev))


def sam_attn_flash_fwd_train(qkv, bias, tbl_h, tbl_w, out, lse, qext, nimg, G, S, H, d, scale):
    """sam_attn_flash_fwd that also writes the per-query log2-sum-exp and the bias columns of the query operand."""
    lib = L.load()
    assert is_half(qkv.dtype) and is_half(out.dtype) and is_half(tbl_h.dtype) and tbl_h.is_contiguous()
    assert lse.dtype == torch.float32 and is_half(qext.dtype) and qext.is_contiguous()
    L.check(lib.vfm_sam_attn_flash_fwd_train(L.ptr(qkv), _ld(qkv), L.ptr(bias), L.ptr(tbl_h), L.ptr(tbl_w), L.ptr(out), _ld(out), nimg, G, S, H, d,
                                             float(scale), L.ptr(lse), L.ptr(qext), L.stream()), "vfm_sam_attn_flash_fwd_train")
    return out


def sam_attn_flash_bwd(qkv, bias, tbl_h, tbl_w, out, dout, lse, qext, dqkv, nimg, G, S, H, d, scale):
    """d(out) [M, H*d] -> dqkv [M, 3*H*d] (bf16, every element written) in two launches (csrc/sam_flash_bwd.hip)."""
    lib = L.load()
    assert all(is_half(t.dtype) for t in (qkv, out, dout, dqkv, qext)) and _ld(out) == _ld(dout)
    dsum = torch.empty_like(lse)
    L.check(lib.vfm_sam_attn_flash_bwd(L.ptr(qkv), _ld(qkv), L.ptr(bias), L.ptr(tbl_h), L.ptr(tbl_w), L.ptr(out), L.ptr(dout), _ld(out), L.ptr(lse),
                                       L.ptr(qext), L.ptr(dsum), L.ptr(dqkv), _ld(dqkv), nimg, G, S, H, d, float(scale), L.stream()),
            "vfm_sam_attn_flash_bwd")
    return dqkv


def sam_attn_prep(qkv, bias, rh, rw, q_aug, k_aug, v_win, nimg, G, S, H, d, scale):
    lib = L.load()
    L.check(lib.vfm_sam_attn_prep(L.ptr(qkv), L.dt_of(qkv), _ld(qkv), L.ptr(bias), L.ptr(rh), L.ptr(rw), L.ptr(q_aug),
                                  L.ptr(k_aug), L.ptr(v_win), nimg, G, S, H, d, q_aug.shape[-1], v_win.shape[1], q_aug.shape[1],
                                  float(scale), L.stream()), "vfm_sam_attn_prep")


def sam_attn_bwd_prep(dao, qkv, bias, dow, dowT, vp, qsT, nimg, G, S, H, d, scale):
    """dO / V window-partitioned with the head dim zero-padded, dO^T and (scale q)^T: the small operands of the backward GEMMs."""
    lib = L.load()
    L.check(lib.vfm_sam_attn_bwd_prep(L.ptr(dao), _ld(dao), L.ptr(qkv), _ld(qkv), L.ptr(bias), L.dt_of(qkv), L.ptr(dow), L.ptr(dowT),
                                      L.ptr(vp), L.ptr(qsT), nimg, G, S, H, d, dow.shape[-1], dow.shape[1], float(scale), L.stream()),
            "vfm_sam_attn_bwd_prep")


def softmax_rows_batched(scores, out, n, rows_per_batch, valid_rows):
    lib = L.load()
    L.check(lib.vfm_softmax_rows_batched(L.ptr(scores), _ld(scores), L.ptr(out), L.dt_of(out), _ld(out), scores.shape[0], n, out.shape[1],
                                         rows_per_batch, valid_rows, L.stream()), "vfm_softmax_rows_batched")
    return out


def softmax_rows_bwd(p, dp, ds, n, rows_per_batch, valid_rows):
    lib = L.load()
    L.check(lib.vfm_softmax_rows_bwd(L.ptr(p), L.ptr(dp), _ld(dp), L.ptr(ds), L.dt_of(p), _ld(p), p.shape[0], n, p.shape[1], rows_per_batch,
                                     valid_rows, L.stream()), "vfm_softmax_rows_bwd")
    return ds


def sam_attn_bwd_merge(dqa, dkT, dvT, rh, rw, dqkv, nimg, G, S, H, d, scale):
    lib = L.load()
    L.check(lib.vfm_sam_attn_bwd_merge(L.ptr(dqa), L.ptr(dkT), L.ptr(dvT), L.dt_of(dqa), L.ptr(rh), L.ptr(rw), L.ptr(dqkv), _ld(dqkv), nimg,
                                       G, S, H, d, dkT.shape[1], dkT.shape[2], dqa.shape[-1], float(scale), L.stream()),
            "vfm_sam_attn_bwd_merge")
    return dqkv


def softmax_rows(scores2d, out2d, n):
    lib = L.load()
    L.check(lib.vfm_softmax_rows(L.ptr(scores2d), _ld(scores2d), L.ptr(out2d), L.dt_of(out2d), _ld(out2d), scores2d.shape[0], n,
                                 out2d.shape[1], L.stream()), "vfm_softmax_rows")
    return out2d


REIN_TOK = 128   # token columns of the fused Rein kernels (token_length padded)


def rein_mix_fwd(x, t, vt, u, m, c, p=None, x16=None):
    """Rein token attention, forward (vfm_rein_mix_fwd): x fp32 [rows, D] (row-strided view), t [128, D] / vt [D, 128] 16-bit contiguous
    (zero pad rows, zero row 0 of v), u [rows, D] 16-bit = softmax(c x t^T) v + x; optional p [rows, 128] and x16 [rows, D] for backward."""
    lib = L.load()
    rows, D = x.shape
    assert x.dtype == torch.float32 and t.shape == (REIN_TOK, D) and vt.shape == (D, REIN_TOK) and t.is_contiguous() and vt.is_contiguous()
    assert is_half(u.dtype) and u.shape == (rows, D) and t.dtype == vt.dtype == u.dtype
    assert p is None or (p.shape == (rows, REIN_TOK) and p.dtype == u.dtype)
    assert x16 is None or (x16.shape == (rows, D) and x16.dtype == u.dtype)
    L.check(lib.vfm_rein_mix_fwd(L.ptr(x), _ld(x), L.ptr(t), L.ptr(vt), L.ptr(u), _ld(u), L.ptr(p), _ld(p) if p is not None else 0, L.ptr(x16),
                                 _ld(x16) if x16 is not None else 0, rows, D, int(m), float(c), L.stream()), "vfm_rein_mix_fwd")
    return u


def rein_mix_bwd(du, p, v, tt, ds, dx, m, c):
    """Rein token attention, backward (vfm_rein_mix_bwd): du [rows, D], p [rows, 128], v [128, D], tt [D, 128] 16-bit; writes ds [rows, 128]
    16-bit and accumulates dx (fp32 [rows, D] row-strided view) += du + ds t."""
    lib = L.load()
    rows, D = du.shape
    assert is_half(du.dtype) and p.dtype == v.dtype == tt.dtype == ds.dtype == du.dtype and dx.dtype == torch.float32
    assert v.shape == (REIN_TOK, D) and tt.shape == (D, REIN_TOK) and v.is_contiguous() and tt.is_contiguous()
    assert p.shape == (rows, REIN_TOK) and ds.shape == (rows, REIN_TOK) and dx.shape == (rows, D)
    L.check(lib.vfm_rein_mix_bwd(L.ptr(du), _ld(du), L.ptr(p), _ld(p), L.ptr(v), L.ptr(tt), L.ptr(ds), _ld(ds), L.ptr(dx), _ld(dx), rows, D,
                                 int(m), float(c), L.stream()), "vfm_rein_mix_bwd")
    return dx


def sam_attn_merge(o_win, out, nimg, G, S, H, d):
    lib = L.load()
    L.check(lib.vfm_sam_attn_merge(L.ptr(o_win), L.dt_of(o_win), L.ptr(out), _ld(out), nimg, G, S, H, d, o_win.shape[1],
                                   L.stream()), "vfm_sam_attn_merge")
    return out


def patchify(img, out, box=None, patch=16):
    """img fp32 [B,3,H,W] (any strides with unit x-stride); box=(y0,y1,x0,x1) crop; out [B*nh*nw, >=3*P*P]."""
    lib = L.load()
    B, _, H, W = img.shape
    y0, y1, x0, x1 = box if box is not None else (0, H, 0, W)
    assert img.stride(3) == 1 and img.dtype == torch.float32
    L.check(lib.vfm_patchify(L.ptr(img), img.stride(0), img.stride(1), img.stride(2), y0, x0, y1 - y0, x1 - x0, patch,
                             L.ptr(out), L.dt_of(out), _ld(out), B, L.stream()), "vfm_patchify")
    return out


def assemble_tokens(patch_tok, cls, pos, x, B, np_, C_):
    lib = L.load()
    L.check(lib.vfm_assemble_tokens(L.ptr(patch_tok), L.ptr(cls), L.ptr(pos), L.ptr(x), B, np_, C_, L.stream()),
            "vfm_assemble_tokens")
    return x


def resize_bilinear(inp, in_nchw, B, Hi, Wi, Cc, out, out_mode, virt, window=None, in_ld=None, out_ld=None, scale_factor=None):
    """virt=(Hv,Wv) virtual output size; window=(y0,x0,hc,wc) (default: whole). out_mode 0 NHWC, 1 NCHW, 2 blocked.
    scale_factor=None samples like F.interpolate(size=virt); a number s (or a pair) like F.interpolate(scale_factor=s), whose source
    scale is 1/s rather than in/out (they differ when in*s is not a whole number); virt must then be floor(in*s)."""
    lib = L.load()
    Hv, Wv = virt
    y0, x0, hc, wc = window if window is not None else (0, 0, Hv, Wv)
    in_ld = Cc if in_ld is None else in_ld
    out_ld = Cc if out_ld is None else out_ld
    sy = sx = 0.0
    if scale_factor is not None:
        fy, fx = scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor)
        assert (Hv, Wv) == (int(Hi * fy), int(Wi * fx)) and fy > 0 and fx > 0, (virt, Hi, Wi, scale_factor)
        sy, sx = 1.0 / fy, 1.0 / fx
    L.check(lib.vfm_resize_bilinear(L.ptr(inp), L.dt_of(inp), int(in_nchw), B, Hi, Wi, Cc, in_ld, L.ptr(out), L.dt_of(out),
                                    out_mode, out_ld, Hv, Wv, y0, x0, hc, wc, sy, sx, L.stream()), "vfm_resize_bilinear")
    return out


def resize_bicubic(inp, Hi, Wi, Cc, out, Ho, Wo, scale_y, scale_x):
    lib = L.load()
    L.check(lib.vfm_resize_bicubic(L.ptr(inp), Hi, Wi, Cc, L.ptr(out), Ho, Wo, float(scale_y), float(scale_x), L.stream()),
            "vfm_resize_bicubic")
    return out


def label_resize(lab, out, virt, window=None):
    lib = L.load()
    B, Hi, Wi = lab.shape
    Hv, Wv = virt
    y0, x0, hc, wc = window if window is not None else (0, 0, Hv, Wv)
    assert lab.dtype == torch.int64 and lab.is_contiguous() and out.is_contiguous()
    L.check(lib.vfm_label_resize(L.ptr(lab), B, Hi, Wi, L.ptr(out), Hv, Wv, y0, x0, hc, wc, L.stream()), "vfm_label_resize")
    return out


def unblock(x, y, B, H, W, Cc, levels, inverse=False):
    lib = L.load()
    L.check(lib.vfm_unblock(L.ptr(x), L.ptr(y), B, H, W, Cc, levels, int(inverse), L.stream()), "vfm_unblock")
    return y


def upsample_ce(logits_low, label, ignore_index=255, need_grad=True):
    """logits_low fp32 [B,h,w,C] NHWC; label int64 [B,H,W]. Returns (loss[1], counts int32[2], dlogits or None)."""
    lib = L.load()
    B, h, w, Cc = logits_low.shape
    _, H, W = label.shape
    dev = logits_low.device
    parts = torch.empty(B * h * w, dtype=torch.float32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    dl = torch.empty_like(logits_low) if need_grad else None
    assert logits_low.is_contiguous() and label.is_contiguous() and label.dtype == torch.int64
    L.check(lib.vfm_upsample_ce(L.ptr(logits_low), L.ptr(label), B, h, w, Cc, H, W, ignore_index, L.ptr(parts), L.ptr(counts),
                                L.ptr(dl), L.stream()), "vfm_upsample_ce")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    L.check(lib.vfm_reduce_sum(L.ptr(parts), parts.numel(), 1.0 / (B * H * W), L.ptr(loss), L.stream()), "vfm_reduce_sum")
    return loss, counts, dl


_ce_counts = {}


def upsample_ce_loss_acc(logits_low, label, ignore_index=255, need_grad=True):
    """The training form of upsample_ce: returns (loss[1], acc[1], dlogits) with the loss / accuracy finished by ONE launch and
    a persistent, self-resetting counter pair per device (zeroed once)."""
    lib = L.load()
    B, h, w, Cc = logits_low.shape
    _, H, W = label.shape
    dev = logits_low.device
    counts = _ce_counts.get(dev)
    if counts is None:
        counts = _ce_counts[dev] = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.empty(B * h * w, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits_low) if need_grad else None
    assert logits_low.is_contiguous() and label.is_contiguous() and label.dtype == torch.int64
    L.check(lib.vfm_upsample_ce(L.ptr(logits_low), L.ptr(label), B, h, w, Cc, H, W, ignore_index, L.ptr(parts), L.ptr(counts),
                                L.ptr(dl), L.stream()), "vfm_upsample_ce")
    out = torch.empty(2, dtype=torch.float32, device=dev)
    eps = float(torch.finfo(torch.float32).eps)
    L.check(lib.vfm_ce_finish(L.ptr(parts), parts.numel(), 1.0 / (B * H * W), L.ptr(counts), eps, L.ptr(out), L.ptr(out[1:]), L.stream()),
            "vfm_ce_finish")
    return out[0:1], out[1:2], dl


def _ce_w_launch(lib, logits_low, label, weight, ignore_index, parts, counts, dl):
    B, h, w, Cc = logits_low.shape
    _, H, W = label.shape
    assert logits_low.is_contiguous() and label.is_contiguous() and label.dtype == torch.int64 and logits_low.dtype == torch.float32
    assert weight is None or (weight.dtype == torch.float32 and weight.is_contiguous() and tuple(weight.shape) == tuple(label.shape)), \
        "weight: fp32 [B,H,W] like the label"
    L.check(lib.vfm_upsample_ce_w(L.ptr(logits_low), L.ptr(label), L.ptr(weight), B, h, w, Cc, H, W, ignore_index, L.ptr(parts),
                                  L.ptr(counts), L.ptr(dl), L.stream()), "vfm_upsample_ce_w")


def upsample_ce_w(logits_low, label, weight=None, ignore_index=255, need_grad=True, parts_out=None):
    """upsample_ce with a per-pixel weight map fp32 [B,H,W] (None: the unweighted kernel, bit for bit): loss = sum_valid(w * -log p) / (B*H*W),
    dlogits scaled alike, counts unweighted.  Returns (loss[1], counts int32[2], dlogits or None).  parts_out: fp32 [B*h*w] that receives
    the per-low-res-pixel loss parts (tests)."""
    lib = L.load()
    B, h, w, _ = logits_low.shape
    _, H, W = label.shape
    dev = logits_low.device
    parts = parts_out if parts_out is not None else torch.empty(B * h * w, dtype=torch.float32, device=dev)
    assert parts.dtype == torch.float32 and parts.is_contiguous() and parts.numel() == B * h * w
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    dl = torch.empty_like(logits_low) if need_grad else None
    _ce_w_launch(lib, logits_low, label, weight, ignore_index, parts, counts, dl)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    L.check(lib.vfm_reduce_sum(L.ptr(parts), parts.numel(), 1.0 / (B * H * W), L.ptr(loss), L.stream()), "vfm_reduce_sum")
    return loss, counts, dl


def upsample_ce_w_loss_acc(logits_low, label, weight=None, ignore_index=255, need_grad=True):
    """The training form of upsample_ce_w (as upsample_ce_loss_acc): (loss[1], acc[1], dlogits)."""
    lib = L.load()
    B, h, w, _ = logits_low.shape
    _, H, W = label.shape
    dev = logits_low.device
    counts = _ce_counts.get(dev)
    if counts is None:
        counts = _ce_counts[dev] = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.empty(B * h * w, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits_low) if need_grad else None
    _ce_w_launch(lib, logits_low, label, weight, ignore_index, parts, counts, dl)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    eps = float(torch.finfo(torch.float32).eps)
    L.check(lib.vfm_ce_finish(L.ptr(parts), parts.numel(), 1.0 / (B * H * W), L.ptr(counts), eps, L.ptr(out), L.ptr(out[1:]), L.stream()),
            "vfm_ce_finish")
    return out[0:1], out[1:2], dl


OHEM_STATE_INTS, OHEM_N, OHEM_NLT, OHEM_K, OHEM_T, LABEL_COUNT_INTS = 3080, 0, 1, 2, 6, 33   # include/vfmseg_hip.h VFM_OHEM_* / VFM_LABEL_COUNT_INTS


def ohem_prob(logits_low, label, thresh, ignore_index=255):
    """p fp32 [B,H,W] = softmax(bilinear_up(logits_low))[label] (ignored pixels: -1) and the zero-initialised selection state int32
    [OHEM_STATE_INTS] with n = state[OHEM_N], #(p < thresh) = state[OHEM_NLT] and the first histogram (vfm_ohem_prob)."""
    lib = L.load()
    B, h, w, Cc = logits_low.shape
    _, H, W = label.shape
    assert logits_low.dtype == torch.float32 and logits_low.is_contiguous() and label.dtype == torch.int64 and label.is_contiguous()
    dev = logits_low.device
    p = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    state = torch.zeros(OHEM_STATE_INTS, dtype=torch.int32, device=dev)
    L.check(lib.vfm_ohem_prob(L.ptr(logits_low), L.ptr(label), B, h, w, Cc, H, W, int(ignore_index), float(thresh), L.ptr(p), L.ptr(state),
                              L.stream()), "vfm_ohem_prob")
    return p, state


def ohem_threshold(p, state, k_request, thresh):
    """After ohem_prob: the device float t = max(k-th smallest valid p, thresh), k = min(k_request, n - 1), as a view of `state`
    (vfm_ohem_threshold; exact, no host read)."""
    lib = L.load()
    assert p.dtype == torch.float32 and p.is_contiguous() and state.dtype == torch.int32 and state.numel() == OHEM_STATE_INTS
    L.check(lib.vfm_ohem_threshold(L.ptr(p), p.numel(), int(k_request), float(thresh), L.ptr(state), L.stream()), "vfm_ohem_threshold")
    return state[OHEM_T:OHEM_T + 1].view(torch.float32)


def label_weight(label, num_classes, p=None, state=None, class_weight=None, pix_weight=None, ignore_index=255, avg_non_ignore=False,
                 want_weight=True, want_norm=True):
    """(weight fp32 [B,H,W] or None, norm fp32 [2] or None, counts int32 [LABEL_COUNT_INTS] or None) of vfm_label_weight:
    weight = [valid] * [p < t] * class_weight[label] * pix_weight, norm = (B*H*W / (avg_factor + 2^-23), avg_factor)."""
    lib = L.load()
    assert label.dtype == torch.int64 and label.is_contiguous()
    dev = label.device
    for t_ in (p, pix_weight):
        assert t_ is None or (t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == label.numel())
    assert class_weight is None or (class_weight.dtype == torch.float32 and class_weight.is_contiguous() and class_weight.numel() == num_classes)
    assert (p is None) == (state is None)
    weight = torch.empty(label.shape, dtype=torch.float32, device=dev) if want_weight else None
    counts = torch.zeros(LABEL_COUNT_INTS, dtype=torch.int32, device=dev) if want_norm else None
    norm = torch.empty(2, dtype=torch.float32, device=dev) if want_norm else None
    L.check(lib.vfm_label_weight(L.ptr(label), L.ptr(p), L.ptr(state), L.ptr(class_weight), L.ptr(pix_weight), int(num_classes), label.numel(),
                                 int(ignore_index), int(bool(avg_non_ignore)), L.ptr(weight), L.ptr(counts), L.ptr(norm), L.stream()),
            "vfm_label_weight")
    return weight, norm, counts


def ohem_weight(logits_low, label, thresh, k_request, ignore_index=255, class_weight=None, pix_weight=None, avg_non_ignore=False,
                want_norm=False):
    """The OHEM chain in one call: ohem_prob -> ohem_threshold -> label_weight.  Returns (weight, p, t, state, norm, counts); t is a device
    float [1], state the counters (n, #(p < thresh), k at OHEM_N / OHEM_NLT / OHEM_K)."""
    p, state = ohem_prob(logits_low, label, thresh, ignore_index)
    t = ohem_threshold(p, state, k_request, thresh)
    weight, norm, counts = label_weight(label, logits_low.shape[-1], p, state, class_weight, pix_weight, ignore_index, avg_non_ignore,
                                        want_weight=True, want_norm=want_norm)
    return weight, p, t, state, norm, counts


def dice_blocks(H, W):
    """Rows per image of the Dice sums' slab: one block of 256 threads per 1024 pixels, at most 1024 of them (a function of the map size alone)."""
    return max(1, min(1024, (H * W + 1023) // 1024))


def upsample_dice(logits_low, label, use_sigmoid=True, naive=False, eps=1e-3, drop_class=-1, need_grad=True, ignore_index=255,
                  grad_scale=None, accumulate_into=None, stats=None):
    """Dice loss (mmseg 1.2.2 DiceLoss, reduction 'mean', loss_weight 1) of bilinear_up(logits_low) against label, the full-resolution
    logits never in memory (vfm_upsample_dice_sums -> vfm_dice_finish -> vfm_upsample_dice_bwd).
    logits_low fp32 [B,h,w,C] NHWC; label int64 [B,H,W].  Returns (loss[1], acc[1], coef [B,3], dlogits or None): coef = (alpha, beta,
    gamma) of d loss_n / d p = alpha t + beta p + gamma per image, dlogits = d loss / d logits_low * grad_scale (default 1 / B, the mean
    over the images).  drop_class: a class channel left out of every sum (-1: none).  ignore_index only names the label that the accuracy
    skips (mmseg `accuracy`); the loss knows no ignored label.  accumulate_into: an fp32 [B,h,w,C] gradient the Dice gradient is ADDED to
    (it is then the returned dlogits).  stats: a dict that receives 'sums' fp32 [B,4] = (a, sum p^2 | sum p, sum t, d) and 'counts' int32 [2] =
    (hits, valid)."""
    lib = L.load()
    B, h, w, Cc = logits_low.shape
    _, H, W = label.shape
    dev = logits_low.device
    assert logits_low.dtype == torch.float32 and logits_low.is_contiguous() and label.dtype == torch.int64 and label.is_contiguous()
    assert label.shape[0] == B
    nblk = dice_blocks(H, W)
    fsum = torch.empty(B, nblk, 2, dtype=torch.float32, device=dev)
    isum = torch.empty(B, nblk, 3, dtype=torch.int32, device=dev)
    L.check(lib.vfm_upsample_dice_sums(L.ptr(logits_low), L.ptr(label), B, h, w, Cc, H, W, int(bool(use_sigmoid)), int(bool(naive)),
                                       int(drop_class), int(ignore_index), nblk, L.ptr(fsum), L.ptr(isum), L.stream()),
            "vfm_upsample_dice_sums")
    out = torch.empty(2, dtype=torch.float32, device=dev)
    coef = torch.empty(B, 3, dtype=torch.float32, device=dev)
    sums = counts = None
    if stats is not None:
        sums = stats["sums"] = torch.empty(B, 4, dtype=torch.float32, device=dev)
        counts = stats["counts"] = torch.empty(2, dtype=torch.int32, device=dev)
    acc_eps = float(torch.finfo(torch.float32).eps)
    L.check(lib.vfm_dice_finish(L.ptr(fsum), L.ptr(isum), B, nblk, int(bool(naive)), float(eps), acc_eps, L.ptr(coef), L.ptr(sums),
                                L.ptr(counts), L.ptr(out), L.ptr(out[1:]), L.stream()), "vfm_dice_finish")
    dl = None
    if need_grad:
        dl = accumulate_into if accumulate_into is not None else torch.empty_like(logits_low)
        assert dl.dtype == torch.float32 and dl.is_contiguous() and dl.shape == logits_low.shape
        L.check(lib.vfm_upsample_dice_bwd(L.ptr(logits_low), L.ptr(label), L.ptr(coef), B, h, w, Cc, H, W, int(bool(use_sigmoid)),
                                          int(drop_class), float(1.0 / B if grad_scale is None else grad_scale),
                                          int(accumulate_into is not None), L.ptr(dl), L.stream()), "vfm_upsample_dice_bwd")
    return out[0:1], out[1:2], coef, dl


def pseudo_label(logits_low, size, thr, count, want_prob=False):
    """Teacher logits fp32 NHWC [B,h,w,C] -> (pseudo_label int64 [B,H,W], pseudo_prob fp32 [B,H,W] or None) at size = (H, W): bilinear
    (align_corners=False) + softmax + torch.max in registers; count (int32 [1], device) += #pixels with max prob >= thr."""
    lib = L.load()
    B, h, w, Cc = logits_low.shape
    H, W = int(size[0]), int(size[1])
    assert logits_low.dtype == torch.float32 and logits_low.is_contiguous()
    assert count.dtype == torch.int32 and count.numel() == 1
    dev = logits_low.device
    lab = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    prob = torch.empty(B, H, W, dtype=torch.float32, device=dev) if want_prob else None
    L.check(lib.vfm_pseudo_label(L.ptr(logits_low), B, h, w, Cc, H, W, float(thr), L.ptr(lab), L.ptr(prob), L.ptr(count), L.stream()),
            "vfm_pseudo_label")
    return lab, prob


def class_presence(label):
    """label int64 [B,...] -> uint32-as-int32 [B,8]: the 256-bit set of label values present in each image (255 included)."""
    lib = L.load()
    assert label.dtype == torch.int64 and label.is_contiguous()
    B = label.shape[0]
    bits = torch.zeros(B, 8, dtype=torch.int32, device=label.device)
    L.check(lib.vfm_class_presence(L.ptr(label), B, label.numel() // B, L.ptr(bits), L.stream()), "vfm_class_presence")
    return bits


def class_bits_to_lists(bits):
    """[B,8] bit sets (host or device) -> per image the sorted list of classes (one small device-to-host copy)."""
    rows = bits.cpu().numpy().view("uint32")
    return [[k * 32 + j for k in range(8) for j in range(32) if (int(r[k]) >> j) & 1] for r in rows]


def class_lists_to_bits(lists, device):
    """per image an iterable of classes in [0,256) -> int32 [B,8] bit sets on `device`."""
    import numpy as np
    arr = np.zeros((len(lists), 8), dtype=np.uint32)
    for b, cl in enumerate(lists):
        for c in cl:
            arr[b, int(c) >> 5] |= np.uint32(1 << (int(c) & 31))
    return torch.from_numpy(arr.view(np.int32)).to(device)


def class_mix(src_img, tgt_img, src_label, pseudo_lbl, chosen, count, total, ignore_top, ignore_bottom, want_mask=False):
    """One-pass ClassMix (vfm_class_mix).  images fp32 [B,3,H,W]; labels int64 [B,H,W]; chosen int32 [B,8] bit sets; count int32 [1] device
    counter of pseudo_label, total its denominator.  Returns (mixed_img, mixed_lbl, mix_weight, mask uint8 or None)."""
    lib = L.load()
    B, C3, H, W = src_img.shape
    assert C3 == 3 and tgt_img.shape == src_img.shape and src_img.dtype == tgt_img.dtype == torch.float32
    assert src_img.is_contiguous() and tgt_img.is_contiguous()
    for t in (src_label, pseudo_lbl):
        assert t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == (B, H, W)
    assert chosen.dtype == torch.int32 and chosen.is_contiguous() and tuple(chosen.shape) == (B, 8)
    assert count.dtype == torch.int32 and count.numel() == 1
    dev = src_img.device
    mixed = torch.empty_like(src_img)
    mlbl = torch.empty_like(src_label)
    wgt = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if want_mask else None
    L.check(lib.vfm_class_mix(L.ptr(src_img), L.ptr(tgt_img), L.ptr(src_label), L.ptr(pseudo_lbl), L.ptr(chosen), L.ptr(count), int(total),
                              int(ignore_top), int(ignore_bottom), B, H, W, L.ptr(mixed), L.ptr(mlbl), L.ptr(wgt), L.ptr(mask), L.stream()),
            "vfm_class_mix")
    return mixed, mlbl, wgt, mask


def _hrda_geo(lr, a, hr, offset, mask_box):
    B, h, w, Cc = lr.shape
    _, ha, wa, _ = a.shape
    _, hc, wc, _ = hr.shape
    for t in (lr, a, hr):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == B and t.shape[3] == Cc, "fp32 NHWC maps of one batch"
    Y0, X0 = offset
    my0, my1, mx0, mx1 = mask_box if mask_box is not None else (0, h, 0, w)
    return [int(v) for v in (B, h, w, Cc, ha, wa, hc, wc, Y0, X0, my0, my1, mx0, mx1)]


def hrda_fuse_fwd(lr, a, hr, offset, mask_box, fused, att_out=None, lr_scaled_out=None):
    """fused [B,2h,2w,C] = up2(att) * hr_inserted + up2((1 - att) * lr), att = mask * bilinear(sigmoid(a) -> h x w)  (hrda.py:149-191).
    lr [B,h,w,C], a [B,ha,wa,C], hr [B,hc,wc,C] at `offset` = (Y0, X0) of the output grid; mask_box = (y0, y1, x0, x1) on the lr grid or
    None (no crop).  Optional outputs att_out / lr_scaled_out [B,h,w,C]."""
    lib = L.load()
    geo = _hrda_geo(lr, a, hr, offset, mask_box)
    B, h, w, Cc = geo[:4]
    assert fused.dtype == torch.float32 and fused.is_contiguous() and tuple(fused.shape) == (B, 2 * h, 2 * w, Cc)
    for t in (att_out, lr_scaled_out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, h, w, Cc))
    L.check(lib.vfm_hrda_fuse_fwd(L.ptr(lr), L.ptr(a), L.ptr(hr), *geo, L.ptr(fused), L.ptr(att_out), L.ptr(lr_scaled_out), L.stream()),
            "vfm_hrda_fuse_fwd")
    return fused


def hrda_fuse_bwd(d_fused, lr, a, hr, att, offset, mask_box, d_lr, d_a, d_hr):
    """Backward of hrda_fuse_fwd from d_fused and the saved att; writes every element of d_lr, d_a, d_hr (gathers, no float atomics)."""
    lib = L.load()
    geo = _hrda_geo(lr, a, hr, offset, mask_box)
    B, h, w, Cc = geo[:4]
    assert d_fused.dtype == torch.float32 and d_fused.is_contiguous() and tuple(d_fused.shape) == (B, 2 * h, 2 * w, Cc)
    assert att.dtype == torch.float32 and att.is_contiguous() and att.shape == lr.shape
    for t, s in ((d_lr, lr), (d_a, a), (d_hr, hr)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == s.shape
    ws = workspace(lr.numel(), lr.device, "hrda_d_att")
    L.check(lib.vfm_hrda_fuse_bwd(L.ptr(d_fused), L.ptr(lr), L.ptr(a), L.ptr(hr), L.ptr(att), *geo, L.ptr(d_lr), L.ptr(d_a), L.ptr(d_hr),
                                  L.ptr(ws), L.stream()), "vfm_hrda_fuse_bwd")
    return d_lr, d_a, d_hr


def preprocess_u8(img_u8, out, mean, std, bgr_to_rgb, pad_val=0.0):
    """img_u8 uint8 [3,H,W] (cuda) -> out fp32 [3,Hp,Wp]: channel swap, normalise, pad (mmseg SegDataPreProcessor)."""
    lib = L.load()
    assert img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32
    _, H, W = img_u8.shape
    _, Hp, Wp = out.shape
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    L.check(lib.vfm_preprocess_u8(L.ptr(img_u8), H, W, L.ptr(out), Hp, Wp, m3, s3, int(bool(bgr_to_rgb)), float(pad_val), L.stream()),
            "vfm_preprocess_u8")
    return out


def augment_u8(img_u8, plan, out, mean, std, bgr_to_rgb, pad_val=0.0):
    """img_u8 uint8 [Hs,Ws,3] as decoded (cuda, HWC) -> out fp32 [3,Hp,Wp]: the training chain Resize -> RandomCrop -> RandomFlip ->
    PhotoMetricDistortion with the parameters of `plan` (datasets.Compose(device=True): metainfo["aug_plan"]), then channel swap,
    normalise, pad - equal to preprocess_u8 of the host chain's crop (vfm_augment_u8, one launch)."""
    lib = L.load()
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous()
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == 3
    Hs, Ws, _ = img_u8.shape
    _, Hp, Wp = out.shape
    rs, (cy, cx, ch, cw) = plan.get("resize"), plan["crop"]
    on_b, beta = plan.get("brightness", (0, 0.0))
    pos_c, alpha_c = plan.get("contrast", (0, 1.0))
    on_s, alpha_s = plan.get("saturation", (0, 1.0))
    on_h, delta = plan.get("hue", (0, 0))
    p = L.AugmentPlan(int(rs[0]) if rs else 0, int(rs[1]) if rs else 0, int(cy), int(cx), int(ch), int(cw), int(plan.get("flip", 0)),
                      int(bool(plan.get("wide", False))), int(bool(on_b)), int(pos_c), int(bool(on_s)), int(bool(on_h)), int(delta),
                      float(beta), float(alpha_c), float(alpha_s))
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    L.check(lib.vfm_augment_u8(L.ptr(img_u8), Hs, Ws, C.byref(p), L.ptr(out), Hp, Wp, m3, s3, int(bool(bgr_to_rgb)), float(pad_val), L.stream()),
            "vfm_augment_u8")
    return out


def conf_gate_count(logits_nchw, window, thr, count):
    lib = L.load()
    B, Cc, H, W = logits_nchw.shape
    y0, x0, hc, wc = window
    L.check(lib.vfm_conf_gate(L.ptr(logits_nchw), B, Cc, H, W, y0, x0, hc, wc, float(thr), L.ptr(count), L.stream()),
            "vfm_conf_gate")
    return count


def slide_accumulate(crop, crop_nchw, B, h, w, Cc, preds, count, window):
    lib = L.load()
    _, _, H, W = preds.shape
    y0, x0, hc, wc = window
    L.check(lib.vfm_slide_accumulate(L.ptr(crop), int(crop_nchw), B, h, w, Cc, L.ptr(preds), L.ptr(count), H, W, y0, x0, hc, wc,
                                     L.stream()), "vfm_slide_accumulate")


def slide_gather(wins, preds):
    """wins: list of (logits, nchw, window=(y0, x0, hc, wc)) in accumulation order; logits NHWC [B,h,w,C] or NCHW [B,C,h,w] fp32 contiguous.
    preds [B,C,H,W] = mean over the covering windows of their bilinear samples (vfm_slide_gather); returns False when the table does not fit
    (more than 16 windows / 32 channels): the caller then takes the per-window accumulate path."""
    B, Cc, H, W = preds.shape
    if len(wins) > 16 or Cc > 32 or len(wins) == 0 or os.environ.get("VFMSEG_SLIDE_GATHER", "1") == "0":   # (env: A/B of the two paths)
        return False
    arr = (L.SlideWin * len(wins))()
    for j, (t, nchw, (y0, x0, hc, wc)) in enumerate(wins):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == B
        h, w = (t.shape[2], t.shape[3]) if nchw else (t.shape[1], t.shape[2])
        arr[j] = L.SlideWin(L.ptr(t), int(bool(nchw)), h, w, y0, x0, hc, wc)
    L.check(L.load().vfm_slide_gather(arr, len(wins), B, Cc, L.ptr(preds), H, W, L.stream()), "vfm_slide_gather")
    return True


def conf_gate_windows(logits_nchw, windows, thr, counts):
    """counts[j] += number of pixels of window j = (y0, x0, hc, wc) whose max softmax exceeds thr - all windows in one pass (<= 16)."""
    B, Cc, H, W = logits_nchw.shape
    flat = (L.ci * (4 * len(windows)))(*[int(v) for wdw in windows for v in wdw])
    L.check(L.load().vfm_conf_gate_windows(L.ptr(logits_nchw), B, Cc, H, W, flat, len(windows), float(thr), L.ptr(counts), L.stream()),
            "vfm_conf_gate_windows")
    return counts


def slide_finalize(preds, count, argmax=None):
    lib = L.load()
    B, Cc, H, W = preds.shape
    L.check(lib.vfm_slide_finalize(L.ptr(preds), L.ptr(count), L.ptr(argmax), B, Cc, H, W, L.stream()), "vfm_slide_finalize")
    return preds


def confusion_hist(pred_u8, label, hist, num_classes, ignore_index=255):
    """hist int64 [(nc+1)*nc] += confusion counts of (label, pred) over the pixels with label != ignore_index."""
    lib = L.load()
    assert pred_u8.dtype == torch.uint8 and pred_u8.is_contiguous() and label.is_contiguous() and pred_u8.numel() == label.numel()
    assert hist.dtype == torch.int64 and hist.numel() == (num_classes + 1) * num_classes
    L.check(lib.vfm_confusion_hist(L.ptr(pred_u8), L.ptr(label), L.dt_of(label), pred_u8.numel(), int(num_classes), int(ignore_index),
                                   L.ptr(hist), L.stream()), "vfm_confusion_hist")
    return hist


def postprocess_argmax(logits, window, flip, out_size, pred=None, label=None, hist=None, num_classes=None, ignore_index=255):
    """pred uint8 [oh, ow] = argmax over the classes of the window (y0, x0, h, w) of ONE image's fp32 logits [C, H, W] (a view of a
    batch element of an NCHW map: only its last stride must be 1), un-flipped (flip 0 none, 1 horizontal, 2 vertical) and resized
    bilinearly to out_size (vfm_postprocess_argmax).  With label (int64 / uint8, oh*ow elements) and hist (int64 [(nc+1)*nc]) the
    confusion counts of vfm_confusion_hist are added to hist in the same launch."""
    lib = L.load()
    assert logits.dim() == 3 and logits.dtype == torch.float32 and logits.stride(2) == 1, (logits.shape, logits.dtype, logits.stride())
    Cc, Hm, Wm = logits.shape
    y0, x0, h, w = (int(v) for v in window)
    oh, ow = int(out_size[0]), int(out_size[1])
    if pred is None:
        pred = torch.empty(oh, ow, dtype=torch.uint8, device=logits.device)
    assert pred.dtype == torch.uint8 and pred.is_contiguous() and pred.numel() == oh * ow
    ldt = 0
    if hist is not None:
        assert hist.dtype == torch.int64 and hist.is_contiguous() and num_classes is not None and hist.numel() == (num_classes + 1) * num_classes
        if label is not None:
            assert label.is_contiguous() and label.numel() == oh * ow, (label.shape, (oh, ow))
            ldt = L.dt_of(label)
    L.check(lib.vfm_postprocess_argmax(L.ptr(logits), Cc, logits.stride(0), logits.stride(1), Hm, Wm, y0, x0, h, w, int(flip), L.ptr(pred), oh, ow,
                                       L.ptr(label), ldt, int(num_classes or 0), int(ignore_index), L.ptr(hist), L.stream()),
            "vfm_postprocess_argmax")
    return pred


def adamw(p, g, m, v, seg_start, seg_lr_mult, seg_wd, lr, betas, eps, step, grad_scale=1.0, zero_grad=False, vec4=False, skip=None, amp_state=None,
          clip_coef=None, clip_value=0.0):
    """skip: int32 device tensor [1]; non-zero = leave parameters and moments alone (loss-scaled training: the step's gradients overflowed).
    amp_state: fp32 device tensor [4] {loss scale, growth tracker, steps taken, steps skipped}: un-scale and bias corrections from it.
    clip_coef: fp32 device tensor [1] (grad_norm()'s clip state [1:2]): the gradients are multiplied by it on top of grad_scale;
    clip_value > 0: the un-scaled gradient is clamped to +-clip_value before the moments.  Either one selects vfm_adamw_clip; without
    them the call is vfm_adamw_guarded, as before."""
    lib = L.load()
    assert skip is None or (skip.dtype == torch.int32 and skip.numel() == 1)
    assert amp_state is None or (amp_state.dtype == torch.float32 and amp_state.numel() == 4 and amp_state.is_contiguous())
    args = (L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), L.ptr(seg_start), L.ptr(seg_lr_mult),
            L.ptr(seg_wd), seg_start.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), max(int(step), 1),
            float(grad_scale), int(bool(zero_grad)), int(bool(vec4)), L.ptr(skip), L.ptr(amp_state))
    if clip_coef is None and not clip_value > 0:
        L.check(lib.vfm_adamw_guarded(*args, L.stream()), "vfm_adamw")
        return
    assert clip_coef is None or (clip_coef.dtype == torch.float32 and clip_coef.numel() == 1 and clip_coef.device == p.device)
    L.check(lib.vfm_adamw_clip(*args, L.ptr(clip_coef), float(clip_value), L.stream()), "vfm_adamw_clip")


NORM_KINDS = {2: 2, 1: 1, float("inf"): 0, "inf": 0}   # norm_type (2.0 and 1.0 hash as 2 and 1) -> VFM_NORM_L2 / VFM_NORM_L1 / VFM_NORM_INF


def grad_norm(g, norm_type=2, max_norm=float("inf"), pre_scale=1.0, amp_state=None, clip_state=None, flag=None, workspace=None):
    """vfm_grad_norm: norm of `pre_scale * g` (with amp_state: of `pre_scale / amp_state[0] * g`) over the flat fp32 buffer g and torch's
    clip_grad_norm_ coefficient, left on the device: -> clip_state fp32 [4] {total norm, min(1, max_norm / (total + 1e-6)), 0, 0}.
    flag: int32 [1], set to 1 when g holds an inf / NaN, else to 0.  workspace: float64 [4096] (allocated when not given).  No host read."""
    lib = L.load()
    if norm_type not in NORM_KINDS:
        raise ValueError("grad_norm: norm_type %r (2, 1 and inf are the norms the kernel computes)" % (norm_type,))
    assert g.dtype == torch.float32 and g.dim() == 1 and g.is_contiguous(), (g.dtype, g.shape)
    if clip_state is None:
        clip_state = torch.empty(4, dtype=torch.float32, device=g.device)
    if workspace is None:
        workspace = torch.empty(4096, dtype=torch.float64, device=g.device)
    assert clip_state.dtype == torch.float32 and clip_state.numel() == 4 and clip_state.is_contiguous()
    assert workspace.dtype == torch.float64 and workspace.numel() >= 4096 and workspace.is_contiguous()
    assert flag is None or (flag.dtype == torch.int32 and flag.numel() == 1)
    assert amp_state is None or (amp_state.dtype == torch.float32 and amp_state.numel() == 4 and amp_state.is_contiguous())
    L.check(lib.vfm_grad_norm(L.ptr(g), g.numel(), NORM_KINDS[norm_type], float(max_norm), float(pre_scale), L.ptr(amp_state), L.ptr(workspace),
                              L.ptr(clip_state), L.ptr(flag), L.stream()), "vfm_grad_norm")
    return clip_state


def amp_update(flag, amp_state, growth, backoff, interval, dynamic):
    """GradScaler.update() + the optimiser's step count on the device (vfm_amp_update)."""
    L.check(L.load().vfm_amp_update(L.ptr(flag), L.ptr(amp_state), float(growth), float(backoff), int(interval), int(bool(dynamic)), L.stream()),
            "vfm_amp_update")
