"""Plain-torch / numpy restatements (CPU, any float dtype: float64 for references, float32 where a test needs the exact value a
kernel must store) of what the entries of csrc/elementwise.hip compute, and the per-element rounding bounds of the float32
expressions as the kernels write them.

tests/test_elementwise_cpu.py pins the restatements: the hand-written GEGLU / SwiGLU / act' backward formulas to torch autograd,
`rope_ref` to the oracle's  x * cos + rotate_half(x) * sin  and its inverse to the exact transpose, `split3_ref` to hi + lo = x,
`dropout_mask_ref` to the offset contract (element i depends on (seed, offset + i) alone).

Conventions: h = [a | g] is [rows, 2C]; GEGLU gates with gelu(g), SwiGLU with silu(a).  RoPE pairs are (2i, 2i+1) inside a head of
width d, the table row is row % np, and every table COLUMN is independent (cos[2i] need not equal cos[2i+1]).

Bounds: U = 2^-24 is one float32 rounding relative to the magnitude of what is rounded.  Every product or sum of the kernel's
expression contributes U of its magnitude; an error already made in an operand passes through a subtraction unchanged (so `1 - sg`
carries the absolute error of sg, however small the difference).  The two library functions enter through allowances measured
away from the kernels under test: `erf_ulps` (erff: error of the result in units of 2^-23 |result|) and `exp2_ulps` (the hardware
exp2 behind __expf(x) = exp2(x log2 e), same unit); rounding the product x log2 e shifts the result by 2^-23 |x| relative.  The fast
exponential has no subnormal results (what would land below 2^-126 comes out as 0) and overflows to inf above 2^128: FLOOR covers
the absolute error of such a flushed quantity times the largest factor it meets at the tests' inputs (< 2^8)."""
import math

import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -118
ACT_NONE, ACT_GELU, ACT_RELU, ACT_QGELU = 0, 1, 2, 3
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


# ------------------------------------------------------------------------------------------------------------ counter-based RNG
def hash_u32(seed, idx):
    """csrc/common.h hash_u32 (splitmix-style) on numpy uint64 arrays (arithmetic modulo 2^64) -> uint64 array of 32-bit values."""
    with np.errstate(over="ignore"):
        idx = np.asarray(idx, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return z >> np.uint64(32)


def dropout_mask_ref(n, p, seed, offset, dtype):
    """vfm_dropout_mask: u = (h >> 8) 2^-24 (exact in float32), keep iff u >= float32(p), kept value float32(1) / (float32(1) -
    float32(p)) rounded to `dtype`."""
    with np.errstate(over="ignore"):
        idx = np.uint64(offset % (1 << 64)) + np.arange(n, dtype=np.uint64)
    u = (hash_u32(seed % (1 << 64), idx) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    p32 = np.float32(p)
    ks = np.float32(1.0) / (np.float32(1.0) - p32)
    return torch.from_numpy(np.where(u >= p32, ks, np.float32(0.0)).astype(np.float32)).to(dtype)


# Counters whose uniform equals float32(p) exactly under DROPOUT_TIE_SEED (found by searching the first 2^26 counters with hash_u32;
# float32(0.1) is no multiple of 2^-24, so p = 0.1 has no tie): the elements that tell `u >= p` from `u > p`.
DROPOUT_TIE_SEED = 20240917
DROPOUT_TIES = {0.0: (14803996, 35719958), 0.5: (1832703, 8905800)}


# ------------------------------------------------------------------------------------------------------------ activations
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * SQRT1_2))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * SQRT1_2)) + x * INV_SQRT_2PI * torch.exp(-0.5 * x * x)


def qgelu_grad(x):
    sg = torch.sigmoid(1.702 * x)
    return sg * (1.0 + 1.702 * x * (1.0 - sg))


def relu_grad(x):
    return (x > 0).to(x.dtype)


def act_grad(x, act):
    return {ACT_NONE: torch.ones_like, ACT_GELU: gelu_grad, ACT_RELU: relu_grad, ACT_QGELU: qgelu_grad}[act](x)


def geglu_fwd_ref(a, g):
    return a * gelu(g)


def geglu_bwd_ref(a, g, d):
    """-> (da, dg)"""
    return d * gelu(g), d * a * gelu_grad(g)


def swiglu_fwd_ref(a, g):
    return a * torch.sigmoid(a) * g


def swiglu_bwd_ref(a, g, d):
    """-> (da, dg)"""
    sg = torch.sigmoid(a)
    return d * g * sg * (1.0 + a * (1.0 - sg)), d * a * sg


# ------------------------------------------------------------------------------------------------------------ bounds (float64 in)
def _erf_parts(x, erf_ulps):
    """1 + erf(x / sqrt 2) and the absolute error of its float32 evaluation: the argument carries two roundings (the constant, the
    product) that erf' = 2/sqrt(pi) exp(-t^2) passes on, erff its allowance, the sum one rounding."""
    t = x * SQRT1_2
    e = torch.erf(t)
    s = 1.0 + e
    b = erf_ulps * 2 * U * e.abs() + 2.0 / math.sqrt(math.pi) * torch.exp(-t * t) * t.abs() * 2 * U + U * s.abs()
    return s, b


def gelu_bound(x, erf_ulps):
    s, b = _erf_parts(x, erf_ulps)
    return 0.5 * x.abs() * b + 2 * U * (0.5 * x * s).abs()


def gelu_grad_bound(x, erf_ulps, exp2_ulps):
    """cdf + x pdf: cdf = 0.5 (1 + erf) (the halving is exact); pdf = k exp(q), q = -0.5 x x (one rounding), the fast exponential
    adds 2^-23 |q| and its allowance, k two roundings (constant, product); then the product with x and the sum."""
    s, b = _erf_parts(x, erf_ulps)
    q = 0.5 * x * x
    pdf = INV_SQRT_2PI * torch.exp(-q)
    r_pdf = 3 * U * q + exp2_ulps * 2 * U + 2 * U
    return 0.5 * b + x.abs() * pdf * (r_pdf + U) + U * gelu_grad(x).abs() + FLOOR


def _sigmoid_parts(z, r_arg, exp2_ulps):
    """sg = 1 / (1 + exp(-z)) and its absolute error; r_arg = relative error already in the argument of the exponential."""
    E = torch.exp(-z)
    D = 1.0 + E
    sg = 1.0 / D
    r_E = (r_arg + 2 * U) * z.abs() + exp2_ulps * 2 * U
    return sg, sg * (3 * U + r_E * E / D) + FLOOR           # sum: U, division: 2 U (one ulp, should it be a reciprocal)


def qgelu_grad_bound(x, exp2_ulps):
    """sg (1 + 1.702 x (1 - sg)), sg = 1 / (1 + exp(-1.702 x)): the argument has two roundings (constant, product)."""
    sg, b_sg = _sigmoid_parts(1.702 * x, 2 * U, exp2_ulps)
    w = 1.0 - sg
    b_w = b_sg + U * w.abs()
    m = 1.702 * x * w
    b_m = (1.702 * x).abs() * b_w + 3 * U * m.abs()
    n = 1.0 + m
    b_n = b_m + U * n.abs()
    return n.abs() * b_sg + sg * b_n + U * (sg * n).abs()


def act_grad_bound(x, act, erf_ulps, exp2_ulps):
    if act == ACT_GELU:
        return gelu_grad_bound(x, erf_ulps, exp2_ulps)
    if act == ACT_QGELU:
        return qgelu_grad_bound(x, exp2_ulps)
    return torch.zeros_like(x)                               # NONE, RELU: the factor is exactly 0 or 1


def act_grad_mul_bound(dy, x, act, erf_ulps, exp2_ulps):
    if act in (ACT_NONE, ACT_RELU):
        return torch.zeros_like(x)                           # dy * 1 and dy * 0 are exact
    return dy.abs() * act_grad_bound(x, act, erf_ulps, exp2_ulps) + U * (dy * act_grad(x, act)).abs()


def geglu_fwd_bound(a, g, erf_ulps):
    return a.abs() * gelu_bound(g, erf_ulps) + U * geglu_fwd_ref(a, g).abs()


def geglu_bwd_bound(a, g, d, erf_ulps, exp2_ulps):
    da, dg = geglu_bwd_ref(a, g, d)
    return d.abs() * gelu_bound(g, erf_ulps) + U * da.abs(), (d * a).abs() * gelu_grad_bound(g, erf_ulps, exp2_ulps) + 2 * U * dg.abs()


def swiglu_fwd_bound(a, g, exp2_ulps):
    """a / (1 + exp(-a)) * g: the sum, the division (2 U) and the product, plus what the exponential's error leaves of 1 + E."""
    E = torch.exp(-a)
    r_E = 2 * U * a.abs() + exp2_ulps * 2 * U
    return swiglu_fwd_ref(a, g).abs() * (r_E * E / (1.0 + E) + 4 * U) + FLOOR


def swiglu_bwd_bound(a, g, d, exp2_ulps):
    sg, b_sg = _sigmoid_parts(a, 0.0, exp2_ulps)
    w = 1.0 - sg
    b_w = b_sg + U * w.abs()
    m = a * w
    b_m = a.abs() * b_w + U * m.abs()
    n = 1.0 + m
    b_n = b_m + U * n.abs()
    da, dg = swiglu_bwd_ref(a, g, d)
    return (d * g).abs() * (n.abs() * b_sg + sg * b_n) + 3 * U * da.abs(), (d * a).abs() * b_sg + 2 * U * dg.abs()


# ------------------------------------------------------------------------------------------------------------ RoPE
def _rope_terms(x, cos, sin, np_, ncols, d, inverse):
    rows = x.shape[0]
    t = torch.arange(rows) % np_
    H = ncols // d
    c = cos.to(x.dtype)[t][:, None, :].expand(rows, H, d).reshape(rows, H * d // 2, 2)
    s = sin.to(x.dtype)[t][:, None, :].expand(rows, H, d).reshape(rows, H * d // 2, 2)
    v = x[:, :ncols].reshape(rows, H * d // 2, 2)
    x0, x1, c0, c1, s0, s1 = v[..., 0], v[..., 1], c[..., 0], c[..., 1], s[..., 0], s[..., 1]
    if not inverse:
        return (x0 * c0, -x1 * s0), (x1 * c1, x0 * s1)
    return (x0 * c0, x1 * s1), (x1 * c1, -x0 * s0)


def rope_ref(x, cos, sin, np_, ncols, d, inverse=False):
    """vfm_rope on a copy: columns [0, ncols) of x [rows, >= ncols] are heads of width d; the pair (2i, 2i+1) of the token row % np
    goes to (x0 c[2i] - x1 s[2i], x1 c[2i+1] + x0 s[2i+1]); inverse = the transpose of that map.  Columns >= ncols are kept."""
    (p0, q0), (p1, q1) = _rope_terms(x, cos, sin, np_, ncols, d, inverse)
    out = x.clone()
    out[:, :ncols] = torch.stack((p0 + q0, p1 + q1), dim=-1).reshape(x.shape[0], ncols)
    return out


def rope_abs(x, cos, sin, np_, ncols, d, inverse=False):
    """[rows, ncols]: |R| |x| (inverse: |R^T| |x|), the sum of the magnitudes of the two products behind every output."""
    (p0, q0), (p1, q1) = _rope_terms(x, cos, sin, np_, ncols, d, inverse)
    return torch.stack((p0.abs() + q0.abs(), p1.abs() + q1.abs()), dim=-1).reshape(x.shape[0], ncols)


def rope_bound(x, cos, sin, np_, ncols, d, inverse=False):
    """Two products and their sum, each rounded at the magnitude of the products (not of a cancelling result); (1 + 2 U): the sum
    rounds the already rounded products."""
    return 2 * U * (1 + 2 * U) * rope_abs(x, cos, sin, np_, ncols, d, inverse)


# ------------------------------------------------------------------------------------------------------------ layout entries
def split3_ref(x, pattern, dtype=torch.bfloat16):
    """vfm_split3: float32 x [rows, K] -> [rows, 3 Kp] of `dtype`, Kp = ceil64(K): hi = RNE(x), lo = RNE(x - hi) (the difference is
    exact in float32), pattern 0 = [hi | hi | lo], 1 = [hi | lo | hi], columns K..Kp-1 of every segment zero."""
    rows, K = x.shape
    Kp = (K + 63) // 64 * 64
    hi = x.float().to(dtype)
    lo = (x.float() - hi.float()).to(dtype)
    out = torch.zeros(rows, 3 * Kp, dtype=dtype)
    for seg, v in enumerate((hi, hi, lo) if pattern == 0 else (hi, lo, hi)):
        out[:, seg * Kp:seg * Kp + K] = v
    return out


def lora_pack_ref(A, B, a, at, w, wt, Kw):
    """vfm_lora_pack for one site, on copies: a[:r, :K] = A, at[:K, :r] = A^T, w[:N, Kw:Kw+r] = B, wt[Kw:Kw+r, :N] = B^T (wt may be
    None); everything else is kept."""
    r, K = A.shape
    N = B.shape[0]
    a, at, w = a.clone(), at.clone(), w.clone()
    a[:r, :K] = A.to(a.dtype)
    at[:K, :r] = A.t().to(at.dtype)
    w[:N, Kw:Kw + r] = B.to(w.dtype)
    if wt is not None:
        wt = wt.clone()
        wt[Kw:Kw + r, :N] = B.t().to(wt.dtype)
    return a, at, w, wt


def transpose_ref(x, pad_rows, dtype):
    """vfm_transpose: [rows, cols] -> [cols, pad_rows] of `dtype`, columns rows..pad_rows-1 zero."""
    rows, cols = x.shape
    out = torch.zeros(cols, pad_rows, dtype=dtype)
    out[:, :rows] = x.float().t().to(dtype)
    return out


# ------------------------------------------------------------------------------------------------------------ sums
def gamma(n):
    return n * U / (1.0 - n * U)


def reduce_depth(n, threads=1024):
    """Additions any one term of k_reduce_sum / k_ce_finish passes through: the thread's own loop, six wave shuffles, the serial sum
    over the 16 waves."""
    return -(-n // threads) + 6 + threads // 64


def colsum2_depth(parts):
    """k_colsum2: a group's loop over every fourth part (the unrolled form adds a four-term tree per step), then the LDS tree."""
    return -(-parts // 4) + 2 + 2


def colsum_geometry(rows, cols):
    """(CT, row lanes, parts) as vfm_colsum chooses them."""
    CT = 64
    while CT > 8 and CT // 2 >= cols:
        CT //= 2
    rl = 256 // CT
    parts = min(64, max(1, -(-rows // (rl * 8))))
    return CT, rl, parts


def colsum_depth(rows, cols):
    _, rl, parts = colsum_geometry(rows, cols)
    return -(-rows // (parts * rl)) + rl + colsum2_depth(parts)


def mask_token_geometry(rows):
    """(chunks, rows per chunk) as vfm_mask_token_bwd chooses them."""
    nchunk = min(64, max(1, -(-rows // 32)))
    return nchunk, -(-rows // nchunk)


def mask_token_depth(rows):
    nchunk, rpc = mask_token_geometry(rows)
    return -(-rpc // 4) + 2 + colsum2_depth(nchunk)
