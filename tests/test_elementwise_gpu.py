"""Every entry of csrc/elementwise.hip against the restatements of tests/elementwise_helpers.py (pinned by
tests/test_elementwise_cpu.py), at the smallest shapes that take every kernel form and every selector of the dispatchers.  Output
buffers start as NaN inside a buffer of sentinels (-77, exact in all three types); after every call the sentinels must still be
there bit for bit.  Every produced element is checked, never a global max ratio.  The 16-bit type is spelled torch.bfloat16 so
that the fp16 pass (tests/test_fp16_twin_gpu.py) re-types it; the split-bf16 test carries bf16x3 in its name and stays out of it.

Three kinds of comparison:
  exact    torch.equal with the float32 restatement rounded once (RNE) to the output type: entries with one multiply at most;
  sums     float64 sum of the stored values, bound gamma(n) sum|x| + one rounding for scale / accumulate, n = the additions one term
           passes through in the kernel as written (never more than the number of terms); inputs have magnitude in [0.5, 2], and
           every case asserts 0.5 > 4 x bound on the CPU, so a dropped or doubled term cannot hide;
  formula  (a) the x8 form and the scalar form give the same bits on the same 16-bit data, (b) the scalar form with a 16-bit store
           equals the scalar form with a float32 store rounded RNE, (c) the float32 scalar form lies within the bound derived in
           tests/elementwise_helpers.py of float64.  Together: a float32-level formula error is visible behind a 16-bit store.

The allowances for the two library functions are measured by test_library_function_allowances on ATen's kernels (not ours), over
the arguments these tests use, and doubled: erff 2 x the worst |torch.erf(float32) - float64| in units of 2^-23 |erf|, the hardware
exp2 2 x the worst relative error of torch.exp2(float32) in units of 2^-23 (no document at hand states it).  Measured on the
MI355X: erff worst 0.82 -> allowance 1.64; exp2 worst 0.67 -> allowance 1.33 (profiles/elementwise_gpu.log).

Which case reaches which kernel of elementwise.hip (16 = the 16-bit type, 32 = float32):
  k_cast<TI,TO>                test_cast: all four pairs, cols 1 / 3 (tail loop only), 4, 70, with and without colscale, column
                               slices; test_cast_second_pass (1100 x 4096, the grid-stride loop's second pass)
  k_split3                     test_split3_bf16x3: whole float4 / element-wise last vector, transposed and misaligned sources
  k_transpose<TI,TO>           test_transpose: all four pairs, one / two / three row tiles, a tile wholly in the padding
  k_strided_copy<TI,TO>        test_strided_copy: permutation (all pairs), broadcast source, accumulate into 32 and into 16
  k_axpby                      test_axpby (b == 0 onto NaN, b != 0, second pass at 2^20 + 3)
  k_scale_dev                  tests/test_sam_window_gpu.py::test_scale_by_device_scalar
  k_colsum1<float>, <bf16_t>   test_colsum: CT = 8 / 16 / 32 / 64, both input types
  k_colsum2                    test_colsum: 1 / 3 / 11 parts (remainder loop) and 64 parts (unrolled loop, all four groups);
                               test_mask_token: 1 / 4 / 64 chunks
  k_slab_reduce                tests/test_kernels_gpu.py::test_slab_reduce
  k_strided_copy_batch         tests/test_kernels_gpu.py::test_copy_batch_sums_partials
  k_lora_pack                  test_lora_pack (three sites, second pass of the stride loop, null wt, 16 and 32)
  k_dropout_mask_bf16x8        test_dropout_mask "h16 aligned"
  k_dropout_mask<float>        test_dropout_mask "f32" (second pass: n > 4096 * 256)
  k_dropout_mask<bf16_t>       test_dropout_mask "h16 shifted" and "h16 n % 8 != 0"
  k_mul_mask_bf16x8            test_mul_mask all-16 with cols 8 / 24 (rows_per_group 16, last group partial)
  k_mul_mask_x8<...>           test_mul_mask 16 x 32 -> 16 and all-32 with cols 8 / 24 (the seven mixes: test_kernels_gpu.py)
  k_mul_mask                   test_mul_mask cols = 20, and the shifted all-16 run
  k_geglu_fwd_x8 / bwd_x8      test_geglu all-16 aligned, C = 8 / 48
  k_geglu_fwd / bwd            test_geglu all-16 shifted, 16 -> 32, all-32, and C = 5
  k_swiglu_fwd_x8<true/false>  test_swiglu_fwd 16 -> 16 / 16 -> 32 aligned, C = 8 / 48
  k_swiglu_fwd                 test_swiglu_fwd all-32, shifted 16, C = 5
  k_swiglu_bwd_x8<true/false>  test_swiglu_bwd 16-bit dout / float32 dout aligned, C = 8 / 48
  k_swiglu_bwd                 test_swiglu_bwd all-32, 16-bit h with float32 dh, shifted, C = 5
  k_rope_bf16x8                test_rope 16 aligned, d = 64 / 8
  k_rope                       test_rope float32, 16 shifted, and d = 6
  k_act_grad_mul_bf16x8        test_act_grad_mul all-16 aligned, cols = 24
  k_act_grad_mul               test_act_grad_mul all-16 shifted, all-32, the two mixed runs, cols = 7
  k_mask_token_fwd / bwd       test_mask_token
  k_reduce_sum, k_ce_finish    test_reduce_sum_and_ce_finish"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import elementwise_helpers as E  # noqa: E402
from tests.helpers import _within  # noqa: E402
from vfmseg_amd import lib as L, ops  # noqa: E402

DEV = "cuda"
U = E.U
SENT = -77.0                      # exact in float32, bf16 and fp16
F32 = torch.float32
PAIRS = [(F32, F32), (F32, torch.bfloat16), (torch.bfloat16, F32), (torch.bfloat16, torch.bfloat16)]
SPECIAL = [0.0, 2.0 ** -20, -2.0 ** -20, -1.4142135, 20.0, -20.0, 37.5, -37.5, 60.0, -60.0]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _dtname(dt):
    return "f32" if dt == F32 else "h16"


def _h16(t):
    """The values of t rounded to the 16-bit type, as float32: every form of an entry is then given the same numbers."""
    return t.to(torch.bfloat16).float()


def _bits(t):
    t = t.detach().cpu().reshape(-1).contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Buf:
    """A [rows, cols] view with leading dimension ld (default cols + 8) that starts `shift` elements into a buffer of sentinels:
    shift = 1 puts the base one element past an aligned address, any shift makes it a column slice of a wider buffer.  The view
    holds `data` (an input) or NaN (an output)."""

    def __init__(self, rows, cols, dtype, data=None, ld=None, shift=0):
        self.rows, self.cols, self.ld, self.shift = rows, cols, cols + 8 if ld is None else ld, shift
        self.flat = torch.full((shift + rows * self.ld + 8,), SENT, dtype=dtype, device=DEV)
        self.full = self.flat[shift:shift + rows * self.ld].view(rows, self.ld)
        self.v = self.full[:, :cols]
        if data is None:
            self.v.fill_(float("nan"))
        else:
            self.v.copy_(data.reshape(rows, cols))

    def cpu(self):
        """The view's values, after checking that every sentinel is still there bit for bit."""
        f = self.flat.cpu()
        body = f[self.shift:self.shift + self.rows * self.ld].view(self.rows, self.ld)
        want = _bits(torch.full((1,), SENT, dtype=f.dtype))[0]
        for part in (f[:self.shift], f[self.shift + self.rows * self.ld:], body[:, self.cols:]):
            assert (_bits(part) == want).all(), "sentinel overwritten"
        return body[:, :self.cols].clone()


def _signed_mag(shape, g):
    """Magnitudes in [0.5, 2], random sign, exact in the 16-bit type."""
    v = (torch.rand(shape, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    return _h16(v).clamp(-2, 2)


def _preact(rows, C, g):
    """rows x C pre-activations: a grid over [-9, 9] and the special points (0, +-2^-20, the minimum of gelu' near -1.414, values in
    +-[20, 60] where exp overflows / underflows), shuffled, exact in the 16-bit type."""
    n = rows * C
    v = torch.cat((torch.linspace(-9, 9, n - len(SPECIAL)), torch.tensor(SPECIAL)))
    return _h16(v[torch.randperm(n, generator=g)].view(rows, C))


# ------------------------------------------------------------------------------------------------------------ allowances
_ALLOW = {}


def _allowances():
    """(erf_ulps, exp2_ulps): twice the worst error of ATen's float32 erf / exp2 on the GPU against float64 over the arguments the
    activation tests feed erff and the fast exponential, in units of 2^-23 |result|."""
    if not _ALLOW:
        x = torch.cat((torch.linspace(-9, 9, 18 * 256 + 1), _h16(torch.linspace(-9, 9, 18 * 256 + 1)), torch.tensor(SPECIAL)))
        t = x * torch.tensor(E.SQRT1_2, dtype=F32)
        e32, e64 = torch.erf(t.to(DEV)).cpu().double(), torch.erf(t.double())
        nz = e64 != 0
        worst_erf = ((e32 - e64).abs()[nz] / (2 * U * e64.abs()[nz])).max().item()
        y = torch.cat((-x, -1.702 * x, -0.5 * x * x)) * torch.tensor(1.4426950408889634, dtype=F32)
        y = y[(y.abs() <= 126)]                                                     # results in the normal range
        p32, p64 = torch.exp2(y.to(DEV)).cpu().double(), torch.exp2(y.double())
        worst_exp2 = ((p32 - p64).abs() / (2 * U * p64)).max().item()
        _ALLOW.update(erf=2 * worst_erf, exp2=2 * worst_exp2, worst_erf=worst_erf, worst_exp2=worst_exp2)
    return _ALLOW["erf"], _ALLOW["exp2"]


def test_library_function_allowances():
    erf_ulps, exp2_ulps = _allowances()
    print(f"[allowances] erff: worst {_ALLOW['worst_erf']:.3f} -> allowance {erf_ulps:.3f}; exp2: worst {_ALLOW['worst_exp2']:.3f} -> allowance"
          f" {exp2_ulps:.3f} (units of 2^-23 |result|, ATen float32 on the GPU against float64)")
    assert 0 < erf_ulps < 16 and 0 < exp2_ulps < 16


# ------------------------------------------------------------------------------------------------------------ cast
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "colscale"])
@pytest.mark.parametrize("sdt,ddt", PAIRS, ids=lambda d: _dtname(d))
def test_cast(sdt, ddt, scaled):
    rows = 37
    for cols in (1, 3, 4, 70):
        g = _gen(cols, 1)
        x = (torch.randn(rows, cols, generator=g) * 3).to(sdt)
        cs = torch.randn(cols, generator=g) if scaled else None
        src, dst = Buf(rows, cols, sdt, x, shift=3), Buf(rows, cols, ddt, shift=2)
        ops.cast(src.v, dst.v, None if cs is None else cs.to(DEV))
        want = (x.float() * cs if scaled else x.float()).to(ddt)
        assert torch.equal(dst.cpu(), want), cols
        src.cpu()
    print(f"[cast {_dtname(sdt)}->{_dtname(ddt)} {'colscale' if scaled else 'plain'}] equal to the float32 value rounded once")


def test_cast_second_pass():
    rows, cols = 1100, 4096
    assert rows * cols // 4 > 4096 * 256
    x = torch.randn(rows, cols, generator=_gen(2))
    dst = Buf(rows, cols, torch.bfloat16)
    ops.cast(x.to(DEV), dst.v)
    assert torch.equal(dst.cpu(), x.to(torch.bfloat16))
    print("[cast 1100x4096 f32->h16] equal (second pass of the grid-stride loop)")


# ------------------------------------------------------------------------------------------------------------ split3
@pytest.mark.parametrize("source", ["plain", "transposed", "offset1"])
@pytest.mark.parametrize("K", [1, 63, 64, 100, 101])
def test_split3_bf16x3(K, source):
    rows, Kp = 5, (K + 63) // 64 * 64
    x = torch.randn(rows, K, generator=_gen(K, 3)) * 3
    x[0, 0] = 1.5                                                                   # lo exactly 0
    if source == "transposed":
        xs = x.t().contiguous().to(DEV).t()                                        # stride_c != 1
    elif source == "offset1":
        flat = torch.full((rows * K + 1,), float("nan"), device=DEV)              # starts one float past a 16-byte boundary
        flat[1:] = x.reshape(-1).to(DEV)
        xs = flat[1:].view(rows, K)
    else:
        xs = x.to(DEV)
    for pattern in (0, 1):
        dst = Buf(rows, 3 * Kp, torch.bfloat16, ld=3 * Kp + 8)
        L.check(L.load().vfm_split3(L.ptr(xs), xs.stride(0), xs.stride(1), L.ptr(dst.v), dst.ld, rows, K, pattern, L.stream()), "vfm_split3")
        got, want = dst.cpu(), E.split3_ref(x, pattern, torch.bfloat16)
        assert torch.equal(got, want), (K, source, pattern)
        assert (got.view(rows, 3, Kp)[:, :, K:] == 0).all()
    print(f"[split3 K={K} {source}] equal, pad columns zero")


# ------------------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("sdt,ddt", PAIRS, ids=lambda d: _dtname(d))
@pytest.mark.parametrize("rows,cols,pad_rows", [(1, 1, 1), (37, 70, 64), (130, 70, 192), (60, 70, 192)])
def test_transpose(rows, cols, pad_rows, sdt, ddt):
    """(60, 70, 192): the row tiles 64..127 and 128..191 lie wholly in the padding and must still be zero-filled."""
    x = torch.randn(rows, cols, generator=_gen(rows, cols)).to(sdt)
    src, dst = Buf(rows, cols, sdt, x, shift=3), Buf(cols, pad_rows, ddt)
    ops.transpose(src.v, dst.v, pad_rows)
    got = dst.cpu()
    assert torch.equal(got, E.transpose_ref(x, pad_rows, ddt))
    assert (got[:, rows:] == 0).all()
    print(f"[transpose {rows}x{cols} pad {pad_rows} {_dtname(sdt)}->{_dtname(ddt)}] equal")


# ------------------------------------------------------------------------------------------------------------ strided copy
@pytest.mark.parametrize("sdt,ddt", PAIRS, ids=lambda d: _dtname(d))
def test_strided_copy(sdt, ddt):
    g = _gen(5)
    x = torch.randn(3, 4, 5, 6, generator=g).to(sdt)
    v = x.permute(2, 0, 3, 1)                                                     # [5, 3, 6, 4]
    dst = Buf(1, v.numel(), ddt)
    cst = list(torch.empty(v.shape, device="meta").stride())
    ops.strided_copy(x.to(DEV), dst.v, list(v.shape), list(v.stride()), cst)
    assert torch.equal(dst.cpu().view(v.shape), v.float().to(ddt))
    # broadcast source (zero strides) into a strided destination
    b = torch.randn(4, 6, generator=g).to(sdt)
    e = b.view(1, 4, 1, 6).expand(3, 4, 5, 6)
    dst = Buf(1, e.numel(), ddt)
    ops.strided_copy(b.to(DEV), dst.v, list(e.shape), list(e.stride()), list(torch.empty(e.shape, device="meta").stride()))
    assert torch.equal(dst.cpu().view(e.shape), e.float().to(ddt))
    # accumulate: RNE(float(dst) + v)
    base = torch.randn(v.shape, generator=g).to(ddt)
    dst = Buf(1, v.numel(), ddt, base.reshape(-1))
    ops.strided_copy(x.to(DEV), dst.v, list(v.shape), list(v.stride()), cst, accumulate=True)
    assert torch.equal(dst.cpu().view(v.shape), (base.float() + v.float()).to(ddt))
    print(f"[strided_copy {_dtname(sdt)}->{_dtname(ddt)}] permutation, broadcast and accumulate equal")


# ------------------------------------------------------------------------------------------------------------ LoRA re-pack
@pytest.mark.parametrize("dt", [F32, torch.bfloat16], ids=_dtname)
def test_lora_pack(dt):
    """One table, three sites; r (K + N) = 67200 > 256 * 256 at the middle site: the stride loop's second pass.  The first site has no
    wt.  Whole buffers are compared, so everything outside the four sub-blocks must still hold the sentinel."""
    sites, refs = [], []
    for i, (r, K, N, Kw) in enumerate([(4, 24, 40, 64), (16, 2100, 2100, 2112), (1, 8, 8, 0)]):
        g = _gen(r, K, N)
        A, B = torch.randn(r, K, generator=g), torch.randn(N, r, generator=g)
        s = lambda *sh: torch.full(sh, SENT, dtype=dt)  # noqa: E731
        a, at, w, wt = s(r + 2, K + 8), s(K + 3, r + 8), s(N + 1, Kw + r + 8), (None if i == 0 else s(Kw + r + 2, N + 8))
        refs.append(E.lora_pack_ref(A, B, a, at, w, wt, Kw))
        dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
        sites.append((A.to(DEV), B.to(DEV), dev(a), dev(at), dev(w), dev(wt), r, K, N, Kw))
    assert max(s_[6] * (s_[7] + s_[8]) for s_ in sites) > 256 * 256
    ops.LoraPackTable(sites, sites[0][2]).run()
    for site, ref in zip(sites, refs):
        for nm, got, want in zip(("a", "at", "w", "wt"), site[2:6], ref):
            assert (got is None and want is None) or torch.equal(got.cpu(), want), (site[6:], nm)
    print(f"[lora_pack {_dtname(dt)}] three sites equal, everything else untouched")


# ------------------------------------------------------------------------------------------------------------ axpby
@pytest.mark.parametrize("n", [1, 999, 2 ** 20 + 3])
def test_axpby(n):
    g = _gen(n, 7)
    x, y0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a, b = 1.7, -0.6
    y = Buf(1, n, F32)                                                             # NaN: b == 0 must not read it
    ops.axpby(x.to(DEV), a, y.v.view(-1), 0.0)
    assert torch.equal(y.cpu().view(-1), x * torch.tensor(a, dtype=F32))
    y = Buf(1, n, F32, y0)
    ops.axpby(x.to(DEV), a, y.v.view(-1), b)
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    ref = a32 * x.double() + b32 * y0.double()
    _within(f"axpby n={n}", y.cpu().view(-1), ref, 2 * U * (1 + 2 * U) * ((a32 * x.double()).abs() + (b32 * y0.double()).abs()))


# ------------------------------------------------------------------------------------------------------------ sums
def _sum_bound(name, depth, terms, abs_sum):
    """gamma(n) sum|x|, n = min(additions one term passes through, number of terms); callers add U |result| per further rounding."""
    n = min(depth, max(terms, 1))
    bound = E.gamma(n) * abs_sum
    assert 0.5 > 4 * bound.max().item(), (name, bound.max().item())                 # one dropped or doubled term (>= 0.5) cannot hide
    return bound


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("dt", [F32, torch.bfloat16], ids=_dtname)
@pytest.mark.parametrize("rows,cols", [(5, 3), (300, 12), (700, 19), (2100, 70)])
def test_colsum(rows, cols, dt, accumulate):
    g = _gen(rows, cols)
    x = _signed_mag((rows, cols), g)
    out0 = _signed_mag((cols,), g)
    for shift in (0, 3):                                                            # plain ld > cols, and a column slice
        src = Buf(rows, cols, dt, x, shift=shift)
        out = Buf(1, cols, F32, out0 if accumulate else None)
        ops.colsum(src.v, out.v.view(-1), accumulate=accumulate)
        s = x.double().sum(0)
        ref = s + out0.double() if accumulate else s
        bound = _sum_bound("colsum", E.colsum_depth(rows, cols), rows, x.double().abs().sum(0)) + (U * ref.abs() if accumulate else 0)
        _within(f"colsum {rows}x{cols} {_dtname(dt)} {'accumulate' if accumulate else 'store'} shift={shift}", out.cpu().view(-1), ref, bound)
        src.cpu()


@pytest.mark.parametrize("keep_mode", ["random", "ones", "zeros"])
@pytest.mark.parametrize("rows,C", [(1, 5), (100, 70), (2100, 130)])
def test_mask_token(rows, C, keep_mode):
    g = _gen(rows, C)
    x, tok, dout = torch.randn(rows, C, generator=g), torch.randn(C, generator=g), _signed_mag((rows, C), g)
    keep = {"random": torch.rand(rows, generator=g) > 0.4, "ones": torch.ones(rows, dtype=torch.bool), "zeros": torch.zeros(rows, dtype=torch.bool)}[keep_mode]
    k8 = keep.to(torch.uint8).to(DEV)
    out = Buf(1, rows * C, F32)
    ops.mask_token_fwd(x.to(DEV), k8, tok.to(DEV), out.v.view(rows, C))
    assert torch.equal(out.cpu().view(rows, C), torch.where(keep[:, None], x, tok[None]))
    dx, dtok = Buf(1, rows * C, F32), Buf(1, C, F32)
    ops.mask_token_bwd(dout.to(DEV), k8, dx.v.view(rows, C), dtok.v.view(-1))
    assert torch.equal(dx.cpu().view(rows, C), torch.where(keep[:, None], dout, torch.zeros(())))
    masked = torch.where(keep[:, None], torch.zeros((), dtype=torch.float64), dout.double())
    ref = masked.sum(0)
    bound = _sum_bound("mask_token", E.mask_token_depth(rows), int((~keep).sum()), masked.abs().sum(0))
    got = dtok.cpu().view(-1)
    _within(f"mask_token_bwd dtoken rows={rows} C={C} keep={keep_mode}", got, ref, bound)
    if keep_mode == "ones":
        assert (got == 0).all()
    if keep_mode == "zeros":
        assert (dx.cpu() == 0).all()


@pytest.mark.parametrize("n", [0, 1, 63, 1024, 1025, 5000])
def test_reduce_sum_and_ce_finish(n):
    lib = L.load()
    scale = 0.37
    s32 = float(np.float32(scale))
    x = _signed_mag((max(n, 1),), _gen(n, 11))
    xd = x.to(DEV)
    ref = x[:n].double().sum() * s32
    bound = _sum_bound("reduce_sum", E.reduce_depth(n), n, x[:n].double().abs().sum() * abs(s32)) + U * ref.abs()   # + the scale
    out = Buf(1, 1, F32)
    L.check(lib.vfm_reduce_sum(L.ptr(xd), n, scale, L.ptr(out.v), L.stream()), "vfm_reduce_sum")
    loss_rs = out.cpu().view(())
    _within(f"reduce_sum n={n}", loss_rs, ref, bound)
    eps = 1e-6
    for hits, valid in ((0, 0), (7, 9), (2 ** 24 + 1, 2 ** 24 + 3)):
        counts = torch.tensor([hits, valid], dtype=torch.int32, device=DEV)
        res = Buf(1, 2, F32)
        L.check(lib.vfm_ce_finish(L.ptr(xd), n, scale, L.ptr(counts), eps, L.ptr(res.v), L.ptr(res.v[:, 1:]), L.stream()), "vfm_ce_finish")
        loss, acc = res.cpu().view(-1)
        assert _same_bits(loss, loss_rs), "loss: the value vfm_reduce_sum gives"
        acc_ref = torch.tensor(float(np.float32(hits)) * (100.0 / (float(np.float32(valid)) + float(np.float32(eps)))), dtype=torch.float64)
        _within(f"ce_finish n={n} counts=({hits},{valid}) acc", acc, acc_ref, 3 * U * acc_ref.abs())
        assert counts.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------ dropout mask
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_mask(p):
    """Element for element against dropout_mask_ref: keep iff u >= float32(p) (not >), value float32(1) / (1 - float32(p)) rounded to
    the output type, element i a function of (seed, offset + i) alone - also past the first pass of the grid-stride loop (n > 4096 *
    256), for a 64-bit offset, and across two calls."""
    n, seed = 2 ** 20 + 8 * 37, E.DROPOUT_TIE_SEED
    assert n % 8 == 0 and n > 4096 * 256
    for offset in (0, 77, 2 ** 33 + 5):
        ref32 = E.dropout_mask_ref(n + 3, p, seed, offset, F32)
        got = {}
        for form, dt, cnt, shift in (("f32", F32, n, 0), ("h16 aligned", torch.bfloat16, n, 0), ("h16 shifted", torch.bfloat16, n, 1),
                                     ("h16 n % 8 != 0", torch.bfloat16, n + 3, 0)):
            out = Buf(1, cnt, dt, shift=shift)
            ops.dropout_mask(out.v.view(-1), p, seed, offset)
            got[form] = out.cpu().view(-1)
            assert torch.equal(got[form], ref32[:cnt].to(dt)), (p, offset, form)
        assert _same_bits(got["h16 aligned"], got["h16 shifted"]) and _same_bits(got["h16 aligned"], got["h16 n % 8 != 0"][:n])
        if p == 0.0:
            assert (got["f32"] == 1.0).all()
    # u == float32(p) exactly (counters found by search with the restatement; test_elementwise_cpu.py pins them): kept, since the compare
    # is >=.  The element sits at index 5 of a 16-element call, in the float32, the x8 and the shifted scalar form.
    for tie in E.DROPOUT_TIES.get(p, ()):
        ref = E.dropout_mask_ref(16, p, E.DROPOUT_TIE_SEED, tie - 5, F32)
        assert ref[5] > 0
        for dt, shift in ((F32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1)):
            out = Buf(1, 16, dt, shift=shift)
            ops.dropout_mask(out.v.view(-1), p, E.DROPOUT_TIE_SEED, tie - 5)
            assert torch.equal(out.cpu().view(-1), ref.to(dt)), (p, tie, dt, shift)
    # the offset contract across two calls, on the GPU alone
    a = torch.empty(4096, dtype=F32, device=DEV)
    b = torch.empty(4096 - 77, dtype=F32, device=DEV)
    ops.dropout_mask(a, p, seed, 0)
    ops.dropout_mask(b, p, seed, 77)
    assert torch.equal(a[77:], b)
    print(f"[dropout_mask p={p}] equal to the restatement in all four forms at offsets 0, 77, 2^33+5")


# ------------------------------------------------------------------------------------------------------------ mul_mask
@pytest.mark.parametrize("sdt,mdt,ddt", [(torch.bfloat16, torch.bfloat16, torch.bfloat16), (F32, F32, F32), (torch.bfloat16, F32, torch.bfloat16)], ids=lambda d: _dtname(d))
@pytest.mark.parametrize("cols", [8, 24, 20])
def test_mul_mask(cols, sdt, mdt, ddt):
    rows, rpg = 37, 16                                                             # three groups, the last one of 5 rows
    g = _gen(cols, 13)
    x = torch.randn(rows, cols, generator=g).to(sdt)
    m = ((torch.rand(3, cols, generator=g) > 0.3).float() * 1.25).to(mdt)
    want = (x.float() * m.float().repeat_interleave(rpg, 0)[:rows]).to(ddt)
    res = []
    for shift in (0, 1):                                                           # aligned (x8 when cols % 8 == 0), then the scalar kernel
        src, msk, dst = Buf(rows, cols, sdt, x, shift=shift), Buf(3, cols, mdt, m, shift=shift), Buf(rows, cols, ddt, shift=shift)
        ops.mul_mask(src.v, msk.v, dst.v, rows_per_group=rpg)
        res.append(dst.cpu())
        assert torch.equal(res[-1], want), (cols, shift)
        src.cpu(), msk.cpu()
    assert _same_bits(res[0], res[1])
    print(f"[mul_mask cols={cols} {_dtname(sdt)}*{_dtname(mdt)}->{_dtname(ddt)}] equal, aligned and shifted")


# ------------------------------------------------------------------------------------------------------------ formula entries
def _chain(name, run, forms, refs, bounds):
    """run(form) -> tuple of CPU outputs.  forms: "x8" (all 16-bit aligned; left out when the shape has no x8 form), and always the scalar
    kernel as "s16" (all 16-bit, shifted), "s32" (float32 store from 16-bit inputs), "f32" (all float32).  (a) x8 == s16 bit for bit,
    (b) s16 == RNE(s32) and s32 == f32 bit for bit, (c) f32 within `bounds` of `refs`."""
    res = {f: run(f) for f in forms}
    for i, (ref, bound) in enumerate(zip(refs, bounds)):
        if "x8" in res:
            assert _same_bits(res["x8"][i], res["s16"][i]), (name, i, "(a) x8 form != scalar form")
        assert _same_bits(res["s16"][i], res["s32"][i].to(torch.bfloat16)), (name, i, "(b) 16-bit store != RNE of the float32 store")
        assert _same_bits(res["s32"][i], res["f32"][i]), (name, i, "(b) float32 store from 16-bit inputs != all-float32")
        assert torch.isfinite(res["f32"][i]).all(), (name, i, "not finite")
        _within(f"{name} out{i} float32 scalar form", res["f32"][i], ref, bound)
    return res


GLU_C = [8, 48, 5]
GLU_ROWS = 37


def _glu_inputs(C, gate_is_second, seed):
    """h = [a | g] with the pre-activation in the gated half, the other half and dout N(0, 1), all exact in the 16-bit type."""
    g_ = _gen(C, seed)
    pre, other = _preact(GLU_ROWS, C, g_), _h16(torch.randn(GLU_ROWS, C, generator=g_))
    d = _h16(torch.randn(GLU_ROWS, C, generator=g_))
    a, g = (other, pre) if gate_is_second else (pre, other)
    return a, g, d, torch.cat((a, g), dim=1)


def _glu_layout(form):
    """(input dtype, output dtype, shift) of a form."""
    return {"x8": (torch.bfloat16, torch.bfloat16, 0), "s16": (torch.bfloat16, torch.bfloat16, 1), "s32": (torch.bfloat16, F32, 0),
            "f32": (F32, F32, 0), "x8_32": (torch.bfloat16, F32, 0)}[form]


@pytest.mark.parametrize("C", GLU_C)
def test_geglu(C):
    """out = a gelu(g); da = d gelu(g), dg = d a gelu'(g).  At |g| >= 20 erff is exactly +-1 and the pdf underflows: gelu(g) is
    exactly g or -0, gelu'(g) exactly 1 or -0, so the outputs are the plain products or zero."""
    erf_ulps, exp2_ulps = _allowances()
    a, g, d, h = _glu_inputs(C, True, 1)
    forms = (["x8"] if C % 8 == 0 else []) + ["s16", "s32", "f32"]

    def fwd(form):
        idt, odt, sh = _glu_layout(form)
        hb, ob = Buf(GLU_ROWS, 2 * C, idt, h, shift=sh), Buf(GLU_ROWS, C, odt, shift=sh)
        ops.geglu_fwd(hb.v, ob.v)
        hb.cpu()
        return (ob.cpu(),)

    def bwd(form):
        idt, odt, sh = _glu_layout(form)
        hb, db, ob = Buf(GLU_ROWS, 2 * C, idt, h, shift=sh), Buf(GLU_ROWS, C, idt, d, shift=sh), Buf(GLU_ROWS, 2 * C, odt, shift=sh)
        ops.geglu_bwd(hb.v, db.v, ob.v)
        o = ob.cpu()
        return o[:, :C], o[:, C:]

    a64, g64, d64 = a.double(), g.double(), d.double()
    rf = _chain(f"geglu_fwd C={C}", fwd, forms, (E.geglu_fwd_ref(a64, g64),), (E.geglu_fwd_bound(a64, g64, erf_ulps),))
    rb = _chain(f"geglu_bwd C={C}", bwd, forms, E.geglu_bwd_ref(a64, g64, d64), E.geglu_bwd_bound(a64, g64, d64, erf_ulps, exp2_ulps))
    hi, lo = g >= 20, g <= -20
    assert hi.any() and lo.any()
    for got in (rf["f32"][0], rb["f32"][0], rb["f32"][1]):
        assert (got[lo] == 0).all(), "g <= -20: exactly 0 / -0"
    assert torch.equal(rf["f32"][0][hi], (a * g)[hi]) and torch.equal(rb["f32"][0][hi], (d * g)[hi]) and torch.equal(rb["f32"][1][hi], (d * a)[hi])


@pytest.mark.parametrize("C", GLU_C)
def test_swiglu_fwd(C):
    """out = a / (1 + exp(-a)) g.  x8<true> (16 -> 16) and x8<false> (16 -> 32) against the scalar kernel; at a = -60 the result is
    -60 e^-60 g (about 5e-25 g, not 0), at a = +60 it is a g: finite either way, held by the bound."""
    _, exp2_ulps = _allowances()
    a, g, _, h = _glu_inputs(C, False, 2)

    def fwd(form):
        idt, odt, sh = _glu_layout(form)
        if form == "s32":
            sh = 1                                                                  # aligned 16 -> 32 would be x8<false>
        hb, ob = Buf(GLU_ROWS, 2 * C, idt, h, shift=sh), Buf(GLU_ROWS, C, odt, shift=sh)
        ops.swiglu_fwd(hb.v, ob.v, C)
        hb.cpu()
        return (ob.cpu(),)

    a64, g64 = a.double(), g.double()
    res = _chain(f"swiglu_fwd C={C}", fwd, (["x8"] if C % 8 == 0 else []) + ["s16", "s32", "f32"], (E.swiglu_fwd_ref(a64, g64),),
                 (E.swiglu_fwd_bound(a64, g64, exp2_ulps),))
    if C % 8 == 0:
        assert _same_bits(fwd("x8_32")[0], res["s32"][0]), "x8<false> != scalar form"


@pytest.mark.parametrize("C", GLU_C)
def test_swiglu_bwd(C):
    """sg = 1 / (1 + exp(-a)); da = d g sg (1 + a (1 - sg)), dg = d a sg.  x8<true> takes 16-bit dout, x8<false> float32 dout (dh
    16-bit in both); the scalar kernel runs all-float32, 16-bit h with float32 dh, and shifted."""
    _, exp2_ulps = _allowances()
    a, g, d, h = _glu_inputs(C, False, 3)

    def bwd(form, do_dt=None):
        idt, odt, sh = _glu_layout(form)
        hb, db, ob = Buf(GLU_ROWS, 2 * C, idt, h, shift=sh), Buf(GLU_ROWS, C, do_dt or idt, d, shift=sh), Buf(GLU_ROWS, 2 * C, odt, shift=sh)
        ops.swiglu_bwd(hb.v, db.v, ob.v, C)
        hb.cpu(), db.cpu()
        o = ob.cpu()
        return o[:, :C], o[:, C:]

    a64, g64, d64 = a.double(), g.double(), d.double()
    res = _chain(f"swiglu_bwd C={C}", bwd, (["x8"] if C % 8 == 0 else []) + ["s16", "s32", "f32"], E.swiglu_bwd_ref(a64, g64, d64),
                 E.swiglu_bwd_bound(a64, g64, d64, exp2_ulps))
    if C % 8 == 0:
        mixed = bwd("x8", do_dt=F32)                                                # x8<false>: float32 dout, 16-bit dh
        assert _same_bits(mixed[0], res["s16"][0]) and _same_bits(mixed[1], res["s16"][1]), "x8<false> != scalar form"


@pytest.mark.parametrize("cols", [24, 7])
@pytest.mark.parametrize("act", [E.ACT_NONE, E.ACT_GELU, E.ACT_RELU, E.ACT_QGELU], ids=["none", "gelu", "relu", "qgelu"])
def test_act_grad_mul(act, cols):
    """out = dy act'(pre), ld = 40.  NONE and RELU multiply by exactly 1 or 0: bound 0.  At pre >= 20 every act' is exactly 1 (erff = 1
    and the pdf underflows; 1 + exp(-34) rounds to 1), at pre <= -20 gelu' and relu' are exactly (-)0; qgelu' is exactly 0 only where
    exp overflows (pre = -60), elsewhere about -34 e^-34: finite, held by the bound."""
    assert (L.ACT_NONE, L.ACT_GELU, L.ACT_RELU, L.ACT_QGELU) == (E.ACT_NONE, E.ACT_GELU, E.ACT_RELU, E.ACT_QGELU)
    erf_ulps, exp2_ulps = _allowances()
    rows, ld = 37, 40
    g_ = _gen(cols, act, 5)
    pre, dy = _preact(rows, cols, g_), _h16(torch.randn(rows, cols, generator=g_))

    def run(form, dts=None):
        idt, odt, sh = _glu_layout(form)
        ddt, pdt, odt = dts or (idt, idt, odt)
        db, pb, ob = Buf(rows, cols, ddt, dy, ld=ld, shift=sh), Buf(rows, cols, pdt, pre, ld=ld, shift=sh), Buf(rows, cols, odt, ld=ld, shift=sh)
        ops.act_grad_mul(db.v, pb.v, ob.v, act)
        db.cpu(), pb.cpu()
        return (ob.cpu(),)

    p64, d64 = pre.double(), dy.double()
    res = _chain(f"act_grad_mul act={act} cols={cols}", run, (["x8"] if cols % 8 == 0 else []) + ["s16", "s32", "f32"],
                 (d64 * E.act_grad(p64, act),), (E.act_grad_mul_bound(d64, p64, act, erf_ulps, exp2_ulps),))
    f32 = res["f32"][0]
    assert _same_bits(run("f32", (torch.bfloat16, F32, F32))[0], f32), "dy 16-bit, pre / out float32"
    assert _same_bits(run("f32", (F32, torch.bfloat16, torch.bfloat16))[0], res["s16"][0]), "dy float32, pre / out 16-bit"
    hi, lo = pre >= 20, pre <= -20
    assert torch.equal(f32[hi], dy[hi])
    zero = lo if act in (E.ACT_GELU, E.ACT_RELU) else (pre == -60 if act == E.ACT_QGELU else torch.zeros_like(lo))
    assert (f32[zero] == 0).all()
    if act == E.ACT_NONE:
        assert torch.equal(f32, dy)


@pytest.mark.parametrize("np_,H,d", [(16, 4, 64), (5, 3, 8), (7, 2, 6)])
def test_rope(np_, H, d):
    """rows = 3 np + 2 (row % np wraps and ends mid-period), ncols = H d inside ld = 2 H d + 8 with the sentinel right of ncols,
    independent random cos and sin per column (which table column each output reads is pinned).  Forward, inverse, and inverse(forward)
    against R^T R x in float64 - not x for generic tables.  d = 6: the 16-bit tensor takes the scalar kernel."""
    g = _gen(np_, H, d)
    rows, nc = 3 * np_ + 2, H * d
    ld = 2 * nc + 8
    x = _h16(torch.randn(rows, nc, generator=g))
    cos, sin = torch.randn(np_, d, generator=g), torch.randn(np_, d, generator=g)
    cd, sd = cos.to(DEV), sin.to(DEV)
    c64, s64 = cos.double(), sin.double()

    def run(dt, shift, data, passes):
        b = Buf(rows, nc, dt, data, ld=ld, shift=shift)
        for inv in passes:
            ops.rope(b.v, rows, np_, nc, d, cd, sd, inverse=inv)
        return b.cpu()

    for inv in (False, True):
        name = f"rope np={np_} H={H} d={d} {'inverse' if inv else 'forward'}"
        f32, a16, s16 = run(F32, 0, x, [inv]), run(torch.bfloat16, 0, x, [inv]), run(torch.bfloat16, 1, x, [inv])
        assert _same_bits(a16, s16), (name, "(a) x8 form != scalar form")
        assert _same_bits(s16, f32.to(torch.bfloat16)), (name, "(b) 16-bit store != RNE of the float32 store")
        _within(name + " float32 scalar form", f32, E.rope_ref(x.double(), c64, s64, np_, nc, d, inv), E.rope_bound(x.double(), c64, s64, np_, nc, d, inv))
    # inverse(forward(x))
    name = f"rope np={np_} H={H} d={d} inverse(forward)"
    y64 = E.rope_ref(x.double(), c64, s64, np_, nc, d)
    b1 = E.rope_bound(x.double(), c64, s64, np_, nc, d)
    ref = E.rope_ref(y64, c64, s64, np_, nc, d, inverse=True)
    bound = E.rope_abs(b1, c64, s64, np_, nc, d, inverse=True) + E.rope_bound(y64.abs() + b1, c64, s64, np_, nc, d, inverse=True)
    _within(name + " float32", run(F32, 0, x, [False, True]), ref, bound)
    a16, s16 = run(torch.bfloat16, 0, x, [False, True]), run(torch.bfloat16, 1, x, [False, True])
    assert _same_bits(a16, s16), (name, "(a)")
    fwd16 = run(torch.bfloat16, 1, x, [False])
    assert _same_bits(s16, run(F32, 0, fwd16.float(), [True]).to(torch.bfloat16)), (name, "(b)")
