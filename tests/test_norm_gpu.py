"""Every entry of csrc/norm.hip (the one-launch GroupNorm tile pair aside: tests/test_segformer_gpu.py) against the float64
restatements of tests/norm_helpers.py (pinned by tests/test_norm_cpu.py), at the smallest shapes that reach every kernel form of the
dispatchers.  Inputs and outputs live in Buf views (tests/test_elementwise_gpu.py): NaN-filled inside a field of sentinels that must
survive bit for bit; every produced element is compared through tests.helpers._within with a per-element bound, never a global max
ratio.  A 16-bit dy holds values exact in the 16-bit type and the reference is computed from those values; a 16-bit output's bound is
the float32 bound plus one rounding at |ref| + bound.  The 16-bit type is spelled torch.bfloat16 so that the fp16 pass
(tests/test_fp16_twin_gpu.py) re-types it; the split-image test carries bf16x3 in its name and stays out of that pass.

Measure and allowance: tests/norm_helpers.py states the measure.  The allowance is not fixed in advance: test_aten_float32_allowances
runs ATen's float32 F.layer_norm / F.group_norm / F.batch_norm and their autograd on the GPU over the inputs of these cases and takes
the worst error per family (ln / gn / bn), quantity (y, dx, sums) and input class (centred, offset) against the same float64
restatement; the allowance is 4 x that (the kernels add in another order), never below 16 x 2^-24, and never above the project's
present bound (N.CEILING): where 4 x ATen exceeds it the bound itself is the allowance (on the MI355X: LayerNorm y, offset class,
4 x 2.61e-6 against 1e-5), and ATen's own error must stay below it.  Statistics (mean / rstd / mean_var) use the allowance of y, the quantity they feed.  Sets of one element
are left out of the measurement only: BatchNorm at one row has no ATen counterpart (F.batch_norm refuses it in training mode), and
LayerNorm at C = 1 is exact (y = b, dx = 0), which the tests assert.  The inputs of the ReLU cases keep |z| >= 1e-4 (relu' jumps at 0).
BatchNorm is checked link by link, as its ABI splits it: `sums` against float64 in the sum measure; vfm_bn_finalize against float64 of
the float32 sums it was given (two roundings), its mean also against the truth; then y, sums_dy and dx - computed by the kernels from
their own mean_var - against the truth.  The variance is not asserted against the truth on its own: the ABI carries sum x^2 in
float32, so var inherits the bound of `sums` times E[x^2] / var (at one row the true variance is 0 and the float32 sum cannot say
so); what that costs is asserted where it matters, in y and dx of the offset class, and the relative error of var is printed.

Which case reaches which kernel instantiation (derived from the conditions of vfm_layernorm_fwd / ln_bwd_impl as written; _fwd_form /
_bwd_form restate them and every case asserts that its operands select the form its id names; * = no test against a reference before):
  k_ln_fwd<*, 4> *            test_layernorm_fwd s<4>: C = 1, 19, 70; C = 256 with x one element past an aligned address
  k_ln_fwd<*, 16> *           s<16>: C = 257; C = 768 (C / 256 = 3 is no vector width); C = 1024 with ld_x = 1026
  k_ln_fwd<*, 32> *           s<32>: C = 1025 (pitch 1033: neither the 16- nor the 8-byte form); C = 2048 with x shifted
  k_ln_fwd<*, 48>             s<48>: C = 3071; C = 3072 with x shifted
  k_ln_fwd_v4<*, 1|2|4|5|8>   v4<NV>: C = 256, 512 *, 1024, 1280 *, 2048 *, y a column slice of a buffer 64 wider
  k_ln_fwd_v4<h16, NV, DROP>  test_layernorm_dropout_fwd, the five widths
  k_ln_fwd_v4<f32, NV, SPLIT> test_layernorm_fwd_split3_bf16x3, the five widths, with and without the float32 copy
  k_ln_fwd_v4t<*, 11>         v4t<11>: C = 1028 (no partial piece), 1366 in pitch 1368, 2815 in pitch 2816 (partial piece of 3), 1536, 2816
  k_ln_fwd_v2<*, 24>          v2<24>: C = 1366 at pitch 1366, 2818, 3072
  k_ln_bwd_v4<*, 1|2|4|5>     test_layernorm_bwd v4<NV>: C = 256, 512 *, 1024, 1280 *; test_layernorm_bwd_scaled (t_out form) at the same widths
  k_ln_bwd_v4t<*, 11>         v4t<11>: C = 2048 * (the backward v4 list stops at 5), 1028, 1366 in 1368, 2815 in 2816, 2816
  k_ln_bwd_v2<*, 24>          v2<24>: C = 1366 at pitch 1366, 2818, 3072
  k_ln_bwd<*, 4|16|48, false> * s<4>: C = 1, 19, 70, 256 shifted; s<16>: C = 257, 768, 1024 shifted; s<48>: C = 1025, 3071 (the backward has no <32>)
  k_ln_bwd<*, 4|16, true>     test_layernorm_bwd_dw_db s<4,w>: C = 1, 70, 256; s<16,w>: C = 257, 1024; rows 1, 5, 513 (127 idle blocks end at
  + k_ln_bwd_fin              row 512), 1100 (second pass of the grid-stride loop); 16-bit dy *
  k_chan_moments<0, float>    test_groupnorm_general (forward), test_batchnorm / test_batchnorm_two_shards (vfm_bn_moments)
  k_chan_moments<1, *>        test_groupnorm_general (backward, per-group statistics), test_batchnorm* (vfm_bn_bwd_reduce, per-channel)
  k_gn_fin_fwd, k_gn_apply<*>, k_gn_fin_bwd, k_gn_bwd_apply<*>, k_chan_fin_wb      test_groupnorm_general
  k_bn_fin_sums, k_bn_finalize, k_bn_apply<*>, k_bn_bwd_apply<*>                   test_batchnorm, test_batchnorm_two_shards
  k_gn_tile_fwd / _bwd        tests/test_segformer_gpu.py; here only the refusal of VFM_ACT_QGELU and, printed beside the general
                              kernel for the offset class, the forward error at (1, 100, 128, 32)
GroupNorm shapes (B, P, C, G): (3, 1, 6, 3) one row, one partial strip, C / G = 2; (2, 65, 72, 8) two chunks (33 + 32 rows), C / G = 9, a
group across the strip boundary at channel 64; (2, 64, 64, 64) C / G = 1; (1, 63, 130, 1) one group over three strips; (1, 100, 128, 32)
the decoder geometry; (1, 4097, 32, 8) 64 chunks of 65 rows, the last of 2.  BatchNorm (rows, C): (1, 19), (2, 1), (65, 65), (300, 64),
(4097, 130).

Measured on the MI355X (profiles/norm_gpu.log): ATen float32 worst, centred / offset - ln y 1.9e-7 / 2.6e-6, dx 4.6e-7 / 4.6e-7, sums
1.5e-7 / 1.7e-6; gn y 2.1e-7 / 6.9e-7, dx 5.0e-7 / 1.4e-6, sums 1.7e-7 / 1.2e-6; bn y 3.2e-7 / 3.2e-6, dx 4.3e-7 / 4.8e-6, sums 1.0e-7 /
1.2e-7.  Float32 results of this library use at most 0.68 of their bound, except the one-pass moments of the general GroupNorm in the
offset class: 1.9e-6 in y at (2, 64, 64, 64), 2.75 x ATen, err / bound 0.905.  The file takes 8.4 s, its fp16 pass 5.5 s."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import norm_helpers as N  # noqa: E402
from tests.helpers import _rounded, _within  # noqa: E402
from tests.test_elementwise_gpu import Buf, _same_bits  # noqa: E402
from vfmseg_amd import lib as L, ops  # noqa: E402

DEV = "cuda"
F32 = torch.float32
U = N.U
LN_EPS = 1e-6
E_INVAL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = r"\(-1\)", r"\(-2\)", r"\(-3\)", r"\(-5\)"


def _dn(dt):
    return "f32" if dt == F32 else "h16"


def _dev(t):
    return t.float().to(DEV)


def _out_bound(ref, b1, dt):
    return b1 if dt == F32 else _rounded(ref, b1, L.half_dtype())


def _sum_measure(got, ref, abs_terms):
    return N.measure(got, ref, abs_terms - ref.abs())


def _nan_everywhere(buf):
    return bool(torch.isnan(buf.cpu().float()).all())


# ------------------------------------------------------------------------------------------------------------ references (cached)
BN_EPS = 1e-5


def _h(ddt):
    """Cache key of a dy type: None for float32 values, the 16-bit type for values exact in it."""
    return None if ddt in (None, F32) else ddt


@functools.lru_cache(maxsize=24)
def _ln_cached(rows, C, cls, h):
    x = N.ln_inputs(rows, C, cls)
    w, b = N.make_params(C, 1)
    dy = N.make_dy((rows, C), 2, h)
    return x, w, b, dy, N.ln_ref(x, w, b, LN_EPS, dy)


def _ln_case(rows, C, cls, ddt=None):
    return _ln_cached(rows, C, cls, _h(ddt))


@functools.lru_cache(maxsize=8)
def _gn_cached(shape, cls, eps, a, h):
    B, P, C, G = shape
    x = N.gn_inputs(B, P, C, G, cls)
    w, b = N.make_params(C, 3)
    if a == N.ACT_RELU:
        x = N.off_the_relu_kink(x, G, w, b, eps)
    dy = N.make_dy((B, P, C), 4, h)
    return x, w, b, dy, N.gn_ref(x, G, w, b, eps, a, dy)


def _gn_case(shape, cls, eps, a, ddt=None):
    return _gn_cached(shape, cls, eps, a, _h(ddt))


@functools.lru_cache(maxsize=8)
def _bn_cached(shape, cls, a, h, cut):
    rows, C = shape
    x = N.bn_inputs(rows, C, cls)
    w, b = N.make_params(C, 5)
    if a == N.ACT_RELU:
        x = N.off_the_relu_kink(x[None], C, w, b, BN_EPS)[0]
    dy = N.make_dy((rows, C), 6, h)
    xs, dys = ([x], [dy]) if cut is None else ([x[:cut], x[cut:]], [dy[:cut], dy[cut:]])
    return xs, w, b, dys, N.bn_ref(xs, w, b, BN_EPS, a, dys)


def _bn_case(shape, cls, a, ddt=None, cut=None):
    return _bn_cached(shape, cls, a, _h(ddt), cut)


# ------------------------------------------------------------------------------------------------------------ allowances
_ATEN, _ALLOW = {}, {}


def _note(fam, qty, cls, v):
    k = (fam, qty, cls)
    _ATEN[k] = max(_ATEN.get(k, 0.0), v)


def _act_torch(z, a):
    return {0: lambda t: t, 1: F.gelu, 2: F.relu, 3: lambda t: t * torch.sigmoid(1.702 * t)}[a](z)


def _measure_aten():
    """ATen's float32 kernels on the GPU over the inputs of this file's cases, in this file's measure."""
    for cls in N.CLASSES:
        shapes = [(r, C) for C in N.LN_WIDTHS for r in (1, 5)] + [(r, C) for C in N.LN_W_WIDTHS for r in N.LN_W_ROWS if r > 5]
        shapes = [s for s in shapes if s[1] > 1]        # a set of one element: y = b, xhat = 0 and dx = 0 exactly, asserted as such
        for rows, C in shapes:
            x, w, b, dy, r = _ln_case(rows, C, cls)
            xg, wg, bg = (_dev(t).requires_grad_(True) for t in (x, w, b))
            y = F.layer_norm(xg, (C,), wg, bg, LN_EPS)
            y.backward(_dev(dy))
            _note("ln", "y", cls, N.measure(y.detach().cpu(), r["y"], r["S_y"]))
            _note("ln", "dx", cls, N.measure(xg.grad.cpu(), r["dx"], r["S_dx"]))
            _note("ln", "sums", cls, max(_sum_measure(wg.grad.cpu(), r["dw"], r["abs_dw"]), _sum_measure(bg.grad.cpu(), r["db"], r["abs_db"])))
        for shape in N.GN_SHAPES:
            for eps in (1e-5, 1e-6):
                for a in N.ACTS:
                    x, w, b, dy, r = _gn_case(shape, cls, eps, a)
                    xg, wg, bg = (_dev(t).requires_grad_(True) for t in (x, w, b))
                    y = _act_torch(F.group_norm(xg.permute(0, 2, 1), shape[3], wg, bg, eps).permute(0, 2, 1), a)
                    y.backward(_dev(dy))
                    _note("gn", "y", cls, N.measure(y.detach().cpu(), r["y"], r["S_y"]))
                    _note("gn", "dx", cls, N.measure(xg.grad.cpu(), r["dx"], r["S_dx"]))
                    _note("gn", "sums", cls, max(_sum_measure(wg.grad.cpu(), r["dw"], r["abs_dw"]), _sum_measure(bg.grad.cpu(), r["db"], r["abs_db"])))
        for shape in N.BN_SHAPES:
            if shape[0] < 2:
                continue
            for a in N.ACTS:
                xs, w, b, dys, r = _bn_case(shape, cls, a)
                xg, wg, bg = (_dev(t).requires_grad_(True) for t in (xs[0], w, b))
                y = _act_torch(F.batch_norm(xg, None, None, wg, bg, True, 0.1, BN_EPS), a)
                y.backward(_dev(dys[0]))
                _note("bn", "y", cls, N.measure(y.detach().cpu(), r["y"][0], r["S_y"]))
                _note("bn", "dx", cls, N.measure(xg.grad.cpu(), r["dx"][0], r["S_dx"]))
                _note("bn", "sums", cls, max(_sum_measure(bg.grad.cpu(), r["sums_dy"][0], r["abs_sums_dy"][0]),
                                             _sum_measure(wg.grad.cpu(), r["sums_dy"][1], r["abs_sums_dy"][1])))
    for k, v in _ATEN.items():
        _ALLOW[k] = N.allowance(v, N.CEILING[k[0], k[1]])


def _allow(fam, qty, cls):
    if not _ALLOW:
        _measure_aten()
    return _ALLOW[fam, qty, cls]


def test_aten_float32_allowances():
    _allow("ln", "y", "centred")
    for (fam, qty, cls), v in sorted(_ATEN.items()):
        print(f"[norm allowance] {fam} {qty:4s} {cls:7s}: ATen float32 worst {v:.3e} -> allowance {_ALLOW[fam, qty, cls]:.3e} (ceiling {N.CEILING[fam, qty]:.0e})")
    for (fam, qty, cls), v in _ALLOW.items():
        assert N.FLOOR <= v <= N.CEILING[fam, qty], (fam, qty, cls, v)
        # ATen's own float32 error stays inside the project's bound on these inputs: above it, an input would be ill-conditioned
        assert _ATEN[fam, qty, cls] <= N.CEILING[fam, qty], (fam, qty, cls, _ATEN[fam, qty, cls])


class _Worst:
    """Worst err / bound of a case, kept apart for float32 results and for results stored in the 16-bit type (whose ratio is mostly
    the last rounding: half an ulp of the output against a bound of half an ulp plus the float32 allowance)."""

    def __init__(self):
        self.v = {"f32": 0.0, "h16": 0.0}

    def add(self, dt, *ratios):
        k = "f32" if dt == F32 else "h16"
        self.v[k] = max(self.v[k], *ratios)


def _report(case, worst, extra=""):
    if isinstance(worst, _Worst):
        print(f"[norm] {case}: worst err / bound {worst.v['f32']:.3f} (float32 results), {worst.v['h16']:.3f} (16-bit results){extra}")
    else:
        print(f"[norm] {case}: worst err / bound {worst:.3f}{extra}")


# ------------------------------------------------------------------------------------------------------------ LayerNorm forward
def _fwd_form(C, ldx, ldy, px, py):
    """The kernel vfm_layernorm_fwd selects, as its conditions are written (w and b are 16-byte aligned in every case)."""
    nv = C // 256
    if C % 256 == 0 and nv in (1, 2, 4, 5, 8) and ldx % 4 == 0 and ldy % 4 == 0 and px % 16 == 0 and py % 8 == 0:
        return f"v4<{nv}>"
    cp = (C + 3) // 4 * 4
    if 1024 < C <= 2816 and ldx % 4 == 0 and ldy % 4 == 0 and ldx >= cp and ldy >= cp and px % 16 == 0 and py % 16 == 0:
        return "v4t<11>"
    if C > 1024 and C % 2 == 0 and ldx % 2 == 0 and ldy % 2 == 0 and px % 8 == 0 and py % 8 == 0:
        return "v2<24>"
    pl = (C + 63) // 64
    return "s<4>" if pl <= 4 else ("s<16>" if pl <= 16 else ("s<32>" if pl <= 32 else "s<48>"))


LN_FWD = [("s<4>", 1, {}), ("s<4>", 19, {}), ("s<4>", 70, {}), ("s<4>", 256, dict(xs=1)),
          ("s<16>", 257, {}), ("s<16>", 768, {}), ("s<16>", 1024, dict(ldx=1026)),
          ("s<32>", 1025, {}), ("s<32>", 2048, dict(xs=1)), ("s<48>", 3071, {}), ("s<48>", 3072, dict(xs=1)),
          ("v4<1>", 256, dict(ldy=320)), ("v4<2>", 512, dict(ldy=576)), ("v4<4>", 1024, dict(ldy=1088)), ("v4<5>", 1280, dict(ldy=1344)),
          ("v4<8>", 2048, dict(ldy=2112)),
          ("v4t<11>", 1028, {}), ("v4t<11>", 1366, dict(ldx=1368, ldy=1368)), ("v4t<11>", 2815, dict(ldx=2816, ldy=2816)),
          ("v4t<11>", 1536, {}), ("v4t<11>", 2816, {}),
          ("v2<24>", 1366, dict(ldx=1366, ldy=1366)), ("v2<24>", 2818, {}), ("v2<24>", 3072, {})]


def _case_id(form, C, kw):
    return f"{form}-C{C}" + "".join(f"-{k}{v}" for k, v in kw.items())


def _check_ln_stats(name, st, r, allow):
    got = st.cpu()
    a = _within(f"{name} mean", got[:, 0], r["mean"], allow * r["S_x"])
    return max(a, _within(f"{name} rstd", got[:, 1], r["rstd"], allow * r["rstd"]))


@pytest.mark.parametrize("form,C,kw", LN_FWD, ids=[_case_id(*c) for c in LN_FWD])
def test_layernorm_fwd(form, C, kw):
    worst = _Worst()
    for rows in (1, 5):
        for cls in N.CLASSES:
            x, w, b, _, r = _ln_case(rows, C, cls)
            allow = _allow("ln", "y", cls)
            wd, bd = _dev(w), _dev(b)
            assert wd.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
            for ydt in (F32, torch.bfloat16):
                xb = Buf(rows, C, F32, x, ld=kw.get("ldx"), shift=kw.get("xs", 0))
                yb, st = Buf(rows, C, ydt, ld=kw.get("ldy")), Buf(rows, 2, F32, ld=2)
                assert _fwd_form(C, xb.ld, yb.ld, xb.v.data_ptr(), yb.v.data_ptr()) == form
                ops.layernorm_fwd(xb.v, wd, bd, LN_EPS, yb.v, st.v)
                name = f"ln fwd {form} C={C} rows={rows} {cls} {_dn(ydt)}"
                b1 = N.elem_bound(r["y"], r["S_y"], allow)
                worst.add(ydt, _within(name, yb.cpu(), r["y"], _out_bound(r["y"], b1, ydt)))
                worst.add(F32, _check_ln_stats(name, st, r, allow))
                xb.cpu()
                if C == 1 and ydt == F32:
                    assert torch.equal(yb.cpu().double(), b.expand(rows, 1))          # (x - mean) is exactly 0
    _report(f"ln fwd {_case_id(form, C, kw)}", worst)


def test_layernorm_fwd_refusals():
    rows, Cb = 5, 3080
    xb, yb, st = Buf(rows, Cb, F32, torch.ones(rows, Cb)), Buf(rows, Cb, F32), Buf(rows, 2, F32, ld=2)
    w = torch.ones(Cb, device=DEV)
    for C in (3073, 0):
        rc = L.load().vfm_layernorm_fwd(L.ptr(xb.v), xb.ld, L.ptr(w), L.ptr(w), LN_EPS, L.ptr(yb.v), L.dt_of(yb.v), yb.ld, L.ptr(st.v), rows, C,
                                        L.stream())
        assert rc == -2, (C, rc)
    assert _nan_everywhere(yb) and _nan_everywhere(st)
    print("[norm] ln fwd refusals: C = 3073 and C = 0 give VFM_E_SHAPE, outputs untouched")


V4_WIDTHS = [256, 512, 1024, 1280, 2048]


@pytest.mark.parametrize("C", V4_WIDTHS)
def test_layernorm_dropout_fwd(C):
    rows, p, seed, off = 5, 0.1, 1234, 977
    worst = _Worst()
    for cls in N.CLASSES:
        x, w, b, _, r = _ln_case(rows, C, cls)
        allow = _allow("ln", "y", cls)
        xb = Buf(rows, C, F32, x)
        yb, yd, mk, st = Buf(rows, C, torch.bfloat16, ld=C + 64), Buf(rows, C, torch.bfloat16), Buf(rows, C, torch.bfloat16), Buf(rows, 2, F32, ld=2)
        ops.layernorm_dropout_fwd(xb.v, _dev(w), _dev(b), LN_EPS, yb.v, st.v, yd.v, mk.v, p, seed, offset=off)
        y, m, d = yb.cpu(), mk.cpu(), yd.cpu()
        name = f"ln dropout C={C} {cls}"
        b1 = N.elem_bound(r["y"], r["S_y"], allow)
        worst.add(torch.bfloat16, _within(name, y, r["y"], _out_bound(r["y"], b1, torch.bfloat16)))
        worst.add(F32, _check_ln_stats(name, st, r, allow))
        m0 = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
        ops.dropout_mask(m0, p, seed, offset=off)
        assert _same_bits(m, m0.cpu()), "mask differs from vfm_dropout_mask at the same (seed, offset)"
        assert _same_bits(d, (y.float() * m.float()).to(torch.bfloat16)), "y_drop is not the 16-bit y times the mask, rounded once"
        assert 0 < (m == 0).sum().item() < m.numel()
    _report(f"ln dropout C={C}", worst, "; mask bit-equal to vfm_dropout_mask, y_drop = y16 * mask rounded once")


def test_layernorm_dropout_fwd_refusals():
    rows = 5
    for C, ldm, code in ((768, 776, E_SHAPE), (256, 265, E_ALIGN)):
        xb = Buf(rows, C, F32, torch.ones(rows, C))
        yb, yd, mk, st = Buf(rows, C, torch.bfloat16), Buf(rows, C, torch.bfloat16), Buf(rows, C, torch.bfloat16, ld=ldm), Buf(rows, 2, F32, ld=2)
        w = torch.ones(C, device=DEV)
        with pytest.raises(L.HipError, match=code):
            ops.layernorm_dropout_fwd(xb.v, w, w, LN_EPS, yb.v, st.v, yd.v, mk.v, 0.1, 1, offset=0)
        assert all(_nan_everywhere(t) for t in (yb, yd, mk, st))
    print("[norm] ln dropout refusals: C = 768 VFM_E_SHAPE, odd ld_mask VFM_E_ALIGN, outputs untouched")


@pytest.mark.parametrize("C", V4_WIDTHS)
def test_layernorm_fwd_split3_bf16x3(C):
    """hi == bf16(y) at columns c and plane + c, lo == bf16(y - hi) at 2 plane + c, y within the float32 bound of float64; without
    the float32 copy the image is the same bits.  (C = 1024 against vfm_split3's image: test_bf16x3_producers_write_the_split_operand_image.)"""
    rows, plane = 5, C
    worst = 0.0
    for cls in N.CLASSES:
        x, w, b, _, r = _ln_case(rows, C, cls)
        allow = _allow("ln", "y", cls)
        xb, wd, bd = Buf(rows, C, F32, x), _dev(w), _dev(b)
        imgs = []
        for with_y in (True, False):
            yb, y3, st = Buf(rows, C, F32), Buf(rows, 3 * plane, torch.bfloat16, ld=3 * plane + 8), Buf(rows, 2, F32, ld=2)
            L.check(L.load().vfm_layernorm_fwd_split3(L.ptr(xb.v), xb.ld, L.ptr(wd), L.ptr(bd), LN_EPS, L.ptr(yb.v) if with_y else None, yb.ld,
                                                      L.ptr(y3.v), y3.ld, plane, L.ptr(st.v), rows, C, L.stream()), "vfm_layernorm_fwd_split3")
            img = y3.cpu()
            imgs.append(img)
            name = f"ln split3 C={C} {cls} {'y' if with_y else 'no y'}"
            worst = max(worst, _check_ln_stats(name, st, r, allow))
            if with_y:
                y = yb.cpu()
                worst = max(worst, _within(name, y, r["y"], N.elem_bound(r["y"], r["S_y"], allow)))
                hi = y.to(torch.bfloat16)
                assert _same_bits(img[:, :C], hi) and _same_bits(img[:, plane:plane + C], hi)
                assert _same_bits(img[:, 2 * plane:2 * plane + C], (y - hi.float()).to(torch.bfloat16))
            else:
                assert _nan_everywhere(yb) and _same_bits(img, imgs[0])
    _report(f"ln split3 C={C}", worst, "; hi | hi | lo image exact, the same bits without the float32 copy")


# ------------------------------------------------------------------------------------------------------------ LayerNorm backward
def _bwd_form(C, lds, ptrs, pdy, need_w):
    """The kernel ln_bwd_impl selects, as its conditions are written: lds = (ld_x, ld_dx, ld_dy), ptrs = (x, dx) addresses."""
    nv = C // 256
    if not need_w:
        if C % 256 == 0 and nv in (1, 2, 4, 5) and all(v % 4 == 0 for v in lds) and all(p % 16 == 0 for p in ptrs) and pdy % 8 == 0:
            return f"v4<{nv}>"
        cp = (C + 3) // 4 * 4
        if 1024 < C <= 2816 and all(v % 4 == 0 and v >= cp for v in lds) and all(p % 16 == 0 for p in ptrs) and pdy % 16 == 0:
            return "v4t<11>"
        if C > 1024 and C % 2 == 0 and all(v % 2 == 0 for v in lds) and all(p % 8 == 0 for p in ptrs) and pdy % 8 == 0:
            return "v2<24>"
    pl = (C + 63) // 64
    if need_w:
        return "s<4,w>" if pl <= 4 else "s<16,w>"
    return "s<4>" if pl <= 4 else ("s<16>" if pl <= 16 else "s<48>")


LN_BWD = [("v4<1>", 256, {}), ("v4<2>", 512, {}), ("v4<4>", 1024, {}), ("v4<5>", 1280, {}),
          ("v4t<11>", 2048, {}), ("v4t<11>", 1028, {}), ("v4t<11>", 1366, dict(ld=1368)), ("v4t<11>", 2815, dict(ld=2816)), ("v4t<11>", 2816, {}),
          ("v2<24>", 1366, dict(ld=1366)), ("v2<24>", 2818, {}), ("v2<24>", 3072, {}),
          ("s<4>", 1, {}), ("s<4>", 19, {}), ("s<4>", 70, {}), ("s<4>", 256, dict(xs=1)), ("s<16>", 257, {}), ("s<16>", 768, {}),
          ("s<16>", 1024, dict(xs=1)), ("s<48>", 1025, {}), ("s<48>", 3071, {})]


def _ln_stats_dev(r):
    """(mean, rstd) of the float64 reference rounded to float32: the backward is given correct statistics."""
    return torch.stack((r["mean"], r["rstd"]), 1).float().contiguous().to(DEV)


def _dx_expect(r, dx0, acc, allow):
    """Expected dx and its bound: the allowance on the new gradient, plus one rounding of the sum when it is added to dx0."""
    b1 = N.elem_bound(r["dx"], r["S_dx"], allow)
    if not acc:
        return r["dx"], b1
    want = dx0 + r["dx"]
    return want, b1 + U * (want.abs() + b1)


def _run_ln_bwd(form, C, kw, rows, cls, ddt, acc, scaled=False):
    x, w, b, dy, r = _ln_case(rows, C, cls, ddt)
    allow = _allow("ln", "dx", cls)
    ld = kw.get("ld")
    dx0 = N.make_dy((rows, C), 9)
    xb = Buf(rows, C, F32, x, ld=ld, shift=kw.get("xs", 0))
    dyb, dxb = Buf(rows, C, ddt, dy, ld=ld), Buf(rows, C, F32, dx0, ld=ld)
    assert _bwd_form(C, (xb.ld, dxb.ld, dyb.ld), (xb.v.data_ptr(), dxb.v.data_ptr()), dyb.v.data_ptr(), False) == form
    name = f"ln bwd{' scaled' if scaled else ''} {form} C={C} rows={rows} {cls} dy {_dn(ddt)} acc={acc}"
    want, bound = _dx_expect(r, dx0, acc, allow)
    if scaled:
        ts = N.make_params(C, 11)[0]
        tb = Buf(rows, C, torch.bfloat16)
        ops.layernorm_bwd_scaled(dyb.v, xb.v, _dev(w), _ln_stats_dev(r), dxb.v, tb.v, _dev(ts), accumulate_dx=bool(acc))
        got = dxb.cpu()
        assert _same_bits(tb.cpu(), (got * ts.float()).to(torch.bfloat16)), "t_out is not dx_new * t_scale rounded once"
    else:
        ops.layernorm_bwd(dyb.v, xb.v, _dev(w), _ln_stats_dev(r), dxb.v, accumulate_dx=bool(acc))
        got = dxb.cpu()
    ratio = _within(name, got, want, bound)
    xb.cpu(), dyb.cpu()
    if C == 1:
        assert torch.equal(got.double(), dx0 if acc else torch.zeros(rows, 1, dtype=torch.float64))
    return ratio


@pytest.mark.parametrize("form,C,kw", LN_BWD, ids=[_case_id(*c) for c in LN_BWD])
def test_layernorm_bwd(form, C, kw):
    worst = max(_run_ln_bwd(form, C, kw, rows, cls, ddt, acc) for rows in (1, 5) for cls in N.CLASSES for ddt in (F32, torch.bfloat16)
                for acc in (0, 1))
    _report(f"ln bwd {_case_id(form, C, kw)}", worst)


@pytest.mark.parametrize("C", [256, 512, 1024, 1280])
def test_layernorm_bwd_scaled(C):
    worst = max(_run_ln_bwd(f"v4<{C // 256}>", C, {}, rows, cls, ddt, acc, scaled=True) for rows in (1, 5) for cls in N.CLASSES
                for ddt in (F32, torch.bfloat16) for acc in (0, 1))
    _report(f"ln bwd scaled C={C}", worst, "; t_out = dx_new * t_scale rounded once")


@pytest.mark.parametrize("rows", N.LN_W_ROWS)
@pytest.mark.parametrize("C", N.LN_W_WIDTHS)
def test_layernorm_bwd_dw_db(C, rows):
    form = "s<4,w>" if C <= 256 else "s<16,w>"
    w0, b0 = N.make_dy((1, C), 12), N.make_dy((1, C), 13)
    worst = 0.0
    for cls in N.CLASSES:
        al_dx, al_s = _allow("ln", "dx", cls), _allow("ln", "sums", cls)
        for ddt in (F32, torch.bfloat16):
            x, w, b, dy, r = _ln_case(rows, C, cls, ddt)
            for which in (("both", "dw", "db") if rows <= 5 else ("both",)):
                xb, dyb, dxb = Buf(rows, C, F32, x), Buf(rows, C, ddt, dy), Buf(rows, C, F32, N.make_dy((rows, C), 9))
                dwb, dbb = Buf(1, C, F32, w0), Buf(1, C, F32, b0)
                assert _bwd_form(C, (xb.ld, dxb.ld, dyb.ld), (xb.v.data_ptr(), dxb.v.data_ptr()), dyb.v.data_ptr(), True) == form
                ops.layernorm_bwd(dyb.v, xb.v, _dev(w), _ln_stats_dev(r), dxb.v, accumulate_dx=False,
                                  dw=dwb.v[0] if which != "db" else None, db=dbb.v[0] if which != "dw" else None)
                name = f"ln bwd {form} C={C} rows={rows} {cls} dy {_dn(ddt)} {which}"
                worst = max(worst, _within(name + " dx", dxb.cpu(), r["dx"], N.elem_bound(r["dx"], r["S_dx"], al_dx)))
                for key, buf, start, live in (("dw", dwb, w0, which != "db"), ("db", dbb, b0, which != "dw")):
                    want = start[0] + r[key] if live else start[0]
                    bound = (al_s * r["abs_" + key] + U * want.abs()) if live else torch.zeros(C, dtype=torch.float64)
                    worst = max(worst, _within(f"{name} {key}", buf.cpu()[0], want, bound))
    _report(f"ln bwd {form} C={C} rows={rows}", worst, " (dx, dw, db; dw / db accumulate onto non-zero values)")


def test_layernorm_bwd_refusals():
    rows = 5
    keep = N.make_dy((rows, 2056), 9)

    def bufs(C, dxs=0):
        return (Buf(rows, C, F32, torch.ones(rows, C)), Buf(rows, C, F32, torch.ones(rows, C)), Buf(rows, C, F32, keep[:, :C], shift=dxs),
                Buf(rows, C, torch.bfloat16), torch.ones(C, device=DEV), torch.ones(rows, 2, device=DEV))

    xb, dyb, dxb, tb, w, st = bufs(1025)
    dwb = Buf(1, 1025, F32)
    with pytest.raises(L.HipError, match=E_SHAPE):
        ops.layernorm_bwd(dyb.v, xb.v, w, st, dxb.v, dw=dwb.v[0])
    assert torch.equal(dxb.cpu().double(), keep[:, :1025]) and _nan_everywhere(dwb)
    for C, dxs in ((2048, 0), (768, 0), (256, 1)):
        xb, dyb, dxb, tb, w, st = bufs(C, dxs)
        with pytest.raises(L.HipError, match=E_UNSUPPORTED):
            ops.layernorm_bwd_scaled(dyb.v, xb.v, w, st, dxb.v, tb.v, w)
        assert torch.equal(dxb.cpu().double(), keep[:, :C]) and _nan_everywhere(tb)
    print("[norm] ln bwd refusals: dw at C = 1025 VFM_E_SHAPE; scaled at C = 2048, C = 768, shifted dx VFM_E_UNSUPPORTED; dx / t_out unchanged")


# ------------------------------------------------------------------------------------------------------------ GroupNorm, general path
@pytest.mark.parametrize("a", N.ACTS, ids=lambda a: N.ACT_NAMES[a])
@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_general(shape, a):
    B, P, C, G = shape
    w0, b0 = N.make_dy((1, C), 12), N.make_dy((1, C), 13)
    worst, notes = _Worst(), []
    for cls in N.CLASSES:
        al_y, al_dx, al_s = _allow("gn", "y", cls), _allow("gn", "dx", cls), _allow("gn", "sums", cls)
        for eps in (1e-5, 1e-6):
            x, w, b, _, r = _gn_case(shape, cls, eps, a)
            wd, bd = _dev(w), _dev(b)
            xb = Buf(B * P, C, F32, x, ld=C, shift=1)
            tag = f"gn {shape} {N.ACT_NAMES[a]} {cls} eps={eps:g}"
            stats = None
            for ydt in (F32, torch.bfloat16):
                yb, st = Buf(B * P, C, ydt, ld=C, shift=3), Buf(1, B * G * 2, F32, ld=B * G * 2)
                ops.groupnorm_fwd(xb.v, wd, bd, eps, G, a, yb.v, st.v, B, P)
                b1 = N.elem_bound(r["y"], r["S_y"], al_y).reshape(B * P, C)
                got = yb.cpu()
                worst.add(ydt, _within(f"{tag} y {_dn(ydt)}", got, r["y"].reshape(B * P, C), _out_bound(r["y"].reshape(B * P, C), b1, ydt)))
                sg = st.cpu().view(B, G, 2)
                worst.add(F32, _within(f"{tag} mean", sg[..., 0], r["mean"], al_y * r["S_x"]), _within(f"{tag} rstd", sg[..., 1], r["rstd"], al_y * r["rstd"]))
                if ydt == F32:
                    stats = st
                    if cls == "offset" and eps == 1e-5:
                        notes.append(f"general y {N.measure(got.view(B, P, C), r['y'], r['S_y']):.2e}")
            if cls == "offset" and eps == 1e-5 and a in (N.ACT_NONE, N.ACT_RELU) and ops.groupnorm_tile_ok(P, C, G):
                xt, yt, stt = _dev(x).reshape(B * P, C).contiguous(), torch.empty(B * P, C, device=DEV), torch.empty(B, G, 2, device=DEV)
                ops.groupnorm_tile_fwd(xt, wd, bd, eps, G, a, yt, stt, B, P)
                notes.append(f"tile y {N.measure(yt.cpu().view(B, P, C), r['y'], r['S_y']):.2e}")
            for ddt in (F32, torch.bfloat16):
                x, w, b, dy, r = _gn_case(shape, cls, eps, a, ddt)
                variants = ("both", "dw", "db") if (ddt == F32 and cls == "centred" and eps == 1e-5) else ("both",)
                for which in variants:
                    dyb, dxb = Buf(B * P, C, ddt, dy, ld=C, shift=2), Buf(B * P, C, F32, ld=C, shift=1)
                    dwb, dbb = Buf(1, C, F32, w0), Buf(1, C, F32, b0)
                    ops.groupnorm_bwd(dyb.v, xb.v, wd, bd, stats.v, G, a, dxb.v, dwb.v[0] if which != "db" else None,
                                      dbb.v[0] if which != "dw" else None, B, P)
                    name = f"{tag} dy {_dn(ddt)} {which}"
                    got = dxb.cpu()
                    worst.add(F32, _within(name + " dx", got, r["dx"].reshape(B * P, C), N.elem_bound(r["dx"], r["S_dx"], al_dx).reshape(B * P, C)))
                    for key, buf, start, live in (("dw", dwb, w0, which != "db"), ("db", dbb, b0, which != "dw")):
                        want = start[0] + r[key] if live else start[0]
                        bound = (al_s * r["abs_" + key] + U * want.abs()) if live else torch.zeros(C, dtype=torch.float64)
                        worst.add(F32, _within(f"{name} {key}", buf.cpu()[0], want, bound))
                    dyb.cpu()
                    if which == "both" and ddt == F32 and cls == "offset" and eps == 1e-5:
                        notes.append(f"general dx {N.measure(got.view(B, P, C), r['dx'], r['S_dx']):.2e}")
            xb.cpu(), stats.cpu()
    aten = f"ATen y {_ATEN['gn', 'y', 'offset']:.2e} dx {_ATEN['gn', 'dx', 'offset']:.2e}"
    _report(f"gn {'x'.join(map(str, shape))} {N.ACT_NAMES[a]}", worst, f"; offset class, in the measure: {', '.join(notes)} ({aten}, worst over its cases)")


def test_norm_entries_refuse_unknown_activations():
    B, P, C, G = 1, 64, 32, 8
    x, w = torch.ones(B * P, C, device=DEV), torch.ones(C, device=DEV)
    st, mv, sd = torch.ones(B, G, 2, device=DEV), torch.ones(2, C, device=DEV), torch.ones(2, C, device=DEV)
    for bad in (4, -1):
        yb, dxb, dwb, sb = Buf(B * P, C, F32, ld=C), Buf(B * P, C, F32, ld=C), Buf(1, C, F32), Buf(2, C, F32, ld=C)
        for call in (lambda: ops.groupnorm_fwd(x, w, w, 1e-5, G, bad, yb.v, st, B, P),
                     lambda: ops.groupnorm_bwd(x, x, w, w, st, G, bad, dxb.v, dwb.v[0], dwb.v[0], B, P),
                     lambda: ops.bn_apply(x, mv, w, w, 1e-5, bad, yb.v),
                     lambda: ops.bn_bwd_reduce(x, x, mv, w, w, 1e-5, bad, sb.v),
                     lambda: ops.bn_bwd_apply(x, x, mv, w, w, 1e-5, bad, sd, B * P, dxb.v)):
            with pytest.raises(L.HipError, match=E_INVAL):
                call()
        assert all(_nan_everywhere(t) for t in (yb, dxb, dwb, sb)), bad
    # the one-launch tile pair covers this shape and keeps refusing everything but NONE / RELU
    assert ops.groupnorm_tile_ok(P, C, G)
    yb, dxb = Buf(B * P, C, F32, ld=C), Buf(B * P, C, F32, ld=C)
    with pytest.raises(L.HipError, match=E_UNSUPPORTED):
        ops.groupnorm_tile_fwd(x, w, w, 1e-5, G, ops.ACT_QGELU, yb.v, st, B, P)
    with pytest.raises(L.HipError, match=E_UNSUPPORTED):
        ops.groupnorm_tile_bwd(x, x, w, w, st, G, ops.ACT_QGELU, dxb.v, None, None, B, P)
    assert _nan_everywhere(yb) and _nan_everywhere(dxb)
    print("[norm] act = 4 and act = -1 give VFM_E_INVAL in the five GroupNorm / BatchNorm entries, act = 3 VFM_E_UNSUPPORTED in the tile pair; outputs untouched")


# ------------------------------------------------------------------------------------------------------------ BatchNorm
def _bn_finalize_checks(tag, sums_dev, count, C, truth, al_y, rm0, rv0):
    """vfm_bn_finalize with running statistics (momentum 0.1 and 1.0) and without: mean_var against float64 of the same float32 sums and
    against the truth; the running update against float64 of the mean_var the kernel wrote.  Returns (mean_var buffer, worst ratio)."""
    worst, first = 0.0, None
    s64 = sums_dev.cpu().double()
    same = N.bn_mean_var(s64, float(count))
    ex2 = s64[1] / count
    for mom, running in ((0.1, True), (1.0, True), (0.1, False)):
        mvb = Buf(2, C, F32, ld=C)
        rmb, rvb = Buf(1, C, F32, rm0), Buf(1, C, F32, rv0)
        ops.bn_finalize(sums_dev, count, mvb.v, rmb.v[0] if running else None, rvb.v[0] if running else None, mom)
        mv = mvb.cpu()
        if first is None:
            first = mv
            worst = max(worst, _within(f"{tag} mean | sums", mv[0], same[0], 2 * U * same[0].abs()),
                        _within(f"{tag} var | sums", mv[1], same[1], 2 * U * same[1] + 4 * 2.0 ** -53 * ex2),
                        _within(f"{tag} mean", mv[0], truth["mean_var"][0], al_y * truth["S_x"]))
            nz = truth["mean_var"][1] > 0
            if nz.any():
                print(f"[{tag}] var against the truth: worst relative error {((mv[1].double() - truth['mean_var'][1]).abs()[nz] / truth['mean_var'][1][nz]).max().item():.2e}")
        else:
            assert _same_bits(mv, first)
        rm, rv = rmb.cpu()[0], rvb.cpu()[0]
        if not running:
            assert torch.equal(rm.double(), rm0[0]) and torch.equal(rv.double(), rv0[0])
            continue
        want_m, want_v = N.bn_running(rm0[0], rv0[0], mv.double(), float(count), mom)
        if mom == 1.0:
            assert torch.equal(rm, mv[0])                                        # 0 * old + 1 * mean
        worst = max(worst, _within(f"{tag} running mean m={mom}", rm, want_m, 4 * U * (((1 - mom) * rm0[0]).abs() + (mom * mv[0].double()).abs())),
                    _within(f"{tag} running var m={mom}", rv, want_v, 6 * U * (((1 - mom) * rv0[0]).abs() + (want_v - (1 - mom) * rv0[0]).abs())))
    mvb = Buf(2, C, F32, first, ld=C)
    return mvb, worst


def _bn_shard_pass(tag, xs, dys, ddt, ydt, w, b, a, mvb, r, al, rows_total, sums_dy_dev=None):
    """Forward per shard; with sums_dy_dev also dx per shard.  Without it: returns the per-shard sums_dy buffers."""
    worst, outs = _Worst(), []
    wd, bd = _dev(w), _dev(b)
    for i, (x, dy) in enumerate(zip(xs, dys)):
        n, C = x.shape
        xb, dyb = Buf(n, C, F32, x, ld=C, shift=1), Buf(n, C, ddt, dy, ld=C, shift=2)
        if sums_dy_dev is None:
            yb, sb = Buf(n, C, ydt, ld=C, shift=3), Buf(2, C, F32, ld=C)
            ops.bn_apply(xb.v, mvb.v, wd, bd, BN_EPS, a, yb.v)
            b1 = N.elem_bound(r["y"][i], r["S_y"], al["y"])
            worst.add(ydt, _within(f"{tag} shard {i} y {_dn(ydt)}", yb.cpu(), r["y"][i], _out_bound(r["y"][i], b1, ydt)))
            ops.bn_bwd_reduce(dyb.v, xb.v, mvb.v, wd, bd, BN_EPS, a, sb.v)
            outs.append(sb)
        else:
            dxb = Buf(n, C, F32, ld=C, shift=1)
            ops.bn_bwd_apply(dyb.v, xb.v, mvb.v, wd, bd, BN_EPS, a, sums_dy_dev, rows_total, dxb.v)
            worst.add(F32, _within(f"{tag} shard {i} dx, dy {_dn(ddt)}", dxb.cpu(), r["dx"][i], N.elem_bound(r["dx"][i], r["S_dx"], al["dx"])))
        xb.cpu(), dyb.cpu()
    return worst, outs


def _bn_run(shape, a, cut):
    rows, C = shape
    rm0, rv0 = N.make_params(C, 7)[1][None], N.make_params(C, 8)[0][None]
    worst = _Worst()
    for cls in N.CLASSES:
        al = {q: _allow("bn", q, cls) for q in ("y", "dx", "sums")}
        for ddt, ydt in ((F32, F32), (torch.bfloat16, torch.bfloat16)):
            xs, w, b, dys, r = _bn_case(shape, cls, a, ddt, cut)
            tag = f"bn {shape} {N.ACT_NAMES[a]} {cls}{'' if cut is None else ' two shards'}"
            parts = []
            for i, x in enumerate(xs):
                xb, sb = Buf(x.shape[0], C, F32, x, ld=C, shift=1), Buf(2, C, F32, ld=C)
                ops.bn_moments(xb.v, sb.v)
                ps, pa = N.bn_sums(x)
                worst.add(F32, _within(f"{tag} shard {i} sums", sb.cpu(), ps, al["sums"] * pa))
                parts.append(sb)
                xb.cpu()
            sums_dev = parts[0].v.clone() if len(parts) == 1 else parts[0].v + parts[1].v      # the all-reduce of the contract
            if ddt == F32:
                mvb, wf = _bn_finalize_checks(tag, sums_dev, rows, C, r, al["y"], rm0, rv0)
                worst.add(F32, wf)
            else:
                mvb = Buf(2, C, F32, ld=C)
                ops.bn_finalize(sums_dev, rows, mvb.v, None, None, 0.1)
            wp, sds = _bn_shard_pass(tag, xs, dys, ddt, ydt, w, b, a, mvb, r, al, rows)
            worst.add(F32, wp.v["f32"]), worst.add(torch.bfloat16, wp.v["h16"])
            sdy_dev = sds[0].v.clone() if len(sds) == 1 else sds[0].v + sds[1].v
            bound = al["sums"] * r["abs_sums_dy"] + (U * r["sums_dy"].abs() if len(sds) > 1 else 0.0)
            worst.add(F32, _within(f"{tag} sums_dy, dy {_dn(ddt)}", sdy_dev.cpu(), r["sums_dy"], bound))
            wp, _ = _bn_shard_pass(tag, xs, dys, ddt, ydt, w, b, a, mvb, r, al, rows, sums_dy_dev=sdy_dev)
            worst.add(F32, wp.v["f32"])
            for sb in sds:
                sb.cpu()
            mvb.cpu()
    return worst


@pytest.mark.parametrize("a", N.ACTS, ids=lambda a: N.ACT_NAMES[a])
@pytest.mark.parametrize("shape", N.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batchnorm(shape, a):
    """moments -> finalize (count = rows; (1, 19) takes the count - 1 -> 1 clamp) -> apply -> bwd_reduce -> bwd_apply, one shard."""
    _report(f"bn {'x'.join(map(str, shape))} {N.ACT_NAMES[a]}", _bn_run(shape, a, None))


@pytest.mark.parametrize("a", N.ACTS, ids=lambda a: N.ACT_NAMES[a])
@pytest.mark.parametrize("shape", list(N.BN_SPLITS), ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_two_shards(shape, a):
    """The SyncBatchNorm contract: the moments of two shards of unequal length added, count = all rows; forward per shard; sums_dy added,
    total_rows = all rows; dx per shard against the float64 restatement over both shards (pinned to autograd over their concatenation)."""
    _report(f"bn two shards {'x'.join(map(str, shape))} ({N.BN_SPLITS[shape]} + {shape[0] - N.BN_SPLITS[shape]} rows) {N.ACT_NAMES[a]}",
            _bn_run(shape, a, N.BN_SPLITS[shape]))
