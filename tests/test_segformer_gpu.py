"""The one-launch GroupNorm kernels (vfm_groupnorm_tile_fwd / _bwd) against a float64 evaluation, and SegformerHead's choice between
them and the three- / four-launch kernels of group_norm_act.

Bound (the convention of the HRDA kernel tests): 4 x the error of the plain fp32 torch GroupNorm against the same float64 result on the
same input, floor one fp32 rounding - no absolute tolerance.  A 16-bit output is additionally allowed its own rounding of the value
(unit roundoff 2^-8 bf16 / 2^-11 fp16 of the element, plus fp16's smallest subnormal step)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests.helpers import rel_err  # noqa: E402
from vfmseg_amd import lib as L, ops  # noqa: E402
from vfmseg_amd.precision import set_compute_dtype  # noqa: E402

DEV = "cuda"
NAN = float("nan")
ACTS = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU}
# (B, P, C, G): the head's embedding stage and fusion; P no multiple of any row step with an odd batch; sixteen channels per group
SHAPES = [(2, 1024, 1024, 128), (2, 1024, 256, 32), (3, 23 * 31, 256, 32), (1, 64, 64, 4)]
OUTSIDE = (1, 1025, 64, 4)    # one row more than the tile kernel holds


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    set_compute_dtype("bf16")


@functools.lru_cache(maxsize=None)
def _case(shape, act, kind="unit"):
    """inputs + float64 and plain-fp32 evaluations (CPU), computed once per case and shared by the tests that need them"""
    B, P, C, G = shape
    g = torch.Generator().manual_seed(1000 * C + P + 7 * G + (1 if kind == "unit" else 2))
    x = torch.randn(B * P, C, generator=g)
    if kind == "mean100":
        x = x + 100.0
    w = 1.0 + 0.3 * torch.randn(C, generator=g)
    b = 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(B * P, C, generator=g).bfloat16().float()   # exactly representable in both 16-bit types' range and in fp32
    dy = dy.half().float()

    def run(dt):
        xx, ww, bb = (t.to(dt).requires_grad_(True) for t in (x, w, b))
        y = F.group_norm(xx.view(B, P, C).permute(0, 2, 1), G, ww, bb, 1e-5)
        y = F.relu(y) if act == "relu" else y
        y = y.permute(0, 2, 1).reshape(B * P, C)
        y.backward(dy.to(dt))
        return dict(y=y.detach(), dx=xx.grad, dw=ww.grad, db=bb.grad)
    ref, plain = run(torch.float64), run(torch.float32)
    bound = {n: 4.0 * max(rel_err(plain[n], ref[n]), 2.0 ** -24) for n in ref}
    return dict(x=x, w=w, b=b, dy=dy, ref=ref, bound=bound)


def _run(shape, act, c, y_dtype, dy_dtype, tile, fill=NAN, prefill=0.0):
    B, P, C, G = shape
    x, w, b = (c[k].to(DEV) for k in ("x", "w", "b"))
    y = torch.full((B * P, C), fill, dtype=y_dtype, device=DEV)
    stats = torch.full((B, G, 2), fill, device=DEV)
    dx = torch.full((B * P, C), fill, device=DEV)
    dw, db = torch.full((C,), prefill, device=DEV), torch.full((C,), prefill, device=DEV)
    dy = c["dy"].to(DEV).to(dy_dtype)
    fwd, bwd = (ops.groupnorm_tile_fwd, ops.groupnorm_tile_bwd) if tile else (ops.groupnorm_fwd, ops.groupnorm_bwd)
    fwd(x, w, b, 1e-5, G, ACTS[act], y, stats, B, P)
    bwd(dy, x, w, b, stats, G, ACTS[act], dx, dw, db, B, P)
    return dict(y=y, dx=dx, dw=dw, db=db, stats=stats)


def _check(got, c, y_dtype, tag, prefill=0.0):
    ref, bound = c["ref"], c["bound"]
    errs = {}
    for n in ("y", "dx", "dw", "db"):
        g = got[n].double().cpu()
        assert torch.isfinite(g).all(), (tag, n, "an output element was not written")
        r = ref[n] + (prefill if n in ("dw", "db") else 0.0)
        scale = ref[n].abs().max().item()
        tol = torch.full_like(r, bound[n] * scale)
        if n == "y" and y_dtype != torch.float32:
            u = 2.0 ** -8 if y_dtype == torch.bfloat16 else 2.0 ** -11
            tol = tol + u * (r.abs() + tol) + (2.0 ** -25 if y_dtype == torch.float16 else 0.0)
        if n in ("dw", "db") and prefill:
            tol = tol + 2.0 ** -24 * r.abs()      # the one rounding of adding to the prefilled value
        excess = ((g - r).abs() - tol).max().item()
        errs[n] = ((g - r).abs().max() / scale).item()
        print(f"[gn tile {tag}] {n}: rel err {errs[n]:.2e}, bound {bound[n]:.2e}")
        assert excess <= 0.0, (tag, n, errs[n], bound[n])
    return errs


@pytest.mark.parametrize("half", ["bf16", "fp16"])
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", SHAPES)
def test_tile_kernels_match_float64(shape, act, out16, half):
    """Both kernels into NaN-prefilled buffers, y in fp32 or in the 16-bit type of either library (dy then in that type too).  Where the
    existing kernels cover the shape (they always do), the new results are no further from float64 than theirs by more than the bound."""
    set_compute_dtype(half)
    B, P, C, G = shape
    assert ops.groupnorm_tile_ok(P, C, G)
    c = _case(shape, act)
    dt = L.half_dtype() if out16 else torch.float32
    got = _run(shape, act, c, dt, dt, tile=True)
    e_new = _check(got, c, dt, f"{shape} {act} {dt}")
    old = _run(shape, act, c, dt, dt, tile=False)
    for n, e in e_new.items():
        e_old = rel_err(old[n], c["ref"][n])
        slack = c["bound"][n] + ((2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11) if (n == "y" and out16) else 0.0)
        assert e <= e_old + slack, (n, e, e_old)
    # the saved statistics (mean, rstd per image and group) are what the backward reads: an error there shows in y at the same relative size
    xs = c["x"].double().view(B, P, G, C // G)
    mean, var = xs.mean(dim=(1, 3)), xs.var(dim=(1, 3), unbiased=False)
    assert (got["stats"][..., 0].double().cpu() - mean).abs().max() <= c["bound"]["y"] * xs.std().item()
    assert rel_err(got["stats"][..., 1], (var + 1e-5).rsqrt()) <= c["bound"]["y"]


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
def test_mean_100_unit_variance(shape):
    """Variance by cancellation (E[x^2] - mean^2 in fp32 loses everything at mean 100) would miss the bound by orders of magnitude."""
    set_compute_dtype("bf16")
    c = _case(shape, "relu", "mean100")
    _check(_run(shape, "relu", c, torch.float32, torch.float32, tile=True), c, torch.float32, f"{shape} mean 100")


def test_dw_db_accumulate_into_prefilled_buffers():
    set_compute_dtype("bf16")
    shape = SHAPES[2]
    c = _case(shape, "relu")
    _check(_run(shape, "relu", c, torch.float32, torch.float32, tile=True, prefill=3.0), c, torch.float32, "prefilled dw/db", prefill=3.0)


def test_all_negative_group_gives_exact_zeros():
    """ReLU's derivative at <= 0 is 0 (the existing kernels' convention): a group whose pre-activation is negative everywhere has y and dx
    exactly zero, and its channels' dw / db stay untouched."""
    set_compute_dtype("bf16")
    shape = B, P, C, G = SHAPES[3]
    c = dict(_case(shape, "relu"))
    w, b = c["w"].clone(), c["b"].clone()
    w[16:32], b[16:32] = 0.1, -10.0       # group 1: xhat * 0.1 - 10 < 0
    c["w"], c["b"] = w, b
    got = _run(shape, "relu", c, torch.float32, torch.float32, tile=True, prefill=2.5)
    assert (got["y"][:, 16:32] == 0).all() and (got["dx"][:, 16:32] == 0).all()
    assert (got["dw"][16:32] == 2.5).all() and (got["db"][16:32] == 2.5).all()
    assert (got["y"][:, :16] != 0).any() and (got["dx"][:, :16] != 0).any()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_two_runs_are_bit_identical(shape):
    set_compute_dtype("bf16")
    c = _case(shape, "relu")
    r1 = _run(shape, "relu", c, torch.bfloat16, torch.bfloat16, tile=True)
    r2 = _run(shape, "relu", c, torch.bfloat16, torch.bfloat16, tile=True, fill=1e30)
    for n in r1:
        assert torch.equal(r1[n], r2[n]), n


def test_entries_refuse_a_shape_outside_the_coverage():
    set_compute_dtype("bf16")
    B, P, C, G = OUTSIDE
    assert not ops.groupnorm_tile_ok(P, C, G) and ops.groupnorm_tile_ok(P - 1, C, G)
    assert not ops.groupnorm_tile_ok(64, 96, 32) and not ops.groupnorm_tile_ok(64, 64, 1) and not ops.groupnorm_tile_ok(64, 48, 3)
    x = torch.zeros(B * P, C, device=DEV)
    w = torch.ones(C, device=DEV)
    y, stats = torch.empty_like(x), torch.empty(B, G, 2, device=DEV)
    with pytest.raises(L.HipError, match=r"\(-2\)"):
        ops.groupnorm_tile_fwd(x, w, w, 1e-5, G, ops.ACT_RELU, y, stats, B, P)
    with pytest.raises(L.HipError, match=r"\(-2\)"):
        ops.groupnorm_tile_bwd(x, x, w, w, stats, G, ops.ACT_RELU, y, torch.zeros_like(w), torch.zeros_like(w), B, P)
    with pytest.raises(L.HipError):   # GELU is not part of the tile kernels' contract
        ops.groupnorm_tile_fwd(x[:64], w, w, 1e-5, G, ops.ACT_GELU, y[:64], stats, 1, 64)


def _small_head(hp, wp, mode, monkeypatch, force):
    """a 64-wide SegformerHead (4 channels x 16 per group; branch norm 256 channels / 16 groups) on seeded taps: logits and every gradient"""
    from vfmseg_amd.heads import FeatPack
    from vfmseg_amd.precision import compute_dtype
    from vfmseg_amd.registry import MODELS
    from vfmseg_amd.synth import synth_like
    monkeypatch.setenv("VFMSEG_GN_TILE", force)
    set_compute_dtype(mode)
    head = MODELS.build(dict(type="SegformerHead", in_channels=[64] * 4, in_index=[0, 1, 2, 3], channels=64, dropout_ratio=0.0, num_classes=19,
                             norm_cfg=dict(type="GN", num_groups=4), align_corners=False))
    head.load_state_dict(synth_like(head.state_dict()))
    head = head.to(DEV).train()
    g = torch.Generator().manual_seed(hp * 100 + wp)
    xcat = torch.randn(2 * hp * wp, 256, generator=g).to(DEV).to(compute_dtype()).requires_grad_(True)
    lg = head.forward_tokens(FeatPack(xcat, 2, hp, wp))
    lg.backward(torch.randn(lg.shape, generator=g).to(DEV))
    torch.cuda.synchronize()
    return [lg.detach(), xcat.grad] + [p.grad for _, p in sorted(head.named_parameters())]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_head_switch_and_fallback_outside_the_coverage(mode, monkeypatch):
    """VFMSEG_GN_TILE=1 / 0 forces either form inside the coverage (results agree to rounding, and the forced forms really differ in their
    launches); on a 33 x 33 map (P = 1089 > 1024) the head gives the existing kernels' result bit for bit whatever the switch says."""
    from vfmseg_amd import functional as Fh
    calls = []
    real = ops.groupnorm_tile_fwd
    monkeypatch.setattr(ops, "groupnorm_tile_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    inside_tile = _small_head(32, 32, mode, monkeypatch, "1")
    assert len(calls) == 2 and Fh.gn_tile_selected(1024, 64, 4)
    inside_old = _small_head(32, 32, mode, monkeypatch, "0")
    assert len(calls) == 2 and not Fh.gn_tile_selected(1024, 64, 4)
    # both forms are correct GroupNorms whose fp32 results differ in the last bits; in f32 that difference passes two more normalised layers
    # (allow 2^-14, ten bits above one fp32 rounding, seven bits under a wrong statistic), in bf16 it can flip the 2^-8 rounding of a map entry
    tol = 2.0 ** -14 if mode == "f32" else 4 * 2.0 ** -8
    for a, b in zip(inside_tile, inside_old):
        assert rel_err(a.float(), b.float()) <= tol
    out_tile = _small_head(33, 33, mode, monkeypatch, "1")
    assert len(calls) == 2 and not Fh.gn_tile_selected(33 * 33, 64, 4)
    out_old = _small_head(33, 33, mode, monkeypatch, "0")
    for a, b in zip(out_tile, out_old):
        assert torch.equal(a, b)
