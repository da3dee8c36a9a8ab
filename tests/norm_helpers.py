"""Float64 torch restatements of what csrc/norm.hip computes (LayerNorm, GroupNorm on token-major [B, P, C] maps, BatchNorm as
include/vfmseg_hip.h defines it: per-shard sums, a count, and total_rows), the error measure of the norm tests, their input
generators and the mutants of the sensitivity checks.  Nothing here touches the GPU; tests/test_norm_cpu.py pins every restatement
against float64 F.layer_norm / F.group_norm / F.batch_norm and autograd.

One core does the three families: a normalisation set is (image b, group g) of x[B, P, C].
  LayerNorm  = the core on x[rows, 1, C] with one group (set = a row),
  GroupNorm  = the core as it is,
  BatchNorm  = the core on x[1, rows, C] with C groups (set = a channel column); the shard contract has its own functions.

Error measure (err = |got - ref|):
  y, dx       err / (|ref| + S), S = RMS of the float64 reference over the element's normalisation set;
  sums        (dw, db, sums, sums_dy)  err / sum of |terms|;
  mean        err / RMS of x over the set;   rstd, var   err / |ref|.
Two amendments, each with its reason.  (1) A term dz * xhat of dw carries the error of xhat, and xhat is a difference: its error
is absolute (the rounding of x and of the float32 mean times rstd), not relative to |xhat|.  With one row the sum has one term, and
at a column where x meets the mean |xhat| is 1e-4 while its float32 error stays 2e-7: "relative to the sum of |terms|" then reads
5e-3 for ATen's kernels too.  So the xhat factor of a term enters as |xhat| + 1 - its magnitude plus the RMS of xhat over its set,
which is 1 - just as an element of y enters as |ref| + S: the terms of dw are |dz| (|xhat| + 1); db, sums keep |term|.
(2) The input gradient of a set of n <= 2 elements is pure cancellation - exactly 0 for n = 1, and
(g1 - g2) / 2 * eps / (var + eps) for n = 2 (mean and scale take both degrees of freedom) - so the RMS of the reference is not the
scale of any float32 evaluation there, ATen's included (its error would read 1e-2).  For those sets S is the RMS of the unprojected
gradient rstd * w * dz, the term the projection is taken from.  Sets of three and more elements use the reference's RMS."""
import math

import torch

U = 2.0 ** -24
FLOOR = 16 * U                    # no allowance is smaller: four rounded operations plus statistics a few roundings off, doubled
ACT_NONE, ACT_GELU, ACT_RELU, ACT_QGELU = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_GELU, ACT_RELU, ACT_QGELU)
ACT_NAMES = {0: "none", 1: "gelu", 2: "relu", 3: "qgelu"}
CLASSES = ("centred", "offset")
# the project's present bounds (tests/test_kernels_gpu.py): no measured allowance may exceed them
CEILING = {("ln", "y"): 1e-5, ("ln", "dx"): 2e-5, ("ln", "sums"): 2e-5,
           ("gn", "y"): 2e-5, ("gn", "dx"): 5e-5, ("gn", "sums"): 5e-5,
           ("bn", "y"): 2e-5, ("bn", "dx"): 5e-5, ("bn", "sums"): 5e-5}

GN_SHAPES = [(3, 1, 6, 3), (2, 65, 72, 8), (2, 64, 64, 64), (1, 63, 130, 1), (1, 100, 128, 32), (1, 4097, 32, 8)]
BN_SHAPES = [(1, 19), (2, 1), (65, 65), (300, 64), (4097, 130)]
BN_SPLITS = {(2, 1): 1, (65, 65): 23, (300, 64): 100, (4097, 130): 1000}      # rows of the first shard; (1, 19) has one row
# every width the LayerNorm cases of tests/test_norm_gpu.py use
LN_WIDTHS = [1, 19, 70, 256, 257, 512, 768, 1024, 1025, 1028, 1280, 1366, 1536, 2048, 2815, 2816, 2818, 3071, 3072]
LN_W_WIDTHS = [1, 70, 256, 257, 1024]                                          # the dw / db forms
LN_W_ROWS = [1, 5, 513, 1100]


# ------------------------------------------------------------------------------------------------------------ activations
def act(z, a):
    if a == ACT_GELU:
        return 0.5 * z * (1.0 + torch.erf(z * math.sqrt(0.5)))
    if a == ACT_RELU:
        return z.clamp_min(0)
    if a == ACT_QGELU:
        return z * torch.sigmoid(1.702 * z)
    assert a == ACT_NONE
    return z


def act_grad(z, a):
    if a == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(z * math.sqrt(0.5))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    if a == ACT_RELU:
        return (z > 0).to(z.dtype)
    if a == ACT_QGELU:
        sg = torch.sigmoid(1.702 * z)
        return sg * (1.0 + 1.702 * z * (1.0 - sg))
    assert a == ACT_NONE
    return torch.ones_like(z)


# ------------------------------------------------------------------------------------------------------------ the core
def _rms(v2sum, n):
    return (v2sum / n).sqrt()


def core(x, G, w, b, eps, a=ACT_NONE, dy=None, stat_mask=None, gidx=None, drop_s1=False, drop_act_grad=False):
    """x [B, P, C] float64, G groups of adjacent channels.  Returns a dict: y, mean / rstd [B, G], S_y, S_x (RMS of y / x over the set,
    broadcast to x's shape / [B, G]); with dy also dx, dw, db, S_dx, abs_dw, abs_db.
    Mutants: stat_mask [B, P, C] bool = the elements that enter the statistics; gidx [C] = another channel -> group map;
    drop_s1 = the mean-of-gradient term left out of dx; drop_act_grad = act' taken as 1."""
    B, P, C = x.shape
    cg = C // G
    gi = torch.arange(C) // cg if gidx is None else gidx
    M = torch.zeros(C, G, dtype=torch.float64)
    M[torch.arange(C), gi] = 1.0
    m = torch.ones_like(x) if stat_mask is None else stat_mask.to(x.dtype)
    n_stat = m.sum(1) @ M                                                       # [B, G]
    mean = ((x * m).sum(1) @ M) / n_stat
    xc = x - mean[:, gi][:, None, :]
    var = ((xc * xc * m).sum(1) @ M) / n_stat
    rstd = (var + eps).rsqrt()
    xh = xc * rstd[:, gi][:, None, :]
    z = xh * w + b
    y = act(z, a)
    n = float(P * cg)

    def set_rms(v):
        return _rms((v * v).sum(1) @ M, n)[:, gi][:, None, :].expand(B, P, C)

    out = dict(y=y, mean=mean, rstd=rstd, var=var, S_y=set_rms(y), S_x=_rms((x * x).sum(1) @ M, n), xh=xh, z=z)
    if dy is None:
        return out
    dz = dy if drop_act_grad else dy * act_grad(z, a)
    g = dz * w
    s1 = ((g.sum(1) @ M) / n)[:, gi][:, None, :]
    s2 = (((g * xh).sum(1) @ M) / n)[:, gi][:, None, :]
    r = rstd[:, gi][:, None, :]
    dx = r * (g - (0.0 if drop_s1 else s1) - xh * s2)
    out.update(dx=dx, dw=(dz * xh).sum((0, 1)), db=dz.sum((0, 1)), abs_dw=(dz.abs() * (xh.abs() + 1.0)).sum((0, 1)), abs_db=dz.abs().sum((0, 1)),
               S_dx=set_rms(dx) if n >= 3 else set_rms(r * g), dz=dz)
    return out


def ln_ref(x, w, b, eps, dy=None, **mut):
    """x [rows, C] -> the core's dict with [rows, C] maps and mean / rstd / S_x [rows]."""
    if "stat_mask" in mut and mut["stat_mask"] is not None:
        mut = dict(mut, stat_mask=mut["stat_mask"][:, None, :])
    o = core(x[:, None, :], 1, w, b, eps, ACT_NONE, None if dy is None else dy[:, None, :], **mut)
    return {k: (v[:, 0, :] if v.dim() == 3 else (v[:, 0] if v.dim() == 2 else v)) for k, v in o.items()}


def gn_ref(x, G, w, b, eps, a, dy=None, **mut):
    return core(x, G, w, b, eps, a, dy, **mut)


# ------------------------------------------------------------------------------------------------------------ BatchNorm, by entry
def bn_sums(x):
    """vfm_bn_moments of one shard: (sums [2, C] = (sum x, sum x^2), abs [2, C] = the sums of the absolute values of the terms)."""
    return torch.stack((x.sum(0), (x * x).sum(0))), torch.stack((x.abs().sum(0), (x * x).sum(0)))


def bn_mean_var(sums, count):
    """vfm_bn_finalize: mean and BIASED variance (clamped at 0) from sums over `count` rows."""
    mean = sums[0] / count
    return torch.stack((mean, (sums[1] / count - mean * mean).clamp_min(0)))


def bn_running(rmean, rvar, mean_var, count, momentum):
    """The running-stat update of vfm_bn_finalize: the unbiased variance is var * count / max(count - 1, 1)."""
    return ((1 - momentum) * rmean + momentum * mean_var[0],
            (1 - momentum) * rvar + momentum * mean_var[1] * (count / max(count - 1.0, 1.0)))


def _bn_xh(x, mean_var, eps):
    rstd = (mean_var[1] + eps).rsqrt()
    return (x - mean_var[0]) * rstd, rstd


def bn_apply(x, mean_var, w, b, eps, a):
    xh, _ = _bn_xh(x, mean_var, eps)
    return act(xh * w + b, a)


def bn_sums_dy(dy, x, mean_var, w, b, eps, a, drop_act_grad=False):
    """vfm_bn_bwd_reduce of one shard: (sums_dy [2, C] = (sum dz, sum dz * xhat) = (db, dw), abs [2, C])."""
    xh, _ = _bn_xh(x, mean_var, eps)
    dz = dy if drop_act_grad else dy * act_grad(xh * w + b, a)
    return torch.stack((dz.sum(0), (dz * xh).sum(0))), torch.stack((dz.abs().sum(0), (dz.abs() * (xh.abs() + 1.0)).sum(0)))


def bn_dx(dy, x, mean_var, w, b, eps, a, sums_dy, total_rows, drop_s1=False, drop_act_grad=False):
    """vfm_bn_bwd_apply of one shard: dx = rstd w (dz - (sum dz + xhat sum dz xhat) / total_rows).  Also returns rstd w dz."""
    xh, rstd = _bn_xh(x, mean_var, eps)
    dz = dy if drop_act_grad else dy * act_grad(xh * w + b, a)
    return rstd * w * (dz - ((0.0 if drop_s1 else sums_dy[0]) + xh * sums_dy[1]) / total_rows), rstd * w * dz


def bn_ref(shards, w, b, eps, a, dys=None, count=None, total_rows=None, **mut):
    """The whole contract over a list of shards [rows_i, C]: sums added, count = total rows (or the mutant's), forward per shard,
    sums_dy added, dx per shard.  Returns a dict of per-shard lists and the shared statistics, with the S maps of the measure (the
    normalisation set of a channel is its column over ALL shards)."""
    rows = sum(s.shape[0] for s in shards)
    parts = [bn_sums(s) for s in shards]
    sums, abs_sums = sum(p[0] for p in parts), sum(p[1] for p in parts)
    mv = bn_mean_var(sums, float(rows if count is None else count))
    if count is None:                                                           # two-pass variance: the reference proper
        xa = torch.cat(shards)
        mv = torch.stack((xa.mean(0), ((xa - xa.mean(0)) ** 2).mean(0)))
    ys = [bn_apply(s, mv, w, b, eps, a) for s in shards]
    S_y = _rms(sum((y * y).sum(0) for y in ys), rows)
    out = dict(sums=sums, abs_sums=abs_sums, mean_var=mv, y=ys, S_y=S_y, S_x=_rms(sums[1], rows) if count is None else None)
    if dys is None:
        return out
    da = mut.get("drop_act_grad", False)
    parts = [bn_sums_dy(d, s, mv, w, b, eps, a, da) for d, s in zip(dys, shards)]
    sdy, abs_sdy = sum(p[0] for p in parts), sum(p[1] for p in parts)
    tr = float(rows if total_rows is None else total_rows)
    both = [bn_dx(d, s, mv, w, b, eps, a, sdy, tr, mut.get("drop_s1", False), da) for d, s in zip(dys, shards)]
    dxs, raws = [p[0] for p in both], [p[1] for p in both]
    S_dx = _rms(sum((v * v).sum(0) for v in (dxs if rows >= 3 else raws)), rows)
    out.update(sums_dy=sdy, abs_sums_dy=abs_sdy, dx=dxs, S_dx=S_dx)
    return out


# ------------------------------------------------------------------------------------------------------------ the measure
def measure(got, ref, S):
    """max over the elements of |got - ref| / (|ref| + S); 0 / 0 counts as 0 (an exact zero met exactly), anything / 0 as inf."""
    err = (got.double() - ref).abs()
    den = ref.abs() + S
    r = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return torch.nan_to_num(r, nan=float("inf"), posinf=float("inf")).max().item() if r.numel() else 0.0


def elem_bound(ref, S, allow):
    return allow * (ref.abs() + S)


def allowance(worst, ceiling):
    """4 x the worst error of ATen's float32 kernels, never below FLOOR, and never above the project's present bound: where 4 x ATen
    would exceed that bound, the bound stands (the new tests are nowhere looser than the old ones)."""
    return min(max(4.0 * worst, FLOOR), ceiling)


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    return torch.Generator().manual_seed(1000003 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _f32(t):
    return t.float().double()


def _sign(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def make_x(B, P, C, G, cls, seed, ln=False):
    """[B, P, C] float64 values exact in float32: randn * 1.5 + 0.3; magnitude 6 with random sign in the last column (LayerNorm) or
    the last row (GroupNorm, BatchNorm; not where it is the only row) and in channel 64 where there is one; class "offset" adds 4 standard deviations (6.0, random
    sign) of mean per normalisation set."""
    g = _gen(B, P, C, G, seed, CLASSES.index(cls))
    x = torch.randn(B, P, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    if ln:
        if C > 1:
            x[:, :, -1] = 6.0 * _sign((B, P), g)
    elif P > 1:
        x[:, -1, :] = 6.0 * _sign((B, C), g)
    if C > 64:
        x[:, :, 64] = 6.0 * _sign((B, P), g)
    if not ln and P == 1 and C // G == 2:
        # sets of two values: keep them at least 1.5 apart.  Two nearly equal values around a mean of 6 are ill-conditioned for ANY float32
        # statistics (the rounding of the stored mean times rstd: ATen's float32 GroupNorm reads 2e-5 on such a pair), which says nothing
        # about a kernel
        x[:, 0, 1::2] = x[:, 0, 0::2] + (1.5 + torch.randn(B, C // 2, generator=g, dtype=torch.float64).abs()) * _sign((B, C // 2), g)
    if cls == "offset":
        off = 6.0 * _sign((B, G), g)
        x = x + off[:, torch.arange(C) // (C // G)][:, None, :]
    return _f32(x)


def make_params(C, seed):
    g = _gen(C, seed, 77)
    return _f32(torch.randn(C, generator=g, dtype=torch.float64) * 0.1 + 1), _f32(torch.randn(C, generator=g, dtype=torch.float64) * 0.1)


def make_dy(shape, seed, dtype=None):
    """Upstream gradient, exact in float32 and, with `dtype`, exact in that 16-bit type."""
    d = torch.randn(*shape, generator=_gen(seed, 991, *shape), dtype=torch.float64).float()
    return (d if dtype is None else d.to(dtype).float()).double()


def off_the_relu_kink(x, G, w, b, eps, tol=1e-4):
    """relu' jumps at 0: an element whose pre-activation lies within float32 error of 0 may take either side, and the whole set's dx
    moves with it.  Inputs of the ReLU cases are nudged (by 2^-5, a few times at most) until no |z| is below tol, far above the
    float32 error of z (1e-6) and far below anything a kernel defect would need."""
    for _ in range(20):
        z = core(x, G, w, b, eps)["z"]
        bad = z.abs() < tol
        if not bool(bad.any()):
            return x
        x = _f32(torch.where(bad, x + 2.0 ** -5, x))
    raise AssertionError("could not move the inputs off the ReLU kink")


def ln_inputs(rows, C, cls, seed=0):
    return make_x(rows, 1, C, 1, cls, seed, ln=True)[:, 0, :]


def gn_inputs(B, P, C, G, cls, seed=0):
    return make_x(B, P, C, G, cls, seed)


def bn_inputs(rows, C, cls, seed=0):
    return make_x(1, rows, C, C, cls, seed)[0]


# ------------------------------------------------------------------------------------------------------------ mutants
def last_out_mask(B, P, C, ln=False):
    """Statistics without the last valid column (LayerNorm) / the last row (GroupNorm, BatchNorm); None where nothing would be left."""
    m = torch.ones(B, P, C, dtype=torch.bool)
    if ln:
        if C < 2:
            return None
        m[:, :, -1] = False
    else:
        if P < 2:
            return None
        m[:, -1, :] = False
    return m


def stripe_out_mask(B, P, C, G, width=64):
    """Statistics without the highest stripe of `width` columns that holds a valid column; None where a set would be left empty
    (BatchNorm's per-channel sets always would: tests/test_norm_cpu.py zeroes the stripe's sums instead)."""
    lo = (C - 1) // width * width
    if lo == 0:
        return None
    m = torch.ones(B, P, C, dtype=torch.bool)
    m[:, :, lo:] = False
    kept = torch.zeros(G, dtype=torch.float64).index_add_(0, torch.arange(C) // (C // G), m[0, 0].double())
    return m if bool((kept > 0).all()) else None


def group_63_for_64(C, G):
    """The channel -> group map with channel 64 filed under channel 63's group; None where they share a group or C <= 64."""
    cg = C // G
    if C <= 64 or 64 // cg == 63 // cg:
        return None
    gi = torch.arange(C) // cg
    gi[64] = gi[63]
    return gi
