"""Pins the float64 restatements of tests/norm_helpers.py against float64 F.layer_norm / F.group_norm / F.batch_norm and autograd
(the BatchNorm shard contract against autograd over the concatenated shards; QuickGELU is x * sigmoid(1.702 x)), and checks the
sensitivity condition of the GPU suite: at every shape tests/test_norm_gpu.py uses, each mutant - computed in float64, so only the
mutation separates it from the reference - lies at least 4 x the ceiling of the allowance above the reference in the measure the
GPU tests assert.  A kernel with that defect cannot pass, whatever allowance the GPU run measures."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_helpers as N

D = torch.float64


def _act_torch(z, a):
    return {0: lambda t: t, 1: F.gelu, 2: F.relu, 3: lambda t: t * torch.sigmoid(1.702 * t)}[a](z)


def _close(a, b, tol=1e-11):
    scale = max(b.abs().max().item(), 1e-30) if b.numel() else 1.0
    assert ((a - b).abs().max().item() if b.numel() else 0.0) <= tol * scale + 1e-300, ((a - b).abs().max().item(), scale)


# ------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("cls", N.CLASSES)
@pytest.mark.parametrize("C", [1, 19, 70, 257, 1366, 3072])
def test_layernorm_restatement(C, cls):
    rows, eps = 5, 1e-6
    x = N.ln_inputs(rows, C, cls)
    w, b = N.make_params(C, 1)
    dy = N.make_dy((rows, C), 2)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.layer_norm(xr, (C,), wr, br, eps)
    y.backward(dy)
    r = N.ln_ref(x, w, b, eps, dy)
    _close(r["y"], y.detach())
    _close(r["dx"], xr.grad, 1e-9)
    _close(r["dw"], wr.grad)
    _close(r["db"], br.grad)
    _close(r["mean"], x.mean(1))
    _close(r["rstd"], (x.var(1, unbiased=False) + eps).rsqrt())
    if C == 1:
        assert (r["dx"] == 0).all() and torch.equal(r["y"], b.expand(rows, 1))
    assert torch.allclose(r["S_y"][:, 0], y.detach().pow(2).mean(1).sqrt(), rtol=1e-12)


@pytest.mark.parametrize("a", N.ACTS, ids=lambda a: N.ACT_NAMES[a])
@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=str)
def test_groupnorm_restatement(shape, a):
    B, P, C, G = shape
    for cls, eps in zip(N.CLASSES, (1e-5, 1e-6)):
        x = N.gn_inputs(B, P, C, G, cls)
        w, b = N.make_params(C, 3)
        dy = N.make_dy((B, P, C), 4)
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = _act_torch(F.group_norm(xr.permute(0, 2, 1), G, wr, br, eps).permute(0, 2, 1), a)
        y.backward(dy)
        r = N.gn_ref(x, G, w, b, eps, a, dy)
        _close(r["y"], y.detach())
        _close(r["dx"], xr.grad, 1e-8)
        _close(r["dw"], wr.grad)
        _close(r["db"], br.grad)
        xg = x.view(B, P, G, C // G)
        _close(r["mean"], xg.mean((1, 3)))
        _close(r["rstd"], (xg.var((1, 3), unbiased=False) + eps).rsqrt())


@pytest.mark.parametrize("a", N.ACTS, ids=lambda a: N.ACT_NAMES[a])
@pytest.mark.parametrize("shape", N.BN_SHAPES, ids=str)
def test_batchnorm_restatement_and_shards(shape, a):
    """One shard and two shards of unequal length against F.batch_norm + autograd over all rows.  F.batch_norm refuses one row per
    channel in training mode: (1, 19) is pinned against the closed form instead (y = act(b), dx = 0, variance 0, clamp count - 1 -> 1)."""
    rows, C = shape
    eps, mom = 1e-5, 0.1
    for cls in N.CLASSES:
        x = N.bn_inputs(rows, C, cls)
        w, b = N.make_params(C, 5)
        dy = N.make_dy((rows, C), 6)
        rm, rv = N.make_params(C, 7)[1], N.make_params(C, 8)[0]
        cuts = [None] if rows == 1 else [None, N.BN_SPLITS[shape]]
        for cut in cuts:
            xs, dys = ([x], [dy]) if cut is None else ([x[:cut], x[cut:]], [dy[:cut], dy[cut:]])
            r = N.bn_ref(xs, w, b, eps, a, dys)
            mv_from_sums = N.bn_mean_var(r["sums"], float(rows))
            _close(mv_from_sums[0], r["mean_var"][0])
            assert ((mv_from_sums[1] - r["mean_var"][1]).abs() <= 1e-12 * (r["sums"][1] / rows)).all()   # one-pass == two-pass in float64
            got_rm, got_rv = N.bn_running(rm, rv, r["mean_var"], float(rows), mom)
            if rows == 1:
                assert (r["mean_var"][1] == 0).all() and (torch.cat(r["dx"]) == 0).all()
                _close(torch.cat(r["y"]), N.act(b, a).expand(1, C))
                _close(got_rv, (1 - mom) * rv)                                  # var * 1 / max(0, 1) = 0
                _close(r["sums_dy"][0], (dy * N.act_grad(b, a))[0])
                continue
            xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            rm_t, rv_t = rm.clone(), rv.clone()
            y = _act_torch(F.batch_norm(xr, rm_t, rv_t, wr, br, True, mom, eps), a)
            y.backward(dy)
            _close(torch.cat(r["y"]), y.detach())
            _close(torch.cat(r["dx"]), xr.grad, 1e-8)
            _close(r["sums_dy"][0], br.grad)
            _close(r["sums_dy"][1], wr.grad)
            _close(got_rm, rm_t)
            _close(got_rv, rv_t)


def test_core_serves_all_three_families():
    """BatchNorm is the core with one group per channel, LayerNorm the core with one row per image."""
    x = N.bn_inputs(65, 65, "offset")
    w, b = N.make_params(65, 5)
    dy = N.make_dy((65, 65), 6)
    r = N.bn_ref([x], w, b, 1e-5, N.ACT_GELU, [dy])
    c = N.core(x[None], 65, w, b, 1e-5, N.ACT_GELU, dy[None])
    _close(r["y"][0], c["y"][0])
    _close(r["dx"][0], c["dx"][0], 1e-9)
    _close(r["S_dx"], c["S_dx"][0, 0])
    _close(r["S_y"], c["S_y"][0, 0])


def test_measure_conventions():
    ref, S = torch.tensor([0.0, 1.0], dtype=D), torch.tensor([0.0, 1.0], dtype=D)
    assert N.measure(torch.tensor([0.0, 1.0]), ref, S) == 0.0
    assert N.measure(torch.tensor([1e-30, 1.0]), ref, S) == float("inf")
    assert N.measure(torch.tensor([0.0, float("nan")]), ref, S) == float("inf")
    assert abs(N.measure(torch.tensor([0.0, 1.5]), ref, S) - 0.25) < 1e-12
    assert N.allowance(0.0, 1e-5) == N.FLOOR == 16 * 2.0 ** -24 and N.allowance(1e-6, 1e-5) == 4e-6 and N.allowance(3e-6, 1e-5) == 1e-5
    assert all(N.FLOOR < c for c in N.CEILING.values())


# ------------------------------------------------------------------------------------------------------------ sensitivity
def _need(name, got, ref, S, ceiling):
    m = N.measure(got, ref, S)
    assert m >= 4 * ceiling, (name, m, 4 * ceiling)
    return m


@pytest.mark.parametrize("cls", N.CLASSES)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
def test_layernorm_mutants_are_visible(C, cls):
    worst = {}
    for rows in (1, 5):
        x = N.ln_inputs(rows, C, cls)
        w, b = N.make_params(C, 1)
        dy = N.make_dy((rows, C), 2)
        r = N.ln_ref(x, w, b, 1e-6, dy)
        masks = [("last column", N.last_out_mask(rows, 1, C, ln=True))]
        masks += [(f"stripe of {wd}", N.stripe_out_mask(rows, 1, C, 1, wd)) for wd in (64, 128, 256)]
        for name, m in masks:
            if m is not None:
                mu = N.ln_ref(x, w, b, 1e-6, dy, stat_mask=m[:, 0, :])
                worst[name] = min(worst.get(name, 9e9), _need(name, mu["y"], r["y"], r["S_y"], N.CEILING["ln", "y"]))
        if C > 1:
            mu = N.ln_ref(x, w, b, 1e-6, dy, drop_s1=True)
            worst["s1"] = min(worst.get("s1", 9e9), _need("s1", mu["dx"], r["dx"], r["S_dx"], N.CEILING["ln", "dx"]))
    print(f"[ln C={C} {cls}] smallest mutant distance: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("cls", N.CLASSES)
@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=str)
def test_groupnorm_mutants_are_visible(shape, cls):
    B, P, C, G = shape
    x = N.gn_inputs(B, P, C, G, cls)
    w, b = N.make_params(C, 3)
    dy = N.make_dy((B, P, C), 4)
    seen = []
    for eps in (1e-5, 1e-6):
        r = N.gn_ref(x, G, w, b, eps, N.ACT_NONE, dy)
        for name, kw in (("last row", dict(stat_mask=N.last_out_mask(B, P, C))), ("stripe", dict(stat_mask=N.stripe_out_mask(B, P, C, G))),
                         ("group 63 for 64", dict(gidx=N.group_63_for_64(C, G)))):
            if next(iter(kw.values())) is not None:
                mu = N.gn_ref(x, G, w, b, eps, N.ACT_NONE, dy, **kw)
                seen.append((name, _need(name, mu["y"], r["y"], r["S_y"], N.CEILING["gn", "y"])))
        mu = N.gn_ref(x, G, w, b, eps, N.ACT_NONE, dy, drop_s1=True)
        seen.append(("s1", _need("s1", mu["dx"], r["dx"], r["S_dx"], N.CEILING["gn", "dx"])))
        for a in (N.ACT_GELU, N.ACT_RELU, N.ACT_QGELU):
            r = N.gn_ref(x, G, w, b, eps, a, dy)
            mu = N.gn_ref(x, G, w, b, eps, a, dy, drop_act_grad=True)
            if P * (C // G) >= 3:
                seen.append((f"act' {N.ACT_NAMES[a]}", _need("act'", mu["dx"], r["dx"], r["S_dx"], N.CEILING["gn", "dx"])))
            else:                                                               # sets of two: dx is pure cancellation either way; db sees it
                m = ((mu["db"] - r["db"]).abs() / r["abs_db"]).max().item()
                assert m >= 4 * N.CEILING["gn", "sums"], m
                seen.append((f"act' {N.ACT_NAMES[a]} (db)", m))
    print(f"[gn {shape} {cls}] mutant distances: " + ", ".join(f"{k} {v:.2e}" for k, v in seen))
    if shape == (1, 100, 128, 32):
        assert any(k == "group 63 for 64" for k, _ in seen)


@pytest.mark.parametrize("cls", N.CLASSES)
@pytest.mark.parametrize("shape", N.BN_SHAPES, ids=str)
def test_batchnorm_mutants_are_visible(shape, cls):
    rows, C = shape
    eps = 1e-5
    x = N.bn_inputs(rows, C, cls)
    w, b = N.make_params(C, 5)
    dy = N.make_dy((rows, C), 6)
    cy, cd = N.CEILING["bn", "y"], N.CEILING["bn", "dx"]
    seen = []
    r = N.bn_ref([x], w, b, eps, N.ACT_NONE, [dy])
    if rows >= 2:                                                               # the last row left out of both statistics
        mv = N.bn_mean_var(N.bn_sums(x[:-1])[0], rows - 1.0)
        seen.append(("last row", _need("last row", N.bn_apply(x, mv, w, b, eps, 0), r["y"][0], r["S_y"], cy)))
    if C > 64:                                                                  # the highest 64-channel strip never summed
        s = r["sums"].clone()
        s[:, (C - 1) // 64 * 64:] = 0
        seen.append(("stripe", _need("stripe", N.bn_apply(x, N.bn_mean_var(s, float(rows)), w, b, eps, 0), r["y"][0], r["S_y"], cy)))
    mu = N.bn_ref([x], w, b, eps, N.ACT_NONE, [dy], drop_s1=True)
    seen.append(("s1", _need("s1", mu["dx"][0], r["dx"][0], r["S_dx"], cd)))
    for a in (N.ACT_GELU, N.ACT_RELU, N.ACT_QGELU):
        ra = N.bn_ref([x], w, b, eps, a, [dy])
        mu = N.bn_ref([x], w, b, eps, a, [dy], drop_act_grad=True)
        if rows >= 3:
            seen.append((f"act' {N.ACT_NAMES[a]}", _need("act'", mu["dx"][0], ra["dx"][0], ra["S_dx"], cd)))
        else:                                                                   # one or two rows: dx is pure cancellation with or without act'; the sums see it
            m = ((mu["sums_dy"][0] - ra["sums_dy"][0]).abs() / ra["abs_sums_dy"][0]).max().item()
            assert m >= 4 * N.CEILING["bn", "sums"], m
            seen.append((f"act' {N.ACT_NAMES[a]} (sums_dy)", m))
    if shape in N.BN_SPLITS:                                                    # count / total_rows taken as the local row count
        cut = N.BN_SPLITS[shape]
        xs, dys = [x[:cut], x[cut:]], [dy[:cut], dy[cut:]]
        r2 = N.bn_ref(xs, w, b, eps, N.ACT_NONE, dys)
        mu = N.bn_ref(xs, w, b, eps, N.ACT_NONE, dys, count=cut)
        seen.append(("count", _need("count", mu["y"][0], r2["y"][0], r2["S_y"], cy)))
        mu = N.bn_ref(xs, w, b, eps, N.ACT_NONE, dys, total_rows=cut)
        seen.append(("total_rows", _need("total_rows", mu["dx"][0], r2["dx"][0], r2["S_dx"], cd)))
    print(f"[bn {shape} {cls}] mutant distances: " + ", ".join(f"{k} {v:.2e}" for k, v in seen))
