"""CPU pins of tests/attention_helpers.py: the hand-written backward equals float64 autograd, the token layout round-trips, a
kernel that rounds where the 16-bit kernels round stays inside the derived bounds, every mutant is visible at every case's shape
(a condition on the INPUTS: in at least 60 % of the rows a mutant changes, some element of the float64 reference moves by at
least 4 x its bound), and `form_of` puts every case of tests/test_attention_gpu.py and the backbones' shapes in the form it is
named for.  Printed with -s: the rounding-model ratios and the mutant shares."""
import pytest
import torch

from tests import attention_helpers as A

HALVES = [torch.bfloat16, torch.float16]
MIN_SHARE, FACTOR = 0.6, 4.0


def _name(dt):
    return {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dt]


def test_backward_by_hand_equals_autograd():
    shp = A.Shape(2, 2, 64, 70, 1, 37, 1)
    inp = A.make_inputs(shp, torch.bfloat16)
    q, k, v = (inp[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    o = torch.softmax(shp.scale * (q @ k.transpose(-1, -2)), -1) @ v
    o.backward(inp["do"])
    of, lse, P, s = A.forward_ref(inp["q"], inp["k"], inp["v"], shp.scale)
    assert torch.allclose(of, o.detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-14, atol=0) and torch.allclose(P.sum(-1), torch.ones_like(lse), atol=1e-13)
    dq, dk, dv, _, _ = A.backward_ref(inp["q"], inp["k"], inp["v"], of, lse, inp["do"], shp.scale)
    for got, want in ((dq, q.grad), (dk, k.grad), (dv, v.grad)):
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_token_layout_and_nan_checks():
    shp = A.Shape(2, 3, 64, 5, 1, 4, 0)
    x = torch.arange(2 * 3 * 6 * 64, dtype=torch.float64).reshape(2, 3, 6, 64)
    t = A.to_tokens(x, 5, 1)
    assert t.shape == (12, 192)
    # include/vfmseg_hip.h: patch token i of image b is row b*n_main + i, its [cls] token row B*n_main + b
    assert torch.equal(t[1 * 5 + 2, 64:128], x[1, 1, 2]) and torch.equal(t[2 * 5 + 1, 128:], x[1, 2, 5])
    assert torch.equal(A.from_tokens(t, 2, 3, 64, 5, 1), x)
    for packed in (False, True):
        ops = A.Operands(shp, torch.float32, "cpu", packed)
        ops.put(q=x, do=x, o=x)
        assert torch.equal(ops.get("q"), x) and A.outside_is_nan(ops.q)
        assert (ops.q.stride(0) == 3 * 192 + 8) == packed and ops.k.shape == (8, 192)
        assert not A.view_ok(ops.dq)                       # unwritten
        ops.dq.fill_(1.0), ops.dk.fill_(1.0), ops.dv.fill_(1.0)
        assert A.view_ok(ops.dq, ops.dk, ops.dv)
        if packed:
            ops.dq._base[0, 3 * 192] = 0.0                 # a write into the padding
            assert not A.view_ok(ops.dq, ops.dk, ops.dv) and not A.outside_is_nan(ops.dq)


@pytest.mark.parametrize("dt", HALVES, ids=_name)
def test_rounding_model_stays_inside_the_bounds(dt):
    shp = A.Shape(2, 2, 64, 200, 1, 200, 1)
    inp = A.make_inputs(shp, dt)
    q, k, v, do = inp["q"], inp["k"], inp["v"], inp["do"]
    ref = A.forward_ref(q, k, v, shp.scale)
    o16 = A.rnd(ref[0], dt)
    bref = A.backward_ref(q, k, v, o16, ref[1], do, shp.scale)
    b_o, _ = A.forward_bounds(q, k, v, shp.scale, dt, ref=ref)
    b_dq, b_dk, b_dv = A.backward_bounds(q, k, v, o16, ref[1], do, shp.scale, dt, ref=bref)
    model = A.rounding_model(inp, shp.scale, dt)
    ratios = {n: A.worst_ratio(model[n], r, b) for n, r, b in (("o", ref[0], b_o), ("dq", bref[0], b_dq), ("dk", bref[1], b_dk),
                                                                ("dv", bref[2], b_dv))}
    print(f"[attn-cpu] rounding model {_name(dt)} {shp}: worst err/bound " + " ".join(f"{n} {r:.2f}" for n, r in ratios.items()))
    assert all(0.05 < r <= 1.0 for r in ratios.values()), ratios     # inside, and the bound is not slack by more than 20 x


def _all_cases():
    out = []
    for table, f32 in ((A.FWD_CASES, False), (A.BWD_CASES, False), (A.CHAIN_CASES, False), (A.F32_CASES, True)):
        for name, case in table.items():
            out.append(pytest.param(name, case, f32, id=name))
    return out


_SEEN = {}


def _shares(case, dt, f32):
    """{mutant: {output: share}} at one shape and storage type (cached: several cases share a shape)"""
    shp = case["shape"]
    key = (shp.key(), dt, f32)
    if key in _SEEN:
        return _SEEN[key]
    inp = A.make_inputs(shp, dt if dt != torch.float32 else torch.bfloat16)
    q, k, v, do = inp["q"], inp["k"], inp["v"], inp["do"]
    ref = A.forward_ref(q, k, v, shp.scale)
    o16 = A.rnd(ref[0], dt)
    bref = A.backward_ref(q, k, v, o16, ref[1], do, shp.scale)
    f32_path = f32 or shp.d != 64
    bounds = dict(zip(("dq", "dk", "dv"), A.backward_bounds(q, k, v, o16, ref[1], do, shp.scale, dt, f32_path=f32_path, ref=bref)))
    bounds["o"] = A.forward_bounds(q, k, v, shp.scale, dt, f32_path=f32_path, ref=ref)[0]
    refs = {"o": ref[0], "dq": bref[0], "dk": bref[1], "dv": bref[2]}
    res = {}
    for mname, outs in A.mutants(shp, inp, o16, ref[1]).items():
        res[mname] = {n: A.visible_share(m, refs[n], bounds[n], FACTOR) for n, m in outs.items()}
    _SEEN[key] = res
    return res


@pytest.mark.parametrize("name,case,f32", _all_cases())
def test_every_mutant_is_visible(name, case, f32):
    dts = [torch.float32, torch.bfloat16] if case["shape"].d != 64 else ([torch.float32] if f32 else HALVES)
    for dt in dts:
        res = _shares(case, dt, f32)
        kinds = {}
        for mname, outs in res.items():
            kind = mname.rstrip("0123456789")
            for n, share in outs.items():
                lo, hi = kinds.get((kind, n), (1.0, 0.0))
                kinds[(kind, n)] = (min(lo, share), max(hi, share))
        print(f"[attn-cpu] mutants {name} {_name(dt)} {case['shape']}: "
              + " ".join(f"{k}/{n} {lo:.2f}..{hi:.2f}" for (k, n), (lo, hi) in sorted(kinds.items())))
        for mname, outs in res.items():
            for n, share in outs.items():
                assert share >= MIN_SHARE, (name, _name(dt), mname, n, share)


def test_form_of_cases_and_backbones():
    for table in (A.FWD_CASES, A.BWD_CASES, A.CHAIN_CASES):
        for name, case in table.items():
            f = A.landed(case)
            assert f["path"] == "mfma", name
    for name, case in A.F32_CASES.items():
        A.landed(case, half=False)
    assert A.form_of(A.F32_CASES["X3-d80"]["shape"], half=True)["path"] == "f32"          # 16-bit storage, d = 80
    assert A.form_of(A.Shape(2, 2, 64, 64, 0, 64, 0), half=False)["path"] == "f32"
    # xcd_map needs the knob and a pair count that is a multiple of eight
    assert not A.form_of(A.FWD_CASES["F7"]["shape"], short_grid=0, xcd=0)["xcd_map"]
    # the backbones at the default threshold: 1024 + 1 and 1369 + 1 tokens with 32 pairs run 4-wave kernels, the light [cls] block
    # and the scratch path exist only where n_main % 128 == 0; 2048 + 1 is over ATTN_EXTRA_MAX: no light block
    for B, H, n in A.BACKBONE_SHAPES:
        f = A.form_of(A.Shape(B, H, 64, n, 1, n, 1))
        blocks = -(-(n + 1) // 128) * B * H
        assert f["fwd_waves"] == (2 if blocks < 256 else 4) and f["xcd_map"]
        four = f["fwd_waves"] == 4
        assert f["r1"] == four and f["cls"] == (four and n % 128 == 0)
        assert f["light"] == (four and n % 128 == 0 and n + 1 <= A.ATTN_EXTRA_MAX)
        assert f["dq_waves"] == f["dkv_waves"] == f["fwd_waves"]
        if n == 2048 and four:
            assert f["cls_query_alone"] and not f["light"]
        if n == 1369 and four:
            assert f["fwd_k_tail"] and f["fwd_q_ragged"] and not f["cls"] and not f["dq_r1"]
