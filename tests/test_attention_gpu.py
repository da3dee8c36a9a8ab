"""vfm_attn_fwd / vfm_attn_bwd against float64, element by element, over every dispatch form of csrc/attention_bf16.hip and the
tile edges of csrc/attention_f32.hip.  References, bounds, inputs, mutants and the case tables live in
tests/attention_helpers.py (pinned on the CPU by tests/test_attention_cpu.py).

Every case asserts: max |got - ref| / bound <= 1 per element and output; every element of a view finite and every element outside
it still NaN; the lse bound per row; the dispatch form it is named for (`form_of` at the knobs the case sets).  Every case runs
twice: separate contiguous operands, then q | k | v and dq | dk | dv as column slices of packed buffers with a padded leading
dimension.  The 16-bit type is the loaded library's (u16 follows it): tests/test_fp16_twin_gpu.py runs this file against the fp16
twin.  One line per run: [attn-bound] <case> <form> worst err/bound per output (profiles/attention_bounds.log).

The exp2 allowance is tests/test_elementwise_gpu._allowances (ATen float32 exp2 on the GPU against float64, doubled); the log
allowance is measured the same way here, in units of 2^-23 max(1, |log l|) over l in [1, 2^20]."""
import contextlib
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import attention_helpers as A  # noqa: E402
from tests.test_elementwise_gpu import _allowances  # noqa: E402
from vfmseg_amd import ops  # noqa: E402

DEV = "cuda"
F32 = torch.float32
DEFAULTS = {"attn_short_grid": 256, "attn_il": 3, "attn_xcd": 1}     # csrc/attention_bf16.hip
_LOG = {}


@contextlib.contextmanager
def knobs(**kv):
    try:
        for key, val in kv.items():
            ops.tune(key, val)
        yield
    finally:
        for key in kv:
            ops.tune(key, DEFAULTS[key])


def _allow():
    """{"exp2", "log"}: twice the worst error of ATen's float32 exp2 / log on the GPU against float64"""
    if not _LOG:
        l = torch.cat((torch.logspace(0, 20, 20 * 512 + 1, base=2.0), 1.0 + torch.arange(1, 4097) * 2.0 ** -12)).float()
        l32, l64 = torch.log(l.to(DEV)).cpu().double(), torch.log(l.double())
        worst = ((l32 - l64).abs() / (2 * A.U * l64.abs().clamp_min(1.0))).max().item()
        _LOG.update(worst=worst, log=2 * worst)
    return {"exp2": _allowances()[1], "log": _LOG["log"]}


def test_log_allowance():
    a = _allow()
    print(f"[attn-bound] allowances: exp2 {a['exp2']:.3f}, log worst {_LOG['worst']:.3f} -> {a['log']:.3f} (units of 2^-23, ATen float32 on the "
          f"GPU against float64); 16-bit type {A.half_dtype()}")
    assert 0 < a["exp2"] < 16 and 0 < a["log"] < 16


@functools.lru_cache(maxsize=None)
def _reference(key, dt, f32_path):
    """Inputs, float64 references and bounds of one shape, computed once (the backward's o is the rounded float64 output, its lse
    the float32 of the float64 lse: independent of the forward kernel)."""
    shp = A.Shape(*key)
    inp = A.make_inputs(shp, A.half_dtype())
    q, k, v, do = inp["q"], inp["k"], inp["v"], inp["do"]
    fwd = A.forward_ref(q, k, v, shp.scale)
    o_in, lse_in = A.rnd(fwd[0], dt), fwd[1].float()
    bwd = A.backward_ref(q, k, v, o_in, lse_in.double(), do, shp.scale)
    b_o, b_lse = A.forward_bounds(q, k, v, shp.scale, dt, allow=_allow(), f32_path=f32_path, ref=fwd)
    b_dq, b_dk, b_dv = A.backward_bounds(q, k, v, o_in, fwd[1], do, shp.scale, dt, allow=_allow(), f32_path=f32_path, ref=bwd)
    return {"shp": shp, "inp": inp, "o_in": o_in, "lse_in": lse_in,
            "ref": {"o": fwd[0], "lse": fwd[1], "dq": bwd[0], "dk": bwd[1], "dv": bwd[2]},
            "bound": {"o": b_o, "lse": b_lse, "dq": b_dq, "dk": b_dk, "dv": b_dv}}


def _args(shp):
    return (shp.B, shp.H, shp.d, shp.nq_main, shp.nq_extra, shp.nk_main, shp.nk_extra, shp.scale)


def _fwd(R, dt, packed):
    """One ops.attn_fwd on fresh operands -> (Operands, {"o", "lse": float64 on the CPU})"""
    shp = R["shp"]
    op = A.Operands(shp, dt, DEV, packed)
    op.put(q=R["inp"]["q"], k=R["inp"]["k"], v=R["inp"]["v"])
    ops.attn_fwd(op.q, op.k, op.v, op.o, op.lse, *_args(shp))
    torch.cuda.synchronize()
    assert A.view_ok(op.o), (shp, "o: unwritten elements or a write outside the view")
    assert bool(torch.isfinite(op.lse).all()), (shp, "lse: unwritten rows")
    return op, {"o": op.get("o"), "lse": op.lse.cpu().double()}


def _bwd(R, dt, packed, op=None):
    """One ops.attn_bwd; op: the operands of a forward call to chain onto (its o and lse), else the reference's -> (Operands, outputs)"""
    shp = R["shp"]
    if op is None:
        op = A.Operands(shp, dt, DEV, packed)
        op.put(q=R["inp"]["q"], k=R["inp"]["k"], v=R["inp"]["v"], o=R["o_in"])
        op.lse.copy_(R["lse_in"])
    op.put(do=R["inp"]["do"])
    ops.attn_bwd(op.q, op.k, op.v, op.o, op.lse, op.do, op.dq, op.dk, op.dv, *_args(shp))
    torch.cuda.synchronize()
    assert A.view_ok(op.dq, op.dk, op.dv), (shp, "dq / dk / dv: unwritten elements or a write outside the views")
    return op, {n: op.get(n) for n in ("dq", "dk", "dv")}


def _judge(case, form, layout, got, ref, bound):
    """Prints the report line and asserts every output's worst err / bound <= 1."""
    ratios = {n: A.worst_ratio(g, ref[n], bound[n]) for n, g in got.items()}
    print(f"[attn-bound] {case} {layout} {form}: " + " ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    assert all(r <= 1.0 for r in ratios.values()), (case, layout, form, ratios)
    return ratios


def _form(case, half=True, xcd=1):
    return A.landed(case, half=half, xcd=xcd)


LAYOUTS = ((False, "separate"), (True, "packed"))


# ------------------------------------------------------------------------------------------------------------ forward, 16-bit path
@pytest.mark.parametrize("name", [n for n in A.FWD_CASES if n != "F7"])
def test_forward(name):
    case, dt = A.FWD_CASES[name], A.half_dtype()
    R = _reference(case["shape"].key(), dt, False)
    form = A.form_name(_form(case))
    with knobs(attn_short_grid=case["short_grid"]):
        for packed, layout in LAYOUTS:
            _, got = _fwd(R, dt, packed)
            _judge(name, form, layout, got, R["ref"], R["bound"])


def test_short_grid_knob_switches_the_kernels():
    """The forms above are named from `form_of`, a restatement; this is the evidence that the knob reaches the dispatcher: the 4-wave
    forward keeps P of the [cls] key in fp32 (rank-1 form), the 2-wave forward rounds it with its tile, so the two runs of one shape
    cannot agree in every bit - and both are inside the bound (test_forward: F6a, F6a-2w)."""
    dt = A.half_dtype()
    R = _reference(A.FWD_CASES["F6a"]["shape"].key(), dt, False)
    outs = []
    for name in ("F6a", "F6a-2w"):
        with knobs(attn_short_grid=A.FWD_CASES[name]["short_grid"]):
            outs.append(_fwd(R, dt, False)[1]["o"])
    assert not torch.equal(outs[0], outs[1])


def test_forward_request_order_and_block_order_change_no_bit():
    """F7: attn_il moves the next tile's requests, attn_xcd the block order; the forward has no atomics -> the same bits."""
    case, dt = A.FWD_CASES["F7"], A.half_dtype()
    R = _reference(case["shape"].key(), dt, False)
    outs = []
    for il in (0, 3):
        for xcd in (0, 1):
            f = _form(case, xcd=xcd)
            assert f["xcd_map"] == bool(xcd)
            form = A.form_name(f)
            with knobs(attn_short_grid=case["short_grid"], attn_il=il, attn_xcd=xcd):
                for packed, layout in LAYOUTS:
                    _, got = _fwd(R, dt, packed)
                    _judge(f"F7 il={il} xcd={xcd}", form, layout, got, R["ref"], R["bound"])
                    outs.append(got)
    for got in outs[1:]:
        assert torch.equal(got["o"], outs[0]["o"]) and torch.equal(got["lse"], outs[0]["lse"])


# ------------------------------------------------------------------------------------------------------------ backward, 16-bit path
@pytest.mark.parametrize("name", list(A.BWD_CASES))
def test_backward(name):
    case, dt = A.BWD_CASES[name], A.half_dtype()
    R = _reference(case["shape"].key(), dt, False)
    form = A.form_name(_form(case), bwd=True)
    with knobs(attn_short_grid=case["short_grid"]):
        for packed, layout in LAYOUTS:
            _, got = _bwd(R, dt, packed)
            _judge(name, form, layout, got, R["ref"], R["bound"])


def test_backward_cls_scratch_is_left_zeroed_and_rows_repeat():
    """B2: the 192 B H scratch floats behind delta are zero after the call; a second call repeats every non-[cls] row bit for bit;
    the [cls] rows (fp32 atomics, no fixed order: cls_partial) agree within 2 u16 of their row's magnitude."""
    case, dt = A.BWD_CASES["B2"], A.half_dtype()
    shp = case["shape"]
    R = _reference(shp.key(), dt, False)
    assert _form(case)["cls"]
    u16 = A.u16_of(dt)
    with knobs(attn_short_grid=case["short_grid"]):
        op, first = _bwd(R, dt, True)
        ws = ops._attn_bwd_delta(op.q, shp.B, shp.H, shp.nq)
        scratch = ws[shp.B * shp.H * shp.nq:]
        assert scratch.numel() == 192 * shp.B * shp.H and bool((scratch == 0).all())
        _, second = _bwd(R, dt, True)
        torch.cuda.synchronize()
        assert bool((scratch == 0).all())
    worst = 0.0
    for n in ("dq", "dk", "dv"):
        a, b = first[n], second[n]
        assert torch.equal(a[:, :, :shp.nq_main], b[:, :, :shp.nq_main]), n
        ca, cb = a[:, :, shp.nq_main], b[:, :, shp.nq_main]
        mag = torch.maximum(ca.abs(), cb.abs()).amax(-1, keepdim=True)
        worst = max(worst, ((ca - cb).abs() / (2 * u16 * mag)).max().item())
    print(f"[attn-bound] B2 second call: non-[cls] rows bit-identical, [cls] rows differ by {worst:.3f} of 2 u16 |row|")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(A.CHAIN_CASES))
def test_forward_then_backward(name):
    """B5: the backward on the forward kernel's own o and lse, as the backbones run it.  delta is taken from that o; P is the float64
    softmax, and the forward's lse bound enters the backward's bound as the error of the lse handed in."""
    case, dt = A.CHAIN_CASES[name], A.half_dtype()
    shp = case["shape"]
    R = _reference(shp.key(), dt, False)
    f = _form(case)
    inp = R["inp"]
    with knobs(attn_short_grid=case["short_grid"]):
        for packed, layout in LAYOUTS:
            op, got = _fwd(R, dt, packed)
            _judge(name, A.form_name(f), layout, got, R["ref"], R["bound"])
            o_k = got["o"]
            ref = A.backward_ref(inp["q"], inp["k"], inp["v"], o_k, R["ref"]["lse"], inp["do"], shp.scale)
            bound = A.backward_bounds(inp["q"], inp["k"], inp["v"], o_k, R["ref"]["lse"], inp["do"], shp.scale, dt, allow=_allow(),
                                      lse_err=R["bound"]["lse"], ref=ref)
            _, grads = _bwd(R, dt, packed, op=op)
            _judge(name, A.form_name(f, bwd=True), layout, grads, dict(zip(("dq", "dk", "dv"), ref[:3])), dict(zip(("dq", "dk", "dv"), bound)))


# ------------------------------------------------------------------------------------------------------------ fp32 path
@pytest.mark.parametrize("name", ["X1", "X2"])
def test_f32_path(name):
    case = A.F32_CASES[name]
    R = _reference(case["shape"].key(), F32, True)
    _form(case, half=False)
    for packed, layout in LAYOUTS:
        _, got = _fwd(R, F32, packed)
        _judge(name, "f32 fwd", layout, got, R["ref"], R["bound"])
        _, grads = _bwd(R, F32, packed)
        _judge(name, "f32 bwd", layout, grads, R["ref"], R["bound"])


@pytest.mark.parametrize("storage", ["fp32", "half"])
def test_f32_path_head_dim_80_forward(storage):
    case = A.F32_CASES["X3-d80"]
    dt = F32 if storage == "fp32" else A.half_dtype()
    R = _reference(case["shape"].key(), dt, True)
    _form(case, half=dt != F32)
    for packed, layout in LAYOUTS:
        _, got = _fwd(R, dt, packed)
        _judge("X3-d80", f"f32 fwd {storage} storage", layout, got, R["ref"], R["bound"])


# ------------------------------------------------------------------------------------------------------------ the comparison itself
def test_comparison_rejects_every_mutant():
    """The verdict helper of this file, fed the kernel's results and a MUTATED float64 reference, must say no for every mutant and
    every output it changes (nothing on the GPU is made to misbehave); with the true reference it says yes."""
    dt = A.half_dtype()
    case = A.BWD_CASES["B1"]
    shp = case["shape"]
    R = _reference(shp.key(), dt, False)
    with knobs(attn_short_grid=case["short_grid"]):
        _, got = _fwd(R, dt, False)
        _, grads = _bwd(R, dt, False)
    got.update(grads)
    for n in ("o", "dq", "dk", "dv"):
        assert A.within(got[n], R["ref"][n], R["bound"][n]), n
    muts = A.mutants(shp, R["inp"], R["o_in"], R["ref"]["lse"])
    assert {m.rstrip("0123456789") for m in muts} == {"drop_key", "drop_query", "other_image_cls", "next_head"}
    for mname, outs in muts.items():
        for n, mref in outs.items():
            assert not A.within(got[n], mref, R["bound"][n]), (mname, n)
