"""clip_grad / accumulative_counts on the device: vfm_grad_norm against float64, the clipped fused AdamW against torch.optim.AdamW after
clip_grad_norm_ / clip_grad_value_, and the wrappers end to end (plain, piecewise, accumulating, under the loss scaler, in Runner.train)."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")

# ---------------------------------------------------------------------------------------------------------------- 1: ops.grad_norm
GRID_STRIDE = 2048 * 256 * 4                       # floats per grid stride of the float4 path (csrc/gradnorm.hip: GN_GRID blocks x 256 x 4)
SIZES = [0, 1, 3, 255, 4097, GRID_STRIDE + 5]     # the last: a second stride with one active vector, plus a one-element tail
REL = 1e-5


def _chain(n, vec):
    """the longest per-thread fp32 chain csrc/gradnorm.hip states"""
    return 4 * math.ceil(n / 2 ** 21) + 1 if vec else math.ceil(n / 2 ** 19)


def test_the_tolerance_covers_the_fp32_chain_of_the_grid():
    # per-thread fp32 chain, one rounding of each square, then 8 + 11 tree levels (those are in double: counted anyway)
    for n in SIZES:
        for vec in (True, False):
            assert (_chain(n, vec) + 1 + 19) * 2.0 ** -24 < REL
    assert (_chain(16_600_000, True) + 1 + 19) * 2.0 ** -24 < REL      # the dinov2_ms_masked buffer


@pytest.fixture(scope="module")
def buffers():
    """size -> (device buffer with one float of slack in front, float64 CPU copy of it), built once and never written"""
    out = {}
    for n in SIZES:
        cpu = torch.randn(n + 1, generator=torch.Generator().manual_seed(100 + n % 97))
        out[n] = (cpu.to(DEV), cpu.double())
    return out


def _ref(x64, kind):
    if x64.numel() == 0:
        return 0.0
    return torch.linalg.vector_norm(x64, kind).item()


@pytest.mark.parametrize("kind", [2, 1, INF])
def test_grad_norm_against_float64(buffers, kind):
    from vfmseg_amd import ops
    amp = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=DEV)
    ws = torch.empty(4096, dtype=torch.float64, device=DEV)
    for n in SIZES:
        dev, cpu = buffers[n]
        for shift in (0, 1):                 # 16-byte aligned start (float4 path) / shifted by one float (scalar path)
            g, g64 = dev[shift:shift + n], cpu[shift:shift + n]
            assert n == 0 or (g.data_ptr() % 16 == 0) == (shift == 0)
            ref = _ref(g64, kind)
            for pre, amp_state, s in ((0.5, None, 0.5), (1.0, amp, 1.0 / 1024.0)):
                want = ref * s
                for max_norm in (want / 2, 1e30):
                    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
                    st = ops.grad_norm(g, kind, max_norm, pre, amp_state, None, flag, ws).clone()
                    st2 = ops.grad_norm(g, kind, max_norm, pre, amp_state, None, None, ws)
                    assert torch.equal(st, st2), (n, shift, kind)          # a second call: identical bits
                    tn, coef = st[0].item(), st[1].item()
                    assert flag.item() == 0 and st[2].item() == 0 and st[3].item() == 0
                    if kind == INF:          # exact up to the one multiply by the pre-scale
                        assert tn == torch.tensor(want, dtype=torch.float64).float().item(), (n, shift, tn, want)
                    else:
                        assert abs(tn - want) <= REL * want, (n, shift, kind, tn, want)
                    if n == 0:
                        assert tn == 0.0 and coef == 1.0
                    elif max_norm == 1e30:
                        assert coef == 1.0
                    else:                    # torch: clamp(max_norm / (total + 1e-6), max=1) in fp32
                        tc = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (st[0].cpu() + 1e-6), max=1.0).item()
                        assert abs(coef - tc) <= 1e-6 * tc and coef < 1.0, (n, shift, coef, tc)


@pytest.mark.parametrize("kind", [2, 1, INF])
@pytest.mark.parametrize("poison", [float("nan"), INF, -INF])
def test_grad_norm_flags_a_non_finite_element(buffers, kind, poison):
    from vfmseg_amd import ops
    for n, at in ((4097, 4000), (4097, 4096), (GRID_STRIDE + 5, GRID_STRIDE + 4), (GRID_STRIDE + 5, GRID_STRIDE + 1)):
        for shift in (0, 1):
            g = buffers[n][0][shift:shift + n].clone()
            g[at] = poison
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            st = ops.grad_norm(g, kind, 1.0, 1.0, None, None, flag)
            assert flag.item() == 1 and not math.isfinite(st[0].item()), (n, at, shift, st.tolist())


# ---------------------------------------------------------------------------------------------------------------- 2: clipped AdamW
def _rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# Bound on the second moment.  The kernel forms 1 - beta2 in fp32 from float(0.999), which is off 0.999 by up to half an ulp, 2^-25:
# relative to 1 - beta2 = 1e-3 that is up to 3e-5 on every term of v (torch forms 1 - beta2 in double).  On top of it the 1e-5 of the
# parameters.  (1 - beta1 = 0.1 is off by at most 3e-7: the first moment keeps the plain bound.)
V_REL = 1e-5 + 2.0 ** -25 / (1 - 0.999)


def _adamw_setup(n, cut=6000):
    p, g = _rnd(n, 58), _rnd(n, 59)
    q1, q2 = p[:cut].clone().requires_grad_(True), p[cut:].clone().requires_grad_(True)
    opt = torch.optim.AdamW([dict(params=[q1], weight_decay=0.05, lr=1e-3), dict(params=[q2], weight_decay=0.0, lr=2e-3)])
    dev = dict(p=p.to(DEV), m=torch.zeros(n, device=DEV), v=torch.zeros(n, device=DEV),
               seg=torch.tensor([0, cut], dtype=torch.int64, device=DEV), lrm=torch.tensor([1.0, 2.0], device=DEV),
               wd=torch.tensor([0.05, 0.0], device=DEV))
    return g, (q1, q2), opt, dev, cut


@pytest.mark.parametrize("vec4", [True, False])
@pytest.mark.parametrize("kind", [2, INF])
def test_clipped_adamw_against_torch_after_clip_grad_norm(vec4, kind):
    """test_adamw's layout (two segments, three steps, gradients handed over 4x too large with grad_scale 0.25) and its bound on the
    parameters.  AdamW's update is nearly invariant to the gradient's scale, so the moments - which carry the three coefficients
    directly - are held to the same bound."""
    from vfmseg_amd import ops
    n = 10000 + (0 if vec4 else 3)
    g, (q1, q2), opt, d, cut = _adamw_setup(n)
    max_norm = 150.0 if kind == 2 else 5.0        # |g| ~ 100 (2-norm) / ~ 4 (max) at step 1: unclipped, then clipped twice
    coefs = []
    for step in (1, 2, 3):
        q1.grad, q2.grad = g[:cut].clone() * step, g[cut:].clone() * step
        total = torch.nn.utils.clip_grad_norm_([q1, q2], max_norm, norm_type=kind)
        opt.step()
        gd = (g * step * 4.0).to(DEV)
        st = ops.grad_norm(gd, kind, max_norm, pre_scale=0.25)
        ops.adamw(d["p"], gd, d["m"], d["v"], d["seg"], d["lrm"], d["wd"], 1e-3, (0.9, 0.999), 1e-8, step, grad_scale=0.25, zero_grad=True,
                  vec4=vec4, clip_coef=st[1:2])
        assert gd.abs().sum().item() == 0
        assert abs(st[0].item() - total.item()) <= 1e-5 * total.item()
        coefs.append(st[1].item())
    assert coefs[0] == 1.0 and coefs[2] < coefs[1] < 1.0
    assert _relerr(d["p"], torch.cat([q1, q2])) < 1e-5
    assert _relerr(d["m"], torch.cat([opt.state[q]["exp_avg"] for q in (q1, q2)])) < 1e-5
    assert _relerr(d["v"], torch.cat([opt.state[q]["exp_avg_sq"] for q in (q1, q2)])) < V_REL


@pytest.mark.parametrize("vec4", [True, False])
@pytest.mark.parametrize("guarded", [False, True])
def test_a_coefficient_of_one_changes_no_bit(vec4, guarded):
    from vfmseg_amd import ops
    n = 10000 + (0 if vec4 else 3)
    g, _, _, a, _ = _adamw_setup(n)
    _, _, _, b, _ = _adamw_setup(n)
    one = torch.ones(1, device=DEV)
    kw = dict(skip=torch.zeros(1, dtype=torch.int32, device=DEV), amp_state=torch.tensor([4.0, 0.0, 0.0, 0.0], device=DEV)) if guarded else {}
    for step in (1, 2, 3):
        ga, gb = (g * step * 4.0).to(DEV), (g * step * 4.0).to(DEV)
        ops.adamw(a["p"], ga, a["m"], a["v"], a["seg"], a["lrm"], a["wd"], 1e-3, (0.9, 0.999), 1e-8, step, grad_scale=0.25, zero_grad=True, vec4=vec4, **kw)
        ops.adamw(b["p"], gb, b["m"], b["v"], b["seg"], b["lrm"], b["wd"], 1e-3, (0.9, 0.999), 1e-8, step, grad_scale=0.25, zero_grad=True, vec4=vec4,
                  clip_coef=one, clip_value=0.0, **kw)
        if guarded:
            kw["amp_state"][2] += 1
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k]), k
    assert a["p"].ne(_rnd(n, 58).to(DEV)).any()


@pytest.mark.parametrize("vec4", [True, False])
def test_clip_value_against_clip_grad_value(vec4):
    from vfmseg_amd import ops
    n = 10000 + (0 if vec4 else 3)
    g, (q1, q2), opt, d, cut = _adamw_setup(n)
    for step in (1, 2, 3):
        q1.grad, q2.grad = g[:cut].clone() * step, g[cut:].clone() * step
        torch.nn.utils.clip_grad_value_([q1, q2], 1.5)
        opt.step()
        gd = (g * step * 4.0).to(DEV)
        ops.adamw(d["p"], gd, d["m"], d["v"], d["seg"], d["lrm"], d["wd"], 1e-3, (0.9, 0.999), 1e-8, step, grad_scale=0.25, zero_grad=False,
                  vec4=vec4, clip_value=1.5)
    assert (g.abs() > 1.5).sum() > 500 and (g.abs() < 0.5).sum() > 500
    assert _relerr(d["p"], torch.cat([q1, q2])) < 1e-5
    # the second moment is where a clamp that came too late (or not at all) shows: v = sum of (clamped g)^2 terms
    qv = torch.cat([opt.state[q]["exp_avg_sq"] for q in (q1, q2)])
    assert _relerr(d["v"], qv) < V_REL


# ---------------------------------------------------------------------------------------------------------------- 3-5: end to end
def _build(wrapper_type="OptimWrapper", **keys):
    """tests/test_amp_gpu.py::_run's setting in f32 mode: depth 4, dropout off, fixed crop box and keep mask"""
    import vfmseg_amd  # noqa: F401
    from tests.helpers import full_state_dict
    from vfmseg_amd import functional as Fh
    from vfmseg_amd import presets
    from vfmseg_amd.optim import PEFTOptimWrapperConstructor
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import MODELS
    set_compute_dtype("f32")
    Fh.manual_seed(4321)
    torch.manual_seed(0)
    depth = 4
    cfg = presets.dinov2_ms_masked(depth=depth)
    cfg["backbone"]["backbone"]["out_indices"] = [0, 1, 2, 3]
    model = MODELS.build(cfg)
    model.load_state_dict(full_state_dict(depth=depth))
    model = model.cuda().train()
    for m in model.modules():
        if hasattr(m, "dropout_ratio"):
            m.dropout_ratio = 0.0
        if hasattr(m, "p") and isinstance(getattr(m, "p"), float):
            m.p = 0.0
    oc = presets.optim_cfg()
    ocw = dict(oc["optim_wrapper"], type=wrapper_type, **keys)
    if wrapper_type == "AmpOptimWrapper":
        ocw["loss_scale"] = "dynamic"
    return model, PEFTOptimWrapperConstructor(ocw)(model, oc["param_scheduler"])


def _batch(model, step, poison=False, same=False):
    from vfmseg_amd.segmentors import SegDataSample
    from vfmseg_amd.synth import synth_image, synth_label
    seed = 500 + (0 if same else step)
    keep = torch.rand(3, 2, 1, 32, 32, generator=torch.Generator().manual_seed(12)) > 0.2
    imgs, labs = synth_image(2, 1024, seed=seed).cuda(), synth_label(2, 1024, seed=seed)
    model.fixed_crop_box = (256, 768, 128, 640)
    model.aux_decoder.transformer_decoder.fixed_keep = keep[0 if same else step]
    if poison:
        imgs[0, 0, 5, 5] = float("nan")
    return dict(inputs=imgs, data_samples=[SegDataSample(gt_sem_seg=labs[k]) for k in range(2)])


def _state(model):
    torch.cuda.synchronize()
    return {k: v.detach().float().cpu() for k, v in model.state_dict().items() if "lora_" in k or not k.startswith("backbone.")}


def _worst(a_state, b_state):
    """tests/test_amp_gpu.py::_worst: trainable parameters, BatchNorm running statistics left out"""
    worst, where = 0.0, None
    for k, a in a_state.items():
        if "running_" in k or "num_batches" in k or k == "decode_head.output_upscaling.0.bias":
            continue
        d = (a - b_state[k]).abs().mean().item() / max(a.abs().mean().item(), 1e-12)
        if d > worst:
            worst, where = d, k
    return worst, where


def _train(steps=2, wrapper_type="OptimWrapper", poison_at=None, same=False, **keys):
    model, ow = _build(wrapper_type, **keys)
    for step in range(steps):
        model.train_step(_batch(model, step, poison_at == step, same), ow)
    return model, ow


class _Snapshot:
    """update_params with a copy of the gradient buffer taken between backward and step (the copy changes nothing else)"""

    def __init__(self, ow):
        self.ow, self.snaps = ow, []
        ow._backward = self._backward
        self._inner = type(ow)._backward

    def _backward(self, loss):
        self._inner(loss)
        self.snaps.append(self.ow.optimizer.gflat.clone())


@pytest.fixture(scope="module")
def plain():
    """the plain wrapper: state after 1 step, flat parameters after 2, float64 norms of both steps' gradients (shared; never written)"""
    from vfmseg_amd.precision import set_compute_dtype
    try:
        model, ow = _build()
        snap = _Snapshot(ow)
        model.train_step(_batch(model, 0), ow)
        one = _state(model)
        model.train_step(_batch(model, 1), ow)
        torch.cuda.synchronize()
        return dict(one=one, flat=ow.optimizer.flat.clone(), norms=[g.double().norm().item() for g in snap.snaps])
    finally:
        set_compute_dtype("bf16")


@pytest.fixture(autouse=True)
def _back_to_bf16():
    yield
    from vfmseg_amd.precision import set_compute_dtype
    set_compute_dtype("bf16")


class _Piecewise:
    """train_step's update_params through the piecewise surface (what DACS uses), with a snapshot of the gradients before the step"""

    def __init__(self, ow):
        self.ow, self.snaps = ow, []

    def update_params(self, loss):
        self.ow.backward(self.ow.scale_loss(loss))
        self.snaps.append(self.ow.optimizer.gflat.clone())
        self.ow.step()
        self.ow.zero_grad()


def test_end_to_end_clipping_in_f32_mode(plain):
    model, ow = _train(2, clip_grad=dict(max_norm=1e30))
    torch.cuda.synchronize()
    assert torch.equal(ow.optimizer.flat, plain["flat"])          # a coefficient of 1: bit-identical to the plain wrapper
    g0 = ow.grad_norm()
    assert abs(g0 - plain["norms"][1]) <= 1e-5 * g0, (g0, plain["norms"])
    # clipped, through backward / step / zero_grad, against float64 AdamW on the clipped snapshots
    model, ow = _build(clip_grad=dict(max_norm=g0 / 2))
    opt = ow.optimizer
    pw = _Piecewise(ow)
    p = opt.flat.double().cpu()
    lr_mult, wd = torch.zeros_like(p), torch.zeros_like(p)
    offs = opt.offsets
    for i in range(len(opt.names)):
        lr_mult[offs[i]:offs[i + 1]] = float(opt.seg_lr[i])
        wd[offs[i]:offs[i + 1]] = float(opt.seg_wd[i])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    b1, b2 = opt.betas
    for step in range(2):
        model.train_step(_batch(model, step), pw)
        g = pw.snaps[-1].double().cpu()
        total = g.norm().item()
        assert abs(ow.grad_norm() - total) <= 1e-5 * total, (ow.grad_norm(), total)
        if step == 1:
            assert total > g0 / 2                                   # the clip was active (g0 is this step's norm in the unclipped run)
        g = g * min(1.0, (g0 / 2) / (total + 1e-6))
        lr = ow.scheduler.lr(step) * lr_mult
        t = step + 1
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p * (1 - lr * wd) - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + opt.eps)
    assert ow.iter == 2 and opt.step_count == 2 and opt.gflat.abs().sum().item() == 0
    assert _relerr(opt.flat, p) < 1e-5


def test_accumulation_in_f32_mode():
    """two update_params with accumulative_counts=2 on the same batch = one plain step on that batch (halving is exact, backward is
    linear in the incoming gradient: only the order of the fp32 atomics differs)"""
    model, ow = _train(1, same=True)
    want = _state(model)
    model, ow = _build(accumulative_counts=2)
    opt = ow.optimizer
    flat0 = opt.flat.clone()
    model.train_step(_batch(model, 0, same=True), ow)
    torch.cuda.synchronize()
    assert torch.equal(opt.flat, flat0) and opt.gflat.abs().sum().item() > 0 and opt.step_count == 0 and ow.iter == 1
    model.train_step(_batch(model, 1, same=True), ow)
    torch.cuda.synchronize()
    assert opt.step_count == 1 and ow.iter == 2 and opt.gflat.abs().sum().item() == 0
    worst, where = _worst(want, _state(model))
    assert worst < 2e-5, (where, worst)


def test_amp_wrapper_with_clipping(plain):
    g1 = plain["norms"][0]
    max_norm = g1 / 2                                              # an active clip
    # a good step equals the plain wrapper with the same clipping
    model, ow = _train(1, "AmpOptimWrapper", clip_grad=dict(max_norm=max_norm))
    good = _state(model)
    assert abs(ow.grad_norm() - g1) <= 1e-4 * g1, (ow.grad_norm(), g1)      # the norm of the UN-scaled gradients, not 65536 x it
    model, ow_plain = _train(1, clip_grad=dict(max_norm=max_norm))
    worst, where = _worst(_state(model), good)
    assert worst < 2e-5, (where, worst)
    assert abs(ow_plain.grad_norm() - g1) <= 1e-5 * g1
    # the poisoned step: skipped, scale halved, parameters those after the good step, norm non-finite
    model, ow = _train(2, "AmpOptimWrapper", poison_at=1, clip_grad=dict(max_norm=max_norm))
    assert ow._stale                                               # nothing was read back during the steps
    assert ow.skipped == 1 and ow.scale == 32768.0 and ow.iter == 2 and ow.optimizer.step_count == 1
    worst, where = _worst(good, _state(model))
    assert worst < 1e-6, (where, worst)
    assert not math.isfinite(ow.grad_norm())


# ---------------------------------------------------------------------------------------------------------------- 6: Runner.train
def test_runner_logs_grad_norm_and_accumulates(tmp_path):
    from tests import val_loop_helpers as Hh
    from vfmseg_amd.runner import Runner
    cfg = Hh.train_cfg(str(tmp_path), 4)
    cfg["optim_wrapper"] = dict(cfg["optim_wrapper"], clip_grad=dict(max_norm=1.0, norm_type=2), accumulative_counts=2)
    runner = Runner.from_cfg(cfg)
    runner.train(log_interval=1, ckpt_interval=0)
    torch.cuda.synchronize()
    recs = [json.loads(l) for l in open(os.path.join(str(tmp_path), "scalars_rank0.jsonl"))]
    assert [r["iter"] for r in recs] == [1, 2, 3, 4]
    assert "grad_norm" not in recs[0]                              # no optimiser step yet
    assert all(math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 for r in recs[1:])
    assert recs[1]["grad_norm"] == recs[2]["grad_norm"] != recs[3]["grad_norm"]   # the LAST step's value
    assert runner.ow.optimizer.step_count == 2 and runner.ow.iter == 4 and runner.iter == 4
