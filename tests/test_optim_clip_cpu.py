"""mmengine OptimWrapper's `clip_grad` and `accumulative_counts` on the host path (CPU tensors, a stub optimiser as in test_optim_cpu.py):
the accumulation schedule, clipping against torch.nn.utils.clip_grad_norm_ / clip_grad_value_ in float64, clipping under the loss scaler,
what the constructor passes on and refuses, and the held all-reduce under gloo."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import vfmseg_amd  # noqa: F401
from vfmseg_amd import optim, presets
from vfmseg_amd.optim import AmpOptimWrapper, OptimWrapper, PEFTOptimWrapperConstructor, parse_clip_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


class _StubOpt:
    """What the wrappers need of FusedAdamW (tests/test_optim_cpu.py _StubOpt) plus a record of the calls."""

    def __init__(self, n=8):
        self.w = torch.zeros(n)
        self.gflat = torch.zeros(n)
        self.param_groups = [dict(lr=0.0)]
        self.calls, self.seen = [], []
        self.step_count = 0

    def step(self, lr=None, grad_scale=1.0, zero_grad=False, skip_flag=None):
        self.step_count += 1
        self.calls.append(("step", lr, float(grad_scale), bool(zero_grad), None if skip_flag is None else int(skip_flag.item())))
        if skip_flag is not None and int(skip_flag.item()):
            if zero_grad:
                self.gflat.zero_()
            return
        self.seen.append(self.gflat.clone() * grad_scale)   # the gradients as the optimiser sees them
        self.w -= 0.1 * self.gflat * grad_scale
        if zero_grad:
            self.gflat.zero_()

    def zero_grad(self):
        self.calls.append(("zero_grad",))
        self.gflat.zero_()


class _Loss:
    """Stands in for the loss tensor: backward() deposits grad * (whatever the loss was multiplied / divided by) into the stub's buffer."""

    def __init__(self, opt, grad, mult=1.0, log=None):
        self.opt, self.grad, self.mult, self.log = opt, grad, mult, log

    def __mul__(self, k):
        return _Loss(self.opt, self.grad, self.mult * k, self.log)

    def __truediv__(self, k):
        if self.log is not None:
            self.log.append(k)
        return _Loss(self.opt, self.grad, self.mult / k, self.log)

    def backward(self):
        self.opt.gflat += self.grad * self.mult


class _Sched:
    def lr(self, t):
        return 100.0 + t


# ---------------------------------------------------------------------------------------------------------------- 1, 2: accumulation
def test_accumulation_schedule_n4_over_10_iterations():
    opt = _StubOpt()
    ow = OptimWrapper(opt, _Sched(), None, accumulative_counts=4)
    ow.initialize_count_status(0, 10)
    g = torch.arange(8, dtype=torch.float32) + 1
    divisors, stepped_after = [], []
    for it in range(1, 11):
        before = opt.step_count
        ow.update_params(_Loss(opt, g * it, log=divisors))
        if opt.step_count != before:
            stepped_after.append(it)
            assert float(opt.gflat.abs().sum()) == 0.0
        else:
            assert float(opt.gflat.abs().sum()) > 0.0     # held: the gradients stay and keep adding up
    assert divisors == [4, 4, 4, 4, 4, 4, 4, 4, 2, 2]
    assert stepped_after == [4, 8, 10]
    assert ow.iter == 10 and opt.step_count == 3
    # each step saw the mean of its window's gradients, at the schedule's value of the iteration that performed it
    for seen, window in zip(opt.seen, ([1, 2, 3, 4], [5, 6, 7, 8], [9, 10])):
        assert torch.allclose(seen, g * sum(window) / len(window), rtol=1e-6)
    assert [c[1] for c in opt.calls if c[0] == "step"] == [103.0, 107.0, 109.0]


def test_accumulation_without_max_counts_and_resume_warning():
    opt = _StubOpt()
    ow = OptimWrapper(opt, None, None, accumulative_counts=3)
    divisors = []
    for _ in range(7):
        ow.update_params(_Loss(opt, torch.ones(8), log=divisors))
    assert divisors == [3] * 7 and opt.step_count == 2 and ow.iter == 7
    with pytest.warns(UserWarning, match="accumulative_counts"):
        ow.initialize_count_status(7, 12)     # a resume inside a window
    with pytest.raises(ValueError, match="accumulative_counts"):
        OptimWrapper(_StubOpt(), None, None, accumulative_counts=0)


@pytest.mark.parametrize("amp", [False, True])
def test_accumulation_off_leaves_the_call_sequence_alone(amp):
    """accumulative_counts=1, no clip_grad: what the stub sees is what it saw before these options existed - per update_params one
    step(lr, grad_scale, zero_grad=True[, skip_flag]) and one zero_grad(), and the loss is neither divided nor wrapped."""
    g = torch.arange(8, dtype=torch.float32)
    runs = []
    for kw in ({}, dict(clip_grad=None, accumulative_counts=1)):
        opt = _StubOpt()
        ow = (AmpOptimWrapper(opt, _Sched(), None, loss_scale=512.0, **kw) if amp else OptimWrapper(opt, _Sched(), None, **kw))
        ow.initialize_count_status(0, 3) if kw else None
        divisors = []
        for _ in range(3):
            ow.update_params(_Loss(opt, g, log=divisors))
        assert divisors == [] and ow.iter == 3 and ow.grad_norm() is None
        runs.append((opt.calls, opt.w.clone()))
    scale, flag = (1.0 / 512.0, 0) if amp else (1.0, None)
    want = []
    for t in range(3):
        want += [("step", 100.0 + t, scale, True, flag), ("zero_grad",)]
    assert runs[0][0] == want and runs[1][0] == want and torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------------------------- 3, 4: clipping
def _grads(n=1000, seed=0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("norm_type", [2, 1, INF, "inf"])
@pytest.mark.parametrize("factor", [0.5, 2.0])   # max_norm = factor * the norm: clipped / below max_norm
def test_norm_clipping_against_torch_float64(norm_type, factor):
    g = _grads()
    nt = INF if norm_type == "inf" else norm_type
    total64 = torch.linalg.vector_norm(g.double(), nt).item()
    max_norm = factor * total64
    p = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
    p.grad = g.double().clone()
    ref_total = torch.nn.utils.clip_grad_norm_([p], max_norm, norm_type=nt)
    opt = _StubOpt(1000)
    ow = OptimWrapper(opt, None, None, clip_grad=dict(max_norm=max_norm, norm_type=norm_type))
    ow.update_params(_Loss(opt, g))
    seen = opt.seen[0]
    assert abs(ow.grad_norm() - ref_total.item()) <= 1e-6 * ref_total.item()
    if factor > 1:
        assert torch.equal(seen, g)           # coefficient exactly 1: the buffer is untouched
    else:
        assert not torch.equal(seen, g)
        assert (seen.double() - p.grad).abs().max().item() <= 1e-6 * p.grad.abs().max().item()


def test_value_clipping_against_torch():
    g = _grads(seed=1)
    p = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
    p.grad = g.double().clone()
    torch.nn.utils.clip_grad_value_([p], 0.3)
    opt = _StubOpt(1000)
    ow = OptimWrapper(opt, None, None, clip_grad=dict(type="value", clip_value=0.3))
    ow.update_params(_Loss(opt, g))
    assert (g.abs() > 0.3).sum() > 100
    assert (opt.seen[0].double() - p.grad).abs().max().item() <= 1e-7
    assert ow.grad_norm() is None             # clip_grad_value_ returns no norm (mmengine logs none either)


def test_piecewise_step_clips_too():
    g = _grads(seed=2)
    opt = _StubOpt(1000)
    ow = OptimWrapper(opt, None, None, clip_grad=dict(max_norm=1.0))
    ow.backward(ow.scale_loss(_Loss(opt, g)))
    ow.backward(ow.scale_loss(_Loss(opt, g)))
    ow.step()
    ow.zero_grad()
    assert abs(ow.grad_norm() - 2 * g.double().norm().item()) <= 1e-5 * ow.grad_norm()
    assert abs(opt.seen[0].double().norm().item() - 1.0) <= 1e-5 and ow.iter == 1


# ---------------------------------------------------------------------------------------------------------------- 5: under amp
def test_clipping_under_amp_uses_the_unscaled_norm_and_skips_an_inf():
    g = _grads(seed=3)
    total64 = g.double().norm().item()
    opt = _StubOpt(1000)
    ow = AmpOptimWrapper(opt, None, None, loss_scale=dict(init_scale=1024.0, growth_interval=100), clip_grad=dict(max_norm=total64 / 4))
    ow.update_params(_Loss(opt, g))
    assert abs(ow.grad_norm() - total64) <= 1e-5 * total64           # not 1024 x that
    assert (opt.seen[0].double() - g.double() / 4).abs().max().item() <= 1e-5 * g.abs().max().item()
    assert ow.scale == 1024.0 and ow.skipped == 0
    bad = g.clone()
    bad[17] = INF
    w = opt.w.clone()
    ow.update_params(_Loss(opt, bad))
    assert ow.skipped == 1 and ow.scale == 512.0 and torch.equal(opt.w, w) and len(opt.seen) == 1
    assert not torch.isfinite(torch.tensor(ow.grad_norm())) and float(opt.gflat.abs().sum()) == 0.0
    assert ow.iter == 2 and opt.step_count == 1
    # value clipping under the scale: the UN-scaled gradient is clamped
    opt2 = _StubOpt(1000)
    ow2 = AmpOptimWrapper(opt2, None, None, loss_scale=1024.0, clip_grad=dict(type="value", clip_value=0.3))
    ow2.update_params(_Loss(opt2, g))
    assert (opt2.seen[0] - g.clamp(-0.3, 0.3)).abs().max().item() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- 6: constructor
def _construct(monkeypatch, **keys):
    def stub(model, lr, *a, **k):
        o = _StubOpt()
        o.lr = lr
        return o

    monkeypatch.setattr(optim, "FusedAdamW", stub)
    oc = presets.optim_cfg()
    return PEFTOptimWrapperConstructor(dict(oc["optim_wrapper"], **keys))(torch.nn.Linear(2, 2), oc["param_scheduler"])


@pytest.mark.parametrize("wtype,cls", [("OptimWrapper", OptimWrapper), ("AmpOptimWrapper", AmpOptimWrapper)])
def test_constructor_passes_both_keys_on(monkeypatch, wtype, cls):
    ow = _construct(monkeypatch, type=wtype, clip_grad=dict(max_norm=1.0, norm_type="inf"), accumulative_counts=4)
    assert type(ow) is cls and ow.clip_grad == dict(type="norm", max_norm=1.0, norm_type=INF) and ow._accumulative_counts == 4
    ow = _construct(monkeypatch, type=wtype, clip_grad=dict(type="value", clip_value=0.5))
    assert ow.clip_grad == dict(type="value", clip_value=0.5) and ow._accumulative_counts == 1
    ow = _construct(monkeypatch, type=wtype)
    assert ow.clip_grad is None and ow._accumulative_counts == 1
    assert _construct(monkeypatch, type=wtype, clip_grad=dict(max_norm=2.0, error_if_nonfinite=False)).clip_grad["norm_type"] == 2.0


def test_presets_optim_cfg_keeps_its_defaults():
    base = presets.optim_cfg()["optim_wrapper"]
    assert "clip_grad" not in base and "accumulative_counts" not in base
    got = presets.optim_cfg(clip_grad=dict(max_norm=1.0), accumulative_counts=4)["optim_wrapper"]
    assert got["clip_grad"] == dict(max_norm=1.0) and got["accumulative_counts"] == 4
    assert {k: v for k, v in got.items() if k not in ("clip_grad", "accumulative_counts")} == base


@pytest.mark.parametrize("clip_grad,exc,names", [
    (dict(max_norm=1.0, norm_type=3), NotImplementedError, "norm_type"),
    (dict(max_norm=1.0, norm_type=0.5), NotImplementedError, "norm_type"),
    (dict(max_norm=1.0, error_if_nonfinite=True), NotImplementedError, "error_if_nonfinite"),
    (dict(max_norm=1.0, foreach=True), NotImplementedError, "foreach"),
    (dict(max_norm=1.0, bogus=1), NotImplementedError, "bogus"),
    (dict(type="value", clip_value=1.0, max_norm=1.0), NotImplementedError, "max_norm"),
    (dict(type="adaptive", max_norm=1.0), NotImplementedError, "type"),
    (dict(norm_type=2), ValueError, "max_norm"),
    (dict(type="value"), ValueError, "clip_value"),
    (1.0, TypeError, "clip_grad"),
])
def test_refusals_name_their_option(monkeypatch, clip_grad, exc, names):
    with pytest.raises(exc, match=names):
        parse_clip_grad(clip_grad)
    for wtype in ("OptimWrapper", "AmpOptimWrapper"):
        with pytest.raises(exc, match=names):
            _construct(monkeypatch, type=wtype, clip_grad=clip_grad)


def test_dacs_refuses_accumulation_and_takes_clip_grad():
    from vfmseg_amd.config import Config
    from vfmseg_amd.registry import MODELS
    m = copy.deepcopy(dict(Config.fromfile(os.path.join(ROOT, "configs", "uda_rein_dinov2_segformer.py"))["model"]))
    m["backbone"] = dict(m["backbone"], depth=1, out_indices=[0, 0, 0, 0])
    m["backbone"]["reins_config"] = dict(m["backbone"]["reins_config"], num_layers=1)
    m["backbone"].pop("init_cfg", None)
    model = MODELS.build(m)
    with pytest.raises(NotImplementedError, match="accumulative_counts"):
        model.train_step({}, OptimWrapper(_StubOpt(), None, None, accumulative_counts=2))
    with pytest.raises(KeyError):     # clip_grad passes the gate: the step gets as far as reading the (empty) batch
        model.train_step({}, OptimWrapper(_StubOpt(), None, None, clip_grad=dict(max_norm=1.0)))


def test_cfg_options_create_the_nested_keys():
    """The README's spelling: --cfg-options optim_wrapper.clip_grad.max_norm=1.0 optim_wrapper.accumulative_counts=4"""
    from vfmseg_amd.config import Config, parse_cfg_options
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "dg_lora_dinov2_ms_masked.py"))
    assert cfg["optim_wrapper"].get("clip_grad") is None and cfg["optim_wrapper"].get("accumulative_counts") is None
    cfg.merge_from_dict(parse_cfg_options(["optim_wrapper.clip_grad.max_norm=1.0", "optim_wrapper.accumulative_counts=4"]))
    ow_cfg = dict(cfg["optim_wrapper"])
    assert dict(ow_cfg["clip_grad"]) == dict(max_norm=1.0) and ow_cfg["accumulative_counts"] == 4
    assert parse_clip_grad(dict(ow_cfg["clip_grad"])) == dict(type="norm", max_norm=1.0, norm_type=2.0)
    OptimWrapper(_StubOpt(), None, None, clip_grad=dict(ow_cfg["clip_grad"]), accumulative_counts=ow_cfg["accumulative_counts"])


# ---------------------------------------------------------------------------------------------------------------- 7: gloo, world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    from vfmseg_amd import parallel
    from vfmseg_amd.optim import production_order
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    parallel.init_from_env("gloo")
    names = production_order([f"backbone.model.base_model.model.blocks.{i}.attn.qkv.lora_A.default.weight" for i in range(3)]
                             + ["decode_head.conv_seg.weight", "aux_decoder.conv_seg.weight"])
    offs = [100 * i for i in range(len(names) + 1)]
    n = offs[-1]
    opt = _StubOpt(n)
    buckets = parallel.make_buckets(names, offs)
    gs = parallel.GradSync(opt.gflat, buckets, None)
    ow = OptimWrapper(opt, None, gs, accumulative_counts=2)
    sent = []
    real = dist.all_reduce

    def counting(t, *a, **k):
        sent.append(t.numel())
        return real(t, *a, **k)

    dist.all_reduce = counting
    micro = [torch.arange(n, dtype=torch.float32) * (rank + 1) + 10 * k for k in range(2)]

    class L(_Loss):
        def backward(self):
            super().backward()
            gs.ready(0)      # what the backward hooks do (parallel.attach): a bucket leaves as soon as it is final

        def __truediv__(self, k):
            return L(self.opt, self.grad, self.mult / k)

    ow.update_params(L(opt, micro[0]))
    after_first = (len(sent), opt.step_count, opt.gflat.clone())
    ow.update_params(L(opt, micro[1]))
    dist.all_reduce = real
    # mean over ranks of the summed micro-gradients (each divided by the window length 2)
    expect = sum((torch.arange(n, dtype=torch.float32) * (r + 1) + 10 * k) / 2 for r in range(world) for k in range(2)) / world
    ok = (after_first[0] == 0 and after_first[1] == 0 and torch.equal(after_first[2], micro[0] / 2)
          and len(sent) == len(buckets) and sum(sent) == n and opt.step_count == 1 and len(opt.seen) == 1
          and torch.allclose(opt.seen[0], expect, rtol=1e-6) and ow.iter == 2 and gs.hold is False)
    q.put((rank, ok, after_first[0], len(sent), len(buckets), opt.step_count))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_accumulation_window_issues_one_set_of_all_reduces_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=100) for _ in range(2)]
    for p in ps:
        p.join(30)
    for r in res:
        assert r[1], r
