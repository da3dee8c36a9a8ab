"""The evaluation loop on the GPU (vfmseg_amd/evaluation.py): the fused loop equals today's loop (model.predict + metric.process +
metric.evaluate), validation inside Runner.train does not perturb training, the best checkpoint is kept, and two ranks (gloo,
sharing the one GPU of the test box) give the results of one - in evaluate(), in tools/test.py and in training with validation."""
import ast
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "val_loop_worker.py")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import val_loop_helpers as Hh  # noqa: E402


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    from vfmseg_amd.precision import set_compute_dtype
    set_compute_dtype("bf16")


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    return Hh.tree(str(tmp_path_factory.mktemp("val_loop") / "data"))


@pytest.fixture(scope="module")
def model():
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd.precision import set_compute_dtype
    set_compute_dtype("bf16")
    return Hh.build_model()


def _evaluate(model, root, limit=None):
    from vfmseg_amd.evaluation import evaluate
    from vfmseg_amd.registry import METRICS
    metric = METRICS.build(Hh.evaluator())
    shapes = []
    res, info = evaluate(model, Hh.test_dataset(root), metric, limit=limit, on_output=lambda out, first: shapes.extend(
        (tuple(o.pred_sem_seg.data.shape), o.pred_sem_seg.data.dtype, set(vars(o)) - {"metainfo", "gt_sem_seg"}) for o in out))
    return dict(res), info, shapes


@pytest.fixture(scope="module")
def world1(model, data_root):
    """evaluate() in one process over the three images, and over the first one: the reference of the two-rank tests"""
    return {n: _evaluate(model, data_root, n) for n in (3, 1)}


def test_fused_loop_equals_todays_loop(model, data_root, world1, monkeypatch):
    from vfmseg_amd.datasets import DataLoaderIter
    from vfmseg_amd.registry import METRICS
    # today's loop
    metric = METRICS.build(Hh.evaluator())
    cms, n = [], 0
    with torch.no_grad():
        for b in DataLoaderIter(Hh.test_dataset(data_root), 1, 0, shuffle=False, infinite=False).loader:
            assert tuple(b["inputs"][0].shape) == (3, 401, 512) and tuple(b["data_samples"][0].gt_sem_seg.data.shape) == (1, Hh.H, Hh.W)
            data = model.data_preprocessor(b, False)
            assert tuple(data["inputs"].shape) == (1, 3, 512, 512) and tuple(data["data_samples"][0].metainfo["padding_size"]) == (0, 0, 0, 111)
            out = model.predict(data["inputs"], data["data_samples"])
            metric.process(None, out)
            n += 1
    cms = torch.stack([cm for _, cm in metric.results]).sum(0).cpu()
    want = dict(metric.evaluate(n))
    res, info, shapes = world1[3]
    assert n == 3 and info["samples"] == 3
    bins = 20 * 19
    assert torch.equal(info["state"][:bins], cms) and int(info["state"][bins:2 * bins].sum()) == 0     # "citys", then "unknown"
    assert info["state"][2 * bins:2 * bins + 2].tolist() == [3, 0]
    assert res == want and "citys_mIoU" in res and res["mean_mIoU"] == res["citys_mIoU"]
    assert cms.sum().item() == 3 * (Hh.H - 40) * Hh.W        # every labelled pixel was counted once
    # samples carry the label map alone: uint8 [1, oh, ow] at ori_shape, no logits
    assert shapes == [((1, Hh.H, Hh.W), torch.uint8, {"pred_sem_seg"})] * 3
    # the composition of the existing ops
    monkeypatch.setenv("VFMSEG_POST_FUSED", "0")
    res0, info0, shapes0 = _evaluate(model, data_root)
    assert res0 == res and torch.equal(info0["state"][:-1], info["state"][:-1]) and shapes0 == shapes


def _train(work_dir, val_interval, save_best=None):
    from vfmseg_amd import functional as Fh
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.runner import Runner
    # Precision mode f32: the bf16 attention backward accumulates dQ with fp32 atomics, so two bf16 runs of the SAME configuration
    # already differ in the last bits of the LoRA gradients (the run-to-run noise tests/test_fulldepth_gpu.py describes; seen here
    # as differing lora_A / lora_B after the first or second iteration of two plain runs).  The f32 kernels have no floating-point
    # atomics: two plain runs are bit-identical, so a difference here can only come from the validation.
    set_compute_dtype("f32")
    Fh.manual_seed(0x5EED)     # the dropout / mask counter is process-wide: both runs start it at the same place
    runner = Runner.from_cfg(Hh.train_cfg(work_dir, 4, val_interval=val_interval, save_best=save_best))
    runner.train(log_interval=1, ckpt_interval=2)
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in runner.model.state_dict().items()}
    opt = {k: v.detach().clone() for k, v in runner.ow.optimizer.state_dict().items() if torch.is_tensor(v)}
    rng = (np.random.get_state()[1].copy(), torch.get_rng_state().clone(), dict(Fh._seed_state), runner.loader.i, runner.model.training)
    return state, opt, rng


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("val_train")
    plain = _train(str(d / "plain"), None)
    val = _train(str(d / "val"), 2, save_best="citys_mIoU")
    return str(d / "plain"), plain, str(d / "val"), val


def test_validation_does_not_perturb_training(runs):
    plain_dir, (s0, o0, r0), val_dir, (s1, o1, r1) = runs
    assert set(s0) == set(s1) and any("running_mean" in k for k in s0) and len(o0) > 0 and set(o0) == set(o1)
    for k in s0:      # parameters and BatchNorm running statistics: bit-identical
        assert torch.equal(s0[k], s1[k]), k
    for k in o0:
        assert torch.equal(o0[k], o1[k]), k
    assert np.array_equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1]) and r0[2:] == r1[2:] and r1[4] is True
    rec0, rec1 = Hh.records(plain_dir), Hh.records(val_dir)
    drop = lambda r: {k: v for k, v in r.items() if k not in ("time", "memory")}  # noqa: E731
    assert [drop(r) for r in rec0] == [drop(r) for r in rec1 if "val" not in r] and len(rec0) == 4
    vals = [r for r in rec1 if "val" in r]
    assert [r["iter"] for r in vals] == [2, 4] and all(r["val_samples"] == 2 and r["val_time"] > 0 and "citys_mIoU" in r["val"] for r in vals)
    assert not any("val" in r for r in rec0)
    # each record follows its iteration's training record and checkpoint
    order = [(r["iter"], "val" in r) for r in rec1]
    assert order == [(1, False), (2, False), (2, True), (3, False), (4, False), (4, True)]


def test_validation_record_equals_evaluate_on_the_checkpoint(runs):
    from vfmseg_amd.evaluation import evaluate, synthetic_set
    from vfmseg_amd.registry import METRICS
    from vfmseg_amd.precision import set_compute_dtype
    val_dir = runs[2]
    set_compute_dtype("f32")     # the mode the runs trained and validated in
    fresh = Hh.build_model(os.path.join(val_dir, "iter_2.pth"))
    res, info = evaluate(fresh, synthetic_set(2, (512, 512), Hh.KEYS), METRICS.build(Hh.evaluator()))
    rec = [r for r in Hh.records(val_dir) if "val" in r][0]
    assert rec["iter"] == 2 and rec["val"] == {k: float(v) for k, v in res.items()} and info["samples"] == 2


def test_save_best_keeps_one_file(runs):
    val_dir = runs[2]
    vals = [r for r in Hh.records(val_dir) if "val" in r]
    best_it = max(vals, key=lambda r: (r["val"]["citys_mIoU"], -r["iter"]))["iter"]     # rule "greater": the first of equal values stays
    assert sorted(f for f in os.listdir(val_dir) if f.startswith("best_")) == [f"best_citys_mIoU_iter_{best_it}.pth"]
    assert sorted(f for f in os.listdir(runs[0]) if f.startswith("best_")) == []
    ck = torch.load(os.path.join(val_dir, f"best_citys_mIoU_iter_{best_it}.pth"), map_location="cpu")
    assert ck["meta"]["iter"] == best_it
    assert open(os.path.join(val_dir, "last_checkpoint")).read().strip().endswith("iter_4.pth")      # a resume continues from the last one


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ranks(world, argv, timeout=300, **extra):
    """`world` children of argv under their own timeout; nothing is started after a failure (all start together, any failure ends the test)"""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", VFMSEG_DIST_BACKEND="gloo", **extra)
        procs.append(subprocess.Popen([sys.executable] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return outs


@pytest.mark.parametrize("n", [3, 1])
def test_two_ranks_equal_one_rank(n, data_root, world1, tmp_path):
    """three images: the ranks hold two and one; one image: rank 1 holds none, the run ends and the metrics are those of one process"""
    out = str(tmp_path / "eval.json")
    _ranks(2, [WORKER, "eval", data_root, str(n), out])
    res, info, _ = world1[n]
    got = [json.load(open(f"{out}.rank{r}")) for r in range(2)]
    assert [g["seen"] for g in got] == [list(range(0, n, 2)), list(range(1, n, 2))]
    for g in got:
        assert g["samples"] == n and g["metrics"] == res and g["state"] == info["state"][:-1].tolist()


def _result_lines(text):
    return [ast.literal_eval(l) for l in text.splitlines() if l.startswith("{") and "evaluated_samples" in l]


def test_tool_under_two_ranks(data_root, tmp_path):
    cfg = Hh.write_config(str(tmp_path / "cfg.py"), data_root)
    tool = os.path.join(ROOT, "tools", "test.py")
    one = _ranks(1, [tool, cfg, "--out", str(tmp_path / "out1")])
    two = _ranks(2, [tool, cfg, "--launcher", "pytorch", "--out", str(tmp_path / "out2")])
    a, b = _result_lines(one[0]), _result_lines("\n".join(two))
    assert len(a) == 1 and len(b) == 1, (one, two)
    a, b = a[0], b[0]
    assert set(a) == set(b) and {"citys_mIoU", "mean_mIoU", "ms_per_img", "evaluated_samples", "dataset_size"} <= set(a)
    assert all(a[k] == b[k] for k in a if k != "ms_per_img") and b["evaluated_samples"] == 3 and b["ms_per_img"] > 0
    names = sorted(f"citys_{i}.png" for i in range(3))
    assert sorted(os.listdir(tmp_path / "out1")) == names and sorted(os.listdir(tmp_path / "out2")) == names
    from PIL import Image
    for f in names:
        x, y = np.asarray(Image.open(tmp_path / "out1" / f)), np.asarray(Image.open(tmp_path / "out2" / f))
        assert x.shape == (Hh.H, Hh.W) and np.array_equal(x, y)


@pytest.fixture(scope="module")
def dp_runs(tmp_path_factory):
    """three iterations with val_interval=2 (precision mode f32, no dropout - the ranks would draw other masks -, AdamW eps 1): one
    process with the global batch of two, and two ranks with one sample each"""
    d = tmp_path_factory.mktemp("val_dp")
    _ranks(1, [WORKER, "train", str(d / "w1"), "2"])
    _ranks(2, [WORKER, "train", str(d / "w2"), "1"])
    return str(d / "w1"), str(d / "w2")


def test_two_rank_validation_scores_the_weights_the_ranks_hold(dp_runs):
    """the val record two ranks write after iteration 2 (two images on rank 0, one on rank 1, one all-reduce) is evaluate() in one
    process on the checkpoint rank 0 wrote at that iteration: integer counts, so exactly"""
    from vfmseg_amd.evaluation import evaluate, synthetic_set
    from vfmseg_amd.precision import set_compute_dtype
    from vfmseg_amd.registry import METRICS
    set_compute_dtype("f32")
    for d in dp_runs:
        fresh = Hh.build_model(os.path.join(d, "iter_2.pth"), dropout=False)
        res, info = evaluate(fresh, synthetic_set(3, (512, 512), Hh.KEYS), METRICS.build(Hh.evaluator()))
        rec = [r for r in Hh.records(d) if "val" in r]
        assert [r["iter"] for r in rec] == [2, 3] and all(r["val_samples"] == 3 for r in rec)
        assert rec[0]["val"] == {k: float(v) for k, v in res.items()}


def test_two_rank_training_with_validation(dp_runs):
    """Two ranks with one sample each write the same val record as one process with the global batch - every metric, exactly.

    The two worlds sum the gradient and the SyncBN moments in another order, so their parameters agree to fp32 rounding, not
    bitwise, and the synthetic-weight model predicts at chance level, where a last-bit change of a logit can flip a near-tie
    pixel.  The configuration keeps those differences at rounding size: precision mode f32 (no floating-point atomics) and
    AdamW eps = 1 (updates smooth in the gradient).  With the recipe's eps = 1e-8 the first updates are sign-like, last-bit
    gradient differences become +-lr steps, and the records differed by one unit of the second decimal (f32: iteration 2
    citys_mAcc 5.08 against 5.09; bf16: iteration 3 citys_aAcc 5.09 against 5.08, citys_mAcc 5.06 against 5.05) - the training
    of the two worlds, not their validation: the test above holds in every one of these configurations."""
    w1, w2 = dp_runs
    v1, v2 = ([r for r in Hh.records(d) if "val" in r] for d in (w1, w2))
    assert [r["iter"] for r in v1] == [2, 3] == [r["iter"] for r in v2]
    for a, b in zip(v1, v2):
        print("val record, one process:", a, "two ranks:", b)
        assert a["val_samples"] == b["val_samples"] == 3 and a["val"] == b["val"]
