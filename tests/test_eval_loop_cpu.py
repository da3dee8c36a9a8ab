"""The evaluation loop's host side without a GPU (vfmseg_amd/evaluation.py, the running histograms of vfmseg_amd/metrics.py, the
Runner's validation rule and best-checkpoint book-keeping): sharding, compute_from_hists == compute_metrics, the one all-reduce
between two gloo ranks (one of which may hold no sample), when validation runs, and which best_* file is kept."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "eval_loop_worker.py")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_loop_worker as W  # noqa: E402


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 5, 7])
def test_shards_cover_every_index_once(n, world):
    from vfmseg_amd.evaluation import shard
    got = sorted(i for r in range(world) for i in shard(n, r, world))
    assert got == list(range(n))
    assert all(list(shard(n, r, world)) == list(range(r, n, world)) for r in range(world))


def _fill(metric, samples):
    """the per-sample confusions as process() would store them, and the same samples accumulated into the running histograms"""
    metric.reset_hists(None)
    results = []
    for pred, lab, path in samples:
        cm = W.counts(pred, lab, metric.num_classes)
        batch = [dict(seg_map_path=path)]
        hist, row = metric.hist_for(batch)
        hist += cm
        metric.count_samples(row, 1)
        results.append(cm if not hasattr(metric, "dataset_keys") else [metric.key_of(batch), cm])
    return results


def _same(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


def test_dg_metric_from_histograms_equals_per_sample_results():
    m = W.metric()
    assert m.hist_keys == ["citys", "bdd", "unknown"] and m.mean_used_keys == ["citys"]
    results = _fill(m, W.samples(7))
    want = m.compute_metrics(results)
    want_per_class, want_n = {k: v.copy() for k, v in m.last_per_class.items()}, dict(m.samples_per_dataset)
    got = m.compute_from_hists()
    _same(got, want)
    assert {"citys_mIoU", "bdd_mIoU", "unknown_mIoU", "citys_mFscore", "mean_mIoU", "mean_aAcc"} <= set(got)
    assert got["mean_mIoU"] == got["citys_mIoU"]      # the mean runs over mean_used_keys only
    assert m.samples_per_dataset == want_n == {"citys": 3, "bdd": 2, "unknown": 2}
    for k, v in want_per_class.items():
        np.testing.assert_array_equal(m.last_per_class[k], v)
    # a dataset without samples is left out, as compute_metrics leaves it out
    results = _fill(m, [s for s in W.samples(7) if "bdd" not in s[2]])
    _same(m.compute_from_hists(), m.compute_metrics(results))
    assert "bdd_mIoU" not in m.compute_from_hists()
    # the state vector round-trips
    state = m.hist_state()
    assert state.dtype == torch.int64 and state.numel() == 3 * (W.NC + 1) * W.NC + 3
    before = m.compute_from_hists()
    m.load_hist_state(state)
    _same(m.compute_from_hists(), before)


def test_iou_metric_from_histograms_equals_per_sample_results():
    from vfmseg_amd.registry import METRICS
    m = METRICS.build(dict(type="IoUMetric", iou_metrics=["mIoU", "mDice"], num_classes=W.NC, nan_to_num=0))
    results = _fill(m, W.samples(5))
    want = m.compute_metrics(results)
    per_class = {k: v.copy() for k, v in m.last_per_class.items()}
    _same(m.compute_from_hists(), want)
    for k, v in per_class.items():
        np.testing.assert_array_equal(m.last_per_class[k], v)
    assert set(want) == {"aAcc", "mIoU", "mAcc", "mDice"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_ranks(n, tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"n{n}_rank{r}.json") for r in range(2)]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, WORKER, str(n), outs[r]], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for p, o in zip(procs, logs):
        assert p.returncode == 0, o[-3000:]
    return [json.load(open(o)) for o in outs]


@pytest.mark.parametrize("n", [1, 3])
def test_two_gloo_ranks_hold_the_sums(n, tmp_path):
    """n = 3: the ranks hold two samples and one; n = 1: rank 1 holds none and still joins the one collective."""
    one = W.run(n, 0, 1)
    ranks = _two_ranks(n, tmp_path)
    assert [r["seen"] for r in ranks] == [list(range(0, n, 2)), list(range(1, n, 2))] and one["seen"] == list(range(n))
    for r in ranks:
        assert r["samples"] == n == one["samples"]
        assert r["state"][:-1] == one["state"][:-1]       # histograms and sample counts (the last entry is the time)
        assert r["metrics"] == one["metrics"] and r["samples_per_dataset"] == one["samples_per_dataset"]
    assert ranks[0]["state"] == ranks[1]["state"]
    # and the sums are those of the per-sample confusions
    m = W.metric()
    _same(one["metrics"], dict(m.compute_metrics(_fill(m, W.samples(n)))))


def test_validation_points():
    from vfmseg_amd.evaluation import validation_due
    due = lambda **kw: [i for i in range(1, kw["max_iters"] + 1) if validation_due(i, kw.get("val_interval"), kw["max_iters"], kw.get("val_begin", 0))]  # noqa: E731
    assert due(val_interval=2, max_iters=4) == [2, 4]
    assert due(val_interval=3, max_iters=10) == [3, 6, 9, 10]          # always at the last iteration
    assert due(val_interval=3, max_iters=10, val_begin=6) == [6, 9, 10]
    assert due(val_interval=4, max_iters=10, val_begin=11) == []
    assert due(val_interval=8000, max_iters=3) == [3]
    assert due(val_interval=None, max_iters=5) == [] and due(val_interval=0, max_iters=5) == []


def test_best_checkpoint_naming_and_replacement(tmp_path):
    from vfmseg_amd.evaluation import BestCheckpoint
    best = BestCheckpoint("citys_mIoU", str(tmp_path))
    saved = []

    def save(path):
        saved.append(os.path.basename(path))
        open(path, "w").write("x")

    files = lambda: sorted(f for f in os.listdir(tmp_path) if f.startswith("best_"))  # noqa: E731
    for it, v in [(2, 10.0), (4, 12.5), (6, 12.5), (8, 11.0), (10, 30.0)]:     # rule "greater": an equal value does not replace
        best.update({"citys_mIoU": v, "mean_mIoU": 1.0}, it, save)
        assert files() == [f"best_citys_mIoU_iter_{ {2: 2, 4: 4, 6: 4, 8: 4, 10: 10}[it] }.pth".replace(" ", "")]
    assert saved == ["best_citys_mIoU_iter_2.pth", "best_citys_mIoU_iter_4.pth", "best_citys_mIoU_iter_10.pth"]
    assert best.best == 30.0
    with pytest.raises(KeyError, match="citys_mIoU.*bdd_mIoU.*mean_mIoU"):
        BestCheckpoint("citys_mIoU", str(tmp_path)).update({"bdd_mIoU": 1.0, "mean_mIoU": 1.0}, 2, save)
