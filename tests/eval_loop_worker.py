"""One rank of the CPU evaluation-loop test (tests/test_eval_loop_cpu.py): vfmseg_amd.evaluation.evaluate over a stub model whose
"prediction" is a stored label map and whose counts are numpy bin counts, gloo between the ranks.
    python eval_loop_worker.py N_SAMPLES OUT_JSON      (RANK / WORLD_SIZE / MASTER_PORT from the environment)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NC = 5
KEYS = ["citys", "bdd"]


def counts(pred, label, nc=NC, ignore=255):
    pred, label = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(label).reshape(-1).astype(np.int64)
    keep = (label != ignore) & (pred < nc)
    row = np.where((label >= 0) & (label < nc), label, nc)
    return torch.from_numpy(np.bincount(row[keep] * nc + pred[keep], minlength=(nc + 1) * nc))


def samples(n):
    """n one-sample batches: (prediction map, label map, seg_map_path) filed under citys, bdd and no known dataset in turn"""
    rng = np.random.RandomState(3)
    out = []
    for i in range(n):
        pred = rng.randint(0, NC, (6, 7)).astype(np.uint8)
        lab = np.where(rng.rand(6, 7) < 0.6, pred, rng.randint(0, NC, (6, 7))).astype(np.int64)
        lab[rng.rand(6, 7) < 0.1] = 255
        lab[rng.rand(6, 7) < 0.05] = 77
        path = ["/d/citys/a_%d.png", "/d/bdd/b_%d.png", "/d/other/c_%d.png"][i % 3] % i
        out.append((pred, lab, path))
    return out


class StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.bn = torch.nn.BatchNorm1d(2)
        self.calls = []

    def data_preprocessor(self, batch, training=False):
        assert training is False
        return batch

    def predict_labels(self, inputs, data_samples, hist=None, num_classes=None, ignore_index=255):
        from vfmseg_amd.segmentors import PixelData, SegDataSample
        assert not self.training and not torch.is_grad_enabled()
        self.calls.append(data_samples[0]["seg_map_path"])
        hist += counts(inputs.numpy(), data_samples[0]["gt"], num_classes, ignore_index)
        s = SegDataSample(metainfo=dict(seg_map_path=data_samples[0]["seg_map_path"]))
        s.pred_sem_seg = PixelData(inputs[None])
        return [s]


def batches(n):
    return [dict(inputs=torch.from_numpy(p), data_samples=[dict(seg_map_path=path, gt=lab)]) for p, lab, path in samples(n)]


def metric():
    from vfmseg_amd.registry import METRICS
    return METRICS.build(dict(type="DGIoUMetric", iou_metrics=["mIoU", "mFscore"], dataset_keys=KEYS, mean_used_keys=["citys"], num_classes=NC))


def run(n, rank, world):
    from vfmseg_amd.evaluation import evaluate
    model, m, seen = StubModel().train(), metric(), []
    res, info = evaluate(model, batches(n), m, rank, world, on_output=lambda out, first: seen.append(first))
    assert model.training     # put back
    return dict(rank=rank, metrics=dict(res), samples=info["samples"], state=info["state"].tolist(), seen=seen,
                samples_per_dataset=m.samples_per_dataset)


if __name__ == "__main__":
    import torch.distributed as dist
    import vfmseg_amd  # noqa: F401
    n, out = int(sys.argv[1]), sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    r = run(n, rank, world)
    with open(out, "w") as f:
        json.dump(r, f)
    dist.destroy_process_group()
