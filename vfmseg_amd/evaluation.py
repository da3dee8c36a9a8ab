"""The evaluation loop shared by validation during training (Runner.train) and tools/test.py: mmengine's ValLoop / TestLoop over
a sharded test set (the reference: `val_cfg = dict(type="ValLoop")`, `val_evaluator = DGIoUMetric`, tools/test.py:96-145).

Rank r takes the samples range(r, n, world) - no sample is padded or duplicated, so the summed confusion counts are those of one
process whatever the world size, and a rank may hold no sample at all.  Per batch: data_preprocessor -> predict_labels, which adds
the batch's confusion counts to the metric's per-dataset histogram on the GPU (vfm_postprocess_argmax) -> on_output.  At the end
ONE all-reduce (SUM) of a single int64 buffer (every histogram, the per-key sample counts, the prediction time in microseconds);
every rank then computes the same metrics dict.  world == 1 needs no process group and runs no collective."""
import time

import torch


def shard(n, rank=0, world=1):
    """The sample indices of `rank`: every world-th one, starting at rank (DataLoaderIter(..., infinite=False) samples the same)."""
    return range(rank, n, world)


def reduce_state(state, world=1, group=None):
    """SUM of the int64 vector `state` (host) over the ranks: one collective; none for world == 1.  A nccl group reduces on the
    device, gloo on the host."""
    if world == 1:
        return state
    import torch.distributed as dist
    buf = state.clone()
    if dist.get_backend(group) == "nccl":
        buf = buf.cuda()
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf.cpu()


def _batches(data, rank, world, limit):
    """(first global index, batch) of this rank's share of `data`: a list of ready batches (dicts with inputs / data_samples, one
    sample each - the synthetic sets), a dataset (or its config) that a DataLoaderIter reads with batch size 1, or a
    DataLoaderIter built with infinite=False for this rank.  `limit`: only the first `limit` samples of the whole set."""
    from .datasets import DataLoaderIter
    if isinstance(data, (list, tuple)):
        n = len(data) if limit is None else min(limit, len(data))
        for i in shard(n, rank, world):
            yield i, data[i]
        return
    if not isinstance(data, DataLoaderIter):
        data = DataLoaderIter(data, 1, 0, shuffle=False, rank=rank, world=world, infinite=False)
    n = len(data.dataset) if limit is None else min(limit, len(data.dataset))
    idx = list(data.sampler)
    step = data.bs
    for k, batch in enumerate(data.loader):
        first = idx[k * step]
        if first >= n:     # (a rank's indices grow: nothing below the limit follows)
            break
        yield first, batch


def dataset_size(data):
    if isinstance(data, (list, tuple)):
        return len(data)
    return len(getattr(data, "dataset", data))


@torch.no_grad()
def evaluate(model, dataset_or_loader, metric, rank=0, world=1, group=None, limit=None, on_output=None):
    """Returns (metrics dict - the same on every rank, info) with info = dict(samples: the global count, seconds: the ranks' summed
    prediction time, state: the reduced int64 buffer).  on_output(outputs, first_global_index) sees every batch's samples
    (`pred_sem_seg` uint8 [1, oh, ow]) of this rank."""
    was_training = model.training
    model.eval()
    try:
        dev = next(model.parameters()).device
        metric.reset_hists(dev)
        nc, ignore = metric.num_classes, metric.ignore_index
        t = 0.0
        for first, batch in _batches(dataset_or_loader, rank, world, limit):
            data = model.data_preprocessor(batch, False)
            samples = data["data_samples"]
            hist, row = metric.hist_for(samples)
            if dev.type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.predict_labels(data["inputs"], samples, hist=None if metric.format_only else hist, num_classes=nc, ignore_index=ignore)
            if dev.type == "cuda":
                torch.cuda.synchronize()
            t += time.perf_counter() - t0
            metric.count_samples(row, len(out))
            if on_output is not None:
                on_output(out, first)
        state = torch.cat([metric.hist_state(), torch.tensor([int(round(t * 1e6))], dtype=torch.int64)])
        state = reduce_state(state, world, group)
        metric.load_hist_state(state[:-1])
        res = metric.compute_from_hists()
        if metric.prefix:
            res = {f"{metric.prefix}/{k}": v for k, v in res.items()}
        return res, dict(samples=sum(metric._hist_counts), seconds=float(state[-1]) * 1e-6, state=state)
    finally:
        model.train(was_training)


def synthetic_set(n, size, keys=("synthetic",), device="cuda"):
    """The fixed synthetic evaluation set tools/test.py scores when no data are there: n one-sample batches (image seed 500 + i and
    its label), filed under the dataset keys in turn."""
    from .segmentors import SegDataSample
    from .synth import synth_image, synth_label
    keys = list(keys) or ["synthetic"]
    out = []
    for i in range(n):
        img, lab = synth_image(1, tuple(size), seed=500 + i).to(device), synth_label(1, tuple(size), seed=500 + i).to(device)
        meta = dict(seg_map_path=f"{keys[i % len(keys)]}/synthetic_{i}.png", ori_shape=tuple(size), img_shape=tuple(size), padding_size=[0, 0, 0, 0])
        out.append(dict(inputs=img, data_samples=[SegDataSample(gt_sem_seg=lab[0], metainfo=meta)]))
    return out


def validation_due(it, val_interval, max_iters, val_begin=0):
    """mmengine IterBasedTrainLoop's rule, restated: validate after iteration `it` when it >= val_begin and (it % val_interval == 0
    or it == max_iters)."""
    return bool(val_interval) and it >= val_begin and (it % val_interval == 0 or it == max_iters)


class BestCheckpoint:
    """CheckpointHook(save_best=KEY, rule="greater"): after a validation that improves KEY, save(path) writes
    best_<KEY>_iter_<i>.pth and the previous best file is removed.  An unknown KEY is an error naming the available keys."""

    def __init__(self, key, work_dir):
        self.key, self.work_dir, self.best, self.path = key, work_dir, None, None

    def file_name(self, it):
        return f"best_{self.key.replace('/', '_')}_iter_{it}.pth"

    def update(self, metrics, it, save):
        import os
        if self.key not in metrics:
            raise KeyError(f"save_best={self.key!r} is not among the validation metrics: {sorted(metrics)}")
        v = metrics[self.key]
        if self.best is not None and not v > self.best:
            return None
        path = os.path.join(self.work_dir, self.file_name(it))
        save(path)
        if self.path and self.path != path and os.path.exists(self.path):
            os.remove(self.path)
        self.best, self.path = v, path
        return path
