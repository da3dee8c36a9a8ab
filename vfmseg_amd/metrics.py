"""mIoU evaluation on the HIP path: mmseg IoUMetric (1.2.2 semantics, restated: SURVEY App. D) and the reference's
DGIoUMetric (rein/dg_metrics.py:24-102: results grouped per dataset by a substring of `seg_map_path`, `<dataset>_<metric>`
keys plus `mean_<metric>` over `mean_used_keys`).

Per sample one launch of vfm_confusion_hist accumulates the (label, prediction) confusion counts into a device int64 matrix;
the three areas mmseg's intersect_and_union returns are its diagonal, column sums and row sums.  The host only sees
(num_classes+1) x num_classes integers per sample group, once, in compute_metrics().

The evaluation loop (vfmseg_amd.evaluation) uses the running form instead: one device histogram per dataset key (reset_hists / hist_for /
count_samples), filled by the segmentor's predict_labels in the launch that makes the label map, summed over the ranks as one int64 vector
(hist_state / load_hist_state) and turned into the same metrics dict by compute_from_hists()."""
from collections import OrderedDict, defaultdict

import numpy as np
import torch

from . import ops
from .registry import METRICS

CITYSCAPES_CLASSES = ("road", "sidewalk", "building", "wall", "fence", "pole", "traffic light", "traffic sign", "vegetation",
                      "terrain", "sky", "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")


def _field(sample, name):
    """`sample[name]['data']` for the dict form mmengine evaluators pass, `.name.data` for SegDataSample objects."""
    v = sample[name] if isinstance(sample, dict) else getattr(sample, name)
    if isinstance(v, dict):
        return v["data"]
    return v.data if hasattr(v, "data") and not torch.is_tensor(v) else v


def _meta(sample, name, default=None):
    if isinstance(sample, dict):
        return sample.get(name, default)
    m = getattr(sample, "metainfo", None) or {}
    return m.get(name, getattr(sample, name, default))


def confusion(pred, label, num_classes, ignore_index=255, out=None):
    """int64 [(nc+1), nc] confusion counts (rows: label, last row = labels outside [0, nc) that are not ignore_index; columns:
    prediction) accumulated into `out` on the GPU."""
    dev = pred.device
    p = pred.reshape(-1)
    if p.dtype != torch.uint8:
        p = p.to(torch.uint8)
    lab = label.reshape(-1).to(dev)
    if lab.dtype not in (torch.uint8, torch.int64):
        lab = lab.long()
    if out is None:
        out = torch.zeros((num_classes + 1) * num_classes, dtype=torch.int64, device=dev)
    ops.confusion_hist(p.contiguous(), lab.contiguous(), out, num_classes, ignore_index)
    return out


def areas_from_confusion(cm, num_classes):
    """(area_intersect, area_union, area_pred_label, area_label) of mmseg IoUMetric.intersect_and_union from the confusion
    counts of one sample (or a sum of samples)."""
    cm = np.asarray(cm, dtype=np.float64).reshape(num_classes + 1, num_classes)
    inter = np.diag(cm[:num_classes]).copy()
    pred = cm.sum(0)
    lab = cm[:num_classes].sum(1)
    return inter, pred + lab - inter, pred, lab


def total_area_to_metrics(inter, union, pred, lab, metrics=("mIoU",), nan_to_num=None, beta=1):
    """mmseg IoUMetric.total_area_to_metrics."""
    ret = OrderedDict(aAcc=inter.sum() / lab.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in metrics:
            if m == "mIoU":
                ret["IoU"], ret["Acc"] = inter / union, inter / lab
            elif m == "mDice":
                ret["Dice"], ret["Acc"] = 2 * inter / (pred + lab), inter / lab
            elif m == "mFscore":
                precision, recall = inter / pred, inter / lab
                ret["Fscore"] = (1 + beta ** 2) * precision * recall / (beta ** 2 * precision + recall)
                ret["Precision"], ret["Recall"] = precision, recall
            else:
                raise KeyError(f"metrics {m} is not supported")
    if nan_to_num is not None:
        ret = OrderedDict((k, np.nan_to_num(v, nan=nan_to_num)) for k, v in ret.items())
    return ret


@METRICS.register_module()
class IoUMetric:
    """mmseg.evaluation.IoUMetric surface: process(data_batch, data_samples) / compute_metrics(results) / evaluate(size),
    `dataset_meta['classes']`, `results`."""

    def __init__(self, ignore_index=255, iou_metrics=("mIoU",), nan_to_num=None, beta=1, collect_device="cpu", output_dir=None,
                 format_only=False, prefix=None, num_classes=None, **kw):
        self.ignore_index, self.metrics, self.nan_to_num, self.beta = ignore_index, list(iou_metrics), nan_to_num, beta
        self.output_dir, self.format_only, self.prefix = output_dir, format_only, prefix
        self.dataset_meta = dict(classes=CITYSCAPES_CLASSES[:num_classes] if num_classes else CITYSCAPES_CLASSES)
        self.results = []

    @property
    def num_classes(self):
        return len(self.dataset_meta["classes"])

    def _sample_confusion(self, sample):
        pred = _field(sample, "pred_sem_seg").squeeze()
        label = _field(sample, "gt_sem_seg").squeeze()
        return confusion(pred, label, self.num_classes, self.ignore_index)

    def process(self, data_batch, data_samples):
        for s in data_samples:
            if not self.format_only:
                self.results.append(self._sample_confusion(s))

    def _summarise(self, cms):
        nc = self.num_classes
        return self._summarise_total(torch.stack(list(cms)).sum(0).cpu().numpy() if cms else np.zeros((nc + 1) * nc))

    def _summarise_total(self, total):
        nc = self.num_classes
        ret = total_area_to_metrics(*areas_from_confusion(total, nc), self.metrics, self.nan_to_num, self.beta)
        out = OrderedDict()
        for k, v in ret.items():
            val = float(np.round(np.nanmean(v) * 100, 2))
            out[k if k == "aAcc" else "m" + k] = val
        self.last_per_class = OrderedDict((k, np.round(np.asarray(v) * 100, 2)) for k, v in ret.items() if k != "aAcc")
        return out

    def compute_metrics(self, results):
        if self.format_only:
            return OrderedDict()
        return self._summarise(results)

    def evaluate(self, size=None):
        m = self.compute_metrics(self.results)
        self.results = []
        return {f"{self.prefix}/{k}": v for k, v in m.items()} if self.prefix else m

    # ---- running histograms (vfmseg_amd.evaluation): one device confusion matrix per dataset key instead of one per sample; the
    # segmentor's predict_labels adds each sample's counts to its key's row on the GPU, the host reads them once per evaluation.
    @property
    def hist_keys(self):
        """The fixed order of the histogram rows."""
        return ["all"]

    def key_of(self, data_samples):
        return "all"

    @property
    def hist_bins(self):
        return (self.num_classes + 1) * self.num_classes

    def reset_hists(self, device=None):
        """Zeroed histograms [len(hist_keys), bins] int64 on `device` (None: host, for tests and ranks without a GPU) and sample counts."""
        self._hists = torch.zeros(len(self.hist_keys), self.hist_bins, dtype=torch.int64, device=device)
        self._hist_counts = [0] * len(self.hist_keys)
        return self._hists

    def hist_for(self, data_samples):
        """(int64 [bins] view of the histogram the batch `data_samples` is filed under, its row index)."""
        if getattr(self, "_hists", None) is None:
            raise RuntimeError("reset_hists() first")
        j = self.hist_keys.index(self.key_of(data_samples))
        return self._hists[j], j

    def count_samples(self, row, n):
        self._hist_counts[row] += int(n)

    def hist_state(self):
        """One int64 vector [K * bins + K]: all histograms, then the per-key sample counts - what the ranks sum."""
        return torch.cat([self._hists.reshape(-1).cpu(), torch.tensor(self._hist_counts, dtype=torch.int64)])

    def load_hist_state(self, state):
        K, bins = len(self.hist_keys), self.hist_bins
        state = torch.as_tensor(state, dtype=torch.int64).cpu()
        assert state.numel() == K * bins + K, (state.numel(), K, bins)
        self._hists = state[:K * bins].reshape(K, bins).clone()
        self._hist_counts = [int(v) for v in state[K * bins:]]

    def compute_from_hists(self):
        """compute_metrics() of the samples that were accumulated into the histograms."""
        if self.format_only:
            return OrderedDict()
        return self._summarise_total(self._hists[0].cpu().numpy())


@METRICS.register_module()
class DGIoUMetric(IoUMetric):
    """rein/dg_metrics.py:24-102: each sample is filed under the first `dataset_keys` entry contained in the batch's
    FIRST sample's `seg_map_path` (:53-58 - the reference indexes data_samples[0], reproduced), else "unknown"; metrics are
    computed per dataset and averaged over `mean_used_keys` (default: all dataset_keys) into `mean_<metric>`."""

    def __init__(self, dataset_keys=(), mean_used_keys=(), **kw):
        super().__init__(**kw)
        self.dataset_keys = list(dataset_keys)
        self.mean_used_keys = list(mean_used_keys) if mean_used_keys else list(dataset_keys)

    def process(self, data_batch, data_samples):
        for s in data_samples:
            if self.format_only:
                continue
            key = "unknown"
            path0 = _meta(data_samples[0], "seg_map_path", "") or ""
            for k in self.dataset_keys:
                if k in path0:
                    key = k
                    break
            self.results.append([key, self._sample_confusion(s)])

    @property
    def hist_keys(self):
        return self.dataset_keys + ["unknown"]

    def key_of(self, data_samples):
        """The filing rule of process(): the first dataset key contained in the batch's FIRST sample's seg_map_path."""
        path0 = (_meta(data_samples[0], "seg_map_path", "") or "") if data_samples else ""
        for k in self.dataset_keys:
            if k in path0:
                return k
        return "unknown"

    def compute_from_hists(self):
        """compute_metrics() from the per-key histograms; the datasets appear in hist_keys order (compute_metrics: in the order
        their first sample arrived, which several ranks do not share)."""
        if self.format_only:
            return OrderedDict()
        metrics, to_mean = OrderedDict(), defaultdict(list)
        total = self._hists.cpu().numpy()
        self.samples_per_dataset = {k: n for k, n in zip(self.hist_keys, self._hist_counts) if n}
        for j, key in enumerate(self.hist_keys):
            if not self._hist_counts[j]:
                continue
            for k, v in self._summarise_total(total[j]).items():
                metrics[f"{key}_{k}"] = v
                if key in self.mean_used_keys:
                    to_mean[k].append(v)
        for k, v in to_mean.items():
            metrics[f"mean_{k}"] = sum(v) / len(v)
        return metrics

    def compute_metrics(self, results):
        per = defaultdict(list)
        for key, cm in results:
            per[key].append(cm)
        metrics, to_mean = OrderedDict(), defaultdict(list)
        self.samples_per_dataset = {k: len(v) for k, v in per.items()}
        for key, cms in per.items():
            for k, v in self._summarise(cms).items():
                metrics[f"{key}_{k}"] = v
                if key in self.mean_used_keys:
                    to_mean[k].append(v)
        for k, v in to_mean.items():
            metrics[f"mean_{k}"] = sum(v) / len(v)
        return metrics
