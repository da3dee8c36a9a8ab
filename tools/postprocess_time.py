#!/usr/bin/env python
"""Times the per-sample post-processing of the evaluation loop in its two forms, in ONE process with the forms alternating:
  fused     one vfm_postprocess_argmax launch (un-pad, un-flip, bilinear resize, argmax, confusion counts; uint8 label map out)
  composed  today's chain: BaseSegmentor.postprocess_result (strided_copy, vfm_resize_bilinear, vfm_slide_finalize) + metrics.confusion
at the three evaluation geometries of the DG targets (network output -> ori_shape): Cityscapes 1024x2048 -> 1024x2048 (argmax and
counts only), BDD100K 1024x1820 -> 720x1280, Mapillary 1024x1365 -> 3000x4000.  Operands (logits and labels) rotate through a
ring larger than the 256 MiB last-level cache; both forms allocate their outputs inside the timed region; each round times
--passes passes over the ring per form (device-synchronised host clock), and the median and range of the rounds are reported per call, with the
peak allocated bytes of one call, the bytes each form moves (from the shapes) and the share of HBM bandwidth that implies.

    python tools/postprocess_time.py [--rounds 9] [--classes 19]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("cityscapes", (1024, 2048), (1024, 2048)), ("bdd100k", (1024, 1820), (720, 1280)), ("mapillary", (1024, 1365), (3000, 4000))]
HBM_PEAK = 8.0e12      # bytes/s, the MI355X specification (about 6.3e12 is reachable by a plain copy)
LLC = 256 << 20


def bytes_moved(C, hw, out):
    """(fused, composed) HBM bytes of one call, from the shapes: every tensor a kernel of the form reads or writes, once."""
    src, n = C * hw[0] * hw[1] * 4, out[0] * out[1]
    full = C * n * 4
    fused = src + n * (1 + 8)
    if tuple(hw) == tuple(out):     # plain: one argmax pass over the logits, then the counts
        composed = src + n + n * (1 + 8)
    else:                           # copy (read + write), resize (read + write full resolution), argmax (read full, write n), counts
        composed = 2 * src + src + full + full + n + n * (1 + 8)
    return fused, composed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--passes", type=int, default=8, help="passes over the ring per timed window")
    a = ap.parse_args()
    import numpy as np
    import torch
    import vfmseg_amd  # noqa: F401
    from vfmseg_amd import ops
    from vfmseg_amd.metrics import confusion
    from vfmseg_amd.segmentors import EncoderDecoder, SegDataSample
    if not torch.cuda.is_available():
        raise SystemExit("postprocess_time: needs the GPU (no timing without one)")
    C, dev = a.classes, "cuda"
    print(f"# rounds {a.rounds}, classes {C}; ms per call: median [min .. max] over the rounds; HBM share = bytes moved / median / {HBM_PEAK / 1e12:.1f} TB/s")
    for name, hw, out in SHAPES:
        ring = max(3, -(-2 * LLC // (C * hw[0] * hw[1] * 4)))
        g = torch.Generator(device=dev).manual_seed(hw[1])
        logits = [torch.randn(1, C, *hw, device=dev, generator=g) for _ in range(ring)]
        labels = [torch.randint(0, C, (1,) + out, device=dev, generator=g) for _ in range(ring)]
        meta = dict(ori_shape=out, img_shape=hw, padding_size=[0, 0, 0, 0])
        hist = torch.zeros((C + 1) * C, dtype=torch.int64, device=dev)

        def fused(i):
            return ops.postprocess_argmax(logits[i][0], (0, 0) + hw, 0, out, label=labels[i], hist=hist, num_classes=C)

        def composed(i):
            ds = EncoderDecoder.postprocess_result(None, logits[i], [SegDataSample(metainfo=meta)], [meta])[0]
            pred = ds.pred_sem_seg.data
            confusion(pred, labels[i], C, 255, out=hist)
            return pred

        forms = dict(fused=fused, composed=composed)
        # same values first (section "when results must not change"), and the peak memory of one call
        hist.zero_()
        pf = fused(0)
        hf = hist.clone()
        hist.zero_()
        pc = composed(0)
        assert torch.equal(pf.reshape(-1), pc.reshape(-1)) and torch.equal(hf, hist), "the two forms disagree"
        del pf, pc
        peak = {}
        for k, f in forms.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            f(0)
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        times = {k: [] for k in forms}
        for r in range(a.rounds + 1):          # round 0 warms up
            for k in (("fused", "composed") if r % 2 == 0 else ("composed", "fused")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.passes * ring):
                    forms[k](i % ring)
                torch.cuda.synchronize()
                if r:
                    times[k].append(1e3 * (time.perf_counter() - t0) / (a.passes * ring))
        moved = dict(zip(("fused", "composed"), bytes_moved(C, hw, out)))
        for k in forms:
            t = np.asarray(times[k])
            med = float(np.median(t))
            print(f"{name:10s} {hw[0]}x{hw[1]} -> {out[0]}x{out[1]}  {k:8s} {med:8.3f} ms [{t.min():.3f} .. {t.max():.3f}]  peak {peak[k] / 2**20:8.1f} MiB"
                  f"  moves {moved[k] / 1e6:8.1f} MB  = {100 * moved[k] / (med * 1e-3) / HBM_PEAK:5.1f} % of HBM peak", flush=True)
        lo = {k: (min(times[k]), max(times[k])) for k in forms}
        print(f"{name:10s} fused range {'below' if lo['fused'][1] < lo['composed'][0] else 'NOT below'} the composed range"
              f" (median ratio composed / fused = {np.median(times['composed']) / np.median(times['fused']):.2f})", flush=True)
        del logits, labels
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
