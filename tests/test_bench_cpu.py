"""bench.py's options (CPU): a plain run is the headline line only, --full brings the other legs back, --dump-outputs writes
the last timed step's outputs as .npy files in float32 / float64 within 64 MB."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_options", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    sys.path.insert(0, ROOT)
    spec.loader.exec_module(bench)
    bench._heavy()
    return bench


def test_plain_run_is_lean_and_full_is_opt_in():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = b.parse_args(["--full", "--no-eval", "--dump-outputs", "out"])
    assert a.full and a.no_eval and a.dump_outputs == "out"


def test_dump_outputs_writes_seeded_sample(tmp_path):
    b = _bench()
    n = 3 * b.DUMP_SAMPLE + 5
    idx = b.dump_sample_index(n, "cpu")
    assert idx.numel() == b.DUMP_SAMPLE and torch.equal(idx, b.dump_sample_index(n, "cpu"))
    assert bool((idx[1:] > idx[:-1]).all()) and int(idx[-1]) < n
    assert b.dump_sample_index(100, "cpu").tolist() == list(range(100))
    flat = torch.randn(n)
    log_vars = {"decode_lr.loss_ce": torch.tensor(2.5), "decode_lr.acc_seg": torch.tensor([40.0]), "loss": torch.tensor(3.0)}
    names = b.dump_outputs(str(tmp_path / "d"), log_vars, flat[idx])
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == sorted(k + ".npy" for k in names)
    total = 0
    for f in files:
        v = np.load(tmp_path / "d" / f)
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all()
        total += v.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "d" / "decode_lr.loss_ce.npy")) == 2.5
    got = np.load(tmp_path / "d" / "trainable_params_sample.npy")
    assert got.dtype == np.float32 and np.array_equal(got, flat[idx].numpy())
