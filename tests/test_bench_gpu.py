"""A plain `bench.py --gpus 1` run end to end on a depth-4 model: the number of timed steps is what --steps says, the line
carries ms_per_step and none of the --full legs, and --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--depth", "4", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["dtype"] == "bf16"
    assert out["unit"] == "images/s" and out["higher_is_better"] is True
    assert abs(out["value"] - out["config"]["global_batch"] * 1e3 / out["ms_per_step"]) <= 1e-2 * out["value"]
    assert not {"roofline", "eval", "other_backbones", "parity_mode", "amp_fp16", "cpu_baseline", "ranks"} & set(out)
    files = sorted(os.listdir(out_dir))
    assert {"loss.npy", "decode_lr.loss_ce.npy", "decode_hr.loss_ce.npy", "trainable_params_sample.npy"} <= set(files)
    total = 0
    for f in files:
        v = np.load(out_dir / f)
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), f
        total += v.nbytes
    assert total <= 64 << 20
    assert float(np.load(out_dir / "loss.npy")) > 0 and np.load(out_dir / "trainable_params_sample.npy").dtype == np.float32
