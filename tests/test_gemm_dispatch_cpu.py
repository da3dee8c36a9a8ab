"""Which kernel a bf16 GEMM runs on, pinned on the CPU.

vfmseg_amd/csrc/gemm_select.h is the whole dispatch of vfm_gemm's bf16 path as a pure function (descriptor, knobs) -> GemmPlan.  This test
compiles tests/gemm_dispatch_main.cpp around it with plain g++ (no ROCm include path: the selector has no HIP in it) under
-fsanitize=undefined,address and compares every field of every plan with tests/golden/gemm_dispatch.npz.

The fixture holds what the dispatcher did BEFORE the selector existed: its launch helpers were replaced by recorders (helper, template
parameters or form, M, N, tail descriptor passed, returned fold flag) and the old vfm_gemm_bf16_impl was run on the host over
  - the (M, N, K) of tools/bench_gemm_step.py CASES / EVAL_CASES and of the test_gemm_* shape lists (transposed-B ones included),
  - a grid of 20 M x 18 N x 9 K x batch {1, 4} x the three operand layouts x {aligned, misaligned} epilogues,
  - rows with A strides that fail the 32-bit span checks,
  - every dispatch knob varied alone on the named shapes, gemm_cfg forced to every live id, two retired ids and one that never existed.
The rows of the retired ids (VFM_E_UNSUPPORTED) are the one intended difference and were written by hand.  `plans_experimental` is the same
recording with the experimental GEMM files built in (-DVFM_EXPERIMENTAL_GEMM).
A dispatch change shows up here as the exact list of cases whose plan moved; regenerate the fixture rows it means to move.

case columns  : M N K batch layout epi sa_m bias | gemm_cfg use_pp use_192 w44_k split_tail fold_tail bt64 batch_tiles deep_tail_k deep_sep_k use_ps
plan columns  : err kind cfg vec tail_rows tail_mode        (gemm_select.h: GemmKind, GemmTail)
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_dispatch_main.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.npz")
SHIPPED = [10, 16, 17, 18, 30, 31, 32, 33, 34, 35, 36, 39, 40, 51, 52]
EXPERIMENTAL = [37, 38, 50]
FIELDS = ["err", "kind", "cfg", "vec", "tail_rows", "tail_mode"]


@pytest.fixture(scope="module", params=[False, True], ids=["shipped", "experimental"])
def selector(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_dispatch") / "gemm_dispatch_main")
    cmd = ["g++", "-std=c++17", "-O1", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "vfmseg_amd", "csrc"), SRC, "-o", exe]
    if request.param:
        cmd.insert(1, "-DVFM_EXPERIMENTAL_GEMM")
    subprocess.run(cmd, check=True)
    return exe, request.param


def test_config_table_ids_are_unique_and_exactly_the_live_ids(selector):
    exe, experimental = selector
    ids = [int(v) for v in subprocess.run([exe, "--ids"], capture_output=True, text=True, check=True).stdout.split()]
    assert len(ids) == len(set(ids)), ids
    assert sorted(ids) == sorted(SHIPPED + (EXPERIMENTAL if experimental else [])), ids


def test_every_plan_equals_the_recorded_dispatch(selector, tmp_path):
    exe, experimental = selector
    fx = np.load(FIXTURE)
    cases, want = fx["cases"].astype(np.int64), fx["plans_experimental" if experimental else "plans"]
    assert cases.shape[0] == want.shape[0] > 40000 and cases.shape[1] == 19 and want.shape[1] == len(FIELDS)
    # the fixture covers what it claims to: every live id forced, retired and unknown ids, every tail mode, every kernel kind
    assert set(SHIPPED + EXPERIMENTAL + [0, 29, 41, -1]) == set(np.unique(cases[:, 8]).tolist())
    assert set(np.unique(want[:, 5]).tolist()) == {0, 1, 2, 3, 4} and set(np.unique(want[:, 1]).tolist()) == {0, 1, 2, 3, 4}
    assert set(np.unique(want[:, 0]).tolist()) == {0, -1, -5}
    cases.tofile(str(tmp_path / "cases.bin"))
    subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "plans.bin")], check=True)
    got = np.fromfile(str(tmp_path / "plans.bin"), dtype=np.int32).reshape(-1, len(FIELDS))
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    report = ["case %s: got %s, recorded %s" % (cases[i].tolist(), dict(zip(FIELDS, got[i].tolist())), dict(zip(FIELDS, want[i].tolist()))) for i in bad[:20]]
    assert bad.size == 0, "%d of %d plans differ\n%s" % (bad.size, len(want), "\n".join(report))
