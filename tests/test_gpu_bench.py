"""GPU: a plain `bench.py --gpus 1` run - the headline line only - and what `--dump-outputs` writes of its last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(cuda, native, oracle, tmp_path):
    lines = [_plain_run(tmp_path / d) for d in ("a", "b")]
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "TFLOP/s" and line["higher_is_better"] is True and line["metric"] and line["dtype"]
    assert not {"roofline", "secondary", "cpu_baseline", "measured_ceilings"} & set(line)   # those are --full's

    sys.path.insert(0, ROOT)
    import bench
    w = bench.Workload("gemm", cuda)   # the same seeds: the same operands the runs timed
    nb = len(w.Bs)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == [f"out_w{nb - 2}.npy", f"out_w{nb - 1}.npy"]
    rows = slice(0, w.M, 32)
    A = w.A.cpu().numpy()[rows]
    for j in (nb - 2, nb - 1):
        got = np.load(tmp_path / "a" / f"out_w{j}.npy")
        assert got.dtype == np.float32 and got.shape == (w.M, w.N)
        assert np.array_equal(got, np.load(tmp_path / "b" / f"out_w{j}.npy"))   # identical inputs, deterministic kernels: identical outputs
        B = w.Bs[j].cpu().numpy()
        exact = oracle.scaled_mm(A, B, [0.01], [0.01], accumulate="f64")
        bound = oracle.abs_dot_bound(A, B, [0.01], [0.01])
        assert np.all(np.abs(got[rows] - exact) <= 1e-3 * bound + 1e-30), f"out_w{j} is not A @ B[{j}]^T"
