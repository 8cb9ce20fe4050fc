"""bench.py's plain run and --dump-outputs on the GPU: the line carries the headline with the step count it was given,
nothing that only --full measures, and the arrays of the last timed step are written as float arrays.  Needs a real
MI355X.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch-log2", "14", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "verifications/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - (1 << 14) / (d["ms_per_step"] * 1e-3)) <= 1e-4 * d["value"]
    for k in ("roofline", "cpu_baseline", "msm_2p20", "pcie_inclusive", "batch_sweep", "small_call", "multi_rank"):
        assert k not in d, k
    valid, bitmap, count = (np.load(out / (name + ".npy")) for name in ("valid", "bitmap", "count"))
    assert valid.dtype == np.float32 and valid.shape == (1 << 14,) and bool((valid == 1).all())
    assert bitmap.dtype == np.float32 and bitmap.shape == (1 << 11,) and bool((bitmap == 255).all())
    assert count.dtype == np.float64 and count.tolist() == [1 << 14]
