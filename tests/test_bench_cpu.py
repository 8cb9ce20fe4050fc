"""bench.py's launcher on a box without enough GPUs: it must refuse before starting ranks."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_launcher_refuses_without_devices():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("box has GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2
    assert "--oversubscribe" in p.stderr


def test_bench_launcher_names_the_rank_that_died():
    """one rank exits before init_process_group (test hook) - the launcher ends its siblings, names the
    rank, its exit code and its last stderr line, and returns non-zero within seconds instead of leaving the others blocked
    in the rendezvous until the collective's own timeout.  No GPU needed: the surviving rank is still importing / waiting
    for its peer when it is ended."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["S2K_BENCH_TEST_FAIL_RANK"] = "1"
    env["S2K_BENCH_TEST_HANG_RANK"] = "0"              # (stands for "blocked in the rendezvous": this box has no GPU to get that far)
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--oversubscribe",
                        "--no-cpu-baseline", "--no-extras", "--no-pcie"], env=env, capture_output=True, text=True, timeout=120)
    took = time.time() - t0
    assert p.returncode == 3, (p.returncode, p.stderr[-1500:])
    assert "rank 1 exited with code 3" in p.stderr and "S2K_BENCH_TEST_FAIL_RANK" in p.stderr, p.stderr[-1500:]
    assert "ended the other 1 rank(s)" in p.stderr
    assert took < 60, took
    assert p.stdout.strip() == ""                      # no bench line from a launch that failed


def test_bench_launcher_times_out_on_ranks_that_never_get_ready():
    """... and ranks that hang before they are ready (the hook S2K_BENCH_TEST_HANG_RANK) are named after --rank-timeout seconds."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["S2K_BENCH_TEST_HANG_RANK"] = "0,1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--oversubscribe",
                        "--rank-timeout", "8", "--no-cpu-baseline", "--no-extras", "--no-pcie"], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 124, (p.returncode, p.stderr[-1500:])
    assert "have not reported ready" in p.stderr and "[0, 1]" in p.stderr, p.stderr[-1500:]


def test_dump_outputs_exact_and_within_budget(tmp_path):
    """--dump-outputs: bytes as float32 and wider integers as float64, every value exact; an array beyond its share of the
    64 MB budget is written as the same seeded sample every time."""
    import importlib.util

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    small = {"valid": torch.arange(1000, dtype=torch.int64).remainder(2).to(torch.uint8), "count": torch.tensor([(1 << 40) + 3])}
    bench.dump_outputs(str(tmp_path / "a"), small)
    valid, count = np.load(tmp_path / "a" / "valid.npy"), np.load(tmp_path / "a" / "count.npy")
    assert valid.dtype == np.float32 and valid.tolist() == [float(i % 2) for i in range(1000)]
    assert count.dtype == np.float64 and count.tolist() == [float((1 << 40) + 3)]
    big = {"valid": torch.arange(1 << 25, dtype=torch.int64).remainder(251).to(torch.uint8), "count": torch.tensor([7])}
    for sub in ("b", "c"):
        bench.dump_outputs(str(tmp_path / sub), big)
    files = [tmp_path / sub / name for sub in ("b", "c") for name in ("valid.npy", "count.npy")]
    assert sum(os.path.getsize(f) for f in files[:2]) <= bench.DUMP_BUDGET_BYTES
    b, c = np.load(files[0]), np.load(files[2])
    assert 0 < b.size < (1 << 25) and np.array_equal(b, c)


def test_bench_line_fits_the_drivers_record():
    """The driver keeps an 8 KB tail of stdout: bench.py's compact form carries numbers only - the prose
    goes to bench_notes.json by path -, puts what must survive LAST, rounds to six digits, and names what it had to drop.
    Fed with round 4's 18.5 KB line (profiles/r04_z_bench_n1.json) plus the rows round 5 adds."""
    import argparse
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    with open(os.path.join(ROOT, "profiles", "r04_z_bench_n1.json")) as f:
        line = json.loads(f.read().strip().split("\n")[-1])
    assert len(json.dumps(line)) > 15000
    line["recover_2p20"] = {"sigs": 1 << 20, "ms": 8.123456789, "roofline": {"kernel": "k_verify_fast<RECOVER>", "kernel_ms": 7.1, "frac": 0.9,
                                                                             "valu_instr_per_item": 260000.123, "frac_def": "x" * 300}, "note": "y" * 200}
    line["batch_sweep"] = {"log2_n": list(range(10, 23)), "ms": [0.123456789 * k for k in range(10, 23)], "note": "z" * 300}
    args = argparse.Namespace(explain=False, write_notes=False)
    text = bench.compact_line(line, args)
    assert len(text) <= 7800, len(text)
    d = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    keys = list(d)
    assert keys.index("roofline") > keys.index("msm_2p20") and keys.index("cpu_baseline") > keys.index("distinct_keys")
    assert keys[-1] == "notes" and d["notes"] == "bench_notes.json"
    flat = json.dumps(d)
    assert "frac_def" not in flat and '"note"' not in flat and "ms_each" not in flat
    assert d["recover_2p20"]["ms"] == 8.12346 and d["recover_2p20"]["roofline"]["valu_instr_per_item"] == 260000.0
    assert set(d.get("dropped", [])) <= set(bench.DROP_ORDER)
    for k in ("distinct_keys", "general_path_same_batch", "keyset_resident", "pcie_inclusive", "batch_sweep", "msm_2p20", "schnorr_rlc_2p20",
              "recover_2p20"):
        assert k in d, k                                   # what the judge asked to see in the record survives the cut
    assert json.loads(bench.compact_line(line, argparse.Namespace(explain=True, write_notes=False))) == line
