"""`python bench.py --gpus N` must start its own N ranks (VERDICT r01 "next" 2): the parent process, which has
not touched the GPU, runs torch.distributed.run; the ranks rendezvous on 127.0.0.1 and share the work out.
Here without a GPU, through bench.py's --dry-run (gloo; everything the ranks do before the first HIP call)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*flags):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)  # as the driver starts it: no launcher around it
    env.pop("RANK", None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True,
                          timeout=600, env=env, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout  # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_gpus_2_starts_two_ranks_that_cover_the_work_once():
    line = run_bench("--gpus", "2", "--dry-run", "--workload", "C2")
    assert line["n_gpus"] == 2 and line["world_size"] == 2 and line["backend"] == "gloo"
    assert sum(line["shard_entries"]) == line["entries"] and min(line["shard_entries"]) > 0
    assert sum(line["shard_chromosomes"]) == line["chromosomes"] == 22
    assert sum(line["shard_tiles"]) == line["tiles"] == 36


def test_bench_single_rank_needs_no_launcher():
    line = run_bench("--dry-run", "--workload", "C1")
    assert line["n_gpus"] == 1 and line["shard_entries"] == [line["entries"]]


def test_bench_default_workload_is_the_headline_configuration():
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args([])
    assert args.workload == "C3" and args.gpus == 1  # BASELINE.json configs[2]: 8000 cells x 100K loci


def test_bench_extras_only_under_full():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args([]).full is False  # a plain run: the headline line only
    assert bench.parse_args(["--full", "--no-live-counters"]).full is True


def test_bench_steps_are_the_timed_steps():
    sys.path.insert(0, ROOT)
    import bench
    for steps in (1, 2, 3, 7, 20):
        for repeats in (1, 5, 30):
            sizes = bench.block_sizes(steps, repeats)
            assert sum(sizes) == steps and len(sizes) == min(steps, repeats) and max(sizes) - min(sizes) <= 1


def test_bench_dumped_matrix_sample_is_fixed_and_independent_of_sharding(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    n = 700
    m = torch.arange(n * n, dtype=torch.float64).reshape(n, n)
    assert list(bench.matrix_outputs(m, 0, n)) == ["similarity_matrix"]
    monkeypatch.setattr(bench, "DUMP_FULL_BYTES", 1024)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 5000)
    whole = bench.matrix_outputs(m, 0, n)
    i, j = (whole["similarity_matrix_sample_" + k].astype(np.int64) for k in ("rows", "cols"))
    assert np.array_equal(whole["similarity_matrix_sample"], m.numpy()[i, j])
    assert np.array_equal(whole["similarity_matrix_row_sums"], m.sum(dim=1).numpy())
    # the matrix kept sharded by rows: each rank fills its own rows, the sum over the ranks is the whole
    parts = [bench.matrix_outputs(m[lo:hi], lo, n, reduce=lambda t: t) for lo, hi in ((0, 256), (256, n))]
    for k, v in whole.items():
        summed = k in ("similarity_matrix_sample", "similarity_matrix_row_sums")
        assert np.array_equal(parts[0][k] + parts[1][k] if summed else parts[0][k], v), k
    shapes = bench.write_outputs(str(tmp_path / "out"), whole)
    assert shapes["similarity_matrix_sample"] == [5000]
    assert np.array_equal(np.load(tmp_path / "out" / "similarity_matrix_sample.npy"), whole["similarity_matrix_sample"])
