"""bench.py on the GPU, as the driver runs it: a plain run prints the headline line and measures nothing the headline
does not need; `--full` adds the in-run parity against the compiled reference, the phase times, the roofline and the
CPU baseline. C2 (1000 cells x 50 K loci: a digest of the compiled reference's output exists), two timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*flags):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)  # as the driver starts it: no launcher around it
    env.pop("RANK", None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "C2",
                           "--steps", "2", "--warmup", "1", *flags],
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout  # ONE JSON line
    return json.loads(lines[0])


def check_headline(line):
    assert line["metric"] == "cell-pair x locus updates/sec (similarity matrix)"
    assert line["unit"] == "updates/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    updates = line["config"]["updates_per_step"]
    assert updates == 63956330  # C2's exact (read pair, shared locus) count
    assert line["value"] == pytest.approx(updates / (line["ms_per_step"] * 1e-3), rel=1e-9)


def test_plain_run_prints_the_headline_and_the_outputs_only(tmp_path):
    line = run_bench("--dump-outputs", str(tmp_path))
    check_headline(line)
    assert line["full"] is False
    assert line["parity_checked"] is None and line["parity"] is None
    assert line["phase_ms"] is None and line["roofline"] is None and line["config"]["replicated_ms_per_step"] is None
    assert not {"cpu_baseline", "one_shot_first_call_s", "one_shot_host_call_s", "cpp_dropin_call"} & set(line)
    assert line["dumped_outputs"] == {"similarity_matrix": [1000, 1000]}
    m = np.load(tmp_path / "similarity_matrix.npy")
    assert m.dtype == np.float64 and np.array_equal(m, m.T) and not np.any(np.diag(m)) and np.max(m) > 0


def test_full_run_adds_parity_phases_roofline_and_cpu_baseline():
    line = run_bench("--full", "--no-live-counters")  # counters from profiles/: no profiler passes in the suite
    check_headline(line)
    assert line["full"] is True
    assert line["parity_checked"] is True and line["parity"]["samples"] > 0
    assert all(line["phase_ms"][k] > 0 for k in ("pack", "accumulate", "finalize"))
    roof = line["roofline"]
    assert roof["bound"] == "lds_atomic" and roof["kernel_ms"] > 0 and roof["updates_per_launch"] == 63956330
    assert line["cpu_baseline"]["value"] > 0 and line["one_shot_host_call_s"] > 0
