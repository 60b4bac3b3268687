"""``secedo_amd.bin_depth`` without a GPU: tests/depth_expected.py, the yardstick of tests/test_gpu_bin_depth.py,
against a three-cell example worked by hand (arrays and file bytes), and the refusals of
``python -m secedo_amd.depth_main``, made before torch is imported."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import depth_expected as de
from tests.test_split_clusters_cpu import cli_inputs  # noqa: F401  -- the fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRAPPER = ("import json, sys\n"
           "from secedo_amd import depth_main\n"
           "try:\n"
           "    code = depth_main.main(sys.argv[1:])\n"
           "except SystemExit as e:\n"
           "    code = e.code\n"
           "print(json.dumps({'code': code, 'torch': 'torch' in sys.modules}))\n")


def refused(args):
    """-> the reason ``main`` gave up with; torch must not have been imported by then."""
    r = subprocess.run([sys.executable, "-c", WRAPPER] + [str(a) for a in args], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["torch"] is False
    assert isinstance(out["code"], str) and "\n" not in out["code"], out
    return out["code"]


@pytest.mark.parametrize("mode", ["reads", "bases"])
def test_expected_against_the_hand_example(mode):
    refs, files, want = de.hand_example()
    pairs, cells = want[mode]
    e = de.expected(files, refs, 1000, [0], mode=mode, names=["a", "b", "c"])
    assert e.bins == [(0, 0, 1000), (0, 1000, 2000), (0, 2000, 2500)]
    assert e.pairs == pairs
    assert e.cells.tolist() == cells
    assert e.stats == dict(records=9, counted=7, dropped_barcode=0, dropped_require=0, dropped_exclude=0,
                           dropped_duplicate=0, dropped_mapq=1, out_of_range=1, pairs=len(pairs))
    assert e.pieces == (7 if mode == "reads" else (1 + 2 + 2) + (1 + 1) + (0 + 3))  # touched bins per record
    b, c, v = e.arrays()
    assert list(zip(b.tolist(), c.tolist())) == sorted(pairs) and v.dtype == np.uint64


def test_expected_files_of_the_hand_example():
    refs, files, _ = de.hand_example()
    e = de.expected(files, refs, 1000, [0], mode="bases", clustering=[1, 1, 3], names=["a", "b b", "c"])
    assert e.files["depth.bins.bed"] == b"chrA\t0\t1000\nchrA\t1000\t2000\nchrA\t2000\t2500\n"
    assert e.files["depth.samples.tsv"] == b"a\nb b\nc\n"
    assert e.files["depth.counts.mtx"] == (b"%%MatrixMarket matrix coordinate integer general\n%\n3\t3\t6\n"
                                           b"1\t1\t25\n1\t3\t10\n2\t1\t15\n2\t2\t20\n3\t2\t5\n3\t3\t10\n")
    assert e.files["depth.cells.tsv"] == (b"cell\tname\trecords\tcounted\tsum\tnonzero_bins\tmax_value\n"
                                          b"0\ta\t4\t3\t40\t2\t25\n1\tb b\t3\t2\t25\t2\t20\n2\tc\t2\t2\t20\t2\t10\n")
    assert e.files["depth.clusters.tsv"] == (b"chrom\tstart\tend\tcluster_0\tcluster_1\tcluster_2\tcluster_3\n"
                                             b"chrA\t0\t1000\t0\t25\t0\t10\nchrA\t1000\t2000\t0\t35\t0\t0\n"
                                             b"chrA\t2000\t2500\t0\t5\t0\t10\n")
    assert e.cluster_sums.tolist() == [[0, 25, 0, 10], [0, 35, 0, 0], [0, 5, 0, 10]]
    # without a clustering there is no clusters file; the selection shows in the counts
    e = de.expected(files, refs, 1000, [0], min_map_quality=0, exclude=0x4, names=["a", "b", "c"])
    assert "depth.clusters.tsv" not in e.files and e.cluster_sums is None
    assert e.pairs[(1, 0)] == 1 and e.stats["dropped_mapq"] == 0 and e.stats["counted"] == 8
    # S > LN, and S == 1
    assert de.expected(files, refs, 5000, [0], names=["a", "b", "c"]).bins == [(0, 0, 2500)]
    e = de.expected(files, refs, 1, [0], mode="bases", names=["a", "b", "c"])
    assert len(e.bins) == 2500 and set(e.pairs.values()) == {1, 2} and e.pairs[(995, 0)] == 2 and e.cells[:, 2].tolist() == [40, 25, 20]


def test_cli_refusals(cli_inputs, tmp_path):  # noqa: F811
    cells, clustering, out = cli_inputs
    base = ["-i", cells, "-o", out, "--chromosomes", "1"]
    assert "Invalid --bin_size 0" in refused(base + ["--bin_size", "0"])
    assert "Invalid --bin_size" in refused(base + ["--bin_size", "4294967296"])
    why = refused(base + ["--mode", "depth"])
    assert "--mode" in why and "reads or bases" in why
    assert "Invalid --min_map_quality 256" in refused(base + ["--min_map_quality", "256"])
    why = refused(base + ["--duplicates", "mark"])
    assert "--duplicates" in why and "off or remove" in why
    assert "plain or bgzf" in refused(base + ["--output", "gzip"])
    assert "share bits 0x400" in refused(base + ["--require_flags", "DUP", "--exclude_flags", "0x400"])
    assert "unknown flag" in refused(base + ["--exclude_flags", "DUPLICATE"])
    assert "--cells needs --cell_tag" in refused(base + ["--cells", clustering])
    assert "--cell_tag needs --cells" in refused(base + ["--cell_tag", "CB"])
    assert "Invalid --cell_tag" in refused(base + ["--cell_tag", "1B", "--cells", clustering])
    assert "does not exist" in refused(base + ["--clustering", tmp_path / "missing"])
    short = tmp_path / "short"
    short.write_text("1,0\n")
    why = refused(base + ["--clustering", short])
    assert "lists 2 cells" in why and "has 3" in why
    names = tmp_path / "names"
    names.write_text("a\nb\n")
    assert "lists 2 names, the input has 3 cells" in refused(base + ["--cell_names", names])
    names.write_text("a\nb\tx\nc\n")
    assert "the name of cell 1 is empty or holds a tab" in refused(base + ["--cell_names", names])
    assert "--build_index with --index off" in refused(base + ["--build_index", "--index", "off"])
    assert "is not a directory" in refused(["-i", cells, "-o", tmp_path / "nowhere"])
    assert "Invalid chromosome" in refused(["-i", cells, "-o", out, "--chromosomes", "23"])
    (out / "depth").mkdir()
    (out / "depth" / "depth.cells.tsv.gz").write_text("x")
    why = refused(base + ["--output", "bgzf"])
    assert "depth.cells.tsv.gz exists" in why and "--overwrite" in why
    assert os.listdir(str(out)) == ["depth"] and os.listdir(str(out / "depth")) == ["depth.cells.tsv.gz"]
