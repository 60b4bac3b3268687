"""Multiplexed BAMs without a GPU: the --cells file parser and the tag-mode flag checks of the pileup CLI (which
exit before torch is imported), and the per-cell split of tests/multiplex_bam.py checked with the Python
restatement of pileup_bams (tests/pileup_bam_ref.py)."""
import os
import subprocess
import sys

import pytest

from secedo_amd import pileup_main
from tests import bam_writer as bw
from tests import multiplex_bam as mx
from tests import pileup_bam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_cells(tmp_path):
    p = tmp_path / "barcodes.tsv"
    p.write_text("# 10x barcodes\nAAACCTGA-1\n\n  \nAAACGGGT-1\tx\r\nTTTGTCAT-1\n#last\n")
    assert pileup_main.read_cells(str(p)) == ["AAACCTGA-1", "AAACGGGT-1", "TTTGTCAT-1"]


def test_tag_flags_parse():
    a = pileup_main.parse_args(["-i", "x", "--cell_tag", "CB", "--cells", "c.txt"])
    assert (a.cell_tag, a.cells, a.min_cell_records) == ("CB", "c.txt", None)
    a = pileup_main.parse_args(["-i", "x"])
    assert (a.cell_tag, a.cells, a.min_cell_records) == (None, None, None)
    assert pileup_main.valid_tag("CB") and pileup_main.valid_tag("x1")
    assert not any(pileup_main.valid_tag(t) for t in ("1B", "C", "CBX", "C-", "", "ÄB"))


def _run(args, cwd):
    """pileup_main.main(args) in a child process; asserts torch was never imported there."""
    code = ("import sys; from secedo_amd import pileup_main as m\n"
            "try:\n    rc = m.main(sys.argv[1:])\nexcept SystemExit as e:\n"
            "    print(e, file=sys.stderr); rc = 2\n"
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)")
    p = subprocess.run([sys.executable, "-c", code, *args], cwd=cwd, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert "torch imported" not in p.stderr, p.stderr
    return p.returncode, p.stdout + p.stderr


def test_tag_flag_errors_exit_before_torch(tmp_path):
    bam = tmp_path / "m.bam"
    bw.write_bam(str(bam), [("1", 100)], [])
    cells = tmp_path / "cells.txt"
    cells.write_text("A\n")
    o = str(tmp_path / "o")
    cases = [
        (["--cell_tag", "1B"], "cell_tag"),
        (["--cell_tag", "CBX"], "cell_tag"),
        (["--cell_tag", "CB", "--cells", str(cells), "--min_cell_records", "2"], "exclude"),
        (["--cell_tag", "CB", "--cells", str(tmp_path / "missing.txt")], "does not exist"),
        (["--cell_tag", "CB", "--min_cell_records", "0"], "at least 1"),
        (["--cells", str(cells)], "need --cell_tag"),
    ]
    for extra, text in cases:
        rc, out = _run(["-i", str(bam), "-o", o, "--chromosomes", "1", *extra], tmp_path)
        assert rc != 0 and text in out, (extra, out)
    rc, out = _run(["-i", str(tmp_path / "nothing.bam"), "-o", o, "--cell_tag", "CB"], tmp_path)
    assert rc != 0 and "does not exist" in out
    empty = tmp_path / "empty.txt"
    empty.write_text("# none\n\n")
    rc, out = _run(["-i", str(bam), "-o", o, "--cell_tag", "CB", "--cells", str(empty)], tmp_path)
    assert rc != 0 and "no barcode" in out


def test_parse_aux_round_trip():
    tags = [("NM", "i", -3), ("AS", "C", 200), ("XS", "Z", "abc"), ("XA", "A", "q"), ("XB", "B", ("s", [1, -2])),
            ("XF", "f", 0.5), ("CB", "Z", "AAAC-1")]
    raw = b"".join(bw._tag(*t) for t in tags)
    assert mx.parse_aux(raw) == tags
    r = bw.Rec("a", 0, 1, [("M", 1)], "A", tags=[("CB", "i", 3), ("CB", "Z", "X")])
    assert mx.barcode_of(r, "CB") is None  # the first CB counts, and it is not Z-typed
    assert mx.barcode_of(bw.Rec("a", 0, 1, [("M", 1)], "A", tags=[("CB", "Z", "X")]), "CB") == "X"


@pytest.mark.parametrize("lanes", [1, 3])
def test_split_matches_cell_files(tmp_path, lanes):
    """Cells of bw.synthetic_set merged into tagged lanes and split again pile up, in the restatement, exactly as
    the original per-cell files (the appended tag changes nothing the reference reads)."""
    refs, cells = mx.synthetic_cells(tmp_path / "orig", n_cells=4, pairs_per_cell=20, n_refs=2, seed=5)
    originals = sorted(str(p) for p in (tmp_path / "orig").iterdir())
    barcodes = ["BC%02d" % c for c in range(len(cells))]
    recs = [r for cell in mx.tagged(cells, barcodes) for r in cell]
    (tmp_path / "mux").mkdir()
    (tmp_path / "split").mkdir()
    paths = mx.write_multiplexed(tmp_path / "mux", refs, recs, n_lanes=lanes, seed=2)
    assert len(paths) == lanes
    split = mx.split(tmp_path / "split", refs, paths, barcodes)
    assert sum(len(bw.read_bam(p)[1]) for p in paths) == sum(len(c) for c in cells)
    for chromosome in (0, 1):
        want = ref.pileup_bams(originals, chromosome, 100, 0, 0, 0, 0)
        got = ref.pileup_bams(split, chromosome, 100, 0, 0, 0, 0)
        assert len(want.loci) > 50
        if lanes == 1:  # one lane keeps every cell's records in their order
            assert got.bin_bytes() == want.bin_bytes() and got.map_text() == want.map_text()
        else:  # lanes may reorder records of one cell at one position: the same loci and coverage
            assert [(p, len(r)) for p, r, _ in got.loci] == [(p, len(r)) for p, r, _ in want.loci]
