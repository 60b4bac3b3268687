"""``secedo_amd.genome_bins`` without a GPU: tests/gc_expected.py, the yardstick of tests/test_gpu_genome_bins.py,
against a small example worked by hand (arrays and file bytes) and on the line rule's quirks, and the refusals of
``python -m secedo_amd.gc_main`` and of ``depth_main --reference_genome``, made before torch is imported."""
import json
import os
import subprocess
import sys

import pytest

from tests import fasta_cases as fc
from tests import gc_expected as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRAPPER = ("import json, sys\n"
           "from secedo_amd import %s as m\n"
           "try:\n"
           "    code = m.main(sys.argv[1:])\n"
           "except SystemExit as e:\n"
           "    code = e.code\n"
           "print(json.dumps({'code': code, 'torch': 'torch' in sys.modules}))\n")


def refused(module, args):
    """-> the reason ``main`` gave up with; torch must not have been imported by then."""
    r = subprocess.run([sys.executable, "-c", WRAPPER % module] + [str(a) for a in args], capture_output=True,
                       text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["torch"] is False
    assert isinstance(out["code"], str) and "\n" not in out["code"], out
    return out["code"]


def test_expected_against_the_hand_example():
    text, S, names, lengths, bins, rows, file = ge.hand_example()
    e = ge.expected(text, S)
    assert (e.names, e.contig_lengths, e.bins) == (names, lengths, bins)
    assert e.counts.tolist() == rows and e.file == file
    assert (e.contigs, e.duplicate_names) == (3, 1)
    # reversed, with lengths; the rows move with their contig
    e = ge.expected(text, S, contigs=["two", "one"], lengths=[6, 10])
    assert e.names == ["two", "one"] and e.counts.tolist() == rows[3:] + rows[:3]
    assert e.bins == [(0, 0, 4), (0, 4, 6), (1, 0, 4), (1, 4, 8), (1, 8, 10)]
    # one bin per contig
    e = ge.expected(text, 1000, contigs=["one"])
    assert e.bins == [(0, 0, 10)] and e.counts.tolist() == [[2, 2, 2, 2, 2, 5]]
    assert e.file == ge.HEADER + b"one\t0\t10\t2\t2\t2\t2\t2\t5\n"


def test_expected_refusals():
    text = ge.hand_example()[0]
    for kw, code, words in [
        (dict(S=0), ge.INVALID_ARG, "bin_size is 0"),
        (dict(contigs=["one", "chrtwo"]), ge.INVALID_ARG, "no contig named 'chrtwo' (names are matched exactly"),
        (dict(contigs=["one", "one"]), ge.INVALID_ARG, "'one' is listed twice"),
        (dict(contigs=[]), ge.INVALID_ARG, "no contig is selected"),
        (dict(contigs=["two", "one"], lengths=[6, 11]), ge.INVALID_ARG, "one: the genome has 10 bases, expected 11"),
    ]:
        with pytest.raises(ge.Refused) as r:
            ge.expected(text, kw.pop("S", 4), path="g.fa", **kw)
        assert r.value.code == code and words in r.value.message
    with pytest.raises(ge.Refused) as r:
        ge.expected(b"", 4, path="g.fa")
    assert r.value.message == "g.fa: the genome is empty"
    with pytest.raises(ge.Refused) as r:
        ge.expected(b">a\nAC\n>" + b"n" * 4097 + b" x\nAC\n", 4, path="g.fa")
    assert r.value.message == "g.fa: contig 1: its name is longer than 4096 bytes"
    assert ge.expected(b">" + b"n" * 4096 + b"\tx\nAC\n", 4).names == ["n" * 4096]


def test_expected_on_the_line_quirks():
    q = fc.QUIRKS
    e = ge.expected(q["sequence_starts_with_gt"], 100)  # '>ACGT' after a header is sequence
    assert e.names == ["a", "b"] and e.contig_lengths == [9, 2] and e.counts.tolist()[0] == [2, 2, 2, 2, 1, 0]
    e = ge.expected(q["alternating_run"], 100)  # >a header, >b sequence, >c header
    assert e.names == ["a", "c"] and e.contig_lengths == [2, 4]
    e = ge.expected(q["crlf"], 100)  # the names stop at '\r'; the '\r' of a sequence line is other
    assert e.names == ["a", "b"] and e.counts.tolist() == [[2, 2, 1, 1, 2, 0], [0, 0, 2, 0, 1, 0]]
    e = ge.expected(q["newline"], 100)  # an empty line 0: a contig with an empty name and no bins
    assert e.names == [""] and e.contig_lengths == [0] and e.bins == [] and e.file == ge.HEADER
    e = ge.expected(q["first_line_not_a_header"], 3)  # line 0 is a header whatever it starts with
    assert e.names == ["CGT", "b"] and e.contig_lengths == [4, 2]
    e = ge.expected(q["lower_u_n"], 5)
    assert e.counts.tolist() == [[1, 1, 1, 2, 0, 5], [1, 0, 0, 1, 3, 2], [0, 1, 1, 1, 0, 0], [0, 0, 0, 0, 4, 4]]
    e = ge.expected(q["no_trailing_newline"], 4)
    assert e.contig_lengths == [4, 4] and e.file.endswith(b"b\t0\t4\t1\t0\t1\t2\t0\t0\n")
    for text in q.values():
        if text:
            e = ge.expected(text, 3)
            assert all(int(sum(r[:5])) == b[2] - b[1] for r, b in zip(e.counts.tolist(), e.bins))


def test_gc_main_refusals(tmp_path):
    genome = tmp_path / "g.fa"
    genome.write_bytes(ge.hand_example()[0])
    out = tmp_path / "out"
    out.mkdir()
    base = ["-r", genome, "-o", out]
    assert "Invalid --bin_size 0" in refused("gc_main", base + ["--bin_size", "0"])
    assert "Invalid --bin_size" in refused("gc_main", base + ["--bin_size", "4294967296"])
    assert "plain or bgzf" in refused("gc_main", base + ["--output", "gzip"])
    assert "listed twice" in refused("gc_main", base + ["--contigs", "one,two,one"])
    assert "does not exist" in refused("gc_main", ["-r", tmp_path / "missing.fa", "-o", out])
    assert "is not a directory" in refused("gc_main", ["-r", genome, "-o", tmp_path / "nowhere"])
    (out / "genome.gc.tsv.gz").write_text("x")
    why = refused("gc_main", base + ["--output", "bgzf"])
    assert "genome.gc.tsv.gz exists" in why and "--overwrite" in why
    assert os.listdir(str(out)) == ["genome.gc.tsv.gz"]


def test_depth_main_reference_genome_refusals(tmp_path):
    from tests import bam_writer as bw

    cells = tmp_path / "cells"
    cells.mkdir()
    bw.write_bam(str(cells / "a.bam"), [("1", 50)], [])
    out = tmp_path / "out"
    out.mkdir()
    base = ["-i", cells, "-o", out, "--chromosomes", "1"]
    why = refused("depth_main", base + ["--reference_genome", tmp_path / "missing.fa"])
    assert "--reference_genome" in why and "does not exist" in why
    genome = tmp_path / "g.fa"
    genome.write_bytes(b">1\nACGT\n")
    (out / "depth").mkdir()
    (out / "depth" / "depth.gc.tsv").write_text("x")
    why = refused("depth_main", base + ["--reference_genome", genome])
    assert "depth.gc.tsv exists" in why and "--overwrite" in why
    # without the flag that file is none of the run's outputs: the refusal is not about it
    (out / "depth" / "depth.bins.bed").write_text("x")
    assert "depth.bins.bed exists" in refused("depth_main", base)
