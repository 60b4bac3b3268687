"""SAM input without a GPU: tests/sam_writer.py writes the records ``bw.encode_record`` encodes (checked with a small
SAM -> BAM record parser that follows the rules of include/secedo_bam.h, tests/sam_ref.py), the golden .sam fixtures
hold their .bam's records, and ``pileup_main`` finds SAM files in a directory that holds no BAM."""
import os
import struct

import pytest

from secedo_amd import pileup_main
from tests import bam_writer as bw
from tests import sam_writer as sw
from tests.golden_util import GOLDEN
from tests.sam_cases import covering_records
from tests.sam_ref import B_FMT, B_RANGE, NT16, SamError, _int, parse_aux, parse_line  # noqa: F401

REFS = [("chr1", 5000), ("chr2", 4000)]


def test_writer_lines_parse_to_encode_record():
    names = [n for n, _ in REFS]
    recs = sw.canonical(covering_records())
    text = sw.sam_text(REFS, recs)
    lines = text.splitlines()
    assert lines[0].startswith("@HD") and lines[1:3] == ["@SQ\tSN:chr1\tLN:5000", "@SQ\tSN:chr2\tLN:4000"]
    for line, r in zip(lines[3:], recs):
        assert parse_line(line, names) == bw.encode_record(r), r.name
    # lowercase bases give the upper-case codes
    low = sw.record_line(recs[0], REFS).split("\t")
    low[9] = low[9].lower()
    assert parse_line("\t".join(low), names) == bw.encode_record(recs[0])


def test_canonical_types():
    r = sw.canonical([bw.Rec("x", 0, 1, [("M", 1)], "A", tags=[("AS", "S", 79), ("XS", "i", -27), ("GP", "i", 698303082),
                                                               ("ZZ", "I", 300), ("ZS", "Z", "v")])])[0]
    assert [t[1] for t in r.tags] == ["C", "c", "I", "S", "Z"]


@pytest.mark.parametrize("line", [
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA\tI\tAS:i-90",      # the second ':' missing
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA",                  # ten fields
    "r\t0\tchr3\t1\t60\t1M\t*\t0\t0\tA\tI",               # RNAME not in @SQ
    "r\t0\tchr1\t1\t60\t2M\t*\t0\t0\tA\tI",               # CIGAR against SEQ
    "r\t0\tchr1\t1\t60\t0M\t*\t0\t0\tA\tI",               # a zero-length op
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA\tII",              # QUAL length
    "r\t65536\tchr1\t1\t60\t1M\t*\t0\t0\tA\tI",           # FLAG range
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA\tI\tXX:i:4294967296",
])
def test_reference_parser_refuses(line):
    with pytest.raises(SamError):
        parse_line(line, ["chr1"])


@pytest.mark.parametrize("name", ["hard_clipping", "soft_clipping", "insert_at_end", "test2", "test3"])
def test_golden_sam_holds_its_bam(name):
    """Each golden .sam parses to its .bam's records (the bin field aside: the fixtures' writer computes it)."""
    refs, _ = bw.read_bam(os.path.join(GOLDEN, "bam", name + ".bam"))
    raw = bw.gzip.decompress(open(os.path.join(GOLDEN, "bam", name + ".bam"), "rb").read())
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    want = []
    while o < len(raw):
        bs = struct.unpack_from("<i", raw, o)[0]
        want.append(raw[o:o + 4 + bs])
        o += 4 + bs
    lines = [l for l in open(os.path.join(GOLDEN, "bam", name + ".sam")).read().split("\n") if l and l[0] != "@"]
    got = [parse_line(l, [n for n, _ in refs]) for l in lines]
    strip = lambda b: b[:14] + b[16:]  # noqa: E731
    assert [strip(g) for g in got] == [strip(w) for w in want]


def test_input_files_falls_back_to_sam(tmp_path):
    d = tmp_path / "sams"
    (d / "sub").mkdir(parents=True)
    for p in ("b_1.sam", "sub/a_2.sam", "notes.txt"):
        (d / p).write_text("")
    assert pileup_main.input_files(str(d)) == sorted([str(d / "b_1.sam"), str(d / "sub" / "a_2.sam")])
    single = str(d / "b_1.sam")
    assert pileup_main.input_files(single) == [single]


def test_input_files_prefers_bam(tmp_path):
    for p in ("x_1.bam", "x_2.sam", "y_3.bam"):
        (tmp_path / p).write_text("")
    assert pileup_main.input_files(str(tmp_path)) == [str(tmp_path / "x_1.bam"), str(tmp_path / "y_3.bam")]


def test_help_names_sam(capsys):
    with pytest.raises(SystemExit):
        pileup_main.parse_args(["--help"])
    assert "SAM" in capsys.readouterr().out
