"""Pileup creation from BAM files without a GPU: the Python restatement of the reference's pileup_bams()
(tests/pileup_bam_ref.py) against every case of the reference's tests/test_pileup.cpp on its own fixtures, the
host-only BAM scan of libsecedo_bam.so on the fixtures and on tests/bam_writer.py output, and the argument
handling of the pileup CLI."""
import gzip
import os
import struct

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup, pileup_main
from tests import bam_writer as bw
from tests import pileup_bam_ref as ref
from tests.golden_util import GOLDEN

BAM = os.path.join(GOLDEN, "bam")


def fx(name):
    return os.path.join(BAM, name + ".bam")


def check_content(p):
    """The reference's check_content (test_pileup.cpp:39-60)."""
    assert len(p.loci) == 9
    for i, (_pos, rids, cbs) in enumerate(p.loci):
        assert rids == [0, 1]
        assert [cb >> 2 for cb in cbs] == [0, 1]
        assert [cb & 3 for cb in cbs] == ([0, 2] if i < 4 else [1, 3])


def test_read_too_few_different():
    files = [fx("test1")] * 3 + [fx("test2")] * 2
    assert len(ref.pileup_bams(files, 0, 10, 1, 0, 0, 3).loci) == 0
    assert len(ref.pileup_bams(files, 0, 10, 1, 0, 0, 1).loci) == 9


@pytest.mark.parametrize("first", ["test1", "soft_clipping", "hard_clipping", "insert_at_end"])
def test_read_content(first, tmp_path):
    p = ref.pileup_bams([fx(first), fx("test2")], 0, 10, 1, 0, 0, 1)
    check_content(p)
    out = tmp_path / "x.bin"
    out.write_bytes(p.bin_bytes())
    flat, cells, max_len = secedo_amd.read_pileup(str(out), [0, 1])
    assert max_len == 423 and cells == 2
    assert flat.n_loci == 9


def test_mapping_quality():
    files = [fx("test1"), fx("test2")]
    assert len(ref.pileup_bams(files, 0, 10, 1, 7, 0, 1).loci) == 0
    assert len(ref.pileup_bams(files, 0, 10, 1, 6, 0, 1).loci) == 9


def test_alignment_score():
    files = [fx("test3"), fx("test3")]
    assert len(ref.pileup_bams(files, 0, 10, 1, 0, 10, 0).loci) == 168
    assert len(ref.pileup_bams(files, 0, 10, 1, 0, 85, 1).loci) == 0
    assert len(ref.pileup_bams(files, 0, 10, 1, 0, 80, 0).loci) == 84


def test_signed_alignment_score_reads_as_zero():
    # test1.sam carries AS:i:-27, stored as a signed type: GetTag(uint32_t&) leaves 0
    _refs, recs = bw.read_bam(fx("test1"))
    assert ref.alignment_score(recs[0]) == 0
    assert len(ref.pileup_bams([fx("test1"), fx("test2")], 0, 10, 1, 0, 1, 1).loci) == 0


def test_writer_round_trip(tmp_path):
    recs = [bw.Rec("a", 0, 5, [("S", 2), ("M", 4), ("I", 1), ("D", 2), ("M", 3)], "GGACGTAACG",
                   qual=[40] * 10, tags=[("AS", "C", 200), ("XS", "Z", "q"), ("AS", "i", -3)]),
            bw.Rec("b", 1, 7, [("M", 4)], "*", tags=[("AS", "s", -2)])]
    path = str(tmp_path / "a.bam")
    bw.write_bam(path, [("1", 100), ("2", 100)], recs)
    refs, back = bw.read_bam(path)
    assert refs == [("1", 100), ("2", 100)]
    assert [r["name"] for r in back] == [b"a", b"b"]
    assert back[0]["cigar"] == recs[0].cigar and back[0]["seq"] == "GGACGTAACG"
    assert ref.aligned_bases(back[0]) == "ACGTA--ACG"
    assert ref.alignment_score(back[0]) == 200 and ref.alignment_score(back[1]) == 0


@pytest.mark.parametrize("name", ["test1", "test2", "test3", "soft_clipping", "hard_clipping", "insert_at_end"])
def test_scan_fixtures(name):
    refs, recs = bw.read_bam(fx(name))
    s = bam_pileup.bam_scan(fx(name))
    assert s["n_ref"] == len(refs) == 1
    assert s["n_records"] == len(recs)
    assert s["sorted"]
    assert s["n_unmapped"] == sum(r["ref"] < 0 for r in recs)
    assert list(s["records_per_ref"]) == [sum(r["ref"] == 0 for r in recs)]
    assert s["n_blocks"] >= 2  # data + EOF


@pytest.mark.parametrize("threads", [1, 16])
def test_scan_synthetic(tmp_path, threads):
    paths = bw.synthetic_set(tmp_path, n_cells=2, pairs_per_cell=400, n_refs=3, seed=3)
    for path in paths:
        refs, recs = bw.read_bam(path)
        s = bam_pileup.bam_scan(path, num_threads=threads)
        assert s["n_ref"] == 3 and s["sorted"]
        assert s["n_blocks"] > 3  # more than one data block
        assert s["n_records"] == len(recs) and s["n_unmapped"] == 1
        assert list(s["records_per_ref"]) == [sum(r["ref"] == k for r in recs) for k in range(3)]


def test_scan_unsorted_and_corrupt(tmp_path):
    recs = [bw.Rec("a", 0, 50, [("M", 4)], "ACGT", qual=[30] * 4), bw.Rec("b", 0, 10, [("M", 4)], "ACGT",
                                                                          qual=[30] * 4)]
    path = str(tmp_path / "u.bam")
    bw.write_bam(path, [("1", 100)], recs)
    s = bam_pileup.bam_scan(path)
    assert not s["sorted"] and s["n_records"] == 2
    # a larger unsorted file (three references, an unmapped record first, more than one block): every count is
    # what the same records give in sorted order
    srt = bw.synthetic_set(tmp_path, n_cells=1, pairs_per_cell=400, n_refs=3, seed=5)[0]
    raw = gzip.decompress(open(srt, "rb").read())
    offs, o = [], 8 + struct.unpack_from("<i", raw, 4)[0]
    for _ in range(struct.unpack_from("<i", raw, o)[0]):
        o += 8 + struct.unpack_from("<i", raw, o + 4)[0]
    o += 4
    first = o
    while o < len(raw):
        offs.append(o)
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    body = b"".join(raw[a:b] for a, b in reversed(list(zip(offs, offs[1:] + [len(raw)]))))
    rev = str(tmp_path / "rev.bam")
    open(rev, "wb").write(bw.bgzf(raw[:first] + body))
    want, got = bam_pileup.bam_scan(srt), bam_pileup.bam_scan(rev)
    assert want["sorted"] and not got["sorted"] and got["n_unmapped"] == 1 and got["n_blocks"] > 3
    for k in ("n_ref", "n_records", "n_unmapped", "inflated_bytes", "l_text"):
        assert got[k] == want[k], k
    assert list(got["records_per_ref"]) == list(want["records_per_ref"])
    # unsorted and cut inside its last record: refused
    cut = str(tmp_path / "cut.bam")
    open(cut, "wb").write(bw.bgzf((raw[:first] + body)[:-7]))
    with pytest.raises(secedo_amd.SecedoError):
        bam_pileup.bam_scan(cut)
    data = bytearray(open(path, "rb").read())
    data[30] ^= 0xFF  # inside the first block's deflate data
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(data))
    with pytest.raises(secedo_amd.SecedoError):
        bam_pileup.bam_scan(bad)
    with pytest.raises(secedo_amd.SecedoError):
        bam_pileup.bam_scan(str(tmp_path / "missing.bam"))


def test_cli_arguments(tmp_path):
    a = pileup_main.parse_args(["-i", "x", "-o", "y"])
    assert a.chromosomes.split(",")[12:14] == ["13", "14"] and a.chromosomes.endswith("X,Y")
    assert (a.num_threads, a.min_base_quality, a.min_map_quality, a.min_map_score, a.max_coverage,
            a.min_different) == (8, 30, 30, 0, 100, 3)
    a = pileup_main.parse_args(["-i", "x", "-o", "y", "--chromosomes", "1,X", "--num_threads", "64",
                                "--max_coverage=50"])
    assert a.chromosomes == "1,X" and a.max_coverage == 50
    assert pileup_main.chromosome_to_id("1") == 0 and pileup_main.chromosome_to_id("X") == 22
    assert pileup_main.chromosome_to_id("Y") == 23
    assert pileup_main.pool_size(64) == 16 and pileup_main.pool_size(0) == 1
    files = pileup_main.input_files(BAM)
    assert [os.path.basename(f) for f in files] == sorted(os.path.basename(f) for f in files)
    assert all(f.endswith(".bam") for f in files) and len(files) == 6
    with pytest.raises(SystemExit):
        pileup_main.main(["-i", BAM, "-o", str(tmp_path)])  # -o must be a prefix, not a directory
    cell_map = pileup_main.cell_map_lines(["/d/cellA_1.bam", "/d/cellB_x_2.bam"])
    assert cell_map == ["cellA\t0\n", "cellB_x\t1\n"]
