"""SAM input on the GPU: a coordinate-sorted SAM file gives what the BAM of the same records gives, byte for byte
(.bin/.map/.txt, resident arrays, num_cells, max_read_length, barcodes), in per-file and tag mode, over ranges, mixed
with BAMs and with either pool size; parse, structural and rule-6 errors name the file and the 1-based line."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_writer as bw
from tests import multiplex_bam as mb
from tests import sam_writer as sw
from tests.golden_util import GOLDEN
from tests.test_gpu_pileup_bam import FIXTURE_CASES

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "bam")


def files_of(out):
    return tuple(open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt"))


def pile(files, out, chromosome=0, params=(100, 0, 0, 0, 0), threads=4, **kw):
    max_cov, min_bq, min_mq, min_as, diff = params
    p = bam_pileup.pileup_bams(files, out, True, chromosome, max_cov, min_bq, min_mq, min_as, threads, diff, **kw)
    return p, files_of(out)


def same(bams, sams, tmp_path, **kw):
    pb, fb = pile(bams, str(tmp_path / "b"), **kw)
    ps, fs = pile(sams, str(tmp_path / "s"), **kw)
    assert fs == fb
    assert ps.n_loci == pb.n_loci
    for k in ("chr_locus_off", "locus_pos", "locus_entry_off", "read_ids", "id_base"):
        assert np.array_equal(getattr(ps, k), getattr(pb, k)), k
    return ps


def fixture_sam(name, tmp_path):
    if name != "test1":
        return os.path.join(BAM, name + ".sam")
    fixed = tmp_path / "test1_fixed.sam"
    text = open(os.path.join(BAM, "test1.sam")).read()
    assert text.count("AS:i-90") == 1
    fixed.write_text(text.replace("AS:i-90", "AS:i:90"))
    return str(fixed)


@pytest.mark.parametrize("case", range(len(FIXTURE_CASES)))
def test_fixture_cases_from_sam(case, tmp_path):
    names, max_cov, mq, score, diff, n_loci = FIXTURE_CASES[case]
    bams = [os.path.join(BAM, n + ".bam") for n in names]
    sams = [fixture_sam(n, tmp_path) for n in names]
    p = same(bams, sams, tmp_path, params=(max_cov, 1, mq, score, diff))
    assert p.n_loci == n_loci


def test_test1_sam_as_is_names_line_5():
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams([os.path.join(BAM, "test1.sam")], None, False, 0, 10, 1, 0, 0, 1, 1)
    assert e.value.code == -1
    assert "file 0 (" in str(e.value) and "test1.sam), line 5" in str(e.value)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """bw.synthetic_set's cells, canonical, as BAM and SAM -> (refs, cell records, bams, sams)."""
    d = tmp_path_factory.mktemp("synth_sam")
    refs, cells = mb.synthetic_cells(d / "raw", n_cells=8, pairs_per_cell=60, n_refs=2, seed=11)
    bams, sams = [], []
    for c, recs in enumerate(cells):
        b, s = sw.write_both(d, "cell_%03d" % c, refs, recs)
        bams.append(b)
        sams.append(s)
    return refs, cells, bams, sams


@pytest.mark.parametrize("params", [(100, 30, 30, 0, 3), (100, 0, 0, 0, 0), (6, 20, 10, 50, 1), (100, 35, 0, 90, 2)])
@pytest.mark.parametrize("chromosome", [0, 1])
def test_synthetic_sets_from_sam(synth, params, chromosome, tmp_path):
    _, _, bams, sams = synth
    p = same(bams, sams, tmp_path, chromosome=chromosome, params=params)
    if params[1] == 0:
        assert p.n_loci > 100


def _resident(files, i2g, **kw):
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, cells, max_len = bam_pileup.pileup_bams_resident(plan, files, [0, 1], 100, 20, 0, 0, 4, 1,
                                                              id_to_group=i2g, **kw)
        return {k: res[k].cpu().numpy() for k in ("chr", "pos", "off", "rid", "idb")}, cells, max_len


def test_resident_two_chromosomes(synth):
    _, _, bams, sams = synth
    i2g = (np.arange(len(bams)) // 2).astype(np.uint16)
    gb, cb, lb = _resident(bams, i2g)
    gs, cs, ls = _resident(sams, i2g)
    assert (cs, ls) == (cb, lb) and gb["chr"][-1] > 0
    for k in gb:
        assert np.array_equal(gs[k], gb[k]), k


def test_small_ranges_give_identical_outputs(synth, tmp_path, monkeypatch):
    refs, cells, _, _ = synth
    recs = [r for c in mb.tagged(cells, ["B%02d" % c for c in range(len(cells))]) for r in c]
    bam, sam = sw.write_both(tmp_path, "big", refs, sorted(recs, key=bw.sort_key))
    assert os.path.getsize(sam) > 4 * 65536
    want = pile([bam], str(tmp_path / "w"))[1]
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", "65536")
    assert pile([sam], str(tmp_path / "r"))[1] == want
    assert pile([bam, sam], str(tmp_path / "m"))[1] == pile([bam, bam], str(tmp_path / "mb"))[1]


def test_mixed_list(synth, tmp_path):
    _, _, bams, sams = synth
    same(bams[:3], [bams[0], sams[1], bams[2]], tmp_path)


def test_tag_mode_and_barcodes(synth, tmp_path):
    refs, cells, _, _ = synth
    barcodes = ["AAC%02d-1" % c for c in range(len(cells))]
    recs = [r for c in mb.tagged(cells, barcodes) for r in c]
    bams, sams = sw.write_multiplexed(tmp_path, refs, recs, n_lanes=2, seed=4)
    listed = barcodes[::-1][:6]
    for chromosome in (0, 1):
        same(bams, sams, tmp_path, chromosome=chromosome, cell_tag="CB", cells=listed)
    vb, cb = bam_pileup.bam_barcodes(bams, "CB", [0, 1], 4)
    vs, cs = bam_pileup.bam_barcodes(sams, "CB", [0, 1], 4)
    assert vs == vb == sorted(barcodes) and np.array_equal(cs, cb)


def _err(tmp_path, text, name="e.sam", files=None):
    path = tmp_path / name
    path.write_text(text)
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams(files or [str(path)], None, False, 0, 100, 0, 0, 0, 1, 0)
    return e.value


HEAD = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:1\tLN:3000000\n@CO\tc\n"
GOOD = "g\t67\t1\t11\t60\t4M\t=\t11\t0\tACGT\tIIII\n"


@pytest.mark.parametrize("bad,code", [
    ("x\t67\t1\t21\t60\t4M\t=\t21\t0\tACGT\n", -1),                 # ten fields
    ("x\t67\t2\t21\t60\t4M\t=\t21\t0\tACGT\tIIII\n", -1),           # RNAME not in @SQ
    ("x\t67\t1\t21\t60\t4M\t9\t21\t0\tACGT\tIIII\n", -1),           # RNEXT not in @SQ
    ("x\t67\t1\t21\t60\t4Q\t=\t21\t0\tACGT\tIIII\n", -1),           # CIGAR op
    ("x\t67\t1\t21\t60\t5M\t=\t21\t0\tACGT\tIIII\n", -1),           # CIGAR against SEQ
    ("x\t67\t1\t21\t60\t4M\t=\t21\t0\tACGT\tIII\n", -1),            # QUAL length
    ("x\t67\t1\t21\t256\t4M\t=\t21\t0\tACGT\tIIII\n", -1),          # MAPQ range
    ("x\t-1\t1\t21\t60\t4M\t=\t21\t0\tACGT\tIIII\n", -1),           # FLAG sign
    ("x\t67\t1\t21\t60\t4M\t=\t21\t0\tACGT\tIIII\tAS:i-90\n", -1),  # aux without its second ':'
    ("x\t67\t1\t21\t60\t4M\t=\t21\t0\tACGT\tIIII\tAS:i:4294967296\n", -1),
    ("x\t67\t1\t21\t60\t4M\t=\t21\t0\tACGT\tIIII\tXB:B:c,200\n", -1),
    ("x\t67\t1\t21\t60\t4M\t=\t21\t0\tACGT\tIIII\tXX:Q:1\n", -1),
    ("@CO\tlate\n", -1),                                                  # header after the first record
    ("\n", -1),                                                           # empty line inside the file
    ("x\t67\t1\t5\t60\t4M\t=\t5\t0\tACGT\tIIII\n", -1),              # not sorted
    ("x\t67\t1\t0\t60\t4M\t=\t1\t0\tACGT\tIIII\n", -1),              # POS 0 -> -1: not sorted either
    ("x\t1\t1\t21\t60\t4M\t=\t21\t0\tACGT\tIIII\n", -1),             # rule 6: not a proper pair
])
def test_errors_name_the_line(bad, code, tmp_path):
    # the bad line is line 5 (three header lines, a good record), followed by a good line
    e = _err(tmp_path, HEAD + GOOD + bad + "y\t67\t1\t30\t60\t4M\t=\t30\t0\tACGT\tIIII\n")
    assert e.code == code and ", line 5" in str(e), str(e)
    assert "file 0 (" + str(tmp_path / "e.sam") + ")" in str(e)
    if not bad.startswith("x\t1\t"):  # a parse error: of several bad lines, the first one is reported
        e = _err(tmp_path, HEAD + GOOD + bad + "z\t67\t1\t31\tbad\n" * 300, "e2.sam")
        assert ", line 5" in str(e), str(e)


def test_rule6_errors_name_the_line(tmp_path):
    """test_abort_cases_are_errors of the BAM route with SAM input: the message names the line."""
    refs = [("1", 3_000_000)]
    good = bw.Rec("g", 0, 10, [("M", 4)], "ACGT", qual=[40] * 4)
    cases = [bw.Rec("x", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4, flag=0x1),
             bw.Rec("x", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4, flag=0x3 | 0x200),
             bw.Rec("x", 0, 999_000, [("M", 10), ("D", 2000), ("M", 10)], "A" * 20, qual=[40] * 20, mapq=5),
             bw.Rec("x", 0, 20, [("M", 10), ("I", 5), ("S", 5)], "A" * 20, qual=[40] * 20)]
    for k, bad in enumerate(cases):
        path = str(tmp_path / ("a%d.sam" % k))
        sw.write_sam(path, refs, [good, bad])
        with pytest.raises(secedo_amd.SecedoError) as e:
            bam_pileup.pileup_bams([path], None, False, 0, 100, 0, 0, 0, 1, 0)
        assert e.value.code == -1 and ("file 0 (%s), line 4:" % path) in str(e.value), str(e.value)
    # tag mode names the line too
    path = str(tmp_path / "t.sam")
    sw.write_sam(path, refs, mb.tagged([[good, cases[0]]], ["A"])[0])
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams([path], None, False, 0, 100, 0, 0, 0, 1, 0, cell_tag="CB", cells=["A"])
    assert ("file 0 (%s), line 4:" % path) in str(e.value)


def test_limits_and_edge_lines(tmp_path):
    ops = "".join("1M1I" for _ in range(32768))
    e = _err(tmp_path, HEAD + "x\t67\t1\t21\t60\t%s\t=\t21\t0\t%s\t*\n" % (ops, "A" * 65536))
    assert e.code == -6 and ", line 4" in str(e)  # SECEDO_E_LIMIT, more than 65535 ops
    # a last line without '\n' and a final empty line are fine; the same records as the plain file
    plain = tmp_path / "p.sam"
    plain.write_text(HEAD + GOOD + GOOD.replace("g\t", "h\t"))
    a = pile([str(plain)], str(tmp_path / "pa"))[1]
    nolf = tmp_path / "q.sam"
    nolf.write_text(HEAD + GOOD + GOOD.replace("g\t", "h\t").rstrip("\n"))
    trail = tmp_path / "r.sam"
    trail.write_text(HEAD + GOOD + GOOD.replace("g\t", "h\t") + "\n")
    assert pile([str(nolf)], str(tmp_path / "pb"))[1] == a == pile([str(trail)], str(tmp_path / "pc"))[1]
    # @SQ needs SN and LN, once each
    e = _err(tmp_path, "@HD\tVN:1.6\n@SQ\tSN:1\n" + GOOD, "h.sam")
    assert "line 2" in str(e)
    e = _err(tmp_path, "@SQ\tSN:1\tLN:9\n@SQ\tSN:1\tLN:9\n" + GOOD, "h2.sam")
    assert "line 2" in str(e) and "twice" in str(e)


def test_plain_gzip_is_refused(tmp_path):
    path = tmp_path / "x.sam.gz"
    path.write_bytes(gzip.compress((HEAD + GOOD).encode()))
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams([str(path)], None, False, 0, 100, 0, 0, 0, 1, 0)
    assert e.value.code == -1 and "not BGZF" in str(e.value) and "decompress" in str(e.value)


def test_cli_on_sam_directory(synth, tmp_path):
    _, _, bams, sams = synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for kind, files in (("bam", bams), ("sam", sams)):
        d = tmp_path / kind
        d.mkdir()
        for f in files[:4]:
            shutil.copy(f, d / os.path.basename(f))
        o = str(tmp_path / ("o_" + kind))
        r = subprocess.run([sys.executable, "-m", "secedo_amd.pileup_main", "-i", str(d), "-o", o, "--chromosomes",
                            "1,2", "--min_base_quality", "0", "--min_map_quality", "0", "--min_different", "0"],
                           cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append([open(o + s, "rb").read() for s in ("_1,2.map", "_1.pileup.bin", "_1.pileup.map",
                                                         "_1.pileup.txt", "_2.pileup.bin", "_2.pileup.txt")])
    assert outs[0] == outs[1] and len(outs[0][1]) > 0


@pytest.mark.parametrize("threads", [1, 16])
def test_pool_sizes(synth, tmp_path, threads):
    _, _, bams, sams = synth
    same(bams, sams, tmp_path, threads=threads)
