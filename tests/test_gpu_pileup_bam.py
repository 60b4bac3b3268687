"""Pileup creation from BAM files on the GPU (libsecedo_bam.so): the written .bin and .map equal the Python
restatement of the reference's pileup_bams() (tests/pileup_bam_ref.py) byte for byte, the .txt wherever a locus
has at most 16 entries, on the reference's fixtures and on seeded synthetic sets; the batch-slot read-name
maps, the multi-chromosome and resident outputs, determinism, the reference's abort cases as errors, and a
clone tree run from BAMs through divide_cluster_resident."""
import os

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_writer as bw
from tests import pileup_bam_ref as ref
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "bam")


def fx(name):
    return os.path.join(BAM, name + ".bam")


def txt_upto16(text):
    return [l for l in text.splitlines() if int(l.split("\t")[2]) <= 16]


def run_both(files, out, chromosome, max_cov, min_bq, min_mq, min_as, min_diff, threads=4):
    got = bam_pileup.pileup_bams(files, out, True, chromosome, max_cov, min_bq, min_mq, min_as, threads, min_diff)
    want = ref.pileup_bams(files, chromosome, max_cov, min_bq, min_mq, min_as, min_diff)
    assert open(out + ".bin", "rb").read() == want.bin_bytes()
    assert open(out + ".map").read() == want.map_text()
    assert txt_upto16(open(out + ".txt").read()) == txt_upto16(want.txt_text())
    assert got.n_loci == len(want.loci)
    for l, (pos, rids, cbs) in enumerate(want.loci):
        b, e = int(got.locus_entry_off[l]), int(got.locus_entry_off[l + 1])
        assert int(got.locus_pos[l]) == pos
        assert got.read_ids[b:e].tolist() == rids and got.id_base[b:e].tolist() == cbs
    return got, want


# the cases of the reference's tests/test_pileup.cpp: (files, max_coverage, min_map_quality, min_alignment_score,
# min_different, expected loci)
FIXTURE_CASES = [
    (["test1"] * 3 + ["test2"] * 2, 10, 0, 0, 3, 0),
    (["test1"] * 3 + ["test2"] * 2, 10, 0, 0, 1, 9),
    (["test1", "test2"], 10, 0, 0, 1, 9),
    (["soft_clipping", "test2"], 10, 0, 0, 1, 9),
    (["hard_clipping", "test2"], 10, 0, 0, 1, 9),
    (["insert_at_end", "test2"], 10, 0, 0, 1, 9),
    (["test1", "test2"], 10, 7, 0, 1, 0),
    (["test1", "test2"], 10, 6, 0, 1, 9),
    (["test3", "test3"], 10, 0, 10, 0, 168),
    (["test3", "test3"], 10, 0, 85, 1, 0),
    (["test3", "test3"], 10, 0, 80, 0, 84),
]


@pytest.mark.parametrize("case", range(len(FIXTURE_CASES)))
def test_fixture_cases(case, tmp_path):
    names, max_cov, mq, score, diff, n_loci = FIXTURE_CASES[case]
    out = str(tmp_path / "p")
    got, _ = run_both([fx(n) for n in names], out, 0, max_cov, 1, mq, score, diff)
    assert got.n_loci == n_loci
    if n_loci == 9 and len(names) == 2:  # test_pileup.cpp read_file / soft / hard clipping / insert at end
        flat, cells, max_len = secedo_amd.read_pileup(out + ".bin", [0, 1])
        assert max_len == 423 and cells == 2 and flat.n_loci == 9


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth")
    return bw.synthetic_set(d, n_cells=8, pairs_per_cell=60, n_refs=2, seed=11)


@pytest.mark.parametrize("params", [(100, 30, 30, 0, 3), (100, 0, 0, 0, 0), (6, 20, 10, 50, 1), (100, 35, 0, 90, 2)])
@pytest.mark.parametrize("chromosome", [0, 1])
def test_synthetic_sets(synth, params, chromosome, tmp_path):
    max_cov, min_bq, min_mq, min_as, diff = params
    got, want = run_both(synth, str(tmp_path / "s"), chromosome, max_cov, min_bq, min_mq, min_as, diff)
    if params[1] == 0:
        assert got.n_loci > 100 and int(got.locus_pos.max()) > 1_000_000  # loci on both sides of the chunk


def test_deterministic_and_pool_size(synth, tmp_path):
    outs = []
    for k, threads in enumerate([1, 16, 16]):
        out = str(tmp_path / ("d%d" % k))
        bam_pileup.pileup_bams(synth, out, True, 0, 100, 0, 0, 0, threads, 0)
        outs.append(tuple(open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt")))
    assert outs[0] == outs[1] == outs[2]


def test_101_files_share_slot_maps(tmp_path):
    paths = []
    for f in range(102):
        recs = [bw.Rec("shared", 0, 100, [("M", 8)], "ACGTACGT", qual=[40] * 8),
                bw.Rec("own%d" % f, 0, 104, [("M", 8)], "CCGTACGT" if f % 2 else "ACGTACGT", qual=[40] * 8)]
        path = str(tmp_path / ("f%03d.bam" % f))
        bw.write_bam(path, [("1", 1000)], recs)
        paths.append(path)
    out = str(tmp_path / "p")
    got, want = run_both(paths, out, 0, 1000, 0, 0, 0, 0)
    ids = {}
    b, e = int(got.locus_entry_off[0]), int(got.locus_entry_off[1])
    for rid, cb in zip(got.read_ids[b:e], got.id_base[b:e]):
        ids[int(cb) >> 2] = int(rid)
    assert ids[0] == ids[100] and ids[1] == ids[101] and ids[0] != ids[1]


def test_multi_chromosome_and_resident(synth, tmp_path):
    i2g = (np.arange(len(synth)) // 2).astype(np.uint16)
    per = []
    for c in (0, 1):
        out = str(tmp_path / ("c%d" % c))
        bam_pileup.pileup_bams(synth, out, False, c, 100, 20, 0, 0, 4, 1)
        per.append(secedo_amd.read_pileup(out + ".bin", i2g))
    assert per[0][0].n_loci > 0 and per[1][0].n_loci > 0
    assert os.path.getsize(str(tmp_path / "c0.txt")) == 0  # created empty without write_text_file
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, cells, max_len = bam_pileup.pileup_bams_resident(plan, synth, [0, 1], 100, 20, 0, 0, 4, 1,
                                                              id_to_group=i2g)
        got = {k: res[k].cpu().numpy() for k in ("chr", "pos", "off", "rid", "idb")}
    assert res["n_chr"] == 2 and res["idb_is16"]
    assert got["chr"].tolist() == [0, per[0][0].n_loci, per[0][0].n_loci + per[1][0].n_loci]
    pos = np.concatenate([p[0].locus_pos for p in per])
    rid = np.concatenate([p[0].read_ids for p in per])
    idb = np.concatenate([p[0].id_base for p in per])
    off = np.concatenate([per[0][0].locus_entry_off, per[1][0].locus_entry_off[1:] + per[0][0].n_entries])
    L, E = len(pos), len(rid)
    assert np.array_equal(got["pos"][:L].view(np.uint32), pos)
    assert np.array_equal(got["off"][:L + 1].view(np.uint64), off)
    assert np.array_equal(got["rid"][:E].view(np.uint32), rid)
    assert np.array_equal(got["idb"][:E].view(np.uint16).astype(np.uint32), idb)
    assert cells == max(p[1] for p in per) and max_len == max(p[2] for p in per)


def _abort_case(tmp_path, recs, **kw):
    path = str(tmp_path / "a.bam")
    bw.write_bam(path, [("1", 3_000_000)], recs)
    with pytest.raises(ref.RefAbort):
        ref.pileup_bams([path], 0, 100, 0, kw.get("mq", 0), 0, 0)
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams([path], str(tmp_path / "o"), True, 0, 100, 0, kw.get("mq", 0), 0, 1, 0)
    assert e.value.code == -1 and "file 0, record" in str(e.value)


def test_abort_cases_are_errors(tmp_path):
    good = bw.Rec("g", 0, 10, [("M", 4)], "ACGT", qual=[40] * 4)
    _abort_case(tmp_path, [good, bw.Rec("x", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4, flag=0x1)])
    _abort_case(tmp_path, [good, bw.Rec("x", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4, flag=0x3 | 0x200)])
    far = bw.Rec("x", 0, 999_000, [("M", 10), ("D", 2000), ("M", 10)], "A" * 20, qual=[40] * 20, mapq=5)
    _abort_case(tmp_path, [good, far])
    # the same read filtered out by its mapping quality is fine in both
    path = str(tmp_path / "f.bam")
    bw.write_bam(path, [("1", 3_000_000)], [good, far])
    bam_pileup.pileup_bams([path], None, False, 0, 100, 0, 6, 0, 1, 0)
    ref.pileup_bams([path], 0, 100, 0, 6, 0, 0)
    _abort_case(tmp_path, [good, bw.Rec("x", 0, 20, [("M", 10), ("I", 5), ("S", 5)], "A" * 20, qual=[40] * 20)])


def test_clone_tree_from_bams(tmp_path):
    """A clone tree written as BAMs -> pileup_bams_resident -> divide_cluster_resident gives the clusters of the
    same BAMs piled up to a .bin and run through read_pileup and the existing resident path."""
    from secedo_amd import cluster
    from tests.clone_tree_gen import clone_tree
    n = 240
    p, truth = clone_tree(n, n_b=140, n_loci=3000, f_ab=0.5, f_a12=0.05, seed=3)
    per_cell = [[] for _ in range(n)]
    for l in range(p.n_loci):
        for e in range(int(p.locus_entry_off[l]), int(p.locus_entry_off[l + 1])):
            c, b = int(p.id_base[e]) >> 2, int(p.id_base[e]) & 3
            per_cell[c].append(bw.Rec("e%d" % e, 0, 1000 + 10 * l, [("M", 1)], "ACGT"[b], qual=[40]))
    paths = []
    for c in range(n):
        path = str(tmp_path / ("cell_%03d.bam" % c))
        bw.write_bam(path, [("1", 1_000_000)], per_cell[c])
        paths.append(path)
    ident = np.arange(n)
    args = (ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, cells, max_len = bam_pileup.pileup_bams_resident(plan, paths, [0], 1000, 0, 0, 0, 8, 0)
        cl, idx, recs = cluster.divide_cluster_resident(plan, res, max(max_len, 1), *args, "ADD_MIN", "BIC",
                                                        "SPECTRAL6", False, True, 40)
    out = str(tmp_path / "tree")
    bam_pileup.pileup_bams(paths, out, False, 0, 1000, 0, 0, 0, 8, 0)
    fp, cells2, max_len2 = secedo_amd.read_pileup(out + ".bin", ident.astype(np.uint16), max_coverage=1000)
    assert (cells, max_len) == (cells2, max_len2) and cells == n
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res2 = plan.upload(fp, ident.astype(np.uint32), n)
        cl2, idx2, recs2 = cluster.divide_cluster_resident(plan, res2, max(max_len2, 1), *args, "ADD_MIN", "BIC",
                                                           "SPECTRAL6", False, True, 40)
    assert np.array_equal(cl, cl2) and idx == idx2 and recs == recs2
    assert recs[0]["stop_reason"] == "split"


def test_cli_writes_what_read_pileup_expects(tmp_path):
    """python -m secedo_amd.pileup_main on a directory holding test1.bam and test2.bam: the reference's read_file
    expectations on <o>_1.pileup.bin, and the cell map."""
    import shutil
    import subprocess
    import sys
    d = tmp_path / "in"
    d.mkdir()
    shutil.copy(fx("test1"), d / "cellA_1.bam")
    shutil.copy(fx("test2"), d / "cellB_2.bam")
    o = str(tmp_path / "x")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "secedo_amd.pileup_main", "-i", str(d), "-o", o, "--chromosomes", "1",
                        "--min_base_quality", "1", "--min_map_quality", "0", "--max_coverage", "10",
                        "--min_different", "1"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    flat, cells, max_len = secedo_amd.read_pileup(o + "_1.pileup.bin", [0, 1])
    assert (flat.n_loci, cells, max_len) == (9, 2, 423)
    assert open(o + "_1.map").read() == "cellA\t0\ncellB\t1\n"
    want = ref.pileup_bams([fx("test1"), fx("test2")], 0, 10, 1, 0, 0, 1)
    assert open(o + "_1.pileup.bin", "rb").read() == want.bin_bytes()
    assert open(o + "_1.pileup.txt").read() == want.txt_text()
