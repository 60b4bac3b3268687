"""Tag mode of the pileup creation (multiplexed BAMs, cell = barcode tag value): every output equals the per-file
run on the per-cell split files of tests/multiplex_bam.py -- .bin and .map byte for byte, .txt wherever a locus has
at most 16 entries, the resident flat layout, num_cells and max_read_length. Also the barcode census, the list
errors, block-range inflate of a large file, determinism, the CLI and a clone tree through divide_cluster."""
import os
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_writer as bw
from tests import multiplex_bam as mx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def txt_upto16(text):
    return [l for l in text.splitlines() if int(l.split("\t")[2]) <= 16]


def files_of(out):
    return tuple(open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt"))


def compare(lanes, split, barcodes, out, chromosome, params=(100, 0, 0, 0, 0), threads=4, tag="CB"):
    """Tag mode on the lanes against per-file mode on the split files: files and returned pileups equal."""
    max_cov, min_bq, min_mq, min_as, diff = params
    got = bam_pileup.pileup_bams(lanes, out + "_tag", True, chromosome, max_cov, min_bq, min_mq, min_as, threads,
                                 diff, cell_tag=tag, cells=barcodes)
    want = bam_pileup.pileup_bams(split, out + "_cell", True, chromosome, max_cov, min_bq, min_mq, min_as, threads,
                                  diff)
    gb, gm, gt = files_of(out + "_tag")
    wb, wm, wt = files_of(out + "_cell")
    assert gb == wb and gm == wm
    assert txt_upto16(gt.decode()) == txt_upto16(wt.decode())
    for k in ("locus_pos", "locus_entry_off", "read_ids", "id_base"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    return got


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("cells")
    refs, cells = mx.synthetic_cells(d / "orig", n_cells=8, pairs_per_cell=60, n_refs=2, seed=11)
    barcodes = ["AAACCTGAGC-%d" % c for c in range(len(cells))]
    recs = [r for cell in mx.tagged(cells, barcodes) for r in cell]
    out = {}
    for lanes in (1, 3):
        md, sd = d / ("mux%d" % lanes), d / ("split%d" % lanes)
        md.mkdir()
        sd.mkdir()
        paths = mx.write_multiplexed(md, refs, recs, n_lanes=lanes, seed=4)
        out[lanes] = (paths, mx.split(sd, refs, paths, barcodes))
    return dict(refs=refs, cells=cells, barcodes=barcodes, recs=recs, sets=out, dir=d)


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("params", [(100, 0, 0, 0, 0), (100, 30, 30, 0, 3), (6, 20, 10, 50, 1)])
def test_lanes_equal_split_files(synth, lanes, params, tmp_path):
    paths, split = synth["sets"][lanes]
    for chromosome in (0, 1):
        got = compare(paths, split, synth["barcodes"], str(tmp_path / ("c%d" % chromosome)), chromosome, params)
        if params[1] == 0:
            assert got.n_loci > 100 and int(got.locus_pos.max()) > 1_000_000  # loci on both sides of the chunk


def test_102_cells_share_slot_maps(tmp_path):
    cells = []
    for f in range(102):
        cells.append([bw.Rec("shared", 0, 100, [("M", 8)], "ACGTACGT", qual=[40] * 8),
                      bw.Rec("own%d" % f, 0, 104, [("M", 8)], "CCGTACGT" if f % 2 else "ACGTACGT", qual=[40] * 8)])
    barcodes = ["B%03d" % f for f in range(102)]
    recs = [r for c in mx.tagged(cells, barcodes) for r in c]
    refs = [("1", 1000)]
    paths = mx.write_multiplexed(tmp_path, refs, recs)
    split = mx.split(tmp_path, refs, paths, barcodes)
    got = compare(paths, split, barcodes, str(tmp_path / "p"), 0, (1000, 0, 0, 0, 0))
    ids = {}
    b, e = int(got.locus_entry_off[0]), int(got.locus_entry_off[1])
    for rid, cb in zip(got.read_ids[b:e], got.id_base[b:e]):
        ids[int(cb) >> 2] = int(rid)
    assert ids[0] == ids[100] and ids[1] == ids[101] and ids[0] != ids[1]


def test_shuffled_list_orders_cells(synth, tmp_path):
    paths, _ = synth["sets"][3]
    order = np.random.default_rng(8).permutation(len(synth["barcodes"]))
    barcodes = [synth["barcodes"][k] for k in order]
    sd = tmp_path / "split"
    sd.mkdir()
    split = mx.split(sd, synth["refs"], paths, barcodes)
    got = compare(paths, split, barcodes, str(tmp_path / "s"), 0)
    cells = np.unique(got.id_base >> 2)
    assert len(cells) == len(barcodes)
    # cell k of the output is barcode order[k] of the original numbering: odd original cells carry the variant
    assert not np.array_equal(order, np.arange(len(order)))


def test_unlisted_untagged_and_typed_records_are_dropped(synth, tmp_path):
    refs, barcodes = synth["refs"], synth["barcodes"]
    recs = list(synth["recs"])
    extra = []
    for k in range(40):
        pos = 999_700 + 13 * k
        extra.append(bw.Rec("untagged%d" % k, 0, pos, [("M", 30)], "ACGT" * 7 + "AC", qual=[40] * 30))
        extra.append(bw.Rec("typed%d" % k, 0, pos, [("M", 30)], "C" * 30, qual=[40] * 30,
                            tags=[("CB", "i", 3), ("CB", "Z", barcodes[0])]))  # the first CB counts: not Z
        extra.append(bw.Rec("other%d" % k, 0, pos, [("M", 30)], "G" * 30, qual=[40] * 30,
                            tags=[("CB", "Z", "NOTLISTED-%d" % (k % 3))]))
    # an improper pair of an unlisted barcode is no error: it is not selected
    extra.append(bw.Rec("bad", 0, 999_800, [("M", 10)], "A" * 10, qual=[40] * 10, flag=0x1,
                        tags=[("CB", "Z", "NOTLISTED-0")]))
    (tmp_path / "m").mkdir()
    (tmp_path / "s").mkdir()
    paths = mx.write_multiplexed(tmp_path / "m", refs, recs + extra, n_lanes=2, seed=9)
    split = mx.split(tmp_path / "s", refs, paths, barcodes)
    compare(paths, split, barcodes, str(tmp_path / "d"), 0)
    with pytest.raises(secedo_amd.SecedoError):  # the improper pair fails once its barcode is listed
        bam_pileup.pileup_bams(paths, None, False, 0, 100, 0, 0, 0, 4, 0, cell_tag="CB",
                               cells=barcodes + ["NOTLISTED-0"])


def test_resident_multi_chromosome_with_groups(synth, tmp_path):
    paths, split = synth["sets"][3]
    barcodes = synth["barcodes"]
    i2g = (np.arange(len(barcodes)) // 2).astype(np.uint16)
    per = []
    for c in (0, 1):
        out = str(tmp_path / ("c%d" % c))
        bam_pileup.pileup_bams(paths, out, False, c, 100, 20, 0, 0, 4, 1, cell_tag="CB", cells=barcodes)
        per.append(secedo_amd.read_pileup(out + ".bin", i2g))
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, cells, max_len = bam_pileup.pileup_bams_resident(plan, paths, [0, 1], 100, 20, 0, 0, 4, 1,
                                                              id_to_group=i2g, cell_tag="CB", cells=barcodes)
        got = {k: res[k].cpu().numpy() for k in ("chr", "pos", "off", "rid", "idb")}
        res2, cells2, max_len2 = bam_pileup.pileup_bams_resident(plan, split, [0, 1], 100, 20, 0, 0, 4, 1,
                                                                 id_to_group=i2g)
        want = {k: res2[k].cpu().numpy() for k in ("chr", "pos", "off", "rid", "idb")}
    assert (cells, max_len) == (cells2, max_len2)
    assert cells == max(p[1] for p in per) and max_len == max(p[2] for p in per)
    L, E = res["n_loci"], res["n_entries"]
    assert (L, E) == (res2["n_loci"], res2["n_entries"]) and L > 0
    assert got["chr"].tolist() == [0, per[0][0].n_loci, per[0][0].n_loci + per[1][0].n_loci]
    for k, n in (("chr", 3), ("pos", L), ("off", L + 1), ("rid", E), ("idb", E)):
        assert np.array_equal(got[k][:n], want[k][:n]), k
    pos = np.concatenate([p[0].locus_pos for p in per])
    idb = np.concatenate([p[0].id_base for p in per])
    assert np.array_equal(got["pos"][:L].view(np.uint32), pos)
    assert np.array_equal(got["idb"][:E].view(np.uint16).astype(np.uint32), idb)


def test_bam_barcodes_counts(synth, tmp_path):
    refs = synth["refs"]
    recs = list(synth["recs"])
    recs.append(bw.Rec("u", 0, 999_000, [("M", 4)], "ACGT", qual=[40] * 4))
    recs.append(bw.Rec("t", 1, 999_000, [("M", 4)], "ACGT", qual=[40] * 4, tags=[("CB", "i", 5)]))
    recs.append(bw.Rec("z", 1, 999_001, [("M", 4)], "ACGT", qual=[40] * 4, tags=[("CB", "Z", "ZZZ-9")]))
    paths = mx.write_multiplexed(tmp_path, refs, recs, n_lanes=3, seed=1)
    for chroms in ([0], [1], [0, 1]):
        vals, counts = bam_pileup.bam_barcodes(paths, "CB", chroms, num_threads=4)
        want = {}
        for r in recs:
            b = mx.barcode_of(r, "CB")
            if r.ref in chroms and b is not None:
                want[b] = want.get(b, 0) + 1
        keys = sorted(want, key=lambda s: s.encode())
        assert vals == keys
        assert counts.dtype == np.uint64 and counts.tolist() == [want[k] for k in keys]
    assert bam_pileup.bam_barcodes(paths, "XX", [0, 1])[0] == []


def test_list_errors(synth, tmp_path):
    paths, _ = synth["sets"][1]
    bcs = synth["barcodes"]
    run = lambda cells, tag="CB": bam_pileup.pileup_bams(paths, None, False, 0, 100, 0, 0, 0, 2, 0, cell_tag=tag,
                                                         cells=cells)
    for cells, tag, code in ((bcs + [bcs[3]], "CB", -1), ([], "CB", -1), (bcs, "1B", -1), (bcs, "C_", -1),
                             (["B%05d" % k for k in range(16385)], "CB", -6)):
        with pytest.raises(secedo_amd.SecedoError) as e:
            run(cells, tag)
        assert e.value.code == code, (tag, len(cells))
    run(["B%05d" % k for k in range(16383)] + [bcs[0]])  # 16384 barcodes are fine
    # a listed improper pair: the message names the input file and its record index there
    good = bw.Rec("g", 0, 10, [("M", 4)], "ACGT", qual=[40] * 4, tags=[("CB", "Z", "A")])
    bad = bw.Rec("x", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4, flag=0x1, tags=[("CB", "Z", "B")])
    other = bw.Rec("o", 0, 5, [("M", 4)], "ACGT", qual=[40] * 4, tags=[("CB", "Z", "C")])
    f0, f1 = str(tmp_path / "f0.bam"), str(tmp_path / "f1.bam")
    bw.write_bam(f0, [("1", 3_000_000)], [good])
    bw.write_bam(f1, [("1", 3_000_000)], [other, good, bad])
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams([f0, f1], None, False, 0, 100, 0, 0, 0, 1, 0, cell_tag="CB", cells=["A", "B"])
    assert e.value.code == -1 and "file 1, record 2:" in str(e.value) and "proper pair" in str(e.value)


def test_block_ranges_give_identical_outputs(synth, tmp_path, monkeypatch):
    """SECEDO_BAM_BATCH_BYTES=65536: the one lane file inflates to many ranges, records cut at range ends."""
    paths, split = synth["sets"][1]
    assert bam_pileup.bam_scan(paths[0])["inflated_bytes"] > 3 * 65536
    want = {}
    for c in (0, 1):
        out = str(tmp_path / ("w%d" % c))
        bam_pileup.pileup_bams(paths, out, True, c, 100, 0, 0, 0, 4, 0, cell_tag="CB", cells=synth["barcodes"])
        want[c] = files_of(out)
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", "65536")
    for c in (0, 1):
        t = {}
        out = str(tmp_path / ("g%d" % c))
        bam_pileup.pileup_bams(paths, out, True, c, 100, 0, 0, 0, 4, 0, times=t, cell_tag="CB",
                               cells=synth["barcodes"])
        assert files_of(out) == want[c]
        assert t["inflated_bytes"] == bam_pileup.bam_scan(paths[0])["inflated_bytes"]
        compare(paths, split, synth["barcodes"], str(tmp_path / ("x%d" % c)), c)  # per-file mode under it too
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, cells, max_len = bam_pileup.pileup_bams_resident(plan, paths, [0, 1], 100, 0, 0, 0, 4, 0,
                                                              cell_tag="CB", cells=synth["barcodes"])
        assert res["n_loci"] > 0
    assert bam_pileup.bam_barcodes(paths, "CB", [0, 1])[0] == sorted(synth["barcodes"])


def test_deterministic_and_pool_size(synth, tmp_path):
    paths, _ = synth["sets"][3]
    outs = []
    for k, threads in enumerate([1, 16, 16]):
        out = str(tmp_path / ("d%d" % k))
        bam_pileup.pileup_bams(paths, out, True, 0, 100, 0, 0, 0, threads, 0, cell_tag="CB", cells=synth["barcodes"])
        outs.append(files_of(out))
    assert outs[0] == outs[1] == outs[2]


def _cli(args):
    r = subprocess.run([sys.executable, "-m", "secedo_amd.pileup_main", *args], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_cell_tag(synth, tmp_path):
    paths, split = synth["sets"][1]
    bcs = synth["barcodes"]
    common = ["--chromosomes", "1,2", "--min_base_quality", "0", "--min_map_quality", "0", "--min_different", "0"]
    d = tmp_path / "cells"
    d.mkdir()
    for c, p in enumerate(split):  # the per-cell directory route, named so that the cell map gives the barcodes
        os.symlink(p, str(d / ("%s_x.bam" % bcs[c])))
    _cli(["-i", str(d), "-o", str(tmp_path / "dir"), *common])
    lst = tmp_path / "barcodes.tsv"
    lst.write_text("".join(b + "\n" for b in bcs))
    _cli(["-i", paths[0], "-o", str(tmp_path / "list"), "--cell_tag", "CB", "--cells", str(lst), *common])
    _cli(["-i", paths[0], "-o", str(tmp_path / "auto"), "--cell_tag", "CB", *common])
    want_map = "".join("%s\t%d\n" % (b, c) for c, b in enumerate(bcs))
    assert sorted(bcs) == bcs
    for o in ("dir", "list", "auto"):
        assert open(str(tmp_path / (o + "_1,2.map"))).read() == want_map
    for chrom in ("1", "2"):
        want = open(str(tmp_path / ("dir_%s.pileup.bin" % chrom)), "rb").read()
        for o in ("list", "auto"):
            path = str(tmp_path / ("%s_%s.pileup.bin" % (o, chrom)))
            assert open(path, "rb").read() == want
            flat, cells, max_len = secedo_amd.read_pileup(path, np.arange(len(bcs)))
            assert flat.n_loci > 0 and cells == len(bcs)
    # --min_cell_records above every count: no cell left is an error
    r = subprocess.run([sys.executable, "-m", "secedo_amd.pileup_main", "-i", paths[0], "-o", str(tmp_path / "n"),
                        "--cell_tag", "CB", "--min_cell_records", "100000", *common], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0


def test_clone_tree_from_one_tagged_bam(tmp_path):
    """The clone tree of test_clone_tree_from_bams as one tagged BAM -> pileup_bams_resident(cell_tag) ->
    divide_cluster_resident gives the clusters of the per-cell route."""
    from secedo_amd import cluster
    from tests.clone_tree_gen import clone_tree
    n = 240
    p, truth = clone_tree(n, n_b=140, n_loci=3000, f_ab=0.5, f_a12=0.05, seed=3)
    per_cell = [[] for _ in range(n)]
    for l in range(p.n_loci):
        for e in range(int(p.locus_entry_off[l]), int(p.locus_entry_off[l + 1])):
            c, b = int(p.id_base[e]) >> 2, int(p.id_base[e]) & 3
            per_cell[c].append(bw.Rec("e%d" % e, 0, 1000 + 10 * l, [("M", 1)], "ACGT"[b], qual=[40]))
    refs = [("1", 1_000_000)]
    paths = []
    for c in range(n):
        path = str(tmp_path / ("cell_%03d.bam" % c))
        bw.write_bam(path, refs, per_cell[c])
        paths.append(path)
    barcodes = ["CELL-%03d" % c for c in range(n)]
    (tmp_path / "m").mkdir()
    merged = mx.write_multiplexed(tmp_path / "m", refs, [r for c in mx.tagged(per_cell, barcodes) for r in c])
    ident = np.arange(n)
    args = (ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01)
    out = []
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        for files, kw in ((paths, {}), (merged, dict(cell_tag="CB", cells=barcodes))):
            res, cells, max_len = bam_pileup.pileup_bams_resident(plan, files, [0], 1000, 0, 0, 0, 8, 0, **kw)
            cl, idx, recs = cluster.divide_cluster_resident(plan, res, max(max_len, 1), *args, "ADD_MIN", "BIC",
                                                            "SPECTRAL6", False, True, 40)
            out.append((cells, max_len, cl, idx, recs))
    (c1, m1, cl1, i1, r1), (c2, m2, cl2, i2, r2) = out
    assert (c1, m1) == (c2, m2) and c1 == n
    assert np.array_equal(cl1, cl2) and i1 == i2 and r1 == r2
    assert r1[0]["stop_reason"] == "split"
