"""``secedo_amd.bin_depth`` on the GPU against tests/depth_expected.py: every fetched array and every byte of every
file, per-file and tag mode, both counting modes, the bin, block and selection edges, every input route, the cluster
sums, both outputs and the refusals. Each test asserts its own preconditions from the expected data."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_select_ref as ref
from tests import bam_writer as bw
from tests import depth_expected as de
from tests import sam_writer as sw
from tests import split_expected as se

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = secedo_amd._lib.E_INVALID_ARG


def write_cells(directory, refs, cells, stem="cell"):
    os.makedirs(str(directory), exist_ok=True)
    paths = []
    for c, recs in enumerate(cells):
        paths.append(os.path.join(str(directory), "%s_%03d.bam" % (stem, c)))
        bw.write_bam(paths[-1], refs, recs)
    return paths


def read_outputs(out_dir, bgzf=False):
    """{plain file name: inflated bytes} of <out_dir>/depth/; the names must be exactly those of the output kind."""
    d = os.path.join(str(out_dir), "depth")
    got = {}
    for name in sorted(os.listdir(d)):
        raw = open(os.path.join(d, name), "rb").read()
        if name.endswith(".gz"):
            assert bgzf and name[:-3] in de.GZ_FILES, name
            assert raw.endswith(se.EOF) and all(isize <= se.CUT for isize, _ in se.member_sizes(raw))
            got[name[:-3]] = gzip.decompress(raw)  # every CRC32 and ISIZE
        else:
            assert not bgzf or name in de.PLAIN_FILES, name
            got[name] = raw
    return got


def check(out, e, out_dir=None, bgzf=False):
    """The fetched arrays, the stats and (with out_dir) the files against the expected ones."""
    bins = np.array(e.bins, np.int64).reshape(-1, 3)
    assert np.array_equal(out["bin_chrom"], bins[:, 0]) and np.array_equal(out["bin_start"], bins[:, 1])
    assert np.array_equal(out["bin_end"], bins[:, 2])
    pb, pc, pv = e.arrays()
    assert out["pair_value"].dtype == np.uint64 and out["cells"].dtype == np.uint64
    assert np.array_equal(out["pair_bin"], pb) and np.array_equal(out["pair_cell"], pc)
    assert np.array_equal(out["pair_value"], pv)
    assert np.array_equal(out["cells"], e.cells)
    if e.cluster_sums is None:
        assert "cluster_sums" not in out
    else:
        assert np.array_equal(out["cluster_sums"], e.cluster_sums)
    st = out["stats"]
    assert st == secedo_amd.depth_stats()
    assert {k: st[k] for k in de.STAT_KEYS} == e.stats
    assert (st["bins"], st["pieces"]) == (len(e.bins), e.pieces)
    assert out["names"] == e.names
    if out_dir is not None:
        got = read_outputs(out_dir, bgzf)
        assert sorted(got) == sorted(e.files)
        for name, want in e.files.items():
            assert got[name] == want, name
        assert not [n for n in os.listdir(os.path.join(str(out_dir), "depth")) if ".tmp." in n]


def run(tmp_path, refs, cells, S, chroms, name="run", out=True, **kw):
    """Writes the cells as BAM files, runs bin_depth on them and checks everything -> (result, expected)."""
    paths = write_cells(tmp_path / (name + "_in"), refs, cells)
    out_dir = None
    if out:
        out_dir = tmp_path / (name + "_out")
        out_dir.mkdir()
    ekw = {k: kw[k] for k in ("mode", "min_map_quality", "duplicates", "clustering") if k in kw}
    e = de.expected(cells, refs, S, chroms, names=[de.default_name(p) for p in paths], **ekw)
    got = secedo_amd.bin_depth(paths, S, chroms, out_dir=out_dir, **kw)
    check(got, e, out_dir, kw.get("output") == "bgzf")
    return got, e


@pytest.fixture(scope="module")
def case1(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_cells")
    cells = se.cell_records()
    paths = write_cells(d, se.REFS, cells)
    names = [de.default_name(p) for p in paths]
    e = de.expected(cells, se.REFS, 1000, [0, 1], names=names)
    return dict(dir=d, cells=cells, paths=paths, names=names, expected=e)


def test_per_file_mode(case1, tmp_path):
    e = case1["expected"]
    # the preconditions, from the expected data: the test cannot go vacuous
    assert max(e.pairs.values()) >= 2
    per_bin = {}
    for b, c in e.pairs:
        per_bin.setdefault(b, set()).add(c)
    assert max(len(v) for v in per_bin.values()) >= 2 and len(per_bin) < len(e.bins) == 200
    assert e.stats["counted"] > 1000 and e.stats["records"] == e.stats["counted"]
    times = {}
    got = secedo_amd.bin_depth(case1["paths"], 1000, [1, 0], out_dir=tmp_path, times=times)
    check(got, e, tmp_path)
    assert times["total_ms"] > 0 and times["inflated_bytes"] > 0
    st = got["stats"]
    assert (st["files"], st["cells"], st["chromosomes"], st["clusters"]) == (12, 12, 2, 0)
    assert st["text_bytes"] == len(e.files["depth.counts.mtx"]) + len(e.files["depth.cells.tsv"])
    assert (st["compressed_bytes"], st["members"]) == (0, 0)
    # one chromosome of the two: its bins are numbered from 0
    e1 = de.expected(case1["cells"], se.REFS, 1000, [1], names=case1["names"])
    assert len(e1.bins) == 100 and e1.pairs
    check(secedo_amd.bin_depth(case1["paths"], 1000, [1]), e1)


def edge_record(k, pos, mapq=60, flag=0, cigar=None, ref_id=0):
    cigar = [("M", 10)] if cigar is None else cigar
    n = sum(x for op, x in cigar if op in "MIS=X")
    return bw.Rec(name="r%04d" % k, ref=ref_id, pos=pos, cigar=cigar, seq="ACGT" * (n // 4) + "A" * (n % 4) if n else "*",
                  qual=[30] * n if n else None, flag=flag, mapq=mapq)


@pytest.mark.parametrize("S,refs", [(30_000, se.REFS), (100_000, se.REFS), (150_000, se.REFS), (1, [("tiny", 300)])])
def test_bin_edges(tmp_path, S, refs):
    ln = refs[0][1]
    positions = sorted({0, S - 1, S, ln - 1, ln})
    cells = [[edge_record(k, p) for k, p in enumerate(positions)], [edge_record(9, ln - 1), edge_record(10, ln)]]
    for mode in ("reads", "bases"):
        got, e = run(tmp_path, refs, cells, S, [0], name=mode, mode=mode)
        assert e.stats["out_of_range"] == sum(1 for c in cells for r in c if r.pos >= ln) >= 2
        assert len(e.bins) == (ln + S - 1) // S and e.bins[-1][2] == ln
        assert e.pairs[(len(e.bins) - 1, 1)] == 1  # the last position of the chromosome, in the (short) last bin
        assert int(got["cells"][1, 0]) == 2 and int(got["cells"][1, 1]) == 1


def test_bases_mode(tmp_path):
    S = 1000
    many = [("M", 3) if k % 2 == 0 else ("D", 2) for k in range(131)]  # more than 64 ops, ends on an M
    cells = [[
        edge_record(0, 980, cigar=[("M", 50)]),                                   # an M across a border
        edge_record(1, 1980, cigar=[("M", 10), ("D", 10), ("M", 10)]),            # a D ending on a border
        edge_record(2, 2990, cigar=[("M", 10), ("N", 1000), ("M", 10)]),          # an N skipping bin 3 whole
        edge_record(3, 4990, cigar=[("S", 5), ("M", 30), ("S", 7)]),              # soft clips
        edge_record(4, 5990, cigar=[("H", 5), ("M", 30), ("H", 7)]),              # hard clips
        edge_record(5, 6995, cigar=[("H", 2), ("S", 3), ("M", 10), ("I", 4), ("M", 10), ("S", 1)]),  # an I
        edge_record(6, 7500, cigar=[]),                                           # no CIGAR
        edge_record(7, 8995, cigar=[("=", 10), ("X", 1), ("=", 10)]),             # = and X
        edge_record(8, 9900, cigar=many),
        edge_record(9, 99_950, cigar=[("M", 100)]),                               # past LN
    ], [
        edge_record(10, 3100, cigar=[("M", 20)]),                                 # another cell inside the skipped bin
    ]]
    got, e = run(tmp_path, se.REFS, cells, S, [0], mode="bases")
    assert (3, 0) not in e.pairs and (3, 1) in e.pairs and (2, 0) in e.pairs and (4, 0) in e.pairs
    assert e.pairs[(0, 0)] == 20 and e.pairs[(1, 0)] == 30 + 10 and e.pairs[(2, 0)] == 10 + 10
    assert e.pairs[(99, 0)] == 50 and int(e.cells[0, 1]) == 10  # the record without a CIGAR is counted
    assert e.pieces > len(e.pairs)  # the zero piece was sorted and dropped
    # the same records in `reads` mode: one per record, at its Position
    got, e = run(tmp_path, se.REFS, cells, S, [0], name="reads")
    assert e.pairs[(7, 0)] == 1 and sum(e.pairs.values()) == 11


def test_long_read(tmp_path):
    cells = se.long_read_cells()
    got, e = run(tmp_path, se.REFS, cells, 1000, [0], mode="bases")
    assert sum(1 for b, c in e.pairs if c == 0) >= 70 and int(e.cells[0, 1]) == 1 and int(e.cells[0, 2]) == 70_000
    assert int(e.cells[0, 4]) == 1000
    got, e = run(tmp_path, se.REFS, cells, 1000, [0], name="reads")
    assert int(e.cells[0, 2]) == 1 and int(e.cells[1, 2]) == 300


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_edges_records(tmp_path, n):
    """Exactly n surviving records (a block of the kernels is 256 threads), among others that are dropped."""
    keep = [edge_record(k, 40 * k) for k in range(n)]
    low = [edge_record(1000 + k, 40 * k + 5, mapq=3) for k in range(3)]
    cells = [sorted(keep[: n // 2] + low, key=bw.sort_key), keep[n // 2:]]
    for mode in ("reads", "bases"):
        got, e = run(tmp_path, se.REFS, cells, 1000, [0], name=mode, mode=mode, out=False)
        assert e.stats["counted"] == n and e.stats["dropped_mapq"] == 3
        assert e.pieces == n  # no record crosses a border: 40 k mod 1000 is at most 960


@pytest.mark.parametrize("pieces", [256, 257])
def test_block_edges_pieces(tmp_path, pieces):
    """`bases` mode with exactly 256 and 257 pieces: one read over pieces - 2 bins and two short ones."""
    S = 100
    long_read = edge_record(0, 50, cigar=[("M", (pieces - 3) * S + 1)])  # bins 0 .. pieces - 3
    cells = [[edge_record(1, 10), long_read], [edge_record(2, 20)]]
    got, e = run(tmp_path, se.REFS, cells, S, [0], mode="bases", out=False)
    assert e.pieces == pieces


def test_tag_mode(case1, tmp_path):
    recs, extra = se.multiplexed_records(case1["cells"])
    path = str(tmp_path / "multiplexed.bam")
    bw.write_bam(path, se.REFS, recs)
    e = de.expected([recs], se.REFS, 1000, [0, 1], tag="CB", barcodes=se.BARCODES)
    assert e.stats["dropped_barcode"] == extra > 0 and e.pairs == case1["expected"].pairs
    assert np.array_equal(e.cells, case1["expected"].cells)
    out = tmp_path / "out"
    out.mkdir()
    got = secedo_amd.bin_depth([path], 1000, [0, 1], out_dir=out, cell_tag="CB", cells=se.BARCODES)
    check(got, e, out)
    assert got["names"] == se.BARCODES
    # two files, the cells' records split between them by position
    half = [[r for r in recs if r.pos < 5000], [r for r in recs if r.pos >= 5000]]
    paths = write_cells(tmp_path / "halves", se.REFS, half, "half")
    e2 = de.expected(half, se.REFS, 1000, [0, 1], tag="CB", barcodes=se.BARCODES)
    assert e2.pairs == e.pairs
    check(secedo_amd.bin_depth(paths, 1000, [0, 1], cell_tag="CB", cells=se.BARCODES), e2)


def test_selection_mapq_and_flags(tmp_path):
    F, R = 0x1 | 0x2 | 0x40, 0x1 | 0x80 | 0x10
    cells = [[edge_record(0, 100, mapq=30, flag=F), edge_record(1, 200, mapq=29, flag=F),
              edge_record(2, 300, mapq=60, flag=R), edge_record(3, 400, mapq=60, flag=F | 0x400),
              edge_record(4, 100_000, mapq=60, flag=F), edge_record(5, 100_000, mapq=10, flag=F)],
             [edge_record(6, 150, mapq=255, flag=F | 0x100), edge_record(7, 250, mapq=0, flag=R)]]
    paths = write_cells(tmp_path / "in", se.REFS, cells)
    names = [de.default_name(p) for p in paths]
    # the threshold: 30 passes, 29 does not; MapQ is tested before the range
    e = de.expected(cells, se.REFS, 1000, [0], names=names)
    assert (e.stats["dropped_mapq"], e.stats["out_of_range"], e.stats["counted"]) == (3, 1, 4)
    check(secedo_amd.bin_depth(paths, 1000, [0]), e)
    e = de.expected(cells, se.REFS, 1000, [0], min_map_quality=0, names=names)
    assert (e.stats["dropped_mapq"], e.stats["out_of_range"]) == (0, 2)
    check(secedo_amd.bin_depth(paths, 1000, [0], min_map_quality=0), e)
    # the masks: require first, then exclude, both in front of MapQ
    e = de.expected(cells, se.REFS, 1000, [0], require=0x2, exclude=0x500, names=names)
    assert (e.stats["dropped_require"], e.stats["dropped_exclude"], e.stats["dropped_mapq"]) == (2, 2, 2)
    got = secedo_amd.bin_depth(paths, 1000, [0], require_flags="PROPER_PAIR", exclude_flags=0x500)
    check(got, e)
    # the process-wide settings of the pileup calls do not leak in
    plain = de.expected(cells, se.REFS, 1000, [0], names=names)
    with bam_pileup._select(require_flags=0x2, exclude_flags=0x500, remove_duplicates=True):
        check(secedo_amd.bin_depth(paths, 1000, [0]), plain)
    with pytest.raises(secedo_amd.SecedoError, match="share"):
        secedo_amd.bin_depth(paths, 1000, [0], require_flags=0x400, exclude_flags=0x400)


def test_selection_duplicates(tmp_path):
    refs, cells, want, _ = ref.worked_example()
    paths = write_cells(tmp_path / "in", refs, cells)
    names = [de.default_name(p) for p in paths]
    off = de.expected(cells, refs, 100, [0], names=names)
    e = de.expected(cells, refs, 100, [0], duplicates="remove", names=names)
    assert e.stats["dropped_duplicate"] == len(want) == 3 and e.pairs != off.pairs
    check(secedo_amd.bin_depth(paths, 100, [0]), off)
    got = secedo_amd.bin_depth(paths, 100, [0], duplicates="remove")
    check(got, e)
    # equals the plain call on files written without the dropped records
    kept = ref.rewrite(tmp_path / "kept", refs, cells, want)
    again = secedo_amd.bin_depth(kept, 100, [0])
    for key in ("pair_bin", "pair_cell", "pair_value"):
        assert np.array_equal(again[key], got[key])
    assert np.array_equal(again["cells"][:, 1:], got["cells"][:, 1:])
    # with a filter in front: the filtered records take no part in the duplicate rule
    e = de.expected(cells, refs, 100, [0], mode="bases", exclude=0x10, duplicates="remove", names=names)
    assert e.stats["dropped_exclude"] > 0 and e.stats["dropped_duplicate"] > 0
    check(secedo_amd.bin_depth(paths, 100, [0], mode="bases", exclude_flags=0x10, duplicates="remove"), e)


def test_routes(case1, tmp_path):
    e, paths = case1["expected"], case1["paths"]
    if not all(os.path.exists(p + ".bai") for p in paths):
        secedo_amd.bam_index_build(paths)
    runs = [dict(inflate="host", index="off"), dict(inflate="device", index="off"),
            dict(inflate="host", index="require"), dict(inflate="device", index="require")]
    for k, kw in enumerate(runs):
        out = tmp_path / ("route_%d" % k)
        out.mkdir()
        check(secedo_amd.bin_depth(paths, 1000, [0, 1], out_dir=out, num_threads=1 + 3 * (k % 2), **kw), e, out)
        assert bam_pileup.bam_index_stats()["files_indexed"] == (12 if kw["index"] == "require" else 0)
        assert (bam_pileup.bam_route_stats()["device_blocks"] > 0) == (kw["inflate"] == "device")
    # two of the files as SAM text and the first as bgzipped SAM, whose @SQ lines then give the bins
    mixed = list(paths)
    for c in (2, 7):
        mixed[c] = sw.sam_of_bam(paths[c], str(tmp_path / ("cell_%03d.sam" % c)))
    text = open(sw.sam_of_bam(paths[0], str(tmp_path / "cell_000.sam")), "rb").read()
    mixed[0] = str(tmp_path / "cell_000.sam.gz")
    open(mixed[0], "wb").write(bw.bgzf(text))
    assert [de.default_name(p) for p in mixed] == case1["names"]
    out = tmp_path / "sam"
    out.mkdir()
    check(secedo_amd.bin_depth(mixed, 1000, [0, 1], out_dir=out), e, out)


def test_clusters(case1, tmp_path):
    e = de.expected(case1["cells"], se.REFS, 1000, [0, 1], clustering=se.CLUSTERING, names=case1["names"])
    assert 3 not in se.CLUSTERING and e.cluster_sums.shape == (200, 5) and not e.cluster_sums[:, 3].any()
    assert e.cluster_sums[:, 0].any() and int(e.cluster_sums.sum()) == sum(e.pairs.values())
    got = secedo_amd.bin_depth(case1["paths"], 1000, [0, 1], out_dir=tmp_path, clustering=se.CLUSTERING)
    check(got, e, tmp_path)
    assert got["stats"]["clusters"] == 5
    # the clustering as secedo_main writes it, in `bases` mode
    clustering = tmp_path / "clustering.txt"
    clustering.write_text(",".join(str(c) for c in se.CLUSTERING) + "\n")
    e = de.expected(case1["cells"], se.REFS, 30_000, [1], mode="bases", clustering=se.CLUSTERING, names=case1["names"])
    check(secedo_amd.bin_depth(case1["paths"], 30_000, [1], mode="bases", clustering=str(clustering)), e)


def test_outputs(case1, tmp_path, monkeypatch):
    names = ["cell %d" % c for c in range(12)]
    e = de.expected(case1["cells"], se.REFS, 1000, [0, 1], mode="bases", clustering=se.CLUSTERING, names=names)
    assert e.stats["pairs"] > 100 and len(e.files) == 5  # many ranges at the small batches below
    kw = dict(mode="bases", clustering=se.CLUSTERING, cell_names=names)
    before = sorted(os.listdir(str(tmp_path)))
    check(secedo_amd.bin_depth(case1["paths"], 1000, [0, 1], **kw), e)  # out_dir=None writes nothing
    assert sorted(os.listdir(str(tmp_path))) == before
    sizes = {}
    for name, env in (("plain", {}), ("bgzf", {}), ("batch", {"SECEDO_DEPTH_BATCH_BYTES": "100"}),
                      ("slice", {"SECEDO_DEPTH_BATCH_BYTES": "1", "SECEDO_BGZF_SLICE_MEMBERS": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for output in ("plain", "bgzf") if name != "plain" else ("plain",):
            out = tmp_path / (name + "_" + output)
            out.mkdir()
            got = secedo_amd.bin_depth(case1["paths"], 1000, [0, 1], out_dir=out, output=output, **kw)
            check(got, e, out, output == "bgzf")
            st = got["stats"]
            assert st["text_bytes"] == sum(len(e.files[n]) for n in de.GZ_FILES)
            if output == "bgzf":
                raws = [open(str(out / "depth" / (n + ".gz")), "rb").read() for n in de.GZ_FILES]
                assert st["compressed_bytes"] == sum(len(r) for r in raws)
                assert st["members"] == sum(len(se.member_sizes(r)) - 1 for r in raws)
            sizes[(name, output)] = st["ranges"]
        for k in env:
            monkeypatch.delenv(k)
    n_lines = sum(e.files[n].count(b"\n") for n in de.GZ_FILES) - 3 - 1 - 1  # without the header lines
    assert sizes[("bgzf", "bgzf")] == 3 and sizes[("slice", "bgzf")] == n_lines > sizes[("batch", "plain")] > 3


def test_empty_and_errors(case1, tmp_path):
    # a requested chromosome without records: its bins are there, no pair is
    cells = [[edge_record(0, 10)], [edge_record(1, 20), edge_record(2, 1500)]]
    got, e = run(tmp_path, se.REFS, cells, 1000, [0, 1], clustering=[0, 1])
    assert len(e.bins) == 200 and all(b < 100 for b, _ in e.pairs) and e.stats["pairs"] == 3
    none = [[bw.Rec(name="u", ref=-1, pos=-1, cigar=[], seq="ACGT", qual=[30] * 4, flag=0x4)]]
    got, e = run(tmp_path, se.REFS, none, 1000, [0], name="none")
    assert e.stats["pairs"] == 0 and e.files["depth.counts.mtx"].endswith(b"\n100\t1\t0\n")

    paths = case1["paths"][:3]
    out = tmp_path / "out"
    out.mkdir()

    def refused(match, files, S, chroms, code=INVALID, **kw):
        before = sorted(os.listdir(str(out)))
        with pytest.raises(secedo_amd.SecedoError, match=match) as err:
            secedo_amd.bin_depth(files, S, chroms, out_dir=out, **kw)
        assert err.value.code == code
        assert sorted(os.listdir(str(out))) == before
        if before:
            assert not [n for n in os.listdir(str(out / "depth")) if ".tmp." in n]
        return str(err.value)

    refused("bin_size is 0", paths, 0, [0])
    d = tmp_path / "refs"
    other = write_cells(d, se.REFS, case1["cells"][:2]) + write_cells(d, [("chr1", 100_000), ("chrX", 100_000)],
                                                                      case1["cells"][2:3], "other")
    why = refused("reference 1 is chrX", other, 1000, [0])
    assert other[2] in why and other[0] in why
    refused("the clustering has 2 cells, there are 3 cells", paths, 1000, [0], clustering=[0, 1])
    refused("cell name 1 is empty or holds a tab or a line break", paths, 1000, [0], cell_names=["a", "b\tc", "d"])
    refused("cell name 2 is empty", paths, 1000, [0], cell_names=["a", "b", ""])
    refused("2 cell names for 3 cells", paths, 1000, [0], cell_names=["a", "b"])
    refused("chromosome id 2 is at or past the 2 references", paths, 1000, [0, 2])
    refused("chromosome id 1 is listed twice", paths, 1000, [1, 0, 1])
    assert os.listdir(str(out)) == []
    # existing outputs without overwrite: nothing is touched; with it, all are replaced
    first = secedo_amd.bin_depth(paths, 1000, [0], out_dir=out)
    kept = read_outputs(out)
    refused("depth.bins.bed exists", paths, 500, [0])
    assert read_outputs(out) == kept
    secedo_amd.bin_depth(paths, 500, [0], out_dir=out, overwrite=True)
    assert read_outputs(out) != kept
    check(secedo_amd.bin_depth(paths, 1000, [0], out_dir=out, overwrite=True), de.expected(
        case1["cells"][:3], se.REFS, 1000, [0], names=case1["names"][:3]), out)
    assert np.array_equal(first["pair_value"], secedo_amd.bin_depth(paths, 1000, [0])["pair_value"])
    with pytest.raises(secedo_amd.SecedoError, match="is not a directory"):
        secedo_amd.bin_depth(paths, 1000, [0], out_dir=tmp_path / "nowhere")


def test_cli_end_to_end(case1, tmp_path):
    clustering = tmp_path / "clustering"
    clustering.write_text(",".join(str(c) for c in se.CLUSTERING) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    e = de.expected(case1["cells"], se.REFS, 1000, [0, 1], mode="bases", clustering=se.CLUSTERING,
                    names=case1["names"])
    base = [sys.executable, "-m", "secedo_amd.depth_main", "-i", str(case1["dir"]), "-o", str(out), "--chromosomes",
            "1,2", "--bin_size", "1000"]
    r = subprocess.run(base + ["--mode", "bases", "--clustering", str(clustering), "--output", "bgzf"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Counted %d of %d records" % (e.stats["counted"], e.stats["records"]) in r.stdout
    got = read_outputs(out, bgzf=True)
    assert got == e.files
    # a bad flag exits 1 before torch loads, and writes nothing more
    before = sorted(os.listdir(str(out / "depth")))
    probe = ("import sys, runpy; sys.argv = %r\ntry:\n    runpy.run_module('secedo_amd.depth_main', run_name='__main__')\n"
             "except SystemExit as e:\n    print('torch' in sys.modules, file=sys.stderr); raise\n")
    r = subprocess.run([sys.executable, "-c", probe % (["depth_main"] + base[3:] + ["--mode", "depth"],)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 1 and "Invalid --mode 'depth'" in r.stderr and r.stderr.splitlines()[0] == "False"
    assert sorted(os.listdir(str(out / "depth"))) == before
