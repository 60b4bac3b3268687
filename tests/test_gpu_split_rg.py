"""Per-cluster BAM files that name each read's cell (secedo_amd.split_clusters(..., read_groups=True),
secedo_bam_split_clusters_rg): every file written equals, byte for byte, what tests/split_rg_expected.py derives on the
CPU from the inputs and the three rules of the contract -- whatever the mode, the route, the index mode, the batch size
and the input kind -- and the stats equal the counts that module makes. tests/test_split_rg_cpu.py checks that the
inputs used here reach the gather's edges. The pileup reads the files back cell by cell; errors leave nothing behind;
without ``read_groups`` nothing changes."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bai_expected as be
from tests import bam_writer as bw
from tests import sam_writer as sw
from tests import split_expected as se
from tests import split_rg_expected as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_BATCH = "1000"  # tests/test_gpu_pileup_bam_device.py's smallest SECEDO_BAM_BATCH_BYTES
ZERO = dict.fromkeys(sr.STAT_KEYS, 0)


def outputs(directory, n):
    return [open(os.path.join(str(directory), "cluster_%d.bam" % k), "rb").read() for k in range(n)]


def check_outputs(directory, expected):
    assert sorted(os.listdir(str(directory))) == sorted("cluster_%d.bam" % k for k in range(len(expected)))
    for k, (got, want) in enumerate(zip(outputs(directory, len(expected)), expected)):
        assert got == want, "cluster_%d.bam differs" % k
        assert gzip.decompress(got) == gzip.decompress(want)  # every CRC32 and ISIZE


def check_stats(info, stats, expected, dropped=0):
    assert {k: info[k] for k in sr.STAT_KEYS} == stats == secedo_amd.split_rg_stats()
    assert {k: v for k, v in info.items() if k not in sr.STAT_KEYS} == secedo_amd.split_stats()
    assert (info["records"], info["dropped_records"]) == (stats["tagged_records"], dropped)
    assert info["compressed_bytes"] == sum(len(raw) for raw in expected)
    assert info["text_bytes"] == sum(len(gzip.decompress(raw)) for raw in expected)


def write_cells(directory, cells, stem="cell_%03d"):
    paths = []
    for c, items in enumerate(cells):
        paths.append(os.path.join(str(directory), (stem % c) + ".bam"))
        sr.write_raw_bam(paths[-1], se.REFS, items)
    return paths


@pytest.fixture(scope="module")
def case1(tmp_path_factory):
    """The twelve cell files with every kind of aux area, their sources and the expected cluster files."""
    d = tmp_path_factory.mktemp("split_rg_cells")
    cells = sr.cell_items()
    paths = write_cells(d, cells)
    sources = [sr.source_of_items(se.REFS, items) for items in cells]
    expected, dropped, stats = sr.expected_files(sources, se.CLUSTERING, [0, 1], sr.NAMES,
                                                 tmp_path_factory.mktemp("split_rg_encode"))
    assert dropped == 0
    return dict(dir=d, cells=cells, paths=paths, sources=sources, expected=expected, stats=stats)


def test_per_file_mode(case1, tmp_path):
    stats = case1["stats"]
    assert stats["unparsed_records"] >= 2 and 0 < stats["replaced_records"] < stats["tagged_records"]
    times = {}
    info = secedo_amd.split_clusters(case1["paths"], se.CLUSTERING, tmp_path, [1, 0], times=times, read_groups=True,
                                     cell_names=sr.NAMES)
    check_outputs(tmp_path, case1["expected"])
    check_stats(info, stats, case1["expected"])
    assert (info["files"], info["clusters"], info["cells"]) == (12, 5, 12) and times["total_ms"] > 0


def test_tile_boundaries_and_default_names(tmp_path):
    """A hole, a block_size word and a suffix on 4 KiB tile boundaries; the cell is named by its file."""
    items = sr.tile_items("tile-cell")
    for ext, write in ((".bam", lambda p: bw.write_bam(p, se.REFS, items[0])),
                       (".sam", lambda p: sw.write_sam(p, se.REFS, items[0])),
                       (".sam.gz", lambda p: open(p, "wb").write(bw.bgzf(sw.sam_text(se.REFS, items[0]).encode())))):
        d = tmp_path / ("in" + ext.replace(".", "_"))
        d.mkdir()
        path = str(d / ("tile-cell" + ext))
        write(path)
        expected, _, stats = sr.expected_files([se.source_of_recs(se.REFS, items[0])], [0], [0], ["tile-cell"], tmp_path)
        out = tmp_path / ("out" + ext.replace(".", "_"))
        out.mkdir()
        info = secedo_amd.split_clusters([path], [0], out, [0], read_groups=True)
        check_outputs(out, expected)
        check_stats(info, stats, expected)


def test_names(tmp_path):
    """Names of 1 and of 254 bytes, a cluster with one record, a cluster number no cell has."""
    cells = se.cell_records(n_cells=2, pairs=4) + [[bw.Rec(name="only", ref=0, pos=77, cigar=[("M", 5)], seq="ACGTA",
                                                           qual=[20] * 5, tags=[("RG", "Z", "x")])]]
    names = ["A", "".join(chr(0x21 + k % 94) for k in range(254)), "single"]
    clustering = [0, 3, 2]
    paths = write_cells(tmp_path, cells)
    sources = [se.source_of_recs(se.REFS, c) for c in cells]
    expected, _, stats = sr.expected_files(sources, clustering, [0, 1], names, tmp_path)
    header_only = gzip.decompress(expected[1])
    assert b"@RG" not in header_only and len(se.member_sizes(expected[1])) == 2
    assert gzip.decompress(expected[2]).count(b"RGZsingle\0") == 1
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, clustering, out, [0, 1], read_groups=True, cell_names=names)
    check_outputs(out, expected)
    check_stats(info, stats, expected)


def test_extent_edges(tmp_path):
    names = ["full-cell", "o", "single"]
    cells = sr.edge_items(names)
    paths = write_cells(tmp_path, cells, "edge_%d")
    sources = [se.source_of_recs(se.REFS, c) for c in cells]
    parts = sr.cluster_parts(sources, [0, 1, 2], [0], names)[0]
    assert [len(ps[1]) for ps in parts[:2]] == [se.CUT, se.CUT + 1]
    expected, _, stats = sr.expected_files(sources, [0, 1, 2], [0], names, tmp_path)
    assert [[isize for isize, _ in se.member_sizes(raw)[1:-1]] for raw in expected[:2]] == [[se.CUT], [se.CUT, 1]]
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, [0, 1, 2], out, [0], read_groups=True, cell_names=names)
    check_outputs(out, expected)
    check_stats(info, stats, expected)


def test_extent_edges_with_one_member_per_slice(tmp_path, monkeypatch):
    """The set above with SECEDO_BGZF_SLICE_MEMBERS=1: the members of cluster 1's file lie in different slices of the
    encoder's driver. The expected files, and the counts of the run without the variable."""
    names = ["full-cell", "o", "single"]
    cells = sr.edge_items(names)
    paths = write_cells(tmp_path, cells, "edge_%d")
    sources = [se.source_of_recs(se.REFS, c) for c in cells]
    expected, _, stats = sr.expected_files(sources, [0, 1, 2], [0], names, tmp_path)
    infos = []
    for value in (None, "1"):
        if value is not None:
            monkeypatch.setenv("SECEDO_BGZF_SLICE_MEMBERS", value)
        out = tmp_path / ("out_%s" % value)
        out.mkdir()
        infos.append(secedo_amd.split_clusters(paths, [0, 1, 2], out, [0], read_groups=True, cell_names=names))
        check_outputs(out, expected)
        check_stats(infos[-1], stats, expected)
    for key in ("members", "stored_members", "compressed_bytes"):
        assert infos[1][key] == infos[0][key], key


def test_long_record(tmp_path):
    """The hole of the 70 000-base read lies behind its ML:B:C array, dozens of tiles from the record's start."""
    cells = sr.long_items()
    paths = write_cells(tmp_path, cells, "long_%d")
    sources = [se.source_of_recs(se.REFS, c) for c in cells]
    _new, hole, parsed = sr.edit_record(sources[0].records[0], "long_0")
    assert parsed and hole[0] > 100_000
    expected, _, stats = sr.expected_files(sources, [0, 0], [0], ["long_0", "long_1"], tmp_path)
    assert stats["replaced_records"] == 1 and stats["tagged_records"] == 301
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, [0, 0], out, [0], read_groups=True)  # the short reads beside it
    check_outputs(out, expected)
    check_stats(info, stats, expected)


def test_tag_mode(tmp_path):
    for tag, cells in (("CB", se.cell_records()), ("RG", sr.rg_keyed_cells())):
        recs, n_extra = se.multiplexed_records(cells)
        path = str(tmp_path / ("multiplexed_%s.bam" % tag))
        bw.write_bam(path, se.REFS, recs)
        expected, dropped, stats = sr.expected_files([se.source_of_recs(se.REFS, recs)], se.CLUSTERING, [0, 1],
                                                     se.BARCODES, tmp_path, tag, se.BARCODES)
        assert dropped == n_extra > 0
        assert stats["replaced_records"] == (stats["tagged_records"] if tag == "RG" else 0)
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        info = secedo_amd.split_clusters([path], se.CLUSTERING, out, [0, 1], cell_tag=tag, cells=se.BARCODES,
                                         read_groups=True)
        check_outputs(out, expected)
        check_stats(info, stats, expected, dropped)
        assert (info["files"], info["cells"]) == (1, 12)


def test_routes(case1, tmp_path, monkeypatch):
    expected, paths = case1["expected"], case1["paths"]
    if not all(os.path.exists(p + ".bai") for p in paths):
        secedo_amd.bam_index_build(paths)
    kw = dict(read_groups=True, cell_names=sr.NAMES)
    runs = [dict(inflate="device", index="off"), dict(inflate="host", index="require"),
            dict(inflate="device", index="require")]
    for k, route in enumerate(runs):
        out = tmp_path / ("route_%d" % k)
        out.mkdir()
        info = secedo_amd.split_clusters(paths, se.CLUSTERING, out, [0, 1], num_threads=1 + 3 * (k % 2), **route, **kw)
        check_outputs(out, expected)
        check_stats(info, case1["stats"], expected)
        assert bam_pileup.bam_index_stats()["files_indexed"] == (12 if route["index"] == "require" else 0)
        assert (bam_pileup.bam_route_stats()["device_blocks"] > 0) == (route["inflate"] == "device")
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", SMALL_BATCH)
    for k, inflate in enumerate(("host", "device")):
        out = tmp_path / ("batch_%d" % k)
        out.mkdir()
        secedo_amd.split_clusters(paths, se.CLUSTERING, out, [0, 1], inflate=inflate, index="off", **kw)
        check_outputs(out, expected)
    monkeypatch.delenv("SECEDO_BAM_BATCH_BYTES")
    # two of the files as SAM text and one, the first, as bgzipped SAM: the names are given, so the files' do not matter
    mixed = list(paths)
    for c in sr.SAM_CELLS[1:]:
        mixed[c] = str(tmp_path / ("cell_%03d.sam" % c))
        sw.write_sam(mixed[c], se.REFS, case1["cells"][c])
    mixed[0] = str(tmp_path / "cell_000.sam.gz")
    open(mixed[0], "wb").write(bw.bgzf(sw.sam_text(se.REFS, case1["cells"][0]).encode()))
    out = tmp_path / "sam"
    out.mkdir()
    info = secedo_amd.split_clusters(mixed, se.CLUSTERING, out, [0, 1], **kw)
    check_outputs(out, expected)
    check_stats(info, case1["stats"], expected)


def loci(p):
    """{position: sorted id_base values} of a one-chromosome FlatPileup."""
    off = p.locus_entry_off.astype(np.int64)
    return {int(pos): sorted(int(x) for x in p.id_base[off[k]:off[k + 1]]) for k, pos in enumerate(p.locus_pos)}


@pytest.fixture(scope="module")
def plain_cells(tmp_path_factory):
    """split_expected's twelve cell files as they are."""
    d = tmp_path_factory.mktemp("split_rg_plain")
    cells = se.cell_records()
    paths = []
    for c, recs in enumerate(cells):
        paths.append(os.path.join(str(d), "cell_%03d.bam" % c))
        bw.write_bam(paths[-1], se.REFS, recs)
    return dict(dir=d, cells=cells, paths=paths)


def test_round_trip(plain_cells, tmp_path):
    """The tagged files are multiplexed BAMs: read back by RG, cluster k gives the pileup of its cells' files."""
    paths = plain_cells["paths"]
    secedo_amd.split_clusters(paths, se.CLUSTERING, tmp_path, [0, 1], read_groups=True, bai=True)
    names = sr.default_names(paths)
    assert names == ["cell_%03d" % c for c in range(12)]
    for k in range(5):
        path = str(tmp_path / ("cluster_%d.bam" % k))
        assert open(path + ".bai", "rb").read() == be.expected_bytes(path), k
    compared = 0
    for k in (0, 1, 2, 4):
        members = [c for c, cl in enumerate(se.CLUSTERING) if cl == k]
        path = str(tmp_path / ("cluster_%d.bam" % k))
        for chrom in (0, 1):
            args = (None, False, chrom, 1000, 30, 30, 0, 4, 1)
            tagged = secedo_amd.pileup_bams([path], *args, cell_tag="RG", cells=[names[c] for c in members],
                                            index="require")
            cells = secedo_amd.pileup_bams([paths[c] for c in members], *args)
            assert loci(tagged) == loci(cells)
            compared += len(loci(cells))
    assert compared > 100


def test_off_is_off(plain_cells, tmp_path):
    paths = plain_cells["paths"]
    sources = [se.source_of_recs(se.REFS, recs) for recs in plain_cells["cells"]]
    expected, _ = se.expected_files(sources, se.CLUSTERING, [0, 1], tmp_path)
    tagged = tmp_path / "tagged"
    tagged.mkdir()
    secedo_amd.split_clusters(paths, se.CLUSTERING, tagged, [0, 1], read_groups=True)
    assert secedo_amd.split_rg_stats()["tagged_records"] > 0
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, se.CLUSTERING, out, [0, 1])
    check_outputs(out, expected)
    assert secedo_amd.split_rg_stats() == ZERO and not set(info) & set(sr.STAT_KEYS)
    with pytest.raises(secedo_amd.SecedoError, match="cell_names needs read_groups") as e:
        secedo_amd.split_clusters(paths, se.CLUSTERING, out, [0, 1], cell_names=sr.NAMES, overwrite=True)
    assert e.value.code == secedo_amd._lib.E_INVALID_ARG
    check_outputs(out, expected)


def test_errors(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    cells = se.cell_records(n_cells=3, pairs=4)
    good = write_cells(tmp_path, cells, "small_%d")

    def refused(match, paths, names, **kw):
        with pytest.raises(secedo_amd.SecedoError, match=match) as e:
            secedo_amd.split_clusters(paths, [0, 1, 0], out, [0], read_groups=True, cell_names=names, **kw)
        assert e.value.code == secedo_amd._lib.E_INVALID_ARG
        assert os.listdir(str(out)) == []
        return str(e.value)

    refused("cell 1 has byte 9", good, ["a", "b\tc", "d"])
    refused("cell 2 is empty", good, ["a", "b", ""])
    refused("cell 0 is 255 bytes", good, ["n" * 255, "b", "c"])
    refused("cells 0 and 2 share the name same", good, ["same", "b", "same"])
    refused("3 cells, the name list 2", good, ["a", "b"])
    refused("3 cells, the name list 4", good, ["a", "b", "c", "d"])
    # default names: two directories hold a small_1.bam
    d = tmp_path / "other"
    d.mkdir()
    twin = str(d / "small_1.bam")
    sr.write_raw_bam(twin, se.REFS, cells[1])
    refused("cells 1 and 2 share the name small_1", [good[0], good[1], twin], None)
    # names are checked before any input is read: a file that is no BAM is not reached
    junk = str(tmp_path / "junk.bam")
    open(junk, "wb").write(b"not a BAM file")
    refused("cell 1 is empty", [good[0], junk, good[2]], ["a", "", "c"])
    # tag mode: the barcodes are the default names and fall under the same rule
    recs, _ = se.multiplexed_records(cells)
    mux = str(tmp_path / "mux.bam")
    bw.write_bam(mux, se.REFS, recs)
    refused("cell 1 has byte 32", [mux], None, cell_tag="CB", cells=[se.BARCODES[0], "with space", se.BARCODES[2]])
    # and the plain call's refusals hold: an existing output
    secedo_amd.split_clusters(good, [0, 1, 0], out, [0], read_groups=True)
    with pytest.raises(secedo_amd.SecedoError, match="cluster_0.bam exists"):
        secedo_amd.split_clusters(good, [0, 1, 0], out, [0], read_groups=True)
    assert sorted(os.listdir(str(out))) == ["cluster_0.bam", "cluster_1.bam"]


def test_cli_end_to_end(case1, tmp_path):
    clustering = tmp_path / "clustering"
    clustering.write_text(",".join(str(c) for c in se.CLUSTERING) + "\n")
    names = tmp_path / "names"
    names.write_text("".join(n + "\n" for n in sr.NAMES))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sys.executable, "-m", "secedo_amd.split_main", "-i", str(case1["dir"]), "--clustering",
                        str(clustering), "-o", str(out), "--chromosomes", "1,2", "--bai", "--read_groups",
                        "--cell_names", str(names)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Written" in r.stdout and "Tagged %d records" % case1["stats"]["tagged_records"] in r.stdout
    for k, want in enumerate(case1["expected"]):
        path = str(out / ("cluster_%d.bam" % k))
        assert open(path, "rb").read() == want
        assert open(path + ".bai", "rb").read() == be.expected_bytes(path)
    assert len(os.listdir(str(out))) == 10
