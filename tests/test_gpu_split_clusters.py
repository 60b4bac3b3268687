"""Per-cluster BAM files from a clustering (secedo_amd.split_clusters, secedo_bam_split_clusters): every file written
equals, byte for byte, what tests/split_expected.py derives on the CPU from the inputs and the contract of
include/secedo_bam.h -- whatever the mode (per file, by barcode tag), the route, the index mode, the batch size and the
input kind -- and ``gzip.decompress`` of it checks every CRC32 and ISIZE. The project's own readers read the files back;
errors leave nothing behind."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_BATCH = "1000"  # tests/test_gpu_pileup_bam_device.py's smallest SECEDO_BAM_BATCH_BYTES


def outputs(directory, n):
    return [open(os.path.join(str(directory), "cluster_%d.bam" % k), "rb").read() for k in range(n)]


def check_outputs(directory, expected):
    assert sorted(os.listdir(str(directory))) == sorted("cluster_%d.bam" % k for k in range(len(expected)))
    for k, (got, want) in enumerate(zip(outputs(directory, len(expected)), expected)):
        assert got == want, "cluster_%d.bam differs" % k
        assert gzip.decompress(got) == gzip.decompress(want)  # every CRC32 and ISIZE


def leftovers(directory, allowed=()):
    return [n for n in os.listdir(str(directory)) if ".tmp." in n or (n.startswith("cluster_") and n not in allowed)]


def members_and_stored(files):
    sizes = [se.member_sizes(raw)[:-1] for raw in files]  # without the EOF members
    return sum(len(s) for s in sizes), sum(1 for s in sizes for _isize, stored in s if stored)


@pytest.fixture(scope="module")
def case1(tmp_path_factory):
    """The twelve cell files, their sources and the expected cluster files."""
    d = tmp_path_factory.mktemp("split_cells")
    cells = se.cell_records()
    paths = []
    for c, recs in enumerate(cells):
        paths.append(os.path.join(str(d), "cell_%03d.bam" % c))
        bw.write_bam(paths[-1], se.REFS, recs)
    sources = [se.source_of_recs(se.REFS, recs) for recs in cells]
    expected, dropped = se.expected_files(sources, se.CLUSTERING, [0, 1], tmp_path_factory.mktemp("split_encode"))
    assert dropped == 0
    return dict(dir=d, cells=cells, paths=paths, sources=sources, expected=expected)


def test_per_file_mode(case1, tmp_path):
    expected = case1["expected"]
    # the preconditions, from the expected bytes: the test cannot go vacuous
    sizes = [se.member_sizes(raw)[:-1] for raw in expected]
    assert max(len(s) for s in sizes) >= 3
    parts, _ = se.cluster_parts(case1["sources"], se.CLUSTERING, [0, 1])
    straddles = False
    for ps in parts:
        for part in ps[1:]:
            starts, o = set(), 0
            while o < len(part):
                starts.add(o)
                o += 4 + int.from_bytes(part[o:o + 4], "little")
            straddles |= any(cut not in starts for cut in range(se.CUT, len(part), se.CUT))
    assert straddles
    assert 3 not in se.CLUSTERING and sizes[3] and len(sizes[3]) == 1  # header only: one member
    assert any(len(bw.encode_record(r)) % 4 for recs in case1["cells"] for r in recs)  # unaligned offsets
    times = {}
    info = secedo_amd.split_clusters(case1["paths"], se.CLUSTERING, tmp_path, [1, 0], times=times)
    check_outputs(tmp_path, expected)
    members, stored = members_and_stored(expected)
    n_records = sum(1 for s in case1["sources"] for rec in s.records if se.ref_pos(rec)[0] >= 0)
    assert info == secedo_amd.split_stats()
    assert (info["files"], info["clusters"], info["cells"]) == (12, 5, 12)
    assert (info["records"], info["dropped_records"]) == (n_records, 0)
    assert (info["members"], info["stored_members"]) == (members, stored)
    assert info["compressed_bytes"] == sum(len(raw) for raw in expected)
    assert info["text_bytes"] == sum(len(gzip.decompress(raw)) for raw in expected)
    assert times["total_ms"] > 0 and times["inflated_bytes"] > 0
    # the clustering as secedo_main writes it, and overwrite
    clustering = tmp_path / "clustering.txt"
    clustering.write_text(",".join(str(c) for c in se.CLUSTERING) + "\n")
    with pytest.raises(secedo_amd.SecedoError, match="cluster_0.bam exists"):
        secedo_amd.split_clusters(case1["paths"], str(clustering), tmp_path, [0, 1])
    os.remove(str(clustering))
    check_outputs(tmp_path, expected)


def test_extent_edges(tmp_path):
    cells = se.edge_cells()
    paths = []
    for c, recs in enumerate(cells):
        paths.append(str(tmp_path / ("edge_%d.bam" % c)))
        bw.write_bam(paths[-1], se.REFS, recs)
    sources = [se.source_of_recs(se.REFS, recs) for recs in cells]
    parts, _ = se.cluster_parts(sources, [0, 1, 2], [0])
    assert [len(ps[1]) for ps in parts[:2]] == [se.CUT, se.CUT + 1] and len(cells[2]) == 1
    expected, _ = se.expected_files(sources, [0, 1, 2], [0], tmp_path)
    assert [[isize for isize, _ in se.member_sizes(raw)[1:-1]] for raw in expected[:2]] == [[se.CUT], [se.CUT, 1]]
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, [0, 1, 2], out, [0])
    check_outputs(out, expected)
    assert info["records"] == sum(len(c) for c in cells)


def test_long_record(tmp_path):
    cells = se.long_read_cells()
    paths = []
    for c, recs in enumerate(cells):
        paths.append(str(tmp_path / ("long_%d.bam" % c)))
        bw.write_bam(paths[-1], se.REFS, recs)
    sources = [se.source_of_recs(se.REFS, recs) for recs in cells]
    expected, _ = se.expected_files(sources, [0, 1], [0], tmp_path)
    long_members = se.member_sizes(expected[0])[1:-1]
    assert len(sources[0].records) == 1 and len(sources[0].records[0]) > se.CUT and len(long_members) >= 2
    assert any(stored for _isize, stored in long_members)
    assert any(not stored for _isize, stored in se.member_sizes(expected[1])[1:-1])
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, [0, 1], out, [0])
    check_outputs(out, expected)
    members, stored = members_and_stored(expected)
    assert (info["members"], info["stored_members"]) == (members, stored)
    assert info["stored_members"] >= 1 and info["members"] > info["stored_members"]


@pytest.mark.parametrize("which", ["edges", "long"])
def test_slice_borders_of_the_encoder(tmp_path, monkeypatch, which):
    """The two sets above with SECEDO_BGZF_SLICE_MEMBERS at 1 and 2 (members of one file on both sides of a slice
    border, in the headers' run and in the chromosome's), at 0 and above the writer's 4096: the expected files, and the
    counts of the run without the variable."""
    cells, clustering = (se.edge_cells(), [0, 1, 2]) if which == "edges" else (se.long_read_cells(), [0, 1])
    paths = []
    for c, recs in enumerate(cells):
        paths.append(str(tmp_path / ("%s_%d.bam" % (which, c))))
        bw.write_bam(paths[-1], se.REFS, recs)
    expected, _ = se.expected_files([se.source_of_recs(se.REFS, recs) for recs in cells], clustering, [0], tmp_path)
    assert max(len(se.member_sizes(raw)) for raw in expected) >= 4  # header, two of the stream, EOF: a border to cross
    infos = {}
    for value in (None, "1", "2", "0", "99999"):
        if value is not None:
            monkeypatch.setenv("SECEDO_BGZF_SLICE_MEMBERS", value)
        out = tmp_path / ("out_%s" % value)
        out.mkdir()
        infos[value] = secedo_amd.split_clusters(paths, clustering, out, [0])
        check_outputs(out, expected)
        for key in ("members", "stored_members", "compressed_bytes", "records", "text_bytes"):
            assert infos[value][key] == infos[None][key], (value, key)
    assert (infos[None]["members"], infos[None]["stored_members"]) == members_and_stored(expected)


def test_tag_mode(case1, tmp_path):
    recs, n_extra = se.multiplexed_records(case1["cells"])
    path = str(tmp_path / "multiplexed.bam")
    bw.write_bam(path, se.REFS, recs)
    expected, dropped = se.expected_files([se.source_of_recs(se.REFS, recs)], se.CLUSTERING, [0, 1], tmp_path, "CB",
                                          se.BARCODES)
    assert expected == case1["expected"] and dropped == n_extra > 0  # the same twelve cells: the same @CO lines too
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters([path], se.CLUSTERING, out, [0, 1], cell_tag="CB", cells=se.BARCODES)
    check_outputs(out, expected)
    assert info["dropped_records"] == dropped and (info["files"], info["cells"]) == (1, 12)
    with pytest.raises(secedo_amd.SecedoError, match="12 cells, the barcode list 11"):
        secedo_amd.split_clusters([path], se.CLUSTERING, out, [0, 1], cell_tag="CB", cells=se.BARCODES[:11],
                                  overwrite=True)
    check_outputs(out, expected)


def test_routes(case1, tmp_path, monkeypatch):
    expected, paths = case1["expected"], case1["paths"]
    if not all(os.path.exists(p + ".bai") for p in paths):
        secedo_amd.bam_index_build(paths)
    runs = [dict(inflate="host", index="off"), dict(inflate="device", index="off"),
            dict(inflate="host", index="require"), dict(inflate="device", index="require")]
    for k, kw in enumerate(runs):
        out = tmp_path / ("route_%d" % k)
        out.mkdir()
        secedo_amd.split_clusters(paths, se.CLUSTERING, out, [0, 1], num_threads=1 + 3 * (k % 2), **kw)
        check_outputs(out, expected)
        assert bam_pileup.bam_index_stats()["files_indexed"] == (12 if kw["index"] == "require" else 0)
        assert (bam_pileup.bam_route_stats()["device_blocks"] > 0) == (kw["inflate"] == "device")
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", SMALL_BATCH)
    for k, inflate in enumerate(("host", "device")):
        out = tmp_path / ("batch_%d" % k)
        out.mkdir()
        secedo_amd.split_clusters(paths, se.CLUSTERING, out, [0, 1], inflate=inflate, index="off")
        check_outputs(out, expected)
    monkeypatch.delenv("SECEDO_BAM_BATCH_BYTES")
    # two of the files as SAM text
    mixed = list(paths)
    for c in (2, 7):
        mixed[c] = sw.sam_of_bam(paths[c], str(tmp_path / ("cell_%03d.sam" % c)))
    # and one as bgzipped SAM, the first file, whose @SQ lines then give the outputs' reference list
    text = open(sw.sam_of_bam(paths[0], str(tmp_path / "cell_000.sam")), "rb").read()
    mixed[0] = str(tmp_path / "cell_000.sam.gz")
    open(mixed[0], "wb").write(bw.bgzf(text))
    out = tmp_path / "sam"
    out.mkdir()
    secedo_amd.split_clusters(mixed, se.CLUSTERING, out, [0, 1])
    check_outputs(out, expected)


def loci(p):
    """{position: sorted id_base values} of a one-chromosome FlatPileup."""
    off = p.locus_entry_off.astype(np.int64)
    return {int(pos): sorted(int(x) for x in p.id_base[off[k]:off[k + 1]]) for k, pos in enumerate(p.locus_pos)}


def test_reading_back(case1, tmp_path):
    secedo_amd.split_clusters(case1["paths"], se.CLUSTERING, tmp_path, [0, 1], bai=True)
    outs = [str(tmp_path / ("cluster_%d.bam" % k)) for k in range(5)]
    for k, path in enumerate(outs):
        assert open(path, "rb").read() == case1["expected"][k]
        assert open(path + ".bai", "rb").read() == be.expected_bytes(path), k
    clustering = np.asarray(se.CLUSTERING)
    for chrom in (0, 1):
        args = (None, False, chrom, 1000, 30, 30, 0, 4, 1)
        merged = secedo_amd.pileup_bams(outs, *args, index="require")
        assert bam_pileup.bam_index_stats()["files_indexed"] == 5
        cells = secedo_amd.pileup_bams(case1["paths"], *args)
        grouped = {pos: sorted(int(clustering[x >> 2]) << 2 | (x & 3) for x in ids) for pos, ids in loci(cells).items()}
        assert len(grouped) > 100 and loci(merged) == grouped


def small_set(tmp_path, texts=None, refs=None):
    cells = se.cell_records(n_cells=3, pairs=4)
    paths = []
    for c, recs in enumerate(cells):
        paths.append(str(tmp_path / ("small_%d.bam" % c)))
        bw.write_bam(paths[-1], (refs or {}).get(c, se.REFS), recs, None if texts is None else texts[c])
    return paths


def test_errors(tmp_path):
    out = tmp_path / "out"
    out.mkdir()

    def refused(match, paths, clustering, chromosomes, **kw):
        before = sorted(os.listdir(str(out)))
        with pytest.raises(secedo_amd.SecedoError, match=match) as e:
            secedo_amd.split_clusters(paths, clustering, out, chromosomes, **kw)
        assert e.value.code == secedo_amd._lib.E_INVALID_ARG
        assert sorted(os.listdir(str(out))) == before and not leftovers(out, allowed=before)
        return str(e.value)

    good = small_set(tmp_path)
    # a differing reference list names the file, the first file and the reference
    d = tmp_path / "refs"
    d.mkdir()
    other = small_set(d, refs={2: [("chr1", 100_000), ("chrX", 100_000)]})
    why = refused("reference 1 is chrX", other, [0, 1, 0], [0])
    assert other[2] in why and other[0] in why
    # an @RG clash names both files
    d = tmp_path / "rg"
    d.mkdir()
    head = se.default_text(se.REFS)
    clash = small_set(d, texts=[head + "@RG\tID:a\tSM:one\n", head, head + "@RG\tID:a\tSM:two\n"])
    why = refused("@RG ID:a", clash, [0, 1, 0], [0])
    assert clash[0] in why and clash[2] in why
    refused("2 cells, there are 3 files", good, [0, 1], [0])
    refused("chromosome id 1 is listed twice", good, [0, 1, 0], [1, 0, 1])
    refused("chromosome id 2 is at or past the 2 references", good, [0, 1, 0], [0, 2])
    # a truncated input: the pileup route's message
    cut = str(tmp_path / "cut.bam")
    raw = open(good[1], "rb").read()
    open(cut, "wb").write(raw[:len(raw) // 2])
    for inflate in ("host", "device"):
        with pytest.raises(secedo_amd.SecedoError) as e:
            secedo_amd.pileup_bams([good[0], cut, good[2]], None, False, 0, 100, 30, 30, 0, 2, 1, inflate=inflate)
        assert refused("cut.bam", [good[0], cut, good[2]], [0, 1, 0], [0], inflate=inflate) == str(e.value)
    # an existing output without overwrite: nothing is touched; with it, all are replaced
    secedo_amd.split_clusters(good, [0, 1, 0], out, [0])
    first = outputs(out, 2)
    refused("cluster_0.bam exists", good, [1, 0, 1], [0])
    assert outputs(out, 2) == first
    secedo_amd.split_clusters(good, [1, 0, 1], out, [0], overwrite=True)
    assert outputs(out, 2) != first and not leftovers(out, allowed=("cluster_0.bam", "cluster_1.bam"))
    # the output directory must be there
    with pytest.raises(secedo_amd.SecedoError, match="is not a directory"):
        secedo_amd.split_clusters(good, [0, 1, 0], tmp_path / "nowhere", [0])


def test_cli_end_to_end(case1, tmp_path):
    clustering = tmp_path / "clustering"
    clustering.write_text(",".join(str(c) for c in se.CLUSTERING) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sys.executable, "-m", "secedo_amd.split_main", "-i", str(case1["dir"]), "--clustering",
                        str(clustering), "-o", str(out), "--chromosomes", "1,2", "--bai"], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Written" in r.stdout
    for k, want in enumerate(case1["expected"]):
        path = str(out / ("cluster_%d.bam" % k))
        assert open(path, "rb").read() == want
        assert open(path + ".bai", "rb").read() == be.expected_bytes(path)
    assert len(os.listdir(str(out))) == 10
