"""Per-cluster BAM files with records selected on the way (secedo_amd.split_clusters(..., require_flags=,
exclude_flags=, duplicates=), secedo_bam_split_clusters_select): every file written equals, byte for byte, what
tests/split_select_expected.py derives on the CPU from the inputs, tests/bam_select_ref.py's restatement of the pileup's
rules and the contract -- whatever the mode, the route, the index mode, the batch size and the input kind -- and the
stats equal the counts that module makes. tests/test_split_select_cpu.py checks that the inputs used here hold every
planted case and reach the gather's edges. The pileup reads marked and removed files back to the same result; with the
options off nothing changes, whatever the process-wide settings say; errors leave nothing behind."""
import ctypes as C
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
from tests import split_select_expected as ss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_BATCH = "1000"  # tests/test_gpu_pileup_bam_device.py's smallest SECEDO_BAM_BATCH_BYTES
CHROMS = [0, 1, 2]
FILTER = dict(require_flags=ss.REQUIRE, exclude_flags=ss.EXCLUDE_KEEP_MARKS)
FILTER_EXP = dict(require=ss.REQUIRE, exclude=ss.EXCLUDE_KEEP_MARKS)


def outputs(directory, n):
    return [open(os.path.join(str(directory), "cluster_%d.bam" % k), "rb").read() for k in range(n)]


def check_outputs(directory, expected):
    assert sorted(os.listdir(str(directory))) == sorted("cluster_%d.bam" % k for k in range(len(expected)))
    for k, (got, want) in enumerate(zip(outputs(directory, len(expected)), expected)):
        assert got == want, "cluster_%d.bam differs" % k
        assert gzip.decompress(got) == gzip.decompress(want)  # every CRC32 and ISIZE


def check_stats(info, stats, expected, dropped=0, rg_stats=None):
    assert {k: info[k] for k in ss.DICT_KEYS} == ss.dict_stats(stats)
    assert secedo_amd.split_select_stats() == stats
    assert bam_pileup.split_stats() == {k: info[k] for k in bam_pileup.split_stats()}
    keys = set(bam_pileup.split_stats()) | set(ss.DICT_KEYS) | (set(sr.STAT_KEYS) if rg_stats is not None else set())
    assert set(info) == keys
    if rg_stats is not None:
        assert {k: info[k] for k in sr.STAT_KEYS} == rg_stats == secedo_amd.split_rg_stats()
    assert info["records"] == sum(len(ss.file_records(raw)) for raw in expected)
    assert info["dropped_records"] == dropped
    assert info["compressed_bytes"] == sum(len(raw) for raw in expected)
    assert info["text_bytes"] == sum(len(gzip.decompress(raw)) for raw in expected)


def write_cells(directory, refs, cells, stem="cell_%03d"):
    paths = []
    for c, recs in enumerate(cells):
        paths.append(os.path.join(str(directory), (stem % c) + ".bam"))
        bw.write_bam(paths[-1], refs, recs)
    return paths


@pytest.fixture(scope="module")
def select_set(tmp_path_factory):
    """The six cell files of the select set, and the expected files of every mode under the filter that lets incoming
    marks through, computed once."""
    d = tmp_path_factory.mktemp("split_select_cells")
    enc = tmp_path_factory.mktemp("split_select_encode")
    cells = ss.select_cells()
    paths = write_cells(d, ss.REFS3, cells)
    expected = {m: ss.expected_files(cells, ss.REFS3, ss.SELECT_CLUSTERING, CHROMS, enc, duplicates=m, **FILTER_EXP)
                for m in ss.MODES}
    return dict(dir=d, enc=enc, cells=cells, paths=paths, expected=expected)


@pytest.mark.parametrize("mode", ["mark", "remove", "off"])
def test_per_file_mode(select_set, tmp_path, mode):
    expected, dropped, stats, _ = select_set["expected"][mode]
    assert (stats["duplicate_records"] > 400) == (mode != "off") and stats["dropped_exclude"] > 0
    info = secedo_amd.split_clusters(select_set["paths"], ss.SELECT_CLUSTERING, tmp_path, [2, 0, 1], duplicates=mode,
                                     **FILTER)
    check_outputs(tmp_path, expected)
    check_stats(info, stats, expected)
    assert (info["files"], info["clusters"], info["cells"]) == (6, 4, 6)


@pytest.mark.parametrize("mode", ["mark", "remove"])
def test_tag_mode_with_untagged_records(select_set, tmp_path, mode):
    recs, n_extra = ss.multiplexed(select_set["cells"])
    path = str(tmp_path / "multiplexed.bam")
    bw.write_bam(path, ss.REFS3, recs)
    expected, dropped, stats, _ = ss.expected_files([recs], ss.REFS3, ss.SELECT_CLUSTERING, CHROMS, select_set["enc"],
                                                    duplicates=mode, tag="CB", barcodes=ss.SELECT_BARCODES,
                                                    **FILTER_EXP)
    assert dropped == n_extra and stats == select_set["expected"][mode][2]
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters([path], ss.SELECT_CLUSTERING, out, CHROMS, cell_tag="CB", cells=ss.SELECT_BARCODES,
                                     duplicates=mode, **FILTER)
    check_outputs(out, expected)
    check_stats(info, stats, expected, dropped)


@pytest.mark.parametrize("mode", ["mark", "remove"])
def test_tie_in_tag_mode(tmp_path, mode):
    """X comes first in input order, Y first in the pileup's order: Y stays."""
    files = ss.tie_files()
    paths = write_cells(tmp_path, se.REFS, files, "tie_%d")
    expected, _, stats, _ = ss.expected_files(files, se.REFS, [0, 0], [0], tmp_path, duplicates=mode, tag="CB",
                                              barcodes=ss.TIE_BARCODES)
    names = [r[36:36 + r[12] - 1] for r in ss.file_records(expected[0])]
    flags = {n: r[18] | r[19] << 8 for n, r in zip(names, ss.file_records(expected[0]))}
    if mode == "mark":
        assert flags[b"X"] & 0x400 and not flags[b"Y"] & 0x400
    else:
        assert b"X" not in names and b"Y" in names
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, [0, 0], out, [0], cell_tag="CB", cells=ss.TIE_BARCODES, duplicates=mode)
    check_outputs(out, expected)
    check_stats(info, stats, expected)
    assert info["filter_records"] == 0  # no filter: no record counted at it


@pytest.mark.parametrize("read_groups", [False, True], ids=["plain", "read_groups"])
def test_residues_and_tile_edges(tmp_path, read_groups):
    """The marked byte on every residue mod 16, on both sides of a 4 KiB tile boundary, in the first and the last
    record of an extent."""
    names = ss.RESIDUE_NAMES if read_groups else None
    cells = ss.residue_cells([4 + len(n) for n in ss.RESIDUE_NAMES] if read_groups else [0, 0])
    paths = write_cells(tmp_path, se.REFS, cells, "res_%d")
    expected, _, stats, rg_stats = ss.expected_files(cells, se.REFS, [0, 1], [0], tmp_path, duplicates="mark",
                                                     names=names)
    out = tmp_path / "out"
    out.mkdir()
    kw = dict(read_groups=True, cell_names=names) if read_groups else {}
    info = secedo_amd.split_clusters(paths, [0, 1], out, [0], duplicates="mark", **kw)
    check_outputs(out, expected)
    check_stats(info, stats, expected, rg_stats=rg_stats)


@pytest.mark.parametrize("read_groups", [False, True], ids=["plain", "read_groups"])
def test_long_read(tmp_path, read_groups):
    cells = ss.long_cells()
    paths = write_cells(tmp_path, se.REFS, cells, "long_%d")
    names = ["long_0", "long_1"] if read_groups else None
    expected, _, stats, rg_stats = ss.expected_files(cells, se.REFS, [0, 0], [0], tmp_path, duplicates="mark",
                                                     names=names)
    assert stats["duplicate_records"] == 1
    out = tmp_path / "out"
    out.mkdir()
    info = secedo_amd.split_clusters(paths, [0, 0], out, [0], duplicates="mark", read_groups=read_groups)
    check_outputs(out, expected)
    check_stats(info, stats, expected, rg_stats=rg_stats)


@pytest.mark.parametrize("mode", ["remove", "mark"])
def test_with_read_groups(select_set, tmp_path, mode):
    expected, _, stats, rg_stats = ss.expected_files(select_set["cells"], ss.REFS3, ss.SELECT_CLUSTERING, CHROMS,
                                                     select_set["enc"], duplicates=mode, names=ss.SELECT_NAMES,
                                                     **FILTER_EXP)
    info = secedo_amd.split_clusters(select_set["paths"], ss.SELECT_CLUSTERING, tmp_path, CHROMS, duplicates=mode,
                                     read_groups=True, cell_names=ss.SELECT_NAMES, **FILTER)
    check_outputs(tmp_path, expected)
    check_stats(info, stats, expected, rg_stats=rg_stats)
    assert rg_stats["tagged_records"] == info["records"]  # the RG edit is applied to what the selection kept


def test_routes(select_set, tmp_path, monkeypatch):
    expected, _, stats, _ = select_set["expected"]["mark"]
    paths = select_set["paths"]
    if not all(os.path.exists(p + ".bai") for p in paths):
        secedo_amd.bam_index_build(paths)
    kw = dict(duplicates="mark", **FILTER)
    for k, route in enumerate((dict(inflate="device", index="off"), dict(inflate="host", index="require"))):
        out = tmp_path / ("route_%d" % k)
        out.mkdir()
        info = secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, out, CHROMS, **route, **kw)
        check_outputs(out, expected)
        check_stats(info, stats, expected)
        assert bam_pileup.bam_index_stats()["files_indexed"] == (6 if route["index"] == "require" else 0)
        assert (bam_pileup.bam_route_stats()["device_blocks"] > 0) == (route["inflate"] == "device")
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", SMALL_BATCH)
    out = tmp_path / "batch"
    out.mkdir()
    secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, out, CHROMS, inflate="host", index="off", **kw)
    check_outputs(out, expected)
    monkeypatch.delenv("SECEDO_BAM_BATCH_BYTES")
    # two of the files as SAM text and one as bgzipped SAM
    mixed = list(paths)
    for c in (1, 5):
        mixed[c] = str(tmp_path / ("cell_%03d.sam" % c))
        sw.write_sam(mixed[c], ss.REFS3, select_set["cells"][c])
    mixed[0] = str(tmp_path / "cell_000.sam.gz")
    open(mixed[0], "wb").write(bw.bgzf(sw.sam_text(ss.REFS3, select_set["cells"][0]).encode()))
    out = tmp_path / "sam"
    out.mkdir()
    info = secedo_amd.split_clusters(mixed, ss.SELECT_CLUSTERING, out, CHROMS, **kw)
    check_outputs(out, expected)
    check_stats(info, stats, expected)
    # the indexes of the outputs
    out = tmp_path / "bai"
    out.mkdir()
    secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, out, CHROMS, bai=True, **kw)
    for k, want in enumerate(expected):
        path = str(out / ("cluster_%d.bam" % k))
        assert open(path, "rb").read() == want
        assert open(path + ".bai", "rb").read() == be.expected_bytes(path), k


def test_two_runs_give_identical_bytes(select_set, tmp_path):
    runs = []
    for k in range(2):
        out = tmp_path / ("run_%d" % k)
        out.mkdir()
        secedo_amd.split_clusters(select_set["paths"], ss.SELECT_CLUSTERING, out, CHROMS, duplicates="mark", **FILTER)
        runs.append(outputs(out, 4))
    assert runs[0] == runs[1]


def same_pileup(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k))
               for k in ("chr_locus_off", "locus_pos", "locus_entry_off", "read_ids", "id_base"))


def test_round_trip_through_the_pileup(select_set, tmp_path):
    """Excluding the marks of a "mark" file gives the pileup of the "remove" file, cell by cell."""
    paths, cells = select_set["paths"], select_set["cells"]
    kw = dict(require_flags=3, exclude_flags=0xF04, read_groups=True, cell_names=ss.SELECT_NAMES)
    dirs, infos = {}, {}
    for mode in ("mark", "remove"):
        dirs[mode] = tmp_path / mode
        dirs[mode].mkdir()
        infos[mode] = secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, dirs[mode], CHROMS, duplicates=mode, **kw)
    off = ss.expected_files(cells, ss.REFS3, ss.SELECT_CLUSTERING, CHROMS, select_set["enc"], require=3, exclude=0xF04,
                            names=ss.SELECT_NAMES)[0]
    arrived_marked = sum(1 for raw in off for r in ss.file_records(raw) if r[19] & 0x04)
    excluded, loci = 0, 0
    for k in (0, 1):
        names = [ss.SELECT_NAMES[c] for c, cl in enumerate(ss.SELECT_CLUSTERING) if cl == k]
        for chrom in (0, 1):
            args = (None, False, chrom, 1000, 30, 30, 0, 4, 1)
            marked = secedo_amd.pileup_bams([str(dirs["mark"] / ("cluster_%d.bam" % k))], *args, cell_tag="RG",
                                            cells=names, exclude_flags=0x400)
            excluded += secedo_amd.bam_select_stats()["dropped_exclude"]
            removed = secedo_amd.pileup_bams([str(dirs["remove"] / ("cluster_%d.bam" % k))], *args, cell_tag="RG",
                                             cells=names)
            assert same_pileup(marked, removed), (k, chrom)
            loci += len(removed.locus_pos)
    assert loci > 100
    assert excluded == infos["mark"]["duplicate_records"] + arrived_marked
    assert infos["mark"]["duplicate_records"] == infos["remove"]["duplicate_records"] > 400


def test_off_is_off(select_set, tmp_path, monkeypatch):
    paths, cells = select_set["paths"], select_set["cells"]
    sources = [se.source_of_recs(ss.REFS3, recs) for recs in cells]
    plain, _ = se.expected_files(sources, ss.SELECT_CLUSTERING, CHROMS, select_set["enc"])
    tagged, _, rg_stats = sr.expected_files(sources, ss.SELECT_CLUSTERING, CHROMS, ss.SELECT_NAMES, select_set["enc"])
    # a call with the options on, so that the stats have something to forget
    first = tmp_path / "first"
    first.mkdir()
    secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, first, CHROMS, duplicates="mark")
    assert secedo_amd.split_select_stats()["duplicate_records"] > 0
    pileup_stats = secedo_amd.bam_select_stats()  # the pileup's getter is not touched by split calls

    def run_both(name, **kw):
        out = tmp_path / name
        out.mkdir()
        info = secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, out, CHROMS, **kw)
        check_outputs(out, plain)
        assert set(info) == set(bam_pileup.split_stats()) and secedo_amd.split_select_stats() == ss.ZERO
        out = tmp_path / (name + "_rg")
        out.mkdir()
        info = secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, out, CHROMS, read_groups=True,
                                         cell_names=ss.SELECT_NAMES, **kw)
        check_outputs(out, tagged)
        assert set(info) == set(bam_pileup.split_stats()) | set(sr.STAT_KEYS)
        assert {k: info[k] for k in sr.STAT_KEYS} == rg_stats and secedo_amd.split_select_stats() == ss.ZERO

    run_both("defaults")
    run_both("explicit", require_flags=0, exclude_flags=None, duplicates="off")
    # the pileup's settings, from the environment and process-wide, have no effect on any split call
    monkeypatch.setenv("SECEDO_BAM_REQUIRE_FLAGS", "3")
    monkeypatch.setenv("SECEDO_BAM_EXCLUDE_FLAGS", "0xF04")
    monkeypatch.setenv("SECEDO_BAM_DUPLICATES", "remove")
    run_both("environment")
    for name in ("SECEDO_BAM_REQUIRE_FLAGS", "SECEDO_BAM_EXCLUDE_FLAGS", "SECEDO_BAM_DUPLICATES"):
        monkeypatch.delenv(name)  # the block below restores what it finds: not these
    with bam_pileup._select(require_flags=3, exclude_flags=0xF04, remove_duplicates=True):
        run_both("process")
        # nor on one with its own options
        expected, _, stats, _ = select_set["expected"]["mark"]
        out = tmp_path / "own"
        out.mkdir()
        info = secedo_amd.split_clusters(paths, ss.SELECT_CLUSTERING, out, CHROMS, duplicates="mark", **FILTER)
        check_outputs(out, expected)
        check_stats(info, stats, expected)
    assert secedo_amd.bam_select_stats() == pileup_stats


def raw_select(paths, clustering, out_dir, require, exclude, duplicates, select_info=True):
    """secedo_bam_split_clusters_select itself, past the checks the Python wrapper makes -> the return code."""
    arr, n = bam_pileup._files(paths)
    cl = np.ascontiguousarray(clustering, dtype=np.uint16)
    ids = np.zeros(1, dtype=np.uint32)
    info, t, rg, sel = bam_pileup.SplitInfo(), bam_pileup.Times(), bam_pileup.SplitRgInfo(), bam_pileup.SelectInfo()
    return bam_pileup.lib().secedo_bam_split_clusters_select(
        arr, n, ids.ctypes.data, 1, cl.ctypes.data, len(cl), None, None, 0, os.fsencode(str(out_dir)), 0, 1,
        C.byref(info), C.byref(t), None, 0, C.byref(rg), 0, require, exclude, duplicates,
        C.byref(sel) if select_info else None)


def test_errors(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    cells = [c[:40] for c in ss.select_cells()[:3]]
    good = write_cells(tmp_path, ss.REFS3, cells, "small_%d")
    junk = str(tmp_path / "junk.bam")
    open(junk, "wb").write(b"not a BAM file")
    invalid = secedo_amd._lib.E_INVALID_ARG

    def refused(match, paths=good, **kw):
        with pytest.raises(secedo_amd.SecedoError, match=match) as e:
            secedo_amd.split_clusters(paths, [0, 1, 0], out, [0], **kw)
        assert e.value.code == invalid
        assert os.listdir(str(out)) == []

    # the wrapper's refusals, made before any input is read: a file that is no BAM is not reached
    refused("share bits 0x400", [good[0], junk, good[2]], require_flags="DUP", exclude_flags=0x400)
    refused("outside 0..0xFFFF", [good[0], junk, good[2]], exclude_flags=0x10000)
    refused("unknown flag", exclude_flags="DUPE")
    refused("duplicates is 'off', 'mark' or 'remove'", duplicates="keep")
    refused("duplicates is 'off', 'mark' or 'remove'", duplicates=True)
    # the library's own
    last = bam_pileup.lib().secedo_bam_last_error
    assert raw_select([good[0], junk, good[2]], [0, 1, 0], out, 0x10000, 0, 0) == invalid and b"0xFFFF" in last()
    assert raw_select([good[0], junk, good[2]], [0, 1, 0], out, 0, 0x1FFFF, 2) == invalid and b"0xFFFF" in last()
    assert raw_select([good[0], junk, good[2]], [0, 1, 0], out, 0x402, 0x400, 1) == invalid and b"share a bit" in last()
    assert raw_select([good[0], junk, good[2]], [0, 1, 0], out, 0, 0, 3) == invalid and b"duplicates 3" in last()
    assert raw_select(good, [0, 1, 0], out, 0, 0, 2, select_info=False) == invalid
    assert os.listdir(str(out)) == []
    # marking is a split option: the pileup's process-wide setting does not take it
    assert bam_pileup.lib().secedo_bam_set_duplicates(2) == invalid
    # a defective input under selection leaves nothing, and the plain call's refusals hold
    refused("junk.bam", [good[0], junk, good[2]], duplicates="mark", exclude_flags=0x400)
    secedo_amd.split_clusters(good, [0, 1, 0], out, [0], duplicates="remove")
    with pytest.raises(secedo_amd.SecedoError, match="cluster_0.bam exists"):
        secedo_amd.split_clusters(good, [0, 1, 0], out, [0], duplicates="mark")
    assert sorted(os.listdir(str(out))) == ["cluster_0.bam", "cluster_1.bam"]


def test_cli_end_to_end(select_set, tmp_path):
    expected, _, stats, _ = select_set["expected"]["mark"]
    clustering = tmp_path / "clustering"
    clustering.write_text(",".join(str(c) for c in ss.SELECT_CLUSTERING) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sys.executable, "-m", "secedo_amd.split_main", "-i", str(select_set["dir"]), "--clustering",
                        str(clustering), "-o", str(out), "--chromosomes", "1,2,3", "--require_flags",
                        "PAIRED,PROPER_PAIR", "--exclude_flags", "0xB04", "--duplicates", "mark"], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Duplicates: %d records of %d templates marked" % (stats["duplicate_records"],
                                                              stats["duplicate_templates"]) in r.stdout
    assert "Flag filter: %d of %d records dropped" % (stats["dropped_require"] + stats["dropped_exclude"],
                                                     stats["records"]) in r.stdout
    check_outputs(out, expected)
