"""secedo_bam_split_clusters_select without a GPU: the marked byte, the mark's packing, the gather's lanes and the mask
rule of secedo_amd/csrc/bam_split.hpp as a program under the sanitizers; tests/split_select_expected.py against itself
(reading an expected "mark" file back gives the "off" file's records with exactly the chosen ones changed, in exactly
one bit; the "remove" file is the "mark" file without the records that carry a new mark); the conditions the GPU
tests' inputs must meet (every planted case of the select set is there, the residue set reaches every edge of the
gather, the tie set's winner is Y); and the refusals of ``python -m secedo_amd.split_main`` for the new options, made
before torch is imported."""
import os
import subprocess

import pytest

from tests import bam_select_ref as ref
from tests import bam_writer as bw
from tests import split_expected as se
from tests import split_select_expected as ss
from tests.test_split_clusters_cpu import cli_inputs, refused  # noqa: F401  -- the fixture and the CLI wrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_split_select_test")
CHROMS = [0, 1, 2]


def test_host_program_under_sanitizers():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and r.stderr == ""


def test_cli_refusals(cli_inputs):  # noqa: F811
    cells, clustering, out = cli_inputs
    base = ["-i", cells, "-o", out, "--chromosomes", "1", "--clustering", clustering]
    why = refused(base + ["--require_flags", "PROPER_PAIR,DUP", "--exclude_flags", "0x400"])
    assert "share bits 0x400" in why
    assert "outside 0..0xFFFF" in refused(base + ["--exclude_flags", "0x10000"])
    assert "outside 0..0xFFFF" in refused(base + ["--require_flags", "65536"])
    assert "unknown flag" in refused(base + ["--exclude_flags", "DUPLICATE"])
    why = refused(base + ["--duplicates", "keep"])
    assert "--duplicates" in why and "off, mark or remove" in why
    assert os.listdir(str(out)) == []


@pytest.fixture(scope="module")
def select_set():
    return ss.select_cells()


def test_select_set_holds_every_planted_case(select_set):
    cells = select_set
    assert len(cells) == 6 and 100 < min(len(c) for c in cells)
    filtered, chosen, stats = ss.selection(cells, CHROMS, ss.REQUIRE, ss.EXCLUDE_KEEP_MARKS, "mark")
    name = {(f, k): r.name for f, recs in enumerate(cells) for k, r in enumerate(recs)}
    chosen_names = {name[x] for x in chosen}
    filtered_names = {name[x] for x in filtered}
    for c in (0, 1, 2, 4, 5):  # cell 3 has every record filtered
        p = "c%d_" % c
        assert p + "d2_b" in chosen_names and p + "d2_a" not in chosen_names
        assert {p + "d3_b", p + "d3_c"} <= chosen_names and p + "d3_a" not in chosen_names  # the tie: the first stays
        wave = [n for n in chosen_names if n.startswith(p + "w")]
        assert len(wave) == 69  # a group longer than a wave: one stays
        assert {p + "s1", p + "s2"} <= chosen_names and not {p + "s0", p + "srev"} & chosen_names
        assert p + "clip" in chosen_names and p + "noclip" not in chosen_names  # the clipped ends; the lower score goes
        assert not {p + "tri", p + "trimate"} & chosen_names
        assert p + "half2" in chosen_names and p + "half" in filtered_names  # halved by the filter
        assert p + "md_b" in chosen_names and not {p + "md_a", p + "md_c"} & chosen_names  # a marked keeper
        assert {p + "flag%d" % k for k in range(5)} <= filtered_names
    assert not {"shared_pair", "shared_single"} & (chosen_names | filtered_names)  # two cells of one cluster
    assert ss.SELECT_CLUSTERING[0] == ss.SELECT_CLUSTERING[2]
    # without the filter the halved pair is whole, and a single is never a duplicate of a pair
    _, plain_chosen, _ = ss.selection(cells, CHROMS, 0, 0, "mark")
    assert "c0_half2" not in {name[x] for x in plain_chosen}
    # cell 4 on chr2, cell 3 everywhere and chr3 for everyone: all filtered
    for f, recs in enumerate(cells):
        for k, r in enumerate(recs):
            if r.ref == 2 or f == 3 or (f == 4 and r.ref == 1):
                assert (f, k) in filtered, (f, r.name)
    assert stats["large_templates"] == 5 and stats["duplicate_templates"] > 5 * 75
    assert stats["records"] == sum(len(c) for c in cells) and stats["dropped_require"] and stats["dropped_exclude"]
    # the callers' filter drops the incoming marks too
    filtered_all, _, _ = ss.selection(cells, CHROMS, ss.REQUIRE, ss.EXCLUDE, "off")
    assert {"c0_md_a", "c0_md_c"} <= {name[x] for x in filtered_all}


@pytest.mark.parametrize("names", [None, ss.SELECT_NAMES], ids=["plain", "read_groups"])
def test_expected_files_against_themselves(select_set, tmp_path, names):
    cells = select_set
    kw = dict(require=ss.REQUIRE, exclude=ss.EXCLUDE_KEEP_MARKS, names=names)
    files = {m: ss.expected_files(cells, ss.REFS3, ss.SELECT_CLUSTERING, CHROMS, tmp_path, duplicates=m, **kw)
             for m in ss.MODES}
    _, chosen, stats = ss.selection(cells, CHROMS, ss.REQUIRE, ss.EXCLUDE_KEEP_MARKS, "mark")
    assert files["mark"][2] == files["remove"][2] == stats and files["off"][2]["templates"] == 0
    new_marks = 0
    for k in range(len(files["off"][0])):
        off, mark, remove = (ss.file_records(files[m][0][k]) for m in ss.MODES)
        assert len(off) == len(mark)
        kept = []
        for a, b in zip(off, mark):
            if a == b:
                kept.append(b)
                continue
            diff = [q for q in range(len(a)) if a[q] != b[q]]
            assert len(a) == len(b) and diff == [19] and a[19] ^ b[19] == 0x04 and b[19] & 0x04  # exactly one bit
            new_marks += 1
        assert remove == kept
        assert any(r[19] & 0x04 for r in kept) == (k in (0, 1))  # incoming marks stay, on keepers too
    assert new_marks == len(chosen) == stats["duplicate_records"]
    # cluster 2 has no cell, cluster 3's cell has every record filtered: header-only files, no member but the header's
    for k in (2, 3):
        assert ss.file_records(files["mark"][0][k]) == [] and len(se.member_sizes(files["mark"][0][k])) == 2
    # chr3 contributes no member to any file: the files of a call without it have as many
    two = ss.expected_files(cells, ss.REFS3, ss.SELECT_CLUSTERING, [0, 1], tmp_path, duplicates="mark", **kw)[0]
    assert [len(se.member_sizes(raw)) for raw in two] == [len(se.member_sizes(raw)) for raw in files["mark"][0]]


def test_tag_mode_chooses_what_per_file_mode_chooses(select_set):
    recs, n_extra = ss.multiplexed(select_set)
    kw = dict(require=ss.REQUIRE, exclude=ss.EXCLUDE_KEEP_MARKS, duplicates="mark")
    parts, dropped, stats, _ = ss.cluster_parts([recs], ss.REFS3, ss.SELECT_CLUSTERING, CHROMS, tag="CB",
                                                barcodes=ss.SELECT_BARCODES, **kw)
    want, none, want_stats, _ = ss.cluster_parts(select_set, ss.REFS3, ss.SELECT_CLUSTERING, CHROMS, **kw)
    assert dropped == n_extra > 0 and none == 0
    assert parts == want and stats == want_stats  # the untagged records reach neither rule


@pytest.mark.parametrize("read_groups", [False, True], ids=["plain", "read_groups"])
def test_residue_set_reaches_every_edge(read_groups):
    names = ss.RESIDUE_NAMES if read_groups else None
    grow = [4 + len(n) for n in ss.RESIDUE_NAMES] if read_groups else [0, 0]
    cells = ss.residue_cells(grow)
    off = ss.cluster_parts(cells, se.REFS, [0, 1], [0], duplicates="off", names=names)[0]
    mark, _, stats, _ = ss.cluster_parts(cells, se.REFS, [0, 1], [0], duplicates="mark", names=names)
    edges = ss.mark_edges(off, mark)
    assert edges["residues"] == set(range(16))
    assert edges["tile_last"] >= 1 and edges["tile_first"] >= 1
    assert edges["extent_first"] == 2 and edges["extent_last"] == 2  # both clusters' extents
    fillers = sum(1 for c in cells for r in c if r.tags)  # they stand alone; every other record is in a group of two
    assert edges["marked"] == stats["duplicate_records"] == (sum(len(c) for c in cells) - fillers) // 2
    assert len(off[0][1]) > 2 * ss.TILE  # more than one workgroup


def test_long_set():
    cells = ss.long_cells()
    _, chosen, stats = ss.selection(cells, [0], 0, 0, "mark")
    assert chosen == {(0, 1)} and cells[0][1].name == "long_twin" and stats["duplicate_records"] == 1
    assert len(bw.encode_record(cells[0][1])) > 140_000


def test_tie_set_winner_is_y():
    files = ss.tie_files()
    assert [r.name for r in files[0]].index("X") < len(files[0])  # X is in the first file: first in input order
    x, y = next(r for r in files[0] if r.name == "X"), next(r for r in files[1] if r.name == "Y")
    assert ref.five_prime(x) == ref.five_prime(y) == (480, 0) and ref.score(x) == ref.score(y)
    assert (x.pos, y.pos) == (500, 480)
    _, chosen, stats = ss.selection(files, [0], 0, 0, "mark", tag="CB", barcodes=ss.TIE_BARCODES)
    names = {files[f][k].name for f, k in chosen}
    assert names == {"X", "other1"}  # Y stays: the pileup's order is by Position inside a cell, then by file
    assert stats["duplicate_records"] == 3
