"""secedo_bam_split_clusters_rg without a GPU: the read-group rules of secedo_amd/csrc/bam_split.hpp as a program under
the sanitizers, tests/split_rg_expected.py against itself (inflating the file it expects and reading it back gives the
cluster's records, each with its cell's RG:Z as the last field and no other RG), the conditions the GPU tests' inputs
must meet to reach the gather's edges, and the refusals of ``python -m secedo_amd.split_main --read_groups`` (made
before torch is imported)."""
import gzip
import os
import subprocess

import pytest

from tests import bam_writer as bw
from tests import split_expected as se
from tests import split_rg_expected as sr
from tests.test_split_clusters_cpu import cli_inputs, refused  # noqa: F401  -- the fixture and the CLI wrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_split_rg_test")


def test_host_program_under_sanitizers():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and r.stderr == ""


# ---- the rules, on records written out by hand

def aux_of(rec: bytes) -> bytes:
    return rec[sr.aux_start(rec):]


def hand_record(aux: bytes) -> bytes:
    r = bw.Rec(name="r", ref=0, pos=5, cigar=[("M", 3)], seq="ACG", qual=[30] * 3)
    return sr.with_raw_aux(r, aux)


def test_edit_record_by_hand():
    suffix = b"RGZcell\0"
    cases = [  # aux before, aux after, hole length or None, parsed
        (b"", suffix, None, True),
        (b"RGZold\0", suffix, 7, True),
        (b"ASC\x05RGZold\0NMC\x01", b"ASC\x05NMC\x01" + suffix, 7, True),
        (b"ASC\x05RGi\x01\x02\x03\x04", b"ASC\x05" + suffix, 7, True),
        (b"XZZabRGZx\0", b"XZZabRGZx\0" + suffix, None, True),
        (b"XCBC\x03\0\0\0RGZRGZcell\0", b"XCBC\x03\0\0\0RGZ" + suffix, 8, True),
        (b"XHH1A\0XBBS\x01\0\0\0\x07\x00RGZa\0RGZb\0", b"XHH1A\0XBBS\x01\0\0\0\x07\x00RGZb\0" + suffix, 5, True),
        (b"RGZold\0XQ?abc", b"RGZold\0XQ?abc" + suffix, None, False),
        (b"RGZold\0XZZno-nul", b"RGZold\0XZZno-nul" + suffix, None, False),
        (b"RGZold\0XY", b"RGZold\0XY" + suffix, None, False),
        (b"XBBi\x02\0\0\0\x01\0\0\0", b"XBBi\x02\0\0\0\x01\0\0\0" + suffix, None, False),
    ]
    for before, after, hole_len, parsed in cases:
        rec = hand_record(before)
        new, hole, ok = sr.edit_record(rec, "cell")
        assert ok == parsed and (hole[1] if hole else None) == hole_len, before
        assert aux_of(new) == after and new[4:sr.aux_start(rec)] == rec[4:sr.aux_start(rec)], before
        assert int.from_bytes(new[:4], "little") == len(new) - 4


def test_names():
    assert sr.default_names(["/a/cell1.bam", "b/cell2.sam", "cell3.sam.gz", "d/cell4.bam.sam", "x.gz"]) == \
        ["cell1", "cell2", "cell3", "cell4.bam", "x.gz"]
    assert sr.name_fault(["a", "~" * 254, "!"]) is None
    for bad in ("", "a" * 255, "a\tb", "a b", "\x7f"):
        assert sr.name_fault(["ok", bad]) == "cell 1"
    assert sr.name_fault(["a", "b", "a"]) == "cells 0 and 2"


# ---- split_rg_expected against itself

def check_expected(sources, clustering, chromosome_ids, names, tmp_path, tag=None, barcodes=None):
    """Every expected file is a BAM of whole members with the cluster's @RG lines that holds the cluster's records in
    order, each as it was except for its RG: exactly one, its cell's name, the last field."""
    files, dropped, stats = sr.expected_files(sources, clustering, chromosome_ids, names, tmp_path, tag, barcodes)
    marks = sr.cluster_parts(sources, clustering, chromosome_ids, names, tag, barcodes)[3]
    plain = se.cluster_parts(sources, clustering, chromosome_ids, tag, barcodes)[0]
    seen = unparsed = 0
    for k, raw in enumerate(files):
        assert raw.endswith(se.EOF) and all(isize <= se.CUT for isize, _ in se.member_sizes(raw))
        path = tmp_path / ("expected_%d.bam" % k)
        path.write_bytes(raw)
        refs, recs = bw.read_bam(str(path))
        assert refs == sources[0].refs
        flat = gzip.decompress(raw)
        text = flat[8:8 + int.from_bytes(flat[4:8], "little")].decode()
        lines = text.split("\n")
        rg = ["@RG\tID:%s\tSM:cluster_%d" % (names[c], k) for c in range(len(names)) if clustering[c] == k]
        assert [x for x in lines if x.startswith("@RG")] == rg
        assert [x[:3] for x in lines if x] == ["@HD"] + ["@SQ"] * len(refs) + ["@RG"] * len(rg) + ["@PG", "@CO"]
        before, o = [], 0  # the unedited records of the cluster, in the same order
        flat = b"".join(plain[k][1:])
        while o < len(flat):
            n = 4 + int.from_bytes(flat[o:o + 4], "little")
            before.append(flat[o:o + n])
            o += n
        cells = [m[5] for here in marks for m in here if m[0] == k]
        assert len(before) == len(recs) == len(cells)
        assert [(r["ref"], r["pos"]) for r in recs] == sorted((r["ref"], r["pos"]) for r in recs)
        for old, r, cell in zip(before, recs, cells):
            suffix = b"RGZ" + names[cell].encode() + b"\0"
            head, aux = old[:sr.aux_start(old)], r["aux"]
            assert (r["ref"], r["pos"]) == se.ref_pos(old) and aux.endswith(suffix)
            fields = sr.aux_fields(old)
            if fields is None:  # kept whole
                unparsed += 1
                assert aux == old[len(head):] + suffix
                continue
            new = head + aux
            new_fields = sr.aux_fields(new)
            assert new_fields is not None
            assert [t for _a, _b, t in new_fields].count(b"RG") == 1
            a, b, _t = new_fields[-1]
            assert new[a:b] == suffix
            assert [new[a:b] for a, b, _t in new_fields[:-1]] == [old[a:b] for a, b, t in fields if t != b"RG"]
        seen += len(recs)
    assert seen == stats["tagged_records"] and unparsed == stats["unparsed_records"]
    return files, dropped, stats


def test_expected_on_the_synthetic_sets(tmp_path):
    cells = sr.cell_items()
    sources = [sr.source_of_items(se.REFS, c) for c in cells]
    _files, dropped, stats = check_expected(sources, se.CLUSTERING, [0, 1], sr.NAMES, tmp_path)
    assert dropped == 0 and stats["unparsed_records"] > 0 and 0 < stats["replaced_records"] < stats["tagged_records"]
    # tag mode: the survivors are tagged with their barcode
    recs, n_extra = se.multiplexed_records(se.cell_records())
    _files, dropped, stats = check_expected([se.source_of_recs(se.REFS, recs)], se.CLUSTERING, [0, 1], se.BARCODES,
                                            tmp_path, "CB", se.BARCODES)
    assert dropped == n_extra and stats["replaced_records"] == 0
    # keyed by RG itself: every survivor's own RG goes, and the same value comes back at the end
    recs, n_extra = se.multiplexed_records(sr.rg_keyed_cells())
    _files, dropped, stats = check_expected([se.source_of_recs(se.REFS, recs)], se.CLUSTERING, [0, 1], se.BARCODES,
                                            tmp_path, "RG", se.BARCODES)
    assert dropped == n_extra and stats["replaced_records"] == stats["tagged_records"] > 0
    assert stats["added_bytes"] == stats["removed_bytes"]
    # the long read: its hole lies far behind the ML array
    long_cells = sr.long_items()
    _new, hole, parsed = sr.edit_record(bw.encode_record(long_cells[0][0]), "L")
    assert parsed and hole[0] > 100_000 and hole[0] // sr.TILE > 24
    check_expected([se.source_of_recs(se.REFS, c) for c in long_cells], [0, 1], [0], ["L", "flat"], tmp_path)


def test_the_gpu_inputs_reach_the_edges():
    """Conditions on the inputs of tests/test_gpu_split_rg.py, from the expected streams alone."""
    cells = sr.cell_items()
    sources = [sr.source_of_items(se.REFS, c) for c in cells]
    parts, _dropped, _stats, marks = sr.cluster_parts(sources, se.CLUSTERING, [0, 1], sr.NAMES)
    edges = sr.stream_edges(parts, marks)
    every = set(range(16))
    assert edges["record"] == every and edges["hole"] == every and edges["suffix"] == every
    assert edges["word_straddles"] >= 1 and edges["suffix_straddles"] >= 1
    # the tile set puts a hole, a block_size word and a suffix on tile boundaries by construction
    name = "tile-cell"
    items = sr.tile_items(name)
    parts, _dropped, _stats, marks = sr.cluster_parts([sr.source_of_items(se.REFS, items[0])], [0], [0], [name])
    edges = sr.stream_edges(parts, marks)
    assert (edges["word_straddles"], edges["hole_straddles"], edges["suffix_straddles"]) == (1, 1, 1)
    assert marks[0][0][2] == sr.TILE and marks[0][1][1] == 2 * sr.TILE - 2 and marks[0][1][3] == 3 * sr.TILE - 3
    # the edited extents of the edge set: exactly one member, and one byte more
    names = ["full-cell", "o", "single"]
    edge = sr.edge_items(names)
    parts, _dropped, _stats, _marks = sr.cluster_parts([se.source_of_recs(se.REFS, c) for c in edge], [0, 1, 2], [0],
                                                       names)
    assert [len(ps[1]) for ps in parts[:2]] == [se.CUT, se.CUT + 1] and len(edge[2]) == 1
    # what the twelve cells hold: every variant, and in the SAM cells only what SAM text holds
    kinds = set()
    for c, items in enumerate(cells):
        for it in items:
            raw = sr.raw_of(it)
            fields = sr.aux_fields(raw)
            if c in sr.SAM_CELLS:
                assert not isinstance(it, bytes) and fields is not None
            if fields is None:
                kinds.add("unparsed")
                continue
            tags = [t for _a, _b, t in fields]
            if not fields:
                kinds.add("no aux")
            if b"RG" in tags:
                a, b, _t = fields[tags.index(b"RG")]
                kinds.add(("first", "middle", "last")[0 if tags[0] == b"RG" else 2 if tags[-1] == b"RG" else 1])
                kinds.add("type " + chr(raw[a + 2]))
                if chr(raw[a + 2]) == "Z":
                    old, new = b - a - 4, len(sr.NAMES[c])
                    kinds.add("shrinks" if old > new else "grows" if old < new else "stays")
                if any(raw[x + 2:x + 3] == b"H" for x, _y, _t in fields[:tags.index(b"RG")]):
                    kinds.add("H in front")
                if any(raw[x + 2:x + 4] == b"BS" for x, _y, _t in fields[:tags.index(b"RG")]):
                    kinds.add("B:S in front")
            if any(raw[x + 2:x + 3] == b"Z" and b"RGZx" in raw[x + 3:y] for x, y, _t in fields):
                kinds.add("RGZx in Z")
            if any(raw[x + 2:x + 4] == b"BC" and b"RGZ" in raw[x + 8:y] for x, y, _t in fields):
                kinds.add("RGZ in B:C")
    assert kinds >= {"unparsed", "no aux", "first", "middle", "last", "type Z", "type i", "type A", "shrinks", "grows",
                     "stays", "H in front", "B:S in front", "RGZx in Z", "RGZ in B:C"}, kinds
    raws = [sr.raw_of(it) for items in cells for it in items]
    assert any(r.endswith(b"XQ?abc") for r in raws) and any(r.endswith(b"XZZno-nul") for r in raws)


# ---- the CLI's refusals

def test_cli_refusals(cli_inputs, tmp_path):  # noqa: F811
    cells, clustering, out = cli_inputs
    base = ["-i", cells, "-o", out, "--chromosomes", "1", "--clustering", clustering]
    names = tmp_path / "names.txt"
    names.write_text("a\nb\nc\n")
    assert "--cell_names needs --read_groups" in refused(base + ["--cell_names", names])
    assert "does not exist" in refused(base + ["--read_groups", "--cell_names", tmp_path / "missing"])
    short = tmp_path / "short.txt"
    short.write_text("a\nb\n")
    why = refused(base + ["--read_groups", "--cell_names", short])
    assert "lists 2 names" in why and "has 3 cells" in why
    assert os.listdir(str(out)) == []
