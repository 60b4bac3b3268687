"""What ``secedo_amd.split_clusters(..., require_flags=, exclude_flags=, duplicates=)`` must write, computed on the CPU
from the contract of secedo_bam_split_clusters_select (include/secedo_bam.h). It sits on tests/split_expected.py (the
sources, the order, the members M(x)), tests/split_rg_expected.py (the read-group edit) and tests/bam_select_ref.py
(rules 3c and 3d of the pileup in plain Python):

  selection       per requested chromosome ``bam_select_ref.select`` twice, filter only and filter plus duplicates:
                  the filtered records, the chosen duplicates and the counts of secedo_bam_select_info
  sources_for     the inputs without the dropped records ("remove"), or with ``flag |= 0x400`` on the chosen ones
                  ("mark"), each record edited the plain way on its ``bw.Rec`` and encoded again
  expected_files  the existing ``expected_files`` of split_expected / split_rg_expected on those sources

so a "remove" file is, by construction, what the plain call writes on inputs that never held the dropped records, and a
"mark" file what it writes on inputs whose chosen records arrived marked. Below that, the input sets of
tests/test_gpu_split_select.py and ``mark_edges``, which says from the expected streams alone where the marked bytes
fall, so that tests/test_split_select_cpu.py can check without a GPU that the sets reach the gather's edges.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from tests import bam_select_ref as ref
from tests import bam_writer as bw
from tests import split_expected as se
from tests import split_rg_expected as sr

TILE = sr.TILE
DUP = 0x400
MODES = ("off", "mark", "remove")
STAT_KEYS = ref.STAT_KEYS
# the keys the dict of split_clusters gains: "records" is the split's own (records written)
DICT_KEYS = tuple("filter_records" if k == "records" else k for k in STAT_KEYS)
ZERO = dict.fromkeys(STAT_KEYS, 0)

# ---------------------------------------------------------------------------------------------------------------------
# the rules


def tag_cell_of(tag: str, barcodes: Sequence[str]):
    """The cell of a ``bw.Rec`` in tag mode: the index of the value of its first field named ``tag`` when that is
    Z-typed and listed, else None."""
    index = {b: c for c, b in enumerate(barcodes)}

    def cell_of(r: bw.Rec) -> Optional[int]:
        for name, typ, value in r.tags:
            if name == tag:
                return index.get(value) if typ == "Z" else None
        return None

    return cell_of


def selection(files: Sequence[Sequence[bw.Rec]], chromosome_ids: Sequence[int], require: int = 0, exclude: int = 0,
              duplicates: str = "off", tag: Optional[str] = None, barcodes: Optional[Sequence[str]] = None):
    """-> (filtered {(f, k)}, chosen duplicates {(f, k)}, stats) over the requested chromosomes."""
    assert duplicates in MODES
    cell_of = None if tag is None else tag_cell_of(tag, barcodes)
    filtered: Set[Tuple[int, int]] = set()
    chosen: Set[Tuple[int, int]] = set()
    stats = dict(ZERO)
    for chrom in sorted(chromosome_ids):
        only_filter, st = ref.select(files, chrom, require, exclude, False, cell_of)
        if duplicates != "off":
            both, st = ref.select(files, chrom, require, exclude, True, cell_of)
            assert only_filter <= both
            chosen |= both - only_filter
        filtered |= only_filter
        stats = ref.add_stats(stats, st)
    return filtered, chosen, stats


def sources_for(files: Sequence[Sequence[bw.Rec]], refs, filtered, chosen, duplicates: str) -> List[se.Source]:
    out = []
    for f, recs in enumerate(files):
        kept = []
        for k, r in enumerate(recs):
            if (f, k) in filtered or (duplicates == "remove" and (f, k) in chosen):
                continue
            if duplicates == "mark" and (f, k) in chosen:
                r = copy.copy(r)
                r.flag |= DUP
            kept.append(r)
        out.append(se.source_of_recs(refs, kept))
    return out


def cluster_parts(files, refs, clustering, chromosome_ids, require=0, exclude=0, duplicates="off", names=None, tag=None,
                  barcodes=None):
    """-> (parts[k] = [header, the records of the 1st requested chromosome, ...], dropped records (those without a
    cell), the select stats, the read-group stats or None). ``names``: with read_groups, the cells' names."""
    filtered, chosen, stats = selection(files, chromosome_ids, require, exclude, duplicates, tag, barcodes)
    sources = sources_for(files, refs, filtered, chosen, duplicates)
    if names is None:
        parts, dropped = se.cluster_parts(sources, clustering, chromosome_ids, tag, barcodes)
        return parts, dropped, stats, None
    parts, dropped, rg_stats, _ = sr.cluster_parts(sources, clustering, chromosome_ids, names, tag, barcodes)
    return parts, dropped, stats, rg_stats


def expected_files(files, refs, clustering, chromosome_ids, tmp_path, require=0, exclude=0, duplicates="off",
                   names=None, tag=None, barcodes=None):
    """-> ([the bytes of cluster_<k>.bam for every k], dropped records, the select stats, the read-group stats)."""
    parts, dropped, stats, rg_stats = cluster_parts(files, refs, clustering, chromosome_ids, require, exclude,
                                                    duplicates, names, tag, barcodes)
    return [b"".join(se.members_of(p, tmp_path) for p in ps) + se.EOF for ps in parts], dropped, stats, rg_stats


def dict_stats(stats: Dict[str, int]) -> Dict[str, int]:
    """The select stats under the keys of the dict ``split_clusters`` returns."""
    return {("filter_records" if k == "records" else k): v for k, v in stats.items()}


def records_of(part: bytes) -> List[bytes]:
    out, o = [], 0
    while o < len(part):
        n = 4 + int.from_bytes(part[o:o + 4], "little")
        out.append(part[o:o + n])
        o += n
    assert o == len(part)
    return out


def file_records(raw_file: bytes) -> List[bytes]:
    """The records of an expected (or written) cluster file, read back."""
    import gzip
    import struct

    raw = gzip.decompress(raw_file)
    l_text = struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, 8 + l_text)[0]
    o = 12 + l_text
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    return records_of(raw[o:])


def mark_edges(off_parts, mark_parts):
    """Where the marked bytes fall in the streams the gather writes (per requested chromosome the clusters' parts one
    after the other, in tiles of TILE bytes from the stream's start), from the expected parts of the same call with
    duplicates "off" and "mark" alone: the two streams differ exactly in byte 19 of the records that gained a mark.
    -> dict(residues: the set of those offsets mod 16, tile_last / tile_first: how many lie on the last / first byte of
    a tile, extent_first / extent_last: how many extents of a cluster start / end with a record that gained a mark,
    marked: how many records gained a mark)."""
    res = dict(residues=set(), tile_last=0, tile_first=0, extent_first=0, extent_last=0, marked=0)
    n_chr = len(off_parts[0]) - 1
    for i in range(n_chr):
        at = 0
        for ps_off, ps_mark in zip(off_parts, mark_parts):
            a, b = ps_off[1 + i], ps_mark[1 + i]
            assert len(a) == len(b)
            recs, o = records_of(a), 0
            for j, rec in enumerate(recs):
                diff = [q for q in range(len(rec)) if a[o + q] != b[o + q]]
                if diff:
                    assert diff == [19] and b[o + 19] == a[o + 19] | 0x04, (i, j, diff)
                    p = at + o + 19
                    res["marked"] += 1
                    res["residues"].add(p % 16)
                    res["tile_last"] += p % TILE == TILE - 1
                    res["tile_first"] += p % TILE == 0
                    res["extent_first"] += j == 0
                    res["extent_last"] += j == len(recs) - 1
                o += len(rec)
            at += len(a)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the input sets of the GPU tests

F, R = 0x1 | 0x2 | 0x40 | 0x20, 0x1 | 0x2 | 0x80 | 0x10  # the two records of a proper pair
REFS3 = [("chr1", 100_000), ("chr2", 100_000), ("chr3", 100_000)]
SELECT_CLUSTERING = [1, 0, 1, 3, 0, 1]  # cluster 2 has no cell; cluster 3's only cell has every record filtered
SELECT_BARCODES = ["SEL%d-%s" % (c, "ACGT"[c % 4] * (2 + c % 3)) for c in range(6)]
SELECT_NAMES = ["s%d%s" % (c, "_x" * (c % 3)) for c in range(6)]
REQUIRE, EXCLUDE = 0x3, 0xF04          # the callers' filter: proper pairs, nothing unmapped, secondary, QC-failed,
EXCLUDE_KEEP_MARKS = 0xB04             # marked or supplementary; and the same that lets incoming marks through


def _seq(rng, n: int) -> str:
    return "".join(rng.choice(list("ACGT"), n))


def _rec(rng, name, ref, pos, flag, tags, cigar=None, qual=None, n=50) -> bw.Rec:
    cigar = cigar or [("M", n)]
    n = sum(k for op, k in cigar if op in "MIS=X")
    return bw.Rec(name=name, ref=ref, pos=pos, cigar=cigar, seq=_seq(rng, n), qual=list(qual or [30] * n), flag=flag,
                  tags=list(tags))


def _pair(rng, name, ref, pos, tags, qual=None, mate=200, flags=(F, R), cigars=(None, None)):
    return [_rec(rng, name, ref, pos, flags[0], tags, cigars[0], qual),
            _rec(rng, name, ref, pos + mate, flags[1], tags, cigars[1], qual)]


def select_cells(seed=11) -> List[List[bw.Rec]]:
    """Six cells on three references, every record with its cell's CB:Z barcode, about 40 random pairs of 2 x 50 bases
    per cell and, planted in every cell unless said otherwise (positions on chr1, 0-based):

      10000  two pairs with the same ends, the second with lower qualities
      11000  three pairs with the same ends, the first two with the same score (the first stays), the third lower
      12000  70 pairs with the same ends (longer than a wave), qualities 20 or 30 at random: ties among the best
      13000  three singles forward with the same end, one single reverse at the same position (no duplicate of them)
      14000  a pair whose forward read is clipped 5S45M at 14005 and whose reverse read 40M10S, and a plain pair with
             the same unclipped ends
      15000  a template of three records, and a pair with the same first two ends: neither is touched
      16000  a pair whose second record failed QC (the filter halves it: a single) and a single with the same end and a
             lower score, which is a duplicate only once the filter is on
      17000  cells 0 and 2 (both of cluster 1): the same pair, names included, and the same single. Duplicates of
             nothing: they are different cells. The case the feature exists for.
      18000  a pair that arrives marked 0x400 with high qualities and an unmarked pair with the same ends and lower
             ones: the marked pair is the keeper
      19000  a pair that arrives marked and is a duplicate of nothing: its mark stays
      20000..  one record each: secondary, supplementary, QC-failed, unmapped but placed (with and without 0x2)

    On chr2 cell 4 has only QC-failed records; cell 3 (alone in cluster 3) has 0x100 set on every record; on chr3
    every record of every cell lacks 0x2 or failed QC."""
    rng = np.random.default_rng(seed)
    low = [30] * 45 + [10] * 5
    cells = []
    for c in range(6):
        t = [("CB", "Z", SELECT_BARCODES[c])]
        recs: List[bw.Rec] = []
        for p in range(25):
            recs += _pair(rng, "c%d_a%d%s" % (c, p, "x" * (p % 5)), 0, 3000 + int(rng.integers(0, 6000)), t,
                          mate=100 + int(rng.integers(0, 200)))
        for p in range(15):
            recs += _pair(rng, "c%d_b%d%s" % (c, p, "y" * (p % 3)), 1, 3000 + int(rng.integers(0, 6000)), t,
                          mate=100 + int(rng.integers(0, 200)), flags=(F | 0x200, R | 0x200) if c == 4 else (F, R))
        recs += _pair(rng, "c%d_d2_a" % c, 0, 10000, t) + _pair(rng, "c%d_d2_b" % c, 0, 10000, t, low)
        recs += (_pair(rng, "c%d_d3_a" % c, 0, 11000, t) + _pair(rng, "c%d_d3_b" % c, 0, 11000, t) +
                 _pair(rng, "c%d_d3_c" % c, 0, 11000, t, low))
        for p in range(70):
            recs += _pair(rng, "c%d_w%02d" % (c, p), 0, 12000, t, [int(q) for q in rng.choice([20, 30], 50)])
        recs += [_rec(rng, "c%d_s%d" % (c, k), 0, 13000, 0x1 | 0x2 | 0x40, t, qual=[30 - k] * 50) for k in range(3)]
        recs.append(_rec(rng, "c%d_srev" % c, 0, 13000, 0x1 | 0x2 | 0x40 | 0x10, t))
        recs += _pair(rng, "c%d_clip" % c, 0, 14005, t, [25] * 50, mate=195,
                      cigars=([("S", 5), ("M", 45)], [("M", 40), ("S", 10)]))
        recs += _pair(rng, "c%d_noclip" % c, 0, 14000, t)
        recs += _pair(rng, "c%d_tri" % c, 0, 15000, t, mate=100) + [_rec(rng, "c%d_tri" % c, 0, 15200, F, t)]
        recs += _pair(rng, "c%d_trimate" % c, 0, 15000, t, mate=100)
        recs += _pair(rng, "c%d_half" % c, 0, 16000, t, flags=(F, R | 0x200))
        recs.append(_rec(rng, "c%d_half2" % c, 0, 16000, 0x1 | 0x2 | 0x40, t, qual=[20] * 50))
        if c in (0, 2):
            recs += _pair(rng, "shared_pair", 0, 17000, t) + [_rec(rng, "shared_single", 0, 17500, 0x1 | 0x2 | 0x40, t)]
        recs += _pair(rng, "c%d_md_a" % c, 0, 18000, t, flags=(F | DUP, R | DUP))
        recs += _pair(rng, "c%d_md_b" % c, 0, 18000, t, low)
        recs += _pair(rng, "c%d_md_c" % c, 0, 19000, t, flags=(F | DUP, R | DUP))
        for k, flag in enumerate((F | 0x100, F | 0x800, F | 0x200, 0x1 | 0x40 | 0x4, F | 0x4)):
            recs.append(_rec(rng, "c%d_flag%d" % (c, k), 0, 20000 + 10 * k, flag, t))
        for k in range(6):
            recs.append(_rec(rng, "c%d_z%d" % (c, k), 2, 500 + 40 * k, (0x1 | 0x40) if k % 2 else (F | 0x200), t))
        if c == 3:
            for r in recs:
                r.flag |= 0x100
        recs.sort(key=bw.sort_key)  # stable: records of one position keep their order
        cells.append(recs)
    return cells


def multiplexed(cells: Sequence[Sequence[bw.Rec]], seed=12) -> Tuple[List[bw.Rec], int]:
    """One multiplexed file of the cells' records, equal positions in (cell, record) order, and records tag mode drops:
    without CB, with CB of another type, with an unlisted CB:Z -> (records, how many of those are placed). Some of the
    dropped ones have the ends of planted duplicates, and flags the filter would drop: they reach neither rule."""
    rng = np.random.default_rng(seed)
    extra = []
    for k in range(8):
        tags = [[], [("CB", "i", 5)], [("CB", "Z", "NOT-LISTED")],
                [("CB", "A", "x"), ("CB", "Z", SELECT_BARCODES[0])]][k % 4]
        extra.append(_rec(rng, "extra_%d" % k, k % 2, [10000, 12000, 13000][k % 3], F | (0x200 if k % 5 == 0 else 0),
                          tags))
    recs = sorted([r for cell in cells for r in cell] + extra, key=bw.sort_key)
    return recs, len(extra)


RESIDUE_NAMES = ["res-a", "rb"]


def residue_cells(grow: Sequence[int] = (0, 0), seed=13) -> List[List[bw.Rec]]:
    """Two cells, one cluster each, all records unpaired forward reads on chr1 in groups of two with the same end: a
    keeper and, with lower qualities, its duplicate. Name lengths pad the records so that, in the stream of the "mark"
    call, byte 19 of a duplicate falls on each residue mod 16, on the last byte of a 4 KiB tile and on the first byte
    of the next one; the first record of each cluster's extent is a duplicate (its keeper follows at the same
    position), and so is the last. ``grow[c]``: the bytes every record of cell c gains on the way, 0 for the plain call,
    4 + len(name) with read_groups, so that the same holds in the edited stream."""
    rng = np.random.default_rng(seed)
    cells, at = [], 0  # at: the offset in the stream where the next record starts
    for c in range(2):
        recs: List[bw.Rec] = []
        state = dict(pos=1000, serial=0)

        def rec(name_len, low, pad=None):
            name = ("%d.%04d" % (c, state["serial"])).ljust(name_len, "n")
            state["serial"] += 1
            tags = [] if pad is None else [("XP", "Z", "p" * pad)]
            return bw.Rec(name=name, ref=0, pos=state["pos"], cigar=[("M", 8)], seq=_seq(rng, 8),
                          qual=[20 if low else 30] * 8, flag=0, tags=tags)

        def size(r):
            return len(bw.encode_record(r)) + grow[c]

        base = size(rec(6, False)) - 6  # a record's size without its name's characters
        state["serial"] = 0

        def group(target, modulus, dup_first=False):
            """A keeper and a duplicate; byte 19 of the duplicate at offset ``target`` mod ``modulus`` of the stream."""
            nonlocal at
            if dup_first:
                out = [rec(6, True), rec(6, False)]
            else:
                need = (target - 19 - at - base) % modulus  # the characters of the keeper's name
                if not 6 <= need <= 254:  # a filler of its own position in front: its XP:Z value takes the rest
                    state["pos"] += 10
                    empty = size(rec(6, False, 0))
                    state["serial"] -= 1
                    rest = (need - 6 - empty) % modulus
                    filler = rec(6, False, rest)
                    recs.append(filler)
                    at += size(filler)
                    state["pos"] += 10
                    need = 6
                out = [rec(need, False), rec(6, True)]
                assert (at + size(out[0]) + 19) % modulus == target % modulus
            for r in out:
                recs.append(r)
                at += size(r)
            state["pos"] += 10

        group(0, 16, dup_first=True)
        if c == 0:
            for residue in range(16):
                group(residue, 16)
            group(TILE - 1, TILE)
            group(0, TILE)
        group(5, 16)  # the extent's last record is a duplicate
        cells.append(recs)
    return cells


def long_cells() -> List[List[bw.Rec]]:
    """split_expected.long_read_cells with a copy of the 70 000-base read under another name and lower qualities in
    the same cell: the copy is a duplicate, its FLAG lies 140 KB and dozens of tiles in front of its end."""
    cells = se.long_read_cells()
    twin = copy.deepcopy(cells[0][0])
    twin.name = "long_twin"
    twin.qual = [max(0, q - 1) for q in twin.qual]
    cells[0].append(twin)
    return cells


TIE_BARCODES = ["TIE-A", "TIE-B"]


def tie_files(seed=14) -> List[List[bw.Rec]]:
    """Tag mode, barcode TIE-A with records in two files. File 0 holds template X at Position 500 with a 20-base leading
    clip, file 1 template Y at Position 480 with the same unclipped 5' end, strand and score. The pileup's global order
    (chunk, cell, Position, file, record) puts Y first, so X is the duplicate, although X comes first in input order.
    Around them a pair of TIE-B with the same ends in each file (another cell: the files' order decides, the first
    file's pair stays) and records that are duplicates of nothing."""
    rng = np.random.default_rng(seed)
    a, b = [("CB", "Z", TIE_BARCODES[0])], [("CB", "Z", TIE_BARCODES[1])]
    single = 0x1 | 0x2 | 0x40
    f0 = [_rec(rng, "before", 0, 100, single, a),
          _rec(rng, "X", 0, 500, single, a, cigar=[("S", 20), ("M", 30)]),
          *_pair(rng, "other0", 0, 700, b)]
    f1 = [_rec(rng, "Y", 0, 480, single, a),
          _rec(rng, "after", 0, 600, single, a),
          *_pair(rng, "other1", 0, 700, b)]
    for f in (f0, f1):
        f.sort(key=bw.sort_key)
    return [f0, f1]
