"""What ``secedo_amd.split_clusters(..., read_groups=True)`` must write, computed on the CPU from the contract of
secedo_bam_split_clusters_rg (include/secedo_bam.h): ``expected_files``. tests/split_expected.py gives the sources, the
order and the members M(x); this module adds the three rules of the read-group call, each written from the contract's
text:

  names          ``default_names``; ``name_fault`` says why a list of names is refused
  header         ``header_bytes``: split_expected's header with one "@RG ID:<name> SM:cluster_<k>" per cell of the
                 cluster in place of the inputs' @RG lines
  records        ``edit_record``: the strict walk of the aux area, the first RG field cut out when the walk succeeds,
                 'R' 'G' 'Z' name NUL appended, block_size patched

and the synthetic sets of tests/test_gpu_split_rg.py with ``stream_edges``, which says where record starts, holes and
suffixes fall in the stream the gather writes, so that the CPU tests can check without a GPU that the sets reach the
gather's edges.
"""
from __future__ import annotations

import copy
import os
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import bam_writer as bw
from tests import split_expected as se

TILE = 4096  # bytes of the stream one workgroup of the gather writes
STAT_KEYS = ("tagged_records", "replaced_records", "unparsed_records", "added_bytes", "removed_bytes")

# ---------------------------------------------------------------------------------------------------------------------
# rule 1: names


def default_names(paths: Sequence[str]) -> List[str]:
    out = []
    for p in paths:
        base = os.path.basename(str(p))
        for ext in (".sam.gz", ".bam", ".sam"):
            if base.endswith(ext):
                base = base[:-len(ext)]
                break
        out.append(base)
    return out


def name_fault(names: Sequence[str]) -> Optional[str]:
    """None for a list the call accepts, else what is wrong with it."""
    for c, n in enumerate(names):
        raw = n.encode() if isinstance(n, str) else n
        if not 1 <= len(raw) <= 254 or any(not 0x21 <= b <= 0x7E for b in raw):
            return "cell %d" % c
    for c, n in enumerate(names):
        if n in names[:c]:
            return "cells %d and %d" % (list(names).index(n), c)
    return None


# ---------------------------------------------------------------------------------------------------------------------
# rule 2: the header

def header_bytes(sources: Sequence[se.Source], names: Sequence[str], clustering: Sequence[int], k: int) -> bytes:
    refs = sources[0].refs
    assert all(s.refs == refs for s in sources)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    text += "".join("@RG\tID:%s\tSM:cluster_%d\n" % (names[c], k) for c, cl in enumerate(clustering) if cl == k)
    text += "@PG\tID:secedo_amd.split\tPN:secedo_amd\n@CO\tsecedo_amd cluster %d: %d of %d cells\n" % (
        k, sum(1 for cl in clustering if cl == k), len(clustering))
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        raw += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return raw


# ---------------------------------------------------------------------------------------------------------------------
# rule 3: the records

VALUE_BYTES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def aux_start(rec: bytes) -> int:
    l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    return 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq


def aux_fields(rec: bytes) -> Optional[List[Tuple[int, int, bytes]]]:
    """[(start, end, tag)] of the fields of the aux area when it is a sequence of whole fields that ends exactly at the
    record's end; None when it is not."""
    p, end, out = aux_start(rec), len(rec), []
    if p > end:
        return None
    while p != end:
        if end - p < 3:
            return None
        typ, value = chr(rec[p + 2]), p + 3
        if typ in VALUE_BYTES:
            stop = value + VALUE_BYTES[typ]
        elif typ in ("Z", "H"):
            nul = rec.find(b"\0", value)
            if nul < 0:
                return None
            stop = nul + 1
        elif typ == "B":
            if end - value < 5:
                return None
            sub = chr(rec[value])
            if sub == "A" or sub not in VALUE_BYTES:
                return None
            stop = value + 5 + struct.unpack_from("<I", rec, value + 1)[0] * VALUE_BYTES[sub]
        else:
            return None
        if stop > end:
            return None
        out.append((p, stop, rec[p:p + 2]))
        p = stop
    return out


def edit_record(rec: bytes, name: str):
    """-> (the edited record, (hole start, hole length) or None, the walk succeeded)."""
    fields = aux_fields(rec)
    hole = None
    if fields is not None:
        hole = next(((a, b - a) for a, b, tag in fields if tag == b"RG"), None)
    body = rec if hole is None else rec[:hole[0]] + rec[hole[0] + hole[1]:]
    body = body[4:] + b"RGZ" + name.encode() + b"\0"
    return struct.pack("<i", len(body)) + body, hole, fields is not None


def cluster_parts(sources: Sequence[se.Source], clustering: Sequence[int], chromosome_ids: Sequence[int],
                  names: Sequence[str], tag: Optional[str] = None, barcodes: Optional[Sequence[str]] = None):
    """-> (parts[k] = [header, edited records of the 1st requested chromosome, ...], dropped records, the stats of
    secedo_bam_split_rg_info, marks). marks[i] lists, for the i-th requested chromosome, (cluster, record start, hole
    start or None, suffix start, suffix length, cell) of every record, offsets in the cluster's part."""
    assert name_fault(list(names)) is None and len(names) == len(clustering)
    n_clusters = max(clustering) + 1
    index = None if tag is None else {b.encode(): c for c, b in enumerate(barcodes)}
    parts = [[header_bytes(sources, names, clustering, k)] for k in range(n_clusters)]
    stats = dict.fromkeys(STAT_KEYS, 0)
    dropped, marks = 0, []
    for chrom in sorted(chromosome_ids):
        per = [[] for _ in range(n_clusters)]  # (pos, file, ordinal, cell, bytes)
        for f, s in enumerate(sources):
            for i, rec in enumerate(s.records):
                ref, pos = se.ref_pos(rec)
                if ref != chrom:
                    continue
                cell = f if index is None else index.get(se.z_value(rec, tag))
                if cell is None:
                    dropped += 1
                    continue
                per[clustering[cell]].append((pos, f, i, cell, rec))
        here = []
        for k in range(n_clusters):
            out = bytearray()
            for _pos, _f, _i, cell, rec in sorted(per[k], key=lambda r: r[:3]):
                new, hole, parsed = edit_record(rec, names[cell])
                suffix = 4 + len(names[cell].encode())
                here.append((k, len(out), None if hole is None else len(out) + hole[0], len(out) + len(new) - suffix,
                             suffix, cell))
                stats["tagged_records"] += 1
                stats["replaced_records"] += hole is not None
                stats["unparsed_records"] += not parsed
                stats["added_bytes"] += suffix
                stats["removed_bytes"] += 0 if hole is None else hole[1]
                out += new
            parts[k].append(bytes(out))
        marks.append(here)
    return parts, dropped, stats, marks


def expected_files(sources, clustering, chromosome_ids, names, tmp_path, tag=None, barcodes=None):
    """-> ([the bytes of cluster_<k>.bam for every k], dropped records, the stats)."""
    parts, dropped, stats, _ = cluster_parts(sources, clustering, chromosome_ids, names, tag, barcodes)
    return [b"".join(se.members_of(p, tmp_path) for p in ps) + se.EOF for ps in parts], dropped, stats


def stream_edges(parts, marks):
    """Where the gather meets its edges. Per requested chromosome it writes one stream: the clusters' parts one after
    the other, in tiles of TILE bytes from the stream's start. -> dict of: the residues mod 16 of the record starts,
    of the hole starts (where the bytes behind a hole continue) and of the suffix starts in the stream; how many
    block_size words and suffixes lie in two tiles, and how many holes have the byte in front of them in one tile and the
    byte behind them in the next."""
    res = dict(record=set(), hole=set(), suffix=set(), word_straddles=0, hole_straddles=0, suffix_straddles=0)

    def straddles(a, n):  # bytes [a, a + n) lie in two tiles
        return n > 1 and a // TILE != (a + n - 1) // TILE

    for i, here in enumerate(marks):
        base, at = [], 0
        for ps in parts:
            base.append(at)
            at += len(ps[1 + i])
        for k, start, hole, suffix, suffix_len, _cell in here:
            res["record"].add((base[k] + start) % 16)
            res["suffix"].add((base[k] + suffix) % 16)
            res["word_straddles"] += straddles(base[k] + start, 4)
            res["suffix_straddles"] += straddles(base[k] + suffix, suffix_len)
            if hole is not None:
                res["hole"].add((base[k] + hole) % 16)
                # in the stream a hole is a seam: it straddles when the byte in front of it ends a tile
                res["hole_straddles"] += (base[k] + hole) % TILE == 0
    return res


# ---------------------------------------------------------------------------------------------------------------------
# input files from raw records (a malformed aux area has no bw.Rec)

def raw_of(item) -> bytes:
    return item if isinstance(item, bytes) else bw.encode_record(item)


def write_raw_bam(path, refs, items, text: Optional[str] = None) -> None:
    if text is None:
        text = se.default_text(refs)
    raw = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs)))
    for name, ln in refs:
        raw += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    for it in items:
        raw += raw_of(it)
    with open(path, "wb") as f:
        f.write(bw.bgzf(bytes(raw)))


def source_of_items(refs, items, text: Optional[str] = None) -> se.Source:
    return se.Source(se.default_text(refs) if text is None else text, refs, [raw_of(it) for it in items])


def with_raw_aux(rec: bw.Rec, aux: bytes) -> bytes:
    """The record with ``aux`` behind its own fields, whatever the bytes are."""
    body = bw.encode_record(rec)[4:] + aux
    return struct.pack("<i", len(body)) + body


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic sets of the GPU tests

SAM_CELLS = (0, 2, 7)  # the cells tests write as SAM text: only fields SAM text holds byte for byte
NAMES = ["c%02d%s" % (c, "-sub" * (c % 4)) for c in range(12)]  # 3, 7, 11 and 15 bytes
N_PLAIN, N_VARIANTS = 6, 14


def _variant_tags(v: int, c: int, name: str):
    """The aux fields of variant v of a record of cell c (AS and CB are what split_expected.cell_records gives)."""
    a, cb = ("AS", "C", 40 + c), ("CB", "Z", se.BARCODES[c])
    shorter, equal, longer = name[:-2], "x" * len(name), name + "yy"
    return [
        [],                                                     # 0: no aux area
        [("RG", "Z", shorter), a, cb],                          # 1: RG first, a shorter old value: the record grows
        [a, ("RG", "Z", equal), cb],                            # 2: RG in the middle, the length stays
        [a, cb, ("RG", "Z", longer)],                           # 3: RG last, a longer old value: the record shrinks
        [a, cb],                                                # 4: no RG
        [("XZ", "Z", "abRGZx"), a, cb],                         # 5: RGZx inside a Z value
        [a, ("RG", "Z", ""), cb],                               # 6: an empty old value
        [("RG", "Z", equal)],                                   # 7: RG alone
        [a, ("RG", "i", 7), cb],                                # 8: RG typed i
        [("XH", "H", "1AE3"), ("XB", "B", ("S", [1, 515, 65535])), ("RG", "Z", longer), cb],  # 9: H and B:S in front
        [("XC", "B", ("C", [82, 71, 90, 1, 82, 71, 90, 0])), a, ("RG", "Z", shorter)],  # 10: R G Z inside a B:C array
        [("XF", "f", 1.5), ("XS", "s", -300), ("XI", "I", 70000), ("RG", "A", "r"), ("XA", "A", "q")],  # 11
    ][v]


def cell_items(n_cells=12, pairs=60, seed=3):
    """split_expected.cell_records with the aux areas the read-group edit must tell apart: record i of cell c is variant
    (i + c) mod 6 of ``_variant_tags`` in the cells written as SAM, mod 14 elsewhere, where 12 is a record with an
    unknown type byte and 13 one whose last field runs past the record's end (both with an RG field in front, which
    must stay). -> per cell a list of bw.Rec, or bytes for those two."""
    cells = se.cell_records(n_cells, pairs, seed)
    out = []
    for c, recs in enumerate(cells):
        items = []
        for i, r in enumerate(recs):
            r = copy.deepcopy(r)
            v = (i + c) % (N_PLAIN if c in SAM_CELLS else N_VARIANTS)
            if r.ref < 0:
                items.append(r)
            elif v < 12:
                r.tags = _variant_tags(v, c, NAMES[c % len(NAMES)])
                items.append(r)
            else:
                r.tags = [("AS", "C", 40 + c), ("RG", "Z", "kept")]
                items.append(with_raw_aux(r, b"XQ?abc" if v == 12 else b"XZZno-nul"))
        out.append(items)
    return out


def edge_items(names: Sequence[str], seed=5):
    """Three cells, one cluster each: edited record bytes of exactly 0xFF00, of 0xFF00 + 1, and a single record."""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 4096))
    n_reads = 200
    cells = []
    for c, extra in enumerate((0, 1)):
        grow = (n_reads + 1) * (4 + len(names[c]))
        cells.append(se.padded_cell(rng, genome, "full" if c == 0 else "over", se.CUT + extra - grow, n_reads))
    cells.append([bw.Rec(name="only", ref=0, pos=77, cigar=[("M", 5)], seq="ACGTA", qual=[20] * 5)])
    return cells


def tile_items(name: str):
    """One cell whose records are padded so that, in the edited stream, the hole of the first lies exactly at byte 4096,
    the block_size word of the second at 8190..8193, and the suffix of the second starts at 12285, across byte 12288."""
    def rec(k, tags):
        return bw.Rec(name="tile_%d" % k, ref=0, pos=100 + k, cigar=[("M", 8)], seq="ACGTACGT", qual=[30] * 8, tags=tags)

    def first(n, q):
        return rec(0, [("XP", "Z", "p" * n), ("RG", "Z", "old"), ("XQ", "Z", "q" * q)])

    def second(n):
        return rec(1, [("XP", "Z", "p" * n)])

    def edited(r):
        return edit_record(bw.encode_record(r), name)

    n = TILE - edited(first(0, 0))[1][0]
    q = 2 * TILE - 2 - len(edited(first(n, 0))[0])
    grow = 4 + len(name)
    m = 3 * TILE - 3 - (2 * TILE - 2 + len(edited(second(0))[0]) - grow)
    assert min(n, q, m) >= 1
    return [[first(n, q), second(m), rec(2, [])]]


def long_items():
    """split_expected.long_read_cells with an RG field behind the long read's ML:B:C array: the hole lies more than
    100 KB into the record, dozens of tiles from its start."""
    cells = se.long_read_cells()
    cells[0][0].tags = cells[0][0].tags + [("RG", "Z", "old-group"), ("NM", "C", 3)]
    return cells


def rg_keyed_cells():
    """split_expected.cell_records with the barcode in RG:Z instead of CB:Z: a set keyed by RG itself."""
    cells = se.cell_records()
    for recs in cells:
        for r in recs:
            r.tags = [("RG" if t == "CB" else t, typ, v) for t, typ, v in r.tags]
    return cells
