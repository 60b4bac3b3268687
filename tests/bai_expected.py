"""What ``secedo_amd.bam_index_build`` must write for a BAM, from ``bai_writer.layout`` and the content rules of
include/secedo_bam.h: ``expected_bytes``. It is bai_writer.bai_bytes with the linear index filled backward as htslib
fills it (an untouched window takes the value of the next touched one above it); with that one change it reproduces
the six samtools-written indexes of tests/golden/bam byte for byte (tests/test_bam_index_build_cpu.py).

``builder_input`` writes, for secedo_amd/csrc/build/bam_index_build_test, what the device's index pass hands the host
builder for a file walked in ranges that start at the given record ordinals: the member table, the run heads (one at
every range start too) and the windows each record is the first of its range to overlap, with file-linear offsets.

``layout_bam`` is the synthetic file of the layout cases, ``LAYOUT_WRITERS`` the three ways it is cut into members."""
from __future__ import annotations

import struct

from tests import bai_writer as bi
from tests import bam_index_cases as ic
from tests import bam_writer as bw
from tests import bgzf_writer as gw


def expected_bytes(path) -> bytes:
    _table, recs, n_ref = bi.layout(str(path))
    out = bytearray(b"BAI\1" + struct.pack("<i", n_ref))
    for ref in range(n_ref):
        mine = [r for r in recs if r[0] == ref]
        chunks, linear = [], {}
        for _ref, pos, end, beg_v, end_v, _flag in mine:
            beg, end = max(pos, 0), max(end, 1)
            b = bw.reg2bin(beg, end)
            if chunks and chunks[-1][0] == b:
                chunks[-1][2] = end_v  # the run of one bin goes on: one chunk
            else:
                chunks.append([b, beg_v, end_v])
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                linear.setdefault(w, beg_v)
        bins = sorted({c[0] for c in chunks})
        out += struct.pack("<i", len(bins) + (1 if mine else 0))
        for b in bins:
            of_bin = [c for c in chunks if c[0] == b]
            out += struct.pack("<Ii", b, len(of_bin))
            for _b, beg_v, end_v in of_bin:
                out += struct.pack("<QQ", beg_v, end_v)
        if mine:
            unmapped = sum(1 for r in mine if r[5] & 4)
            out += struct.pack("<IiQQQQ", bi.PSEUDO_BIN, 2, mine[0][3], mine[-1][4], len(mine) - unmapped, unmapped)
        n_intv = max(linear) + 1 if linear else 0
        values, above = [0] * n_intv, 0
        for w in reversed(range(n_intv)):
            above = linear.get(w, above)
            values[w] = above
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in values)
    out += struct.pack("<Q", sum(1 for r in recs if r[0] < 0))
    return bytes(out)


def run_crossings(path, cuts) -> int:
    """Range boundaries (in front of record ordinal c, c in cuts) across which a run of one (RefID, bin, flag 0x4)
    goes on: what the builder counts as joined"""
    _table, recs, _n = bi.layout(str(path))
    key = lambda r: (r[0], bw.reg2bin(max(r[1], 0), max(r[2], 1)), r[5] & 4) if r[0] >= 0 else (-1, 0, 0)  # noqa: E731
    return sum(1 for c in cuts if 0 < c < len(recs) and key(recs[c]) == key(recs[c - 1]))


def builder_input(path, cuts=()) -> str:
    data = open(str(path), "rb").read()
    table = bi.member_table(data)
    raw = bi.inflate(data)
    spans = bi.record_spans(raw)
    _refs, recs = bw.read_bam(str(path))
    n_ref = len(_refs)
    lines = ["R %d" % n_ref]
    lines += ["M %d %d %d" % (coff, lin, isize) for coff, _n, isize, lin in table]
    lines.append("T %d %d" % (len(raw), len(data)))
    cuts = set(cuts) | {0}
    prev_key, prev_ref, reach = None, None, -1
    for i, (r, (s, _e)) in enumerate(zip(recs, spans)):
        if i in cuts:
            prev_key, prev_ref, reach = None, None, -1
        ref = r["ref"]
        if ref < 0:
            key = (-1, 0, 0)
        else:
            length = sum(n for op, n in r["cigar"] if op in "MDN=X")
            beg, end = max(r["pos"], 0), max(r["pos"] + max(length, 1), 1)
            key = (ref, bw.reg2bin(beg, end), 1 if r["flag"] & 4 else 0)
        if key != prev_key:
            lines.append("H %d %d %d %d %d" % (key + (s, i)))
        prev_key = key
        if ref < 0:
            continue
        if ref != prev_ref:
            prev_ref, reach = ref, -1
        last = (end - 1) >> 14
        for w in range(max(beg >> 14, reach + 1), last + 1):
            lines.append("W %d %d %d" % (ref, w, s))
        reach = max(reach, last)
    lines.append("E %d %d" % (len(raw), len(recs)))
    return "\n".join(lines) + "\n"


# ---- the layout cases

LAYOUT_REFS = [("1", 400000), ("2", 400000), ("3", 400000), ("4", 400000)]  # the last has no records


def _rec(name, ref, pos, cigar, flag=0x1 | 0x2 | 0x40):
    n = sum(k for op, k in cigar if op in "MIS=X")
    return bw.Rec(name, ref, pos, cigar, "ACGT" * (n // 4) + "ACGT"[:n % 4], qual=[35] * n, flag=flag)


def layout_records():
    """bam_index_cases.reads' 300 short reads per reference and unmapped tail, plus on reference 1: reads of 60 over
    positions 16384, 32768 and 131072 (window and bin-level boundaries), a cluster three windows and more past the
    last (backward fill), 1000M500N1000M reads that span windows, a CIGAR with every op, a mapped record without a
    CIGAR and a flag-0x4 record with a position."""
    recs = ic.reads()
    extra = []
    for k, at in enumerate((16384, 32768, 131072)):
        extra += [_rec("x%d_%d" % (k, j), 1, at - 30 + 7 * j, [("M", 60)]) for j in range(-3, 4)]
    extra += [_rec("far%d" % j, 1, 131072 + 5 * 16384 + 11 * j, [("M", 50)]) for j in range(12)]
    extra += [_rec("n%d" % j, 1, 48000 + 16384 * j, [("M", 1000), ("N", 500), ("M", 1000)]) for j in range(4)]
    extra.append(_rec("every", 1, 70000, [("H", 3), ("S", 4), ("M", 10), ("I", 2), ("D", 3), ("N", 20000), ("=", 5),
                                         ("X", 2), ("P", 1), ("M", 6), ("S", 2), ("H", 1)]))
    extra.append(bw.Rec("nocigar", 1, 70500, [], "ACGT", qual=[30] * 4))
    extra.append(bw.Rec("placed", 1, 70600, [], "ACGT", qual=[30] * 4, flag=0x1 | 0x4 | 0x40))
    return sorted(recs + extra, key=bw.sort_key)


def _long_header_refs():
    return LAYOUT_REFS + [("contig_%05d_with_a_long_name" % k, 100000 + k) for k in range(3000)]


LAYOUT_WRITERS = {
    "member-per-records": lambda: ic.htslib_members(ic.raw_bam(layout_records(), LAYOUT_REFS), limit=700),
    "cut-997": lambda: gw.bgzf(ic.raw_bam(layout_records(), LAYOUT_REFS), chunk=997),
    "long-header": lambda: bw.bam_bytes(_long_header_refs(), layout_records()),
}


def layout_bam(directory, how) -> str:
    path = str(directory / ("layout_%s.bam" % how))
    with open(path, "wb") as f:
        f.write(LAYOUT_WRITERS[how]())
    return path
