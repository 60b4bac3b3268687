"""A BAI writer and reader for the test BAMs (SAM spec 5.2), built on ``bam_writer.read_bam`` and ``reg2bin``.

``write_bai`` reads the member layout of a BAM (``member_table``) and the start of every record in its inflated bytes,
turns them into virtual offsets the way htslib does (an offset on a member boundary names the member that follows,
uoffset 0) and writes bins, chunks, the 16 kb linear index and, unless ``pseudo_bin`` is False, the pseudo-bin 37450 that
samtools adds. ``ranges`` derives, from the BAM alone, what secedo_amd/csrc/bam_index.hpp must find in such an index;
``parse_ranges`` reads them back from index bytes."""
from __future__ import annotations

import struct
import zlib

from tests import bam_writer as bw

PSEUDO_BIN = 37450


def member_table(data: bytes):
    """-> [(coffset, bytes in the file, ISIZE, offset of its first inflated byte)] by following BSIZE"""
    out, off, lin = [], 0, 0
    while off < len(data):
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        bsize, x = None, off + 12
        while x < off + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        isize = struct.unpack_from("<I", data, off + bsize + 1 - 4)[0]
        out.append((off, bsize + 1, isize, lin))
        off += bsize + 1
        lin += isize
    return out


def inflate(data: bytes) -> bytes:
    return b"".join(zlib.decompress(data[o + 18:o + n - 8], -15) for o, n, _i, _l in member_table(data))


def record_spans(raw: bytes):
    """-> [(start, end)] of every record of inflated BAM bytes"""
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    out = []
    while o < len(raw):
        e = o + 4 + struct.unpack_from("<i", raw, o)[0]
        out.append((o, e))
        o = e
    return out


def voffset(table, lin: int) -> int:
    """htslib's virtual offset of inflated byte ``lin``: the first member that holds a byte at or past it"""
    for coff, _n, isize, start in table:
        if start + isize > lin:
            return coff << 16 | (lin - start)
    for coff, _n, isize, start in table:  # the end of the data: the member behind it (the EOF member)
        if start == lin and isize == 0:
            return coff << 16
    coff, n = table[-1][0], table[-1][1]
    return (coff + n) << 16


def layout(path):
    """-> (member table, [(ref, pos, end, voffset of its start, voffset behind it, flag)] per record, n_ref)"""
    data = open(path, "rb").read()
    table = member_table(data)
    refs, recs = bw.read_bam(path)
    spans = record_spans(inflate(data))
    assert len(spans) == len(recs)
    out = []
    for r, (s, e) in zip(recs, spans):
        length = sum(n for op, n in r["cigar"] if op in "MDN=X")
        out.append((r["ref"], r["pos"], r["pos"] + max(length, 1), voffset(table, s), voffset(table, e), r["flag"]))
    return table, out, len(refs)


def ranges(path):
    """From the BAM alone -> [(start, end, count)] per reference: the virtual offset of its first record, the one
    behind its last record and its record count; (0, 0, 0) for a reference without records."""
    _table, recs, n_ref = layout(path)
    out = []
    for ref in range(n_ref):
        mine = [r for r in recs if r[0] == ref]
        out.append((mine[0][3], mine[-1][4], len(mine)) if mine else (0, 0, 0))
    return out


def bai_bytes(path, pseudo_bin=True) -> bytes:
    _table, recs, n_ref = layout(path)
    out = bytearray(b"BAI\1" + struct.pack("<i", n_ref))
    for ref in range(n_ref):
        mine = [r for r in recs if r[0] == ref]
        bins, order = {}, []
        linear = []
        for _ref, pos, end, beg_v, end_v, _flag in mine:
            b = bw.reg2bin(max(pos, 0), max(end, 1))
            if order and order[-1] == b and bins[b][-1][1] == beg_v:
                bins[b][-1][1] = end_v  # the run of one bin goes on: one chunk
            else:
                bins.setdefault(b, []).append([beg_v, end_v])
                order.append(b)
            for w in range(max(pos, 0) >> 14, ((max(end, 1) - 1) >> 14) + 1):
                while len(linear) <= w:
                    linear.append(0)
                if linear[w] == 0:
                    linear[w] = beg_v
        n_bin = len(bins) + (1 if pseudo_bin and mine else 0)
        out += struct.pack("<i", n_bin)
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b]))
            for beg_v, end_v in bins[b]:
                out += struct.pack("<QQ", beg_v, end_v)
        if pseudo_bin and mine:
            unmapped = sum(1 for r in mine if r[5] & 4)
            out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, mine[0][3], mine[-1][4], len(mine) - unmapped, unmapped)
        for w in range(1, len(linear)):  # htslib fills the windows no record starts in
            if linear[w] == 0:
                linear[w] = linear[w - 1]
        out += struct.pack("<i", len(linear)) + b"".join(struct.pack("<Q", v) for v in linear)
    out += struct.pack("<Q", sum(1 for r in recs if r[0] < 0))
    return bytes(out)


def write_bai(path, out_path=None, pseudo_bin=True) -> str:
    out_path = out_path or str(path) + ".bai"
    with open(out_path, "wb") as f:
        f.write(bai_bytes(str(path), pseudo_bin))
    return out_path


def parse_ranges(data: bytes):
    """Index bytes -> [(start, end, count or -1)] per reference, the rule of bam_index.hpp restated"""
    assert data[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    o, out = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, o)[0]
        o += 4
        begs, ends, count = [], [], -1
        for _b in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", data, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
            if b == PSEUDO_BIN:
                count = chunks[1][0] + chunks[1][1]
            else:
                begs += [c[0] for c in chunks]
                ends += [c[1] for c in chunks]
        n_intv = struct.unpack_from("<i", data, o)[0]
        o += 4 + 8 * n_intv
        out.append((min(begs), max(ends), count) if begs else (0, 0, count))
    return out
