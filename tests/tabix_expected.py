"""What ``secedo_amd.tabix_build`` (and the bgzf writer under ``vcf_index="tbi"``) must write for a .vcf.gz, restated
from the file's bytes and the rules of include/secedo_variant.h: ``expected_bytes`` is the uncompressed .tbi.

A data line is one whose first byte is not '#' and that is not empty; name = column 1, beg = POS - 1 (0 for POS 0),
end = beg + len(REF), or the value of INFO's first END= key where that is a decimal number above beg; end > beg.
Bins ascending, one chunk per run of consecutive data lines in one bin, the pseudo-bin 37450 last, the linear index
filled backward, names in first-appearance order. A chunk begins at its first line and ends where the next run's first
line begins, the last at the end of the data; virtual offsets name the member that holds the byte, the end of the data
the EOF member.

``builder_input`` writes, for secedo_amd/csrc/build/tabix_build_test, what the device's line pass hands the host
builder for a file walked in ranges that start at the given data-line ordinals. ``overlapping`` is the brute-force
answer to a region query."""
from __future__ import annotations

import re
import struct
import zlib

PSEUDO_BIN = 37450
MAX_END = 1 << 29
DECIMAL = re.compile(rb"[0-9]+\Z")

E_COLUMNS = "fewer than two columns"
E_POS = "POS is not a decimal number"
E_END = "the line ends past 2^29: a .tbi index cannot hold it"
E_ORDER = "POS is lower than that of the data line before it: the file is not sorted"
E_BLOCKS = "chromosome blocks not continuous"


class TabixError(Exception):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what))
        self.line, self.what = line, what


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def member_table(data: bytes):
    """[(coffset, first text byte, isize)] of a BGZF file, following BSIZE"""
    out, o, lin = [], 0, 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04", o
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        x, bsize = o + 12, None
        while x < o + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        isize = struct.unpack_from("<I", data, o + bsize + 1 - 4)[0]
        out.append((o, lin, isize))
        lin += isize
        o += bsize + 1
    return out


def inflate(data: bytes) -> bytes:
    out, o = [], 0
    while o < len(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data[o:]))
        o = len(data) - len(d.unused_data)
    return b"".join(out)


def voffset(table, total, file_bytes, lin):
    for coff, out, isize in table:
        if out + isize > lin:
            return coff << 16 | (lin - out)
    # the end of the data: the first empty member behind it, else the file's size
    tail = None
    for coff, out, isize in reversed(table):
        if isize == 0 and out == total:
            tail = coff
        else:
            break
    return (tail if tail is not None else file_bytes) << 16


def parse(line: bytes):
    """a data line without its '\\n' -> (name, POS, beg, end), or the error's words"""
    cols = line.split(b"\t")
    if len(cols) < 2:
        return E_COLUMNS
    if not DECIMAL.match(cols[1]):
        return E_POS
    pos = int(cols[1])
    beg = pos - 1 if pos else 0
    end = beg + (len(cols[3]) if len(cols) > 3 else 0)
    if len(cols) > 7:
        for item in cols[7].split(b";"):
            if item.startswith(b"END="):  # the first END= key decides
                if DECIMAL.match(item[4:]) and int(item[4:]) > beg:
                    end = int(item[4:])
                break
    end = max(end, beg + 1)
    if end > MAX_END:
        return E_END
    return cols[0], pos, beg, end


def data_lines(text: bytes):
    """[(name, beg, end, text offset, line)] of the data lines; TabixError for the first line that breaks a rule"""
    out, seen, o, n = [], [], 0, 0
    prev = None
    while o < len(text):
        e = text.find(b"\n", o)
        e = len(text) if e < 0 else e
        line = text[o:e]
        n += 1
        if line and not line.startswith(b"#"):
            p = parse(line)
            if isinstance(p, str):
                raise TabixError(n, p)
            name, pos, beg, end = p
            if prev and prev[0] == name and pos < prev[1]:
                raise TabixError(n, E_ORDER)
            if not prev or prev[0] != name:
                if name in seen:
                    raise TabixError(n, E_BLOCKS)
                seen.append(name)
            prev = (name, pos)
            out.append((name, beg, end, o, n))
        o = e + 1
    return out


def count_lines(text: bytes) -> int:
    return text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)


def expected_raw(text: bytes, table, file_bytes: int) -> bytes:
    recs = data_lines(text)
    names = []
    for r in recs:
        if r[0] not in names:
            names.append(r[0])
    at = lambda lin: voffset(table, len(text), file_bytes, lin)  # noqa: E731
    l_nm = sum(len(n) + 1 for n in names)
    out = bytearray(b"TBI\1" + struct.pack("<8i", len(names), 2, 1, 2, 0, ord("#"), 0, l_nm))
    for n in names:
        out += n + b"\0"
    for name in names:
        idx = [i for i, r in enumerate(recs) if r[0] == name]
        chunks, linear = [], {}
        for i in idx:
            _n, beg, end, off, _line = recs[i]
            nxt = at(recs[i + 1][3]) if i + 1 < len(recs) else at(len(text))
            b = reg2bin(beg, end)
            if chunks and chunks[-1][0] == b:
                chunks[-1][2] = nxt  # the run of one bin goes on: one chunk
            else:
                chunks.append([b, at(off), nxt])
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                linear.setdefault(w, at(off))
        bins = sorted({c[0] for c in chunks})
        out += struct.pack("<i", len(bins) + 1)
        for b in bins:
            of_bin = [c for c in chunks if c[0] == b]
            out += struct.pack("<Ii", b, len(of_bin))
            for _b, beg_v, end_v in of_bin:
                out += struct.pack("<QQ", beg_v, end_v)
        out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, chunks[0][1], chunks[-1][2], len(idx), 0)
        n_intv = max(linear) + 1
        values, above = [0] * n_intv, 0
        for w in reversed(range(n_intv)):
            above = linear.get(w, above)
            values[w] = above
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in values)
    out += struct.pack("<Q", 0)
    return bytes(out)


def expected_bytes(gz: bytes) -> bytes:
    """the uncompressed .tbi of the .vcf.gz bytes"""
    return expected_raw(inflate(gz), member_table(gz), len(gz))


def builder_input(gz: bytes, cuts=()) -> str:
    text, table = inflate(gz), member_table(gz)
    recs = data_lines(text)
    lines = ["M %d %d %d" % m for m in table]
    lines.append("T %d %d" % (len(text), len(gz)))
    cuts = set(cuts) | {0}
    names, prev_key, reach = [], None, -1
    for i, (name, beg, end, off, _line) in enumerate(recs):
        if i in cuts:
            prev_key, reach = None, -1
        if name not in names:
            names.append(name)
            lines.append("N %s" % name.decode())
        key = (names.index(name), reg2bin(beg, end))
        if prev_key is None or prev_key[0] != key[0]:
            reach = -1  # the windows of another name, or of another range
        if key != prev_key:
            lines.append("H %d %d %d %d" % (key + (off, i)))
        prev_key = key
        last = (end - 1) >> 14
        for w in range(max(beg >> 14, reach + 1), last + 1):
            lines.append("W %d %d %d" % (key[0], w, off))
        reach = max(reach, last)
    lines.append("E %d %d" % (len(text), len(recs)))
    return "\n".join(lines) + "\n"


def run_crossings(gz: bytes, cuts) -> int:
    """range boundaries (in front of data line c) across which a run of one (name, bin) goes on"""
    recs = data_lines(inflate(gz))
    key = lambda r: (r[0], reg2bin(r[1], r[2]))  # noqa: E731
    return sum(1 for c in set(cuts) if 0 < c < len(recs) and key(recs[c]) == key(recs[c - 1]))


def overlapping(text: bytes, name: bytes, beg: int, end: int, recs=None):
    """the data lines of `name` that overlap [beg, end), by looking at every line (recs: data_lines(text), if the
    caller has them)"""
    out = []
    for n, b, e, off, _line in data_lines(text) if recs is None else recs:
        if n == name and b < end and e > beg:
            stop = text.find(b"\n", off)
            out.append(text[off:len(text) if stop < 0 else stop])
    return out
