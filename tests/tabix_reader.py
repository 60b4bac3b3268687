"""The tabix specification's region query, as a reader of a .vcf.gz and its uncompressed .tbi would run it: the bins
of the region (reg2bins), their chunks, the linear index's lower bound, then a seek per chunk with zlib, member by
member, and the lines that overlap. It reads only what the index points at, so a wrong chunk, a wrong virtual offset or
a window value that lies too high loses lines, and tests/test_gpu_tabix.py holds it against the brute-force answer."""
from __future__ import annotations

import struct
import zlib

from tests import tabix_expected as te


def parse_index(raw: bytes):
    """-> {name: (bins {bin: [(beg, end)]}, linear [offsets])} of an uncompressed .tbi, the pseudo-bin left out"""
    assert raw[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    assert (fmt, col_seq, col_beg, col_end, meta, skip) == (2, 1, 2, 0, ord("#"), 0)
    o = 36
    names = raw[o:o + l_nm].split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref and sum(len(n) + 1 for n in names) == l_nm
    o += l_nm
    out = {}
    for name in names:
        n_bin, = struct.unpack_from("<i", raw, o)
        o += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", raw, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
            if b != te.PSEUDO_BIN:
                bins[b] = chunks
        n_intv, = struct.unpack_from("<i", raw, o)
        o += 4
        linear = list(struct.unpack_from("<%dQ" % n_intv, raw, o))
        o += 8 * n_intv
        out[name] = (bins, linear)
    assert o + 8 == len(raw) and struct.unpack_from("<Q", raw, o)[0] == 0
    return out


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


class Bgzf:
    """member-wise access to a BGZF file's bytes"""

    def __init__(self, data: bytes):
        self.data, self.cache = data, {}

    def member(self, coff):
        """-> (text of the member at coff, its size in the file)"""
        if coff not in self.cache:
            size = struct.unpack_from("<H", self.data, coff + 16)[0] + 1
            self.cache[coff] = (zlib.decompress(self.data[coff:coff + size], 31), size)
        return self.cache[coff]

    def lines(self, beg_v, end_v):
        """the lines that start at virtual offsets in [beg_v, end_v), without their '\\n'"""
        coff, u = beg_v >> 16, beg_v & 0xFFFF
        while coff < len(self.data):
            text, size = self.member(coff)
            if u >= len(text):  # the byte lies in the next member that has one
                coff, u = coff + size, 0
                continue
            if (coff << 16 | u) >= end_v:
                return
            line = bytearray()
            while coff < len(self.data):  # to the '\n' or the end of the data, across members
                text, size = self.member(coff)
                stop = text.find(b"\n", u)
                if stop >= 0:
                    line += text[u:stop]
                    u = stop + 1
                    break
                line += text[u:]
                coff, u = coff + size, 0
            yield bytes(line)


class Reader:
    """a .vcf.gz and its uncompressed .tbi, opened once for many queries"""

    def __init__(self, gz: bytes, raw_index: bytes):
        self.index, self.file = parse_index(raw_index), Bgzf(gz)

    def query(self, name: bytes, beg: int, end: int):
        """the data lines of `name` overlapping [beg, end) (0-based, half-open), in file order"""
        if name not in self.index or beg >= end:
            return []
        bins, linear = self.index[name]
        w = beg >> 14
        min_off = linear[w] if w < len(linear) else 0  # past the last window nothing bounds the chunks from below
        chunks = sorted(c for b in reg2bins(beg, min(end, te.MAX_END)) for c in bins.get(b, []) if c[1] > min_off)
        out = []
        for c_beg, c_end in chunks:  # disjoint, in file order
            for line in self.file.lines(max(c_beg, min_off), c_end):
                if not line or line.startswith(b"#"):
                    continue
                n, _pos, b, e = te.parse(line)
                if n != name or b >= end:
                    break  # sorted within a name: nothing further in this chunk overlaps
                if e > beg:
                    out.append(line)
        return out


def query(gz: bytes, raw_index: bytes, name: bytes, beg: int, end: int):
    return Reader(gz, raw_index).query(name, beg, end)
