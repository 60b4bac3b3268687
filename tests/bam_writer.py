"""A small BAM writer and reader for the tests (BGZF through Python's zlib), and synthetic input sets.

``write_bam`` writes a coordinate-sorted BAM (SAM spec 4.2): BGZF blocks of at most 0xff00 input bytes with the
BC extra field, then the empty EOF block. ``read_bam`` decodes one back into plain dicts (the fields the
pileup restatement in tests/pileup_bam_ref.py reads). ``synthetic_set`` builds seeded cell files with every
CIGAR op, low qualities, N bases, AS tags of each integer type and reads that cross a chunk boundary.
"""
from __future__ import annotations

import gzip
import os
import struct
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"


@dataclass
class Rec:
    name: str
    ref: int
    pos: int  # 0-based
    cigar: List[Tuple[str, int]]
    seq: str  # "*" for none
    qual: Optional[Sequence[int]] = None  # raw phred values; None = missing (0xFF)
    flag: int = 0x1 | 0x2 | 0x40
    mapq: int = 60
    tags: List[Tuple[str, str, object]] = field(default_factory=list)  # (tag, type, value)
    next_ref: int = -1
    next_pos: int = -1
    tlen: int = 0
    aux: Optional[bytes] = None  # the aux block verbatim, in place of ``tags`` (layouts ``_tag`` cannot write)


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def _tag(tag: str, typ: str, value) -> bytes:
    out = tag.encode() + typ.encode()
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
    if typ == "A":
        return out + value.encode()
    if typ in ("Z", "H"):
        return out + value.encode() + b"\0"
    if typ == "B":
        sub, vals = value
        return out + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(fmt[sub], v) for v in vals)
    return out + struct.pack(fmt[typ], value)


def ref_length(cigar) -> int:
    return sum(n for op, n in cigar if op in "MDN=X")


def encode_record(r: Rec) -> bytes:
    name = r.name.encode() + b"\0"
    l_seq = 0 if r.seq == "*" else len(r.seq)
    end = r.pos + max(ref_length(r.cigar), 1)
    core = struct.pack("<iiBBHHHIiii", r.ref, r.pos, len(name), r.mapq, reg2bin(max(r.pos, 0), max(end, 1)),
                       len(r.cigar), r.flag, l_seq, r.next_ref, r.next_pos, r.tlen)
    cig = b"".join(struct.pack("<I", n << 4 | CIGAR_OPS.index(op)) for op, n in r.cigar)
    codes = [SEQ_CODES.index(c) if c in SEQ_CODES else 15 for c in (r.seq if l_seq else "")]
    if len(codes) % 2:
        codes.append(0)
    seq = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    qual = bytes([0xFF] * l_seq) if r.qual is None else bytes(r.qual)
    assert len(qual) == l_seq
    body = core + name + cig + seq + qual + (b"".join(_tag(*t) for t in r.tags) if r.aux is None else r.aux)
    return struct.pack("<i", len(body)) + body


def bgzf(data: bytes) -> bytes:
    out = bytearray()
    for i in range(0, len(data), 0xFF00):
        chunk = data[i:i + 0xFF00]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        cdata = c.compress(chunk) + c.flush()
        out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(cdata) + 25)
        out += cdata + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    empty = c.compress(b"") + c.flush()
    out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(empty) + 25)
    out += empty + struct.pack("<II", 0, 0)
    return bytes(out)


def bam_bytes(refs: Sequence[Tuple[str, int]], records: Sequence[Rec], text: Optional[str] = None) -> bytes:
    if text is None:
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    raw = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs)))
    for name, ln in refs:
        raw += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    for r in records:
        raw += encode_record(r)
    return bgzf(bytes(raw))


def write_bam(path, refs, records, text=None) -> None:
    with open(path, "wb") as f:
        f.write(bam_bytes(refs, records, text))


def sort_key(r: Rec):
    return (r.ref if r.ref >= 0 else 1 << 31, r.pos)


def read_bam(path):
    """-> (refs [(name, length)], records [dict]) with the raw fields of every record."""
    raw = gzip.decompress(open(path, "rb").read())
    assert raw[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", raw, o)[0]
        name = raw[o + 4:o + 4 + ln].split(b"\0")[0].decode()
        refs.append((name, struct.unpack_from("<i", raw, o + 4 + ln)[0]))
        o += 8 + ln
    recs = []
    while o < len(raw):
        bs = struct.unpack_from("<i", raw, o)[0]
        b = raw[o + 4:o + 4 + bs]
        ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", b, 0)
        p = 32
        name = b[p:p + l_name].split(b"\0")[0]
        p += l_name
        cig = [(CIGAR_OPS[v & 15] if (v & 15) < 9 else "?", v >> 4)
               for v in struct.unpack_from("<%dI" % n_cig, b, p)]
        p += 4 * n_cig
        seq = "".join(SEQ_CODES[(b[p + k // 2] >> (4 * (1 - k % 2))) & 15] for k in range(l_seq))
        p += (l_seq + 1) // 2
        qual = bytes(b[p:p + l_seq])
        p += l_seq
        recs.append(dict(name=name, ref=ref, pos=pos, mapq=mapq, flag=flag, cigar=cig, seq=seq, qual=qual,
                         aux=bytes(b[p:])))
        o += 4 + bs
    return refs, recs


# ------------------------------------------------------------------------------------------------------------
# synthetic sets

def _read(rng, name, ref, pos, length, genome, variant, cell_allele, low_q=0.05, n_rate=0.01, cigar=None,
          **kw) -> Rec:
    if cigar is None:
        cigar = [("M", length)]
    bases, gpos = [], pos
    for op, n in cigar:
        if op in "M=X":
            for k in range(n):
                g = gpos + k
                b = genome[g % len(genome)]
                if g in variant and cell_allele:
                    b = variant[g]
                if rng.random() < n_rate:
                    b = "N"
                bases.append(b)
            gpos += n
        elif op in "IS":
            bases.extend(rng.choice(list("ACGT"), n))
        elif op in "DNP":
            gpos += n if op != "P" else 0
    seq = "".join(bases)
    qual = [int(q) for q in np.where(rng.random(len(seq)) < low_q, rng.integers(2, 20, len(seq)),
                                     rng.integers(30, 42, len(seq)))]
    return Rec(name=name, ref=ref, pos=pos, cigar=cigar, seq=seq, qual=qual, **kw)


SPECIAL_CIGARS = [
    [("S", 3), ("M", 40), ("I", 2), ("M", 30)],
    [("H", 5), ("M", 20), ("D", 3), ("M", 25)],
    [("S", 6), ("M", 30), ("N", 4), ("M", 30)],  # quality index stays inside SEQ
    [("=", 20), ("X", 1), ("=", 30)],
    [("M", 50), ("I", 3)],  # an I as the last op
    [("S", 10), ("M", 30), ("P", 2), ("M", 20)],
    [("M", 60)],
]


def synthetic_set(directory, n_cells=6, pairs_per_cell=40, n_refs=2, ref_len=1_004_000, read_len=60, seed=0,
                  around=999_900, span=400, tag_types=("C", "S", "I", "c", "i"), extra=None):
    """Writes cell_<k>.bam files into ``directory`` and returns their paths. Reads of every cell cluster
    around ``around`` (crossing the 1,000,000 chunk boundary, mates placed up to ~350 bp later so some fall in
    the next chunk) on every reference; half the cells carry the alternative allele at the planted variants."""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 4096))
    variant = {}
    for v in range(around - span, around + span + 400, 7):
        variant[v] = "ACGT"[("ACGT".index(genome[v % len(genome)]) + 1) % 4]
    refs = [("chr%d" % (r + 1), ref_len) for r in range(n_refs)]
    paths = []
    for cell in range(n_cells):
        recs = []
        for ref in range(n_refs):
            for p in range(pairs_per_cell):
                name = "c%d_r%d_p%d" % (cell % 3, ref, p)  # cells 0 and 3 share names (different slots)
                start = around - span + int(rng.integers(0, 2 * span))
                mate = start + int(rng.integers(0, 350))
                cig1 = SPECIAL_CIGARS[int(rng.integers(0, len(SPECIAL_CIGARS)))] if rng.random() < 0.4 else None
                tt = tag_types[int(rng.integers(0, len(tag_types)))]
                score = int(rng.integers(0, 120)) if tt not in "ci" else -int(rng.integers(1, 100))
                if tt in "C" and score > 255:
                    score = 255
                tags = [("NM", "i", 0), ("AS", tt, score), ("XS", "Z", "x")]
                mq = int(rng.integers(0, 60))
                allele = cell % 2 == 1
                recs.append(_read(rng, name, ref, start, read_len, genome, variant, allele, cigar=cig1,
                                  mapq=mq, tags=tags, flag=0x1 | 0x2 | 0x40 | 0x20))
                recs.append(_read(rng, name, ref, mate, read_len, genome, variant, allele, mapq=mq,
                                  tags=[("AS", tt, score)], flag=0x1 | 0x2 | 0x80 | 0x10))
            # a read without SEQ and one without qualities
            recs.append(Rec(name="noseq_%d_%d" % (cell, ref), ref=ref, pos=around, cigar=[("M", 20)], seq="*"))
            r = _read(rng, "noqual_%d_%d" % (cell, ref), ref, around - 10, 30, genome, variant, cell % 2 == 1)
            r.qual = None
            recs.append(r)
        if extra:
            recs.extend(extra(cell, rng))
        recs.append(Rec(name="unmapped_%d" % cell, ref=-1, pos=-1, cigar=[], seq="ACGT", qual=[30] * 4, flag=0x4))
        recs.sort(key=sort_key)
        path = os.path.join(str(directory), "cell_%03d.bam" % cell)
        write_bam(path, refs, recs)
        paths.append(path)
    return paths


# ------------------------------------------------------------------------------------------------------------
# a uniform set at benchmark size (numpy-built records: 100M reads, AS:C tag)

BASE_CODE = np.array([1, 2, 4, 8], dtype=np.uint8)  # A C G T as 4-bit SEQ codes


def _reg2bin_vec(beg, end):
    end = end - 1
    out = np.zeros_like(beg)
    done = np.zeros(beg.shape, dtype=bool)
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        hit = ~done & ((beg >> shift) == (end >> shift))
        out[hit] = off + (beg[hit] >> shift)
        done |= hit
    return out


def uniform_cell_bam(path, cell, genome, alt, variant_mask, n_pairs, read_len=100, seed=0, low_q=0.02):
    """One cell: n_pairs pairs of read_len M reads, mates 200-400 bp apart, sorted; cells with an odd index
    carry the alternative allele at the planted variants."""
    rng = np.random.default_rng(seed * 100003 + cell)
    L = len(genome)
    p1 = rng.integers(0, L - read_len - 500, n_pairs)
    p2 = p1 + rng.integers(200, 400, n_pairs)
    pos = np.concatenate([p1, p2]).astype(np.int64)
    pair = np.concatenate([np.arange(n_pairs), np.arange(n_pairs)])
    first = np.concatenate([np.ones(n_pairs, bool), np.zeros(n_pairs, bool)])
    order = np.argsort(pos, kind="stable")
    pos, pair, first = pos[order], pair[order], first[order]
    n = len(pos)
    idx = pos[:, None] + np.arange(read_len)[None, :]
    bases = genome[idx]
    if cell % 2:
        bases = np.where(variant_mask[idx], alt[idx], bases)
    codes = BASE_CODE[bases]
    seq = (codes[:, 0::2] << 4) | codes[:, 1::2]
    qual = np.where(rng.random((n, read_len)) < low_q, rng.integers(2, 20, (n, read_len)),
                    rng.integers(30, 42, (n, read_len))).astype(np.uint8)
    name_len = 17  # c<cell>_r<pair>: names unique across cells, as with cell-barcoded reads
    dt = np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("lname", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                   ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<u4"), ("nref", "<i4"), ("npos", "<i4"),
                   ("tlen", "<i4"), ("name", "S%d" % name_len), ("cig", "<u4"), ("seq", "u1", (read_len // 2,)),
                   ("qual", "u1", (read_len,)), ("tag", "S3"), ("as", "u1")])
    rec = np.zeros(n, dtype=dt)
    rec["bs"] = dt.itemsize - 4
    rec["ref"] = 0
    rec["pos"] = pos
    rec["lname"] = name_len
    rec["mapq"] = 60
    rec["bin"] = _reg2bin_vec(pos, pos + read_len)
    rec["ncig"] = 1
    rec["flag"] = np.where(first, 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80)
    rec["lseq"] = read_len
    rec["nref"] = 0
    rec["npos"] = np.where(first, pos + 300, pos - 300)
    rec["name"] = np.char.encode(np.char.add("c%05d_r" % cell, np.char.zfill(pair.astype(str), 9)))
    rec["cig"] = read_len << 4
    rec["seq"] = seq
    rec["qual"] = qual
    rec["tag"] = b"ASC"
    rec["as"] = rng.integers(60, 100, n)
    refs = [("1", L)]
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:1\tLN:%d\n" % L
    raw = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1))
    raw += struct.pack("<i", 2) + b"1\0" + struct.pack("<i", L)
    raw += rec.tobytes()
    with open(path, "wb") as f:
        f.write(bgzf(bytes(raw)))
    return n
