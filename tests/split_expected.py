"""What ``secedo_amd.split_clusters`` must write, computed on the CPU from the contract of include/secedo_bam.h:
``expected_files``. Built from tests/bam_writer.py (``read_bam`` for the reference lists, ``encode_record`` for the
synthetic sets) and tests/bgzf_deflate_cases.py (``host_encode``: the encoder of bgzf_deflate.hpp as a host program
under the sanitizers, which gives the members M(x) of flat bytes x).

A *source* is one input file as the contract sees it: its header text, its reference list and its records as raw bytes
(block_size included) in file order. ``source_of_bam`` reads one from a BAM file; ``source_of_recs`` makes the one
``bw.write_bam(path, refs, recs, text)`` would give. From the sources and a clustering:

  header_bytes   "BAM\\1", l_text, the text (@HD, @SQ per reference, the merged @RG lines, @PG, @CO), n_ref, the list
  cluster_parts  per cluster: the header, then per requested chromosome the records in (Position, file, record) order
  expected_files per cluster: host_encode(part)[:-28] for every part, then the EOF member

and the synthetic sets of tests/test_gpu_split_clusters.py, so that the CPU tests can check them without a GPU.
"""
from __future__ import annotations

import gzip
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import bam_writer as bw
from tests import bgzf_deflate_cases as dc
from tests import bgzf_writer as gw

CUT = 0xFF00
EOF = gw.EOF_MEMBER


class Source:
    def __init__(self, text: str, refs: Sequence[Tuple[str, int]], records: Sequence[bytes]):
        self.text, self.refs, self.records = text, list(refs), list(records)


def default_text(refs) -> str:
    return "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)


def source_of_recs(refs, recs: Sequence[bw.Rec], text: Optional[str] = None) -> Source:
    return Source(default_text(refs) if text is None else text, refs, [bw.encode_record(r) for r in recs])


def source_of_bam(path) -> Source:
    """The header text, the reference list and the raw records of a BAM file."""
    refs, _ = bw.read_bam(path)
    raw = gzip.decompress(open(path, "rb").read())
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].decode()
    o = 12 + l_text + sum(8 + len(n) + 1 for n, _ in refs)
    records = []
    while o < len(raw):
        size = 4 + struct.unpack_from("<i", raw, o)[0]
        records.append(raw[o:o + size])
        o += size
    return Source(text, refs, records)


def ref_pos(record: bytes) -> Tuple[int, int]:
    return struct.unpack_from("<ii", record, 4)


def z_value(record: bytes, tag: str) -> Optional[bytes]:
    """The value of the first aux field named ``tag`` when it is Z-typed (FindTag: the first one counts), else None."""
    l_name, n_cig, l_seq = record[12], struct.unpack_from("<H", record, 16)[0], struct.unpack_from("<I", record, 20)[0]
    p = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p + 3 <= len(record):
        name, typ = record[p:p + 2].decode(), chr(record[p + 2])
        p += 3
        if typ in "ZH":
            end = record.index(b"\0", p)
            if name == tag:
                return record[p:end] if typ == "Z" else None
            p = end + 1
            continue
        if name == tag:
            return None
        if typ == "B":
            sub, count = chr(record[p]), struct.unpack_from("<I", record, p + 1)[0]
            p += 5 + count * sizes[sub]
        else:
            p += sizes[typ]
    return None


def rg_lines(sources: Sequence[Source]) -> List[str]:
    """The distinct @RG lines in order of first appearance; two different lines with one ID are an error."""
    def rg_id(line):
        return next((f for f in line.split("\t")[1:] if f.startswith("ID:")), "")

    out: List[str] = []
    for s in sources:
        for line in s.text.split("\n"):
            if line.startswith("@RG\t") and line not in out:
                assert rg_id(line) not in [rg_id(o) for o in out], line
                out.append(line)
    return out


def header_bytes(sources: Sequence[Source], k: int, m: int, n: int) -> bytes:
    refs = sources[0].refs
    assert all(s.refs == refs for s in sources)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    text += "".join(line + "\n" for line in rg_lines(sources))
    text += "@PG\tID:secedo_amd.split\tPN:secedo_amd\n@CO\tsecedo_amd cluster %d: %d of %d cells\n" % (k, m, n)
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        raw += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return raw


def cluster_parts(sources: Sequence[Source], clustering: Sequence[int], chromosome_ids: Sequence[int],
                  tag: Optional[str] = None, barcodes: Optional[Sequence[str]] = None):
    """-> (parts[k] = [header, records of the 1st requested chromosome, ...], dropped records). Per-file mode: the cell
    of a record is its file's index. Tag mode: the index of its Z-typed ``tag`` value in ``barcodes``."""
    n_clusters = max(clustering) + 1
    index = None if tag is None else {b.encode(): c for c, b in enumerate(barcodes)}
    parts = [[header_bytes(sources, k, sum(1 for c in clustering if c == k), len(clustering))]
             for k in range(n_clusters)]
    dropped = 0
    for chrom in sorted(chromosome_ids):
        per = [[] for _ in range(n_clusters)]  # (pos, file, ordinal, bytes)
        for f, s in enumerate(sources):
            for i, rec in enumerate(s.records):
                ref, pos = ref_pos(rec)
                if ref != chrom:
                    continue
                cell = f if index is None else index.get(z_value(rec, tag))
                if cell is None:
                    dropped += 1
                    continue
                per[clustering[cell]].append((pos, f, i, rec))
        for k in range(n_clusters):
            parts[k].append(b"".join(r[3] for r in sorted(per[k], key=lambda r: r[:3])))
    return parts, dropped


_ENCODED: Dict[bytes, bytes] = {}


def members_of(part: bytes, tmp_path) -> bytes:
    """M(part): the encoder's members for flat bytes, without the EOF member; nothing for no bytes."""
    if not part:
        return b""
    if part not in _ENCODED:
        _ENCODED[part] = dc.host_encode(part, tmp_path, "split%d" % len(_ENCODED))[:-len(EOF)]
    return _ENCODED[part]


def expected_files(sources, clustering, chromosome_ids, tmp_path, tag=None, barcodes=None):
    """-> ([the bytes of cluster_<k>.bam for every k], dropped records)."""
    parts, dropped = cluster_parts(sources, clustering, chromosome_ids, tag, barcodes)
    return [b"".join(members_of(p, tmp_path) for p in ps) + EOF for ps in parts], dropped


def member_sizes(raw: bytes) -> List[Tuple[int, bool]]:
    """(ISIZE, stored) of every member of a file, the EOF member included."""
    out = []
    for member, payload, _crc, isize in dc.split_members(raw):
        out.append((isize, len(payload) > 0 and (payload[0] & 7) == 1))  # BFINAL 1, BTYPE 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic sets of the GPU tests

REFS = [("chr1", 100_000), ("chr2", 100_000)]
BARCODES = ["BC%02d-%s" % (c, "ACGT"[c % 4] * (1 + c % 3)) for c in range(12)]
CLUSTERING = [1, 2, 1, 0, 2, 4, 1, 0, 2, 4, 1, 2]  # 3 of 0..4 has no cell


def _pair(rng, genome, name, ref, pos, length, tags, variant=None, allele=False):
    mate = pos + int(rng.integers(100, 300))
    variant = variant or {}
    a = bw._read(rng, name, ref, pos, length, genome, variant, allele, low_q=0.05, n_rate=0.01, mapq=60, tags=list(tags),
                 flag=0x1 | 0x2 | 0x40 | 0x20)
    b = bw._read(rng, name, ref, mate, length, genome, variant, allele, low_q=0.05, n_rate=0.01, mapq=60, tags=list(tags),
                 flag=0x1 | 0x2 | 0x80 | 0x10)
    return [a, b]


def cell_records(n_cells=12, pairs=60, seed=3) -> List[List[bw.Rec]]:
    """Twelve cells on two references, every record with its cell's CB:Z barcode. Read names are unique per cell and of
    varying (also odd) lengths, so record offsets take every alignment. Every cell has a read at chr1:1000 and two at
    chr1:2000 (ties across files and inside a file); cells 3, 7 and 10 have no record on chr2. Integer aux types are
    the ones a SAM reader stores, so a SAM copy of a file holds byte-equal records. Cells with an odd index carry
    another base every seventh position, so that a pileup of the files has loci."""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 4096))
    variant = {v: "ACGT"[("ACGT".index(genome[v % len(genome)]) + 1) % 4] for v in range(0, 50_000, 7)}
    cells = []
    for c in range(n_cells):
        tags = [("AS", "C", 40 + c), ("CB", "Z", BARCODES[c])]
        recs = []
        for ref in range(2):
            if ref == 1 and c in (3, 7, 10):
                continue
            for p in range(pairs):
                name = "cell%d_r%d_p%d%s" % (c, ref, p, "x" * (p % 4))
                recs += _pair(rng, genome, name, ref, 3000 + int(rng.integers(0, 6_000)), 50 + (p % 7), tags, variant,
                              c % 2 == 1)
        recs += _pair(rng, genome, "cell%d_tie" % c, 0, 1000, 60, tags)[:1]
        recs += _pair(rng, genome, "cell%d_twin_a" % c, 0, 2000, 61, tags)[:1]
        recs += _pair(rng, genome, "cell%d_twin_b" % c, 0, 2000, 59, tags)[:1]
        recs.append(bw.Rec(name="unmapped_%d" % c, ref=-1, pos=-1, cigar=[], seq="ACGT", qual=[30] * 4, flag=0x4,
                           tags=[("CB", "Z", BARCODES[c])]))
        recs.sort(key=bw.sort_key)  # stable: the twins keep their order
        cells.append(recs)
    return cells


def multiplexed_records(cells: Sequence[Sequence[bw.Rec]], seed=4) -> Tuple[List[bw.Rec], int]:
    """One multiplexed file of the cells' records, equal positions in (cell, record) order, plus records that tag mode
    drops: without CB, with CB of another type, with an unlisted CB:Z -> (records, how many of those are mapped)."""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 4096))
    recs = [r for cell in cells for r in cell]
    extra = []
    for k in range(9):
        tags = [[("AS", "C", 7)], [("AS", "C", 7), ("CB", "i", 5)], [("CB", "Z", "NOT-LISTED")],
                [("CB", "A", "x"), ("CB", "Z", BARCODES[0])]][k % 4]
        extra += _pair(rng, genome, "extra_%d" % k, k % 2, [1000, 2000, 5000 + 97 * k][k % 3], 55, tags)[:1]
    recs = sorted(recs + extra, key=bw.sort_key)
    return recs, len(extra)


def padded_cell(rng, genome, name: str, target: int, n_reads: int = 200) -> List[bw.Rec]:
    """Records on chr1 whose encoded bytes sum to exactly ``target``: reads, then one whose XP:Z tag fills the rest."""
    recs, size = [], 0
    for p in range(n_reads):
        r = _pair(rng, genome, "%s_%d" % (name, p), 0, 1000 + 50 * p, 50, [("AS", "C", 9)])[0]
        recs.append(r)
        size += len(bw.encode_record(r))
    last = bw.Rec(name=name + "_pad", ref=0, pos=90_000, cigar=[("M", 10)], seq="ACGTACGTAC", qual=[30] * 10,
                  tags=[("XP", "Z", "")])
    rest = target - size - len(bw.encode_record(last))
    assert rest >= 0, (target, size)
    last.tags = [("XP", "Z", "p" * rest)]
    recs.append(last)
    assert sum(len(bw.encode_record(r)) for r in recs) == target
    return recs


def edge_cells(seed=5) -> List[List[bw.Rec]]:
    """Three cells, one cluster each: record bytes of exactly 0xFF00, of 0xFF00 + 1, and a single record."""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 4096))
    single = [bw.Rec(name="only", ref=0, pos=77, cigar=[("M", 5)], seq="ACGTA", qual=[20] * 5)]
    return [padded_cell(rng, genome, "full", CUT), padded_cell(rng, genome, "over", CUT + 1), single]


def long_read_cells(seed=6) -> List[List[bw.Rec]]:
    """Cell 0: one 70 000-base read with random bases and qualities and, as long reads carry it, an ML:B:C array of
    random bytes; literals from 144 on take 9 bits under the fixed Huffman codes, so members inside that array fall back
    to stored blocks. Cell 1: 300 reads of one base and one quality, which compress."""
    rng = np.random.default_rng(seed)
    n = 70_000
    seq = "".join(rng.choice(list("ACGT"), n))
    qual = [int(q) for q in rng.integers(0, 94, n)]
    ml = [int(v) for v in rng.integers(0, 256, n)]
    long_read = bw.Rec(name="long_read", ref=0, pos=500, cigar=[("M", n)], seq=seq, qual=qual, flag=0,
                       tags=[("ML", "B", ("C", ml))])
    flat = [bw.Rec(name="flat_%03d" % p, ref=0, pos=100 + p, cigar=[("M", 80)], seq="A" * 80, qual=[30] * 80, flag=0)
            for p in range(300)]
    return [[long_read], flat]
