"""Plain Python restatement of the reference's pileup_bams() (pileup.cpp:49-348) at num_threads = 1, the
deterministic run, on records decoded by tests/bam_writer.read_bam. Like tests/variant_ref.py it follows the
reference statement by statement, including BamTools' AlignedBases / Qualities / GetTag("AS", uint32_t&), and
is pinned by the expectations of the reference's tests/test_pileup.cpp and, on the edge inputs of
tests/pileup_edge_cases.py, by the compiled reference itself (tests/test_pileup_edges_cpu.py). The reference's asserts
raise RefAbort; so does a quality index past the quality string, which the reference reads (undefined behaviour).
"""
from __future__ import annotations

import struct
from typing import List, Sequence

from tests.bam_writer import read_bam

CHUNK_SIZE = 1_000_000
MAX_INSERT_SIZE = 1_000
MAX_OPEN_FILES = 100
INT_TO_CHAR = "ACGTNN"


class RefAbort(Exception):
    pass


def char_to_int(c: str) -> int:
    return {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}.get(c, 5)


def aligned_bases(rec) -> str:
    """BamAlignment::BuildCharData's AlignedBases."""
    seq = rec["seq"]
    if not seq or seq == "*":
        return ""
    out, k = [], 0
    for op, n in rec["cigar"]:
        if op in "MI=X":
            out.append(seq[k:k + n])
            k += n
        elif op == "S":
            k += n
        elif op == "D":
            out.append("-" * n)
        elif op == "P":
            out.append("*" * n)
        elif op == "N":
            out.append("N" * n)
    return "".join(out)


def qualities(rec) -> List[int]:
    """BamTools' Qualities as signed chars (0xFF-filled when unstored)."""
    q = rec["qual"]
    if not q:
        return []
    if q[0] == 0xFF:
        return [-1] * len(q)
    return [((v + 33) & 0xFF) - 256 if ((v + 33) & 0xFF) >= 128 else (v + 33) & 0xFF for v in q]


def alignment_score(rec) -> int:
    """GetTag("AS", uint32_t&) starting from 0."""
    d = rec["aux"]
    n, p = len(d), 0
    while p < n:
        if p + 3 > n:
            return 0
        tag, typ = d[p:p + 2], chr(d[p + 2])
        p += 3
        if tag == b"AS":
            size = {"A": 1, "C": 1, "S": 2, "I": 4}.get(typ)
            if size is None or p + size > n:
                return 0
            return int.from_bytes(d[p:p + size], "little")
        if typ in "AcC":
            skip = 1
        elif typ in "sS":
            skip = 2
        elif typ in "fiI":
            skip = 4
        elif typ in "ZH":
            e = d.find(b"\0", p)
            skip = (e - p + 1) if e >= 0 else n - p + 1
        elif typ == "B":
            sub, cnt = chr(d[p]), struct.unpack_from("<I", d, p + 1)[0]
            es = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(sub)
            if es is None:
                return 0
            skip = 5 + cnt * es
        else:
            return 0
        p += skip
        if p >= n or d[p] == 0:
            return 0
    return 0


def walk(rec, start_pos, end_pos, min_base_quality, min_map_quality, min_alignment_score):
    """The base loop of read_bam_file (:93-161): yields (position, base) of the stored bases."""
    ab = aligned_bases(rec)
    q = qualities(rec)
    cig = rec["cigar"]
    out = []
    if not ab:
        return out
    ci = 0
    while cig[ci][0] in "HS":
        ci += 1
    offset = del_offset = 0
    cigar_end = cig[ci][1]
    i = 0
    while i + offset < len(ab):
        while i >= cigar_end:
            ci += 1
            if ci >= len(cig):
                raise RefAbort("cigar_idx < CigarData.size()")
            if cig[ci][0] == "I":
                offset += cig[ci][1]
                if i + offset >= len(ab):
                    if ci != len(cig) - 1:
                        raise RefAbort("insert not last")
                    break
                continue
            elif cig[ci][0] == "D":
                del_offset += cig[ci][1]
            cigar_end += cig[ci][1]
        if i + offset >= len(ab):
            if ci != len(cig) - 1:
                raise RefAbort("cigar_idx == CigarData.size() - 1")
            break
        ch = ab[i + offset]
        base = char_to_int(ch)
        if cig[ci][0] == "D" and ch != "-":
            raise RefAbort("deletion")
        if base == 5:
            i += 1
            continue
        qi = i + offset - del_offset
        if qi >= len(q):
            raise RefAbort("quality index past the quality string")
        if ((q[qi] - 33) & 0xFFFFFFFF) < min_base_quality:
            i += 1
            continue
        if rec["mapq"] < min_map_quality or alignment_score(rec) < min_alignment_score:
            i += 1
            continue
        if rec["pos"] + i >= end_pos + MAX_INSERT_SIZE:
            raise RefAbort("MAX_INSERT_SIZE")
        out.append((rec["pos"] + i, base))
        i += 1
    return out


def chromosome_records(path, chromosome_id):
    """The records a reader returns for the chromosome: RefID == chromosome_id, up to another RefID."""
    _refs, recs = read_bam(path)
    out, started = [], False
    for r in recs:
        if r["ref"] == chromosome_id:
            started = True
            out.append(r)
        elif started:
            break
    return out


class Pileup:
    def __init__(self):
        self.loci = []  # (position, read_ids, cell_bases)
        self.map_lines: List[str] = []
        self.txt_lines: List[str] = []

    def bin_bytes(self) -> bytes:
        out = bytearray()
        for pos, rids, cbs in self.loci:
            out += struct.pack("<IH", pos, len(rids))
            out += struct.pack("<%dI" % len(rids), *rids)
            out += struct.pack("<%dH" % len(cbs), *cbs)
        return bytes(out)

    def map_text(self) -> str:
        return "".join(self.map_lines)

    def txt_text(self) -> str:
        return "".join(self.txt_lines)


def pileup_bams(bam_files: Sequence[str], chromosome_id: int, max_coverage: int, min_base_quality: int,
                min_map_quality: int, min_alignment_score: int, min_different: int) -> Pileup:
    files = [chromosome_records(f, chromosome_id) for f in bam_files]
    cursor = [0] * len(files)
    maps = [dict() for _ in range(min(len(files), MAX_OPEN_FILES))]
    last_read_id = 0
    data, size = {}, {}
    res = Pileup()
    start_pos, is_done = 0, False
    while not is_done:
        is_done = True
        end_pos = start_pos + CHUNK_SIZE
        for f, recs in enumerate(files):
            if not recs:
                continue  # Jump fails: no alignments of this chromosome
            cell = f
            slot = maps[f % MAX_OPEN_FILES]
            while cursor[f] < len(recs):
                r = recs[cursor[f]]
                if r["pos"] >= end_pos:
                    is_done = False
                    break
                cursor[f] += 1
                fl = r["flag"]
                if not (fl & 0x2) or not (fl & 0x1) or (fl & 0x200):
                    raise RefAbort("flags")
                if r["pos"] < start_pos:
                    continue
                name = r["name"]
                if name not in slot:
                    slot[name] = last_read_id
                    res.map_lines.append("%s\t%d\n" % (name.decode(), last_read_id))
                    last_read_id += 1
                read_id = slot[name]
                for pos, base in walk(r, start_pos, end_pos, min_base_quality, min_map_quality,
                                      min_alignment_score):
                    cur = size.get(pos, 0)
                    size[pos] = (cur + 1) & 0xFFFF
                    if cur >= max_coverage:
                        continue
                    data.setdefault(pos, {})[cur] = (read_id, (cell << 2) | base)
        for pos in sorted(p for p in size if start_pos <= p < end_pos):
            cov = size[pos]
            if cov < 2 or cov >= max_coverage:
                continue
            entries = [data[pos][k] for k in range(cov)]
            nb = [0, 0, 0, 0]
            for _, cb in entries:
                nb[cb & 3] += 1
            if cov - max(nb) < min_different:
                continue
            res.loci.append((pos + 1, [e[0] for e in entries], [e[1] for e in entries]))
            srt = sorted(entries, key=lambda e: e[1] >> 2)  # stable: the reference's order up to 16 entries
            res.txt_lines.append("%d\t%d\t%d\t%s\t%s\t%s\n" % (
                chromosome_id + 1, pos + 1, cov, "".join(INT_TO_CHAR[e[1] & 3] for e in srt),
                ",".join(str(e[1] >> 2) for e in srt), ",".join(str(e[0]) for e in srt)))
        for pos in [p for p in size if p < end_pos]:
            del size[pos]
            data.pop(pos, None)
        start_pos = end_pos
    return res
