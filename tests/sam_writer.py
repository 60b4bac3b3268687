"""SAM text for the SAM-input tests: ``bw.Rec`` lists -> coordinate-sorted SAM files holding the same records as the
BAM ``bw.write_bam`` writes from them.

SAM has one integer aux type (``i``) and a reader stores each value as htslib's smallest type (c/s/i for negative
values, C/S/I otherwise). ``canonical`` rewrites the records' integer aux types that way, so that
``bw.write_bam(canonical(recs))`` and ``write_sam(recs)`` hold byte-equal records (the SAM-input contract compares a SAM
file with the BAM ``samtools view -b`` writes from it).
"""
from __future__ import annotations

import copy
import os
import struct
from typing import List, Optional, Sequence, Tuple

from tests import bam_writer as bw
from tests import multiplex_bam as mb

INT_TYPES = "cCsSiI"


def smallest_int_type(v: int) -> str:
    if v < 0:
        return "c" if v >= -128 else "s" if v >= -32768 else "i"
    return "C" if v <= 255 else "S" if v <= 65535 else "I"


def canonical(recs: Sequence[bw.Rec]) -> List[bw.Rec]:
    """Copies with every integer aux field typed as a SAM reader stores it."""
    out = []
    for r in recs:
        r = copy.deepcopy(r)
        r.tags = [(t, smallest_int_type(v) if typ in INT_TYPES else typ, v) for t, typ, v in r.tags]
        out.append(r)
    return out


def _f32(v: float) -> str:
    return "%.9g" % struct.unpack("<f", struct.pack("<f", v))[0]


def aux_text(tag: str, typ: str, value) -> str:
    if typ in INT_TYPES:
        return "%s:i:%d" % (tag, value)
    if typ == "f":
        return "%s:f:%s" % (tag, _f32(value))
    if typ == "B":
        sub, vals = value
        return "%s:B:%s%s" % (tag, sub, "".join("," + (_f32(v) if sub == "f" else "%d" % v) for v in vals))
    return "%s:%s:%s" % (tag, typ, value)


def record_line(r: bw.Rec, refs: Sequence[Tuple[str, int]]) -> str:
    rname = refs[r.ref][0] if r.ref >= 0 else "*"
    if r.next_ref < 0:
        rnext = "*"
    elif r.next_ref == r.ref:
        rnext = "="
    else:
        rnext = refs[r.next_ref][0]
    cigar = "".join("%d%s" % (n, op) for op, n in r.cigar) or "*"
    qual = "*" if r.qual is None or r.seq == "*" else "".join(chr(q + 33) for q in r.qual)
    fields = [r.name, str(r.flag), rname, str(r.pos + 1), str(r.mapq), cigar, rnext, str(r.next_pos + 1),
              str(r.tlen), r.seq, qual] + [aux_text(*t) for t in r.tags]
    return "\t".join(fields)


def header_text(refs: Sequence[Tuple[str, int]]) -> str:
    return "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)


def sam_text(refs, records: Sequence[bw.Rec], text: Optional[str] = None) -> str:
    return (header_text(refs) if text is None else text) + "".join(record_line(r, refs) + "\n" for r in records)


def write_sam(path, refs, records, text=None) -> None:
    with open(path, "w") as f:
        f.write(sam_text(refs, records, text))


def write_both(directory, name: str, refs, records) -> Tuple[str, str]:
    """The canonical records as <name>.bam and <name>.sam in ``directory`` -> (bam path, sam path)."""
    recs = canonical(records)
    bam, sam = os.path.join(str(directory), name + ".bam"), os.path.join(str(directory), name + ".sam")
    bw.write_bam(bam, refs, recs)
    write_sam(sam, refs, recs)
    return bam, sam


def sam_of_bam(bam_path, sam_path) -> str:
    """A BAM written by bw.write_bam (canonical aux types) as SAM text -> sam_path."""
    refs, _ = bw.read_bam(bam_path)
    write_sam(sam_path, refs, mb.records_of(bam_path))
    return sam_path


def write_multiplexed(directory, refs, records: Sequence[bw.Rec], n_lanes: int = 1, seed: int = 0,
                      name: str = "lane") -> Tuple[List[str], List[str]]:
    """mb.write_multiplexed on the canonical records, each lane also as SAM -> (BAM lanes, SAM lanes)."""
    bams = mb.write_multiplexed(directory, refs, canonical(records), n_lanes, seed, name)
    sams = [sam_of_bam(p, os.path.splitext(p)[0] + ".sam") for p in bams]
    return bams, sams
