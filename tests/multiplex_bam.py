"""Multiplexed BAMs for the tag-mode tests: per-cell ``bw.Rec`` lists -> one or several coordinate-sorted BAMs whose
records carry the cell's barcode as a Z-typed tag, and the per-cell split files that the tag-mode contract compares
against (cell c = every record whose first ``tag`` field is Z-typed and equal to barcode c, in (Position, input
file, record) order).
"""
from __future__ import annotations

import copy
import os
import struct
from typing import List, Optional, Sequence

import numpy as np

from tests import bam_writer as bw


def parse_aux(aux: bytes):
    """Raw aux bytes -> [(tag, type, value)] as bw.Rec.tags takes them."""
    out, p = [], 0
    sizes = {"c": ("<b", 1), "C": ("<B", 1), "s": ("<h", 2), "S": ("<H", 2), "i": ("<i", 4), "I": ("<I", 4),
             "f": ("<f", 4)}
    while p + 3 <= len(aux):
        tag, typ = aux[p:p + 2].decode(), chr(aux[p + 2])
        p += 3
        if typ == "A":
            out.append((tag, typ, chr(aux[p])))
            p += 1
        elif typ in "ZH":
            e = aux.index(b"\0", p)
            out.append((tag, typ, aux[p:e].decode()))
            p = e + 1
        elif typ == "B":
            sub, cnt = chr(aux[p]), struct.unpack_from("<I", aux, p + 1)[0]
            fmt, n = sizes[sub]
            vals = [struct.unpack_from(fmt, aux, p + 5 + n * k)[0] for k in range(cnt)]
            out.append((tag, typ, (sub, vals)))
            p += 5 + n * cnt
        else:
            fmt, n = sizes[typ]
            out.append((tag, typ, struct.unpack_from(fmt, aux, p)[0]))
            p += n
    return out


def records_of(path) -> List[bw.Rec]:
    """The records of a BAM written by bw.write_bam, back as bw.Rec."""
    _refs, recs = bw.read_bam(path)
    out = []
    for d in recs:
        qual = None if d["qual"] and d["qual"][0] == 0xFF else list(d["qual"])
        out.append(bw.Rec(name=d["name"].decode(), ref=d["ref"], pos=d["pos"], cigar=list(d["cigar"]),
                          seq=d["seq"] if d["seq"] else "*", qual=qual, flag=d["flag"], mapq=d["mapq"],
                          tags=parse_aux(d["aux"])))
    return out


def barcode_of(rec: bw.Rec, tag: str) -> Optional[str]:
    """The cell value of a record: its first ``tag`` field when Z-typed, else None (FindTag: the first one counts)."""
    for t, typ, v in rec.tags:
        if t == tag:
            return v if typ == "Z" else None
    return None


def tagged(cell_recs: Sequence[Sequence[bw.Rec]], barcodes: Sequence[str], tag: str = "CB") -> List[List[bw.Rec]]:
    """Copies of each cell's records with (tag, "Z", barcode) appended."""
    out = []
    for recs, b in zip(cell_recs, barcodes):
        cell = []
        for r in recs:
            r = copy.deepcopy(r)
            r.tags = list(r.tags) + [(tag, "Z", b)]
            cell.append(r)
        out.append(cell)
    return out


def write_multiplexed(directory, refs, records: Sequence[bw.Rec], n_lanes: int = 1, seed: int = 0,
                      name: str = "lane") -> List[str]:
    """Deals ``records`` (any cells, unsorted) over n_lanes files at random, each written coordinate-sorted (stable
    on the given order) -> the lane paths."""
    rng = np.random.default_rng(seed)
    lane = rng.integers(0, n_lanes, len(records)) if n_lanes > 1 else np.zeros(len(records), dtype=int)
    paths = []
    for f in range(n_lanes):
        recs = [r for r, l in zip(records, lane) if l == f]
        recs.sort(key=bw.sort_key)
        path = os.path.join(str(directory), "%s_%d.bam" % (name, f))
        bw.write_bam(path, refs, recs)
        paths.append(path)
    return paths


def split(directory, refs, lanes: Sequence[str], barcodes: Sequence[str], tag: str = "CB",
          name: str = "cell") -> List[str]:
    """The contract's per-cell files C_c of the multiplexed ``lanes``: the records of barcode c in (Position,
    input file, record) order -> the paths, <directory>/<name>_<c>.bam."""
    index = {b: c for c, b in enumerate(barcodes)}
    per = [[] for _ in barcodes]
    for f, path in enumerate(lanes):
        for k, r in enumerate(records_of(path)):
            c = index.get(barcode_of(r, tag))
            if c is not None:
                per[c].append((bw.sort_key(r), f, k, r))
    paths = []
    for c, items in enumerate(per):
        items.sort(key=lambda x: x[:3])
        path = os.path.join(str(directory), "%s_%05d.bam" % (name, c))
        bw.write_bam(path, refs, [x[3] for x in items])
        paths.append(path)
    return paths


def synthetic_cells(directory, **kw):
    """bw.synthetic_set's cells as records -> (refs, [[bw.Rec] per cell])."""
    os.makedirs(str(directory), exist_ok=True)
    paths = bw.synthetic_set(directory, **kw)
    refs, _ = bw.read_bam(paths[0])
    return refs, [records_of(p) for p in paths]
