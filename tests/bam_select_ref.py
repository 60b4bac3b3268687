"""A plain-Python restatement of rules 3c and 3d of secedo_amd/csrc/bam_kernels.hip (the flag filter and the
duplicate removal of ``pileup_bams``), on the ``bw.Rec`` lists of tests/bam_writer.py.

``select`` says which records one chromosome's call drops and what ``bam_select_stats()`` reports; ``rewrite`` writes
the input files again without the dropped records, which is what the contract compares against: the outputs of a call
with the options on equal those of the same call with the options off on the rewritten files.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence, Set, Tuple

from tests import bam_writer as bw

CHUNK = 1_000_000
STAT_KEYS = ("records", "dropped_require", "dropped_exclude", "templates", "large_templates", "duplicate_templates",
             "duplicate_records")


def five_prime(r: bw.Rec) -> Tuple[int, int]:
    """(u, strand): the unclipped 5' end. Forward: Position minus the leading S/H run; reverse: Position + reflen - 1
    plus the trailing S/H run."""
    lead = trail = 0
    for op, n in r.cigar:
        if op not in "SH":
            break
        lead += n
    for op, n in reversed(r.cigar):
        if op not in "SH":
            break
        trail += n
    if all(op in "SH" for op, _ in r.cigar):  # clips only: one run, leading
        trail = 0
    if r.flag & 0x10:
        return r.pos + bw.ref_length(r.cigar) - 1 + trail, 1
    return r.pos - lead, 0


def score(r: bw.Rec) -> int:
    if r.qual is None or r.seq == "*":
        return 0
    return sum(q for q in r.qual if q >= 15 and q != 0xFF)


def select(files: Sequence[Sequence[bw.Rec]], chromosome: int, require: int = 0, exclude: int = 0,
           remove_duplicates: bool = False, cell_of: Optional[Callable[[bw.Rec], Optional[int]]] = None):
    """files[f] = the records of input file f in file order. Per-file mode: the cell is f; tag mode: ``cell_of(rec)``
    gives the cell, or None for a record of no listed barcode. -> (dropped {(f, k)}, stats dict)."""
    stats: Dict[str, int] = {k: 0 for k in STAT_KEYS}
    dropped: Set[Tuple[int, int]] = set()
    kept = []  # (global order key, cell, f, k, rec)
    for f, recs in enumerate(files):
        for k, r in enumerate(recs):
            if r.ref != chromosome:
                continue
            cell = f if cell_of is None else cell_of(r)
            if cell is None:
                continue
            if require or exclude:
                stats["records"] += 1
                if (r.flag & require) != require:
                    stats["dropped_require"] += 1
                    dropped.add((f, k))
                    continue
                if r.flag & exclude:
                    stats["dropped_exclude"] += 1
                    dropped.add((f, k))
                    continue
            order = (r.pos // CHUNK, cell, k) if cell_of is None else (r.pos // CHUNK, cell, r.pos, f, k)
            kept.append((order, cell, f, k, r))
    if not remove_duplicates:
        return dropped, stats
    kept.sort(key=lambda x: x[0])
    templates: Dict[Tuple[int, str], List[int]] = {}  # (cell, name) -> ordinals, ascending
    for o, (_, cell, _f, _k, r) in enumerate(kept):
        templates.setdefault((cell, r.name), []).append(o)
    stats["templates"] = len(templates)
    groups: Dict[tuple, List[Tuple[int, int, List[int]]]] = {}
    for (cell, _name), members in templates.items():
        if len(members) >= 3:
            stats["large_templates"] += 1
            continue
        ends = sorted(five_prime(kept[o][4]) for o in members)
        key = (cell, len(members)) + tuple(ends)  # a single's key never equals a pair's
        groups.setdefault(key, []).append((sum(score(kept[o][4]) for o in members), members[0], members))
    for cands in groups.values():
        best = max(cands, key=lambda c: (c[0], -c[1]))
        for c in cands:
            if c is best:
                continue
            stats["duplicate_templates"] += 1
            stats["duplicate_records"] += len(c[2])
            for o in c[2]:
                dropped.add((kept[o][2], kept[o][3]))
    return dropped, stats


def add_stats(a: Dict[str, int], b: Dict[str, int]) -> Dict[str, int]:
    return {k: a[k] + b[k] for k in STAT_KEYS}


def without(files: Sequence[Sequence[bw.Rec]], dropped: Set[Tuple[int, int]]) -> List[List[bw.Rec]]:
    return [[r for k, r in enumerate(recs) if (f, k) not in dropped] for f, recs in enumerate(files)]


def rewrite(directory, refs, files: Sequence[Sequence[bw.Rec]], dropped: Set[Tuple[int, int]],
            name: str = "kept") -> List[str]:
    """The files without the dropped records -> <directory>/<name>_<f>.bam paths."""
    os.makedirs(str(directory), exist_ok=True)
    paths = []
    for f, recs in enumerate(without(files, dropped)):
        path = os.path.join(str(directory), "%s_%03d.bam" % (name, f))
        bw.write_bam(path, refs, recs)
        paths.append(path)
    return paths


# ---- the worked example of the duplicate rules (decided by hand; tests/test_bam_select_cpu.py pins it) ----

def _seq(k: int, n: int = 50) -> str:
    return "".join("ACGT"[(k + i * (1 + k % 3)) % 4] for i in range(n))


def worked_example():
    """-> (refs, [cell A records, cell B records], want dropped {(f, k)}, want stats). Read length 50, qualities 30
    unless said otherwise, positions 0-based; every record is paired and a proper pair so that the device passes take
    it. The sequences differ between templates, so a wrong keeper changes the pileup."""
    F, R = 0x1 | 0x2 | 0x40 | 0x20, 0x1 | 0x2 | 0x80 | 0x10
    q = [30] * 50

    def rec(name, pos, cigar, flag, k, qual=None):
        return bw.Rec(name, 0, pos, cigar, _seq(k), qual=list(qual or q), flag=flag)

    low = [10] * 5 + [30] * 45
    a = [
        rec("T1", 1000, [("M", 50)], F, 0), rec("T1", 1200, [("M", 50)], R, 1),
        rec("T2", 1005, [("S", 5), ("M", 45)], F, 2, low), rec("T2", 1200, [("M", 40), ("S", 10)], R, 3, low),
        rec("T4", 1000, [("M", 50)], F, 4),
        bw.Rec("T5", 0, 1000, [("H", 3), ("M", 47)], _seq(5, 47), qual=[30] * 47, flag=F),
        rec("T6", 1000, [("M", 50)], F, 6),
        rec("T7", 1000, [("M", 50)], R, 7),
        rec("T8", 1000, [("M", 50)], F, 8), rec("T8", 1200, [("M", 50)], R, 9), rec("T8", 1100, [("M", 50)], F, 10),
    ]
    b = [rec("T1", 1000, [("M", 50)], F, 0), rec("T1", 1200, [("M", 50)], R, 1)]
    a.sort(key=bw.sort_key)  # stable: T4 stays in front of T6
    names = [(r.name, r.pos) for r in a]
    want = {(0, names.index(("T2", 1005))), (0, names.index(("T2", 1200))), (0, names.index(("T6", 1000)))}
    stats = dict(records=0, dropped_require=0, dropped_exclude=0, templates=8, large_templates=1,
                 duplicate_templates=2, duplicate_records=3)
    return [("1", 100_000)], [a, b], want, stats
