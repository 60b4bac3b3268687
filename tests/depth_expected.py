"""What ``secedo_amd.bin_depth`` must return and write, computed on the CPU in plain Python from the contract of
include/secedo_bam.h and the ``bw.Rec`` lists that tests/bam_writer.py encodes: ``expected``. Builds on
tests/split_expected.py (``z_value`` for a record's barcode, ``REFS`` and the synthetic cell sets) and on
tests/bam_select_ref.py (which records the duplicate rule drops).

The rules, restated: chromosome c has ceil(LN_c / S) bins, global bins run over the requested chromosomes in ascending
id; a record is selected by barcode, flag masks, duplicates, MapQuality and range, in this order; ``reads`` adds 1 to
the bin of the Position, ``bases`` adds per touched bin the reference positions below LN_c that M, = and X ops cover.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import bam_select_ref as ref
from tests import bam_writer as bw
from tests import split_expected as se

CELL_COLUMNS = ("records", "counted", "sum", "nonzero_bins", "max_value")
STAT_KEYS = ("records", "counted", "dropped_barcode", "dropped_require", "dropped_exclude", "dropped_duplicate",
             "dropped_mapq", "out_of_range", "pairs")
PLAIN_FILES = ("depth.bins.bed", "depth.samples.tsv")  # never compressed
GZ_FILES = ("depth.counts.mtx", "depth.cells.tsv", "depth.clusters.tsv")


def default_name(path) -> str:
    base = os.path.basename(str(path))
    for ext in (".sam.gz", ".bam", ".sam"):
        if base.endswith(ext):
            return base[:-len(ext)]
    return base


def covered(rec: bw.Rec, ln: int) -> List[int]:
    """The reference positions < ln that an M, = or X op of the record covers."""
    out, p = [], rec.pos
    for op, n in rec.cigar:
        if op in "M=X":
            out += [q for q in range(p, p + n) if q < ln]
        if op in "MDN=X":
            p += n
    return out


class Expected:
    def __init__(self):
        self.bins: List[Tuple[int, int, int]] = []  # (chromosome id, start, end) per global bin
        self.pairs: Dict[Tuple[int, int], int] = {}  # (global bin, cell) -> value > 0
        self.cells: np.ndarray = np.zeros((0, 5), np.uint64)
        self.cluster_sums: Optional[np.ndarray] = None
        self.stats: Dict[str, int] = {k: 0 for k in STAT_KEYS}
        self.names: List[str] = []
        self.files: Dict[str, bytes] = {}
        self.pieces = 0  # sorted pieces: records in `reads` mode, touched bins in `bases` mode

    def arrays(self):
        keys = sorted(self.pairs)
        return (np.array([k[0] for k in keys], np.uint32), np.array([k[1] for k in keys], np.uint32),
                np.array([self.pairs[k] for k in keys], np.uint64))


def expected(files: Sequence[Sequence[bw.Rec]], refs, bin_size: int, chromosome_ids: Sequence[int], mode: str = "reads",
             min_map_quality: int = 30, require: int = 0, exclude: int = 0, duplicates: str = "off",
             tag: Optional[str] = None, barcodes: Optional[Sequence[str]] = None,
             clustering: Optional[Sequence[int]] = None, names: Optional[Sequence[str]] = None) -> Expected:
    """files[f] = the records of input file f in file order; ``names``: the cell names (the caller gives the default
    ones of per-file mode, which come from the paths; tag mode defaults to the barcodes)."""
    e = Expected()
    S = bin_size
    n_cells = len(files) if tag is None else len(barcodes)
    index = None if tag is None else {b.encode(): c for c, b in enumerate(barcodes)}

    def cell_of(r: bw.Rec):
        return index.get(se.z_value(bw.encode_record(r), tag))

    base = {}
    for c in sorted(chromosome_ids):
        ln = refs[c][1]
        base[c] = len(e.bins)
        for b in range((ln + S - 1) // S):
            e.bins.append((c, b * S, min((b + 1) * S, ln)))
    cells = np.zeros((n_cells, 5), np.uint64)
    for c in sorted(chromosome_ids):
        ln = refs[c][1]
        dropped, _ = ref.select(files, c, require, exclude, duplicates == "remove", None if tag is None else cell_of)
        for f, recs in enumerate(files):
            for k, r in enumerate(recs):
                if r.ref != c:
                    continue
                cell = f if tag is None else cell_of(r)
                if cell is None:
                    e.stats["dropped_barcode"] += 1
                    continue
                e.stats["records"] += 1
                cells[cell, 0] += 1
                if (r.flag & require) != require:
                    e.stats["dropped_require"] += 1
                    continue
                if r.flag & exclude:
                    e.stats["dropped_exclude"] += 1
                    continue
                if (f, k) in dropped:
                    e.stats["dropped_duplicate"] += 1
                    continue
                if r.mapq < min_map_quality:
                    e.stats["dropped_mapq"] += 1
                    continue
                if r.pos < 0 or r.pos >= ln:
                    e.stats["out_of_range"] += 1
                    continue
                e.stats["counted"] += 1
                cells[cell, 1] += 1
                if mode == "reads":
                    key = (base[c] + r.pos // S, cell)
                    e.pairs[key] = e.pairs.get(key, 0) + 1
                    e.pieces += 1
                else:
                    span = bw.ref_length(r.cigar)
                    if span:
                        e.pieces += (min(r.pos + span, ln) - 1) // S - r.pos // S + 1
                    for q in covered(r, ln):
                        key = (base[c] + q // S, cell)
                        e.pairs[key] = e.pairs.get(key, 0) + 1
    for (b, cell), v in e.pairs.items():
        cells[cell, 2] += v
        cells[cell, 3] += 1
        cells[cell, 4] = max(int(cells[cell, 4]), v)
    e.cells = cells
    e.stats["pairs"] = len(e.pairs)
    e.names = list(names) if names is not None else list(barcodes) if tag is not None else []
    if clustering is not None:
        assert len(clustering) == n_cells
        K = max(clustering) + 1
        e.cluster_sums = np.zeros((len(e.bins), K), np.uint64)
        for (b, cell), v in e.pairs.items():
            e.cluster_sums[b, clustering[cell]] += v

    name = [r[0] for r in refs]
    e.files["depth.bins.bed"] = "".join("%s\t%d\t%d\n" % (name[c], a, z) for c, a, z in e.bins).encode()
    e.files["depth.samples.tsv"] = "".join(n + "\n" for n in e.names).encode()
    mtx = "%%MatrixMarket matrix coordinate integer general\n%\n" + "%d\t%d\t%d\n" % (len(e.bins), n_cells, len(e.pairs))
    mtx += "".join("%d\t%d\t%d\n" % (b + 1, cell + 1, e.pairs[(b, cell)]) for b, cell in sorted(e.pairs))
    e.files["depth.counts.mtx"] = mtx.encode()
    tsv = "cell\tname\trecords\tcounted\tsum\tnonzero_bins\tmax_value\n"
    for c in range(n_cells):
        tsv += "%d\t%s\t%s\n" % (c, e.names[c] if e.names else "", "\t".join(str(int(v)) for v in cells[c]))
    e.files["depth.cells.tsv"] = tsv.encode()
    if clustering is not None:
        K = e.cluster_sums.shape[1]
        tsv = "chrom\tstart\tend" + "".join("\tcluster_%d" % k for k in range(K)) + "\n"
        for g, (c, a, z) in enumerate(e.bins):
            tsv += "%s\t%d\t%d%s\n" % (name[c], a, z, "".join("\t%d" % int(v) for v in e.cluster_sums[g]))
        e.files["depth.clusters.tsv"] = tsv.encode()
    return e


def hand_example():
    """Three cells on one 2500 bp reference, S = 1000, worked by hand (tests/test_bin_depth_cpu.py pins it).
    -> (refs, files, want) with want[mode] = (pairs {(bin, cell): value}, cells table rows)."""
    refs = [("chrA", 2500)]

    def rec(name, pos, cigar, mapq=60, flag=0):
        n = sum(k for op, k in cigar if op in "MIS=X")
        return bw.Rec(name=name, ref=0, pos=pos, cigar=cigar, seq="A" * n if n else "*", qual=[30] * n if n else None,
                      flag=flag, mapq=mapq)

    files = [
        # cell 0: two reads in bin 0, one across the border 999|1000, one of low MapQ
        [rec("a", 0, [("M", 10)]), rec("b", 990, [("M", 20)]), rec("c", 995, [("M", 10)]),
         rec("d", 1500, [("M", 10)], mapq=29)],
        # cell 1: a deletion, a read that runs past LN, a read at LN (out of range)
        [rec("e", 1000, [("S", 5), ("M", 10), ("D", 5), ("M", 10), ("H", 2)]), rec("f", 2495, [("M", 10)]),
         rec("g", 2500, [("M", 10)])],
        # cell 2: no CIGAR, and an N that skips bin 1 whole
        [rec("h", 100, []), rec("i", 990, [("M", 10), ("N", 1000), ("M", 10)])],
    ]
    reads = {(0, 0): 3, (1, 1): 1, (2, 1): 1, (0, 2): 2}
    reads_cells = [[4, 3, 3, 1, 3], [3, 2, 2, 2, 1], [2, 2, 2, 1, 2]]
    bases = {(0, 0): 10 + 10 + 5, (1, 0): 10 + 5, (1, 1): 20, (2, 1): 5, (0, 2): 10, (2, 2): 10}
    bases_cells = [[4, 3, 40, 2, 25], [3, 2, 25, 2, 20], [2, 2, 20, 2, 10]]
    return refs, files, {"reads": (reads, reads_cells), "bases": (bases, bases_cells)}
