"""Writers of the reference's pileup file formats, for the loader and CLI tests.

``write_bin``: per locus u32 position, u16 coverage, u32 read_ids[coverage], u16 (cell << 2 | base)[coverage]
(the format secedo_amd/csrc/pileup_io.cpp reads). ``write_text``: chromosome, position, coverage, bases, comma
separated cell ids, comma separated read ids, tab separated. Both take a one-chromosome FlatPileup whose id_base
holds raw cell ids (cell << 2 | base). ``clone_tree_files`` writes a planted clone tree split over chromosomes.
"""
import os

import numpy as np

from secedo_amd.pileup import FlatPileup

BASES = "ACGT"


def records(positions, coverages, read_ids, packed):
    """Raw bytes of the given records (numpy arrays; read_ids / packed concatenated over the records)."""
    out = bytearray()
    e = 0
    for pos, cov in zip(np.asarray(positions, dtype=np.uint32), np.asarray(coverages, dtype=np.uint16)):
        out += np.uint32(pos).tobytes() + np.uint16(cov).tobytes()
        cov = int(cov)
        out += np.asarray(read_ids[e:e + cov], dtype=np.uint32).tobytes()
        out += np.asarray(packed[e:e + cov], dtype=np.uint16).tobytes()
        e += int(cov)
    return bytes(out)


def write_bin(path, p: FlatPileup):
    off = np.asarray(p.locus_entry_off, dtype=np.int64)
    with open(path, "wb") as f:
        f.write(records(p.locus_pos, np.diff(off), p.read_ids, np.asarray(p.id_base, dtype=np.uint16)))


def write_text(path, p: FlatPileup, chromosome="1"):
    off = np.asarray(p.locus_entry_off, dtype=np.int64)
    idb = np.asarray(p.id_base, dtype=np.int64)
    with open(path, "w") as f:
        for i, pos in enumerate(p.locus_pos):
            sl = slice(off[i], off[i + 1])
            bases = "".join(BASES[b & 3] for b in idb[sl])
            cells = ",".join(str(c >> 2) for c in idb[sl])
            rids = ",".join("r%d" % r for r in np.asarray(p.read_ids)[sl])
            f.write("%s\t%d\t%d\t%s\t%s\t%s\n" % (chromosome, pos, off[i + 1] - off[i], bases, cells, rids))


def renumber_reads(p: FlatPileup) -> FlatPileup:
    """Read ids numbered in order of first appearance (what the text reader assigns)."""
    rid = np.asarray(p.read_ids)
    _, first = np.unique(rid, return_index=True)
    order = np.argsort(first)
    new = np.empty(len(first), dtype=np.uint32)
    new[order] = np.arange(len(first), dtype=np.uint32)
    _, inv = np.unique(rid, return_inverse=True)
    return FlatPileup(p.chr_locus_off, p.locus_pos, p.locus_entry_off, new[inv], p.id_base)


def split_chromosomes(p: FlatPileup, chromosomes):
    """A one-chromosome pileup cut into len(chromosomes) consecutive runs of loci, positions shifted to start at
    1 in each run, read ids numbered from 0 in each. -> {chromosome name: FlatPileup}."""
    n = p.n_loci
    cuts = np.linspace(0, n, len(chromosomes) + 1).astype(np.int64)
    off = np.asarray(p.locus_entry_off, dtype=np.int64)
    out = {}
    for name, a, b in zip(chromosomes, cuts[:-1], cuts[1:]):
        sl = slice(off[a], off[b])
        part = FlatPileup(np.asarray([0, b - a], dtype=np.uint32),
                          (np.asarray(p.locus_pos[a:b], dtype=np.int64) - int(p.locus_pos[a]) + 1).astype(np.uint32),
                          (off[a:b + 1] - off[a]).astype(np.uint64), np.asarray(p.read_ids[sl]),
                          np.asarray(p.id_base[sl]))
        out[name] = renumber_reads(part)
    return out


def clone_tree_files(directory, p: FlatPileup, chromosomes=("1", "2", "X"), text=False, prefix="s"):
    """Writes <directory>/<prefix>_<chromosome>.pileup[.bin] per chromosome -> {chromosome: FlatPileup}."""
    os.makedirs(directory, exist_ok=True)
    parts = split_chromosomes(p, chromosomes)
    for name, part in parts.items():
        path = os.path.join(directory, "%s_%s.pileup" % (prefix, name))
        if text:
            write_text(path, part, name)
        else:
            write_bin(path + ".bin", part)
    return parts
