"""Small random fragment pileups for the parity tests (numpy, pure-Python loops: small sizes).

Independent of the product's SYNTH-v1 generator (secedo_amd/csrc/synth.cpp): the tests also use
this one so that a bug in the product's generator cannot hide a bug in the product's kernels.
"""
from __future__ import annotations

import numpy as np

from secedo_amd.pileup import FlatPileup


def random_pileup(seed, n_cells, n_chr, loci_per_chr, cov, gap_max, frag_min=50, frag_max=600,
                  dup_frac=0.02, conflict_frac=0.5, skip_frac=0.0, err=0.02, n_groups=None,
                  shuffle_ids=True, triple_frac=0.0):
    """Fragments start at loci, cover the following loci inside their length.

    dup_frac      fraction of (read, locus) entries that get a second mate entry
    conflict_frac of those, fraction whose second base differs (similarity_matrix.cpp:387-395)
    triple_frac   fraction of duplicated entries that get a THIRD entry at the same locus
    skip_frac     probability that a fragment skips a locus inside its span (paired-end insert)
    n_groups      number of group ids appearing in the pileup (default n_cells)
    """
    rng = np.random.default_rng(seed)
    n_groups = n_groups or n_cells
    chr_off = [0]
    locus_pos, locus_off = [], [0]
    read_ids, id_base = [], []
    next_read = 0
    for c in range(n_chr):
        L = loci_per_chr if np.isscalar(loci_per_chr) else loci_per_chr[c]
        gaps = 1 + rng.integers(0, gap_max, size=L)
        pos = np.cumsum(gaps) + 1000
        clone_diff = rng.random(L) < 0.35
        ref_base = rng.integers(0, 4, size=L)
        # fragments: (start locus, end position, group, id)
        per_locus = [[] for _ in range(L)]
        n_new = rng.poisson(cov * 0.6, size=L) if gap_max > frag_max else rng.poisson(
            max(cov * gap_max / (2.0 * (frag_min + frag_max) / 2.0), 0.3), size=L)
        for l in range(L):
            for _ in range(int(n_new[l])):
                g = int(rng.integers(0, n_groups))
                length = int(rng.integers(frag_min, frag_max + 1))
                rid = next_read
                next_read += 1
                end = pos[l] + length
                k = l
                while k < L and pos[k] < end:
                    if k == l or rng.random() >= skip_frac:
                        per_locus[k].append((rid, g))
                    k += 1
        for l in range(L):
            entries = []
            for (rid, g) in per_locus[l]:
                b = int(ref_base[l])
                if clone_diff[l] and g >= n_groups // 2:
                    b = (b + 1) & 3
                if rng.random() < err:
                    b = int(rng.integers(0, 4))
                entries.append((rid, g, b))
                if rng.random() < dup_frac:
                    b2 = (b + int(rng.integers(1, 4))) & 3 if rng.random() < conflict_frac else b
                    entries.append((rid, g, b2))
                    if rng.random() < triple_frac:
                        entries.append((rid, g, int(rng.integers(0, 4))))
            for (rid, g, b) in entries:
                read_ids.append(rid)
                id_base.append((g << 2) | b)
            locus_pos.append(int(pos[l]))
            locus_off.append(len(read_ids))
        chr_off.append(len(locus_pos))
    read_ids = np.asarray(read_ids, dtype=np.uint32)
    if shuffle_ids and next_read:
        # arbitrary (non-consecutive) ids, still unique per fragment
        perm = rng.permutation(next_read).astype(np.uint32) * np.uint32(7) + np.uint32(13)
        read_ids = perm[read_ids]
    return FlatPileup(np.asarray(chr_off, dtype=np.uint32), np.asarray(locus_pos, dtype=np.uint32),
                      np.asarray(locus_off, dtype=np.uint64), read_ids,
                      np.asarray(id_base, dtype=np.uint32))


def from_rows(rows, n_chr_split=None):
    """rows: list of chromosomes, each a list of (position, [(read_id, group, base), ...])."""
    chr_off = [0]
    pos, off, rid, idb = [], [0], [], []
    for chrom in rows:
        for (p, ents) in chrom:
            pos.append(p)
            for (r, g, b) in ents:
                rid.append(r)
                idb.append((g << 2) | b)
            off.append(len(rid))
        chr_off.append(len(pos))
    return FlatPileup(np.asarray(chr_off, dtype=np.uint32), np.asarray(pos, dtype=np.uint32),
                      np.asarray(off, dtype=np.uint64), np.asarray(rid, dtype=np.uint32),
                      np.asarray(idb, dtype=np.uint32))


def deep_locus_pileup(seed=313, n_cells=100, block=64, deep_other=0):
    """A pileup that takes accumulate_tiles by its own data: two cell blocks of 64, 40 loci 40 bp apart with 60
    entries per block and locus, and early on (its reads are flushed before the pileup ends) one locus with 5000 entries in block 0 -- more than a locus range
    stages (4096 column entries), so it is paired from HBM, and 300 of them in cell 0, so that a cell pair can
    collect 65536 pairs and more (300^2: no 16-bit count tile). About 4 % of the entries belong to reads of two or more loci
    (pairs of two multi-locus reads; too few for the window masks to be staged). deep_other: entries of the other blocks
    at the deep locus (none, or some: the off-diagonal tile then pairs that range from HBM too)."""
    rng = np.random.default_rng(seed)
    n_blocks = (n_cells + block - 1) // block
    rows, rid, last = [], 0, {}
    for l in range(41):
        deep = l == 5
        ref, ents, now = int(rng.integers(0, 4)), [], {}
        for b in range(n_blocks):
            cells_b = min(block, n_cells - b * block)
            if deep and b == 0:
                cells = np.concatenate([np.zeros(300, dtype=np.int64), rng.integers(1, cells_b, size=4700)])
            elif deep:
                cells = rng.integers(0, cells_b, size=deep_other)
            else:
                cells = rng.integers(0, cells_b, size=60)
            for cell in (cells + b * block).tolist():
                base = ref if rng.random() < 0.7 else int(rng.integers(0, 4))
                prev = last.get(cell)
                if prev is not None and cell not in now and rng.random() < 0.1:
                    r = prev  # a multi-locus read (at most one entry per locus)
                else:
                    r, rid = rid, rid + 1
                now[cell] = r
                ents.append((r, cell, base))
        last = {} if deep else now  # (the deep locus' reads are single-locus: the multi-locus share stays small)
        rows.append((1000 + 40 * l, ents))
    return from_rows([rows])


def pair_kernel_pileup(name):
    """(pileup, cells, block_cells or None, the pair kernel it takes by its own data, a non-contiguous tile list or
    None): clustered loci with reads that reach beyond their 8- and 16-locus windows (4 blocks of 64, 10 tiles, 17000
    entries per full block against 2048 staged: many locus ranges and many workgroups per tile), sparse loci, and the
    deep locus above (3 tiles)."""
    if name == "clustered":
        p = random_pileup(311, 200, 2, 900, 30, 12, frag_min=20, frag_max=260, dup_frac=0.03)
        return p, 200, None, "accumulate_masks", [0, 3, 9]
    if name == "sparse":
        p = random_pileup(312, 300, 2, 1500, 40, 30000, frag_min=30, frag_max=500, dup_frac=0.03)
        return p, 300, None, "accumulate_counts", None
    if name == "deep":
        return deep_locus_pileup(), 100, 64, "accumulate_tiles", [0, 2]
    if name == "deep_offdiag":
        # 300 entries of block 1 at the deep locus: the off-diagonal tile pairs that range from HBM as well
        return deep_locus_pileup(deep_other=300), 100, 64, "accumulate_tiles", [0, 2]
    if name in ("clustered_thin", "sparse_thin", "deep_thin"):
        # one more cell block of two cells with one entry each, at an early locus (flushed): the last tile, that block
        # against itself, has two row entries and as many workgroups as the pileup has locus ranges -- shares without
        # a row entry. The tile list is that tile alone.
        p, n, block, kernel, _ = pair_kernel_pileup(name[:-5])
        first = (n + 63) // 64 * 64
        at = int(p.locus_entry_off[4])  # behind the entries of locus 3
        rid = int(p.read_ids.max()) + 1
        off = p.locus_entry_off.copy()
        off[4:] += 2
        thin = FlatPileup(p.chr_locus_off, p.locus_pos, off,
                          np.insert(p.read_ids, at, [rid, rid + 1]).astype(np.uint32),
                          np.insert(p.id_base, at, [(first << 2) | 1, ((first + 1) << 2) | 2]).astype(np.uint32))
        return thin, first + 2, 64, kernel, "last"
    raise KeyError(name)
