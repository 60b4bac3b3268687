"""Synthetic pileup of a clone tree ((A1, A2), B) for the divide_cluster tests and benchmark.

Cells 0 .. nB-1 are clone B, then A1, then A2 (nA1 = nA2 = (n - nB) / 2). Every locus is covered by each cell
with a per-locus probability (uniform in [cov_lo, cov_hi]); one distinct read per entry. A locus is
  * an A|B locus (fraction f_ab): A cells read base 0, B cells base 1,
  * an A1|A2 locus (fraction f_a12): A1 cells base 0, A2 cells base 3, B cells base 0,
  * otherwise uninformative: base 2 everywhere,
and each base is replaced by a uniform random one with probability `error`. The last `n_mixed` cells are
mixtures: each of their entries takes the base of a random A1 or B cell, so no clone explains them; their
per-locus coverage probability is scaled by `mixed_cov`. Returns a
FlatPileup (group ids = cell ids) and the planted labels (0 = B, 1 = A1, 2 = A2, 3 = mixed).
"""
import numpy as np

from secedo_amd.pileup import FlatPileup


def clone_tree(n_cells=300, n_b=None, n_loci=6000, f_ab=0.3, f_a12=0.3, cov_lo=0.05, cov_hi=0.3, error=0.01,
               seed=1, n_mixed=0, mixed_cov=1.0):
    rng = np.random.default_rng(seed)
    n_b = (n_cells - n_mixed) // 2 if n_b is None else n_b
    n_a = n_cells - n_mixed - n_b
    truth = np.zeros(n_cells, dtype=np.int64)
    truth[n_b:n_b + n_a // 2] = 1
    truth[n_b + n_a // 2:n_b + n_a] = 2
    truth[n_b + n_a:] = 3
    kind = rng.random(n_loci)
    kind = np.where(kind < f_ab, 1, np.where(kind < f_ab + f_a12, 2, 0))
    cov = rng.uniform(cov_lo, cov_hi, n_loci)
    scale = np.where(truth == 3, mixed_cov, 1.0)
    covered = rng.random((n_loci, n_cells)) < cov[:, None] * scale[None, :]
    base = np.full((n_loci, n_cells), 2, dtype=np.int8)
    base[kind == 1] = np.where(truth[None, :] == 0, 1, 0)
    base[kind == 2] = np.where(truth[None, :] == 2, 3, 0)
    if n_mixed:
        like_b = rng.random((n_loci, n_mixed)) < 0.5
        base[:, n_b + n_a:] = np.where(like_b, base[:, :1], base[:, n_b:n_b + 1])
    err = rng.random((n_loci, n_cells)) < error
    base = np.where(err, rng.integers(0, 4, (n_loci, n_cells), dtype=np.int8), base)
    loc, cell = np.nonzero(covered)  # row-major: loci ascending, cells ascending within a locus
    idb = (cell.astype(np.uint32) << 2) | base[loc, cell].astype(np.uint32)
    off = np.zeros(n_loci + 1, dtype=np.uint64)
    off[1:] = np.cumsum(covered.sum(axis=1))
    p = FlatPileup(np.asarray([0, n_loci], dtype=np.uint32), np.arange(n_loci, dtype=np.uint32), off,
                   np.arange(len(idb), dtype=np.uint32), idb.astype(np.uint32))
    return p, truth


def purity(labels, truth):
    """Fraction of the clone cells (mixed cells not counted) whose label is the majority label of their planted
    clone, with distinct clones required to have distinct majority labels (0 otherwise)."""
    labels = np.asarray(labels)
    majors, good = [], 0
    for c in np.unique(truth[truth < 3]):
        vals, counts = np.unique(labels[truth == c], return_counts=True)
        majors.append(vals[np.argmax(counts)])
        good += counts.max()
    if len(set(majors)) != len(majors):
        return 0.0
    return good / int((truth < 3).sum())
