"""Inputs that put the locus filter's kernels (secedo_amd/csrc/filter_device.hip) on their edges, shared by the CPU
tests (tests/test_filter_cpu.py: what each case must do on the oracle) and the GPU tests (tests/test_gpu_filter.py:
exact equality with the oracle).

Every case keeps id_to_pos longer than the largest group id: oracle_filter indexes id_to_pos[group] unchecked, the
kernel treats a group beyond it as outside the cluster.

  kat_pileup(theta, cp)  the decisions of the compiled reference in tests/golden/filter_kat.npz as pileups, one per
                         (theta, cell_proportion): a locus per count vector, at position row + 1. Coverage 2..259
                         reaches every threshold column, the ties of rint(coverage / 10) and the clamp to column 19.
  tie_clamp()            coverages on the ties (5, 15, 25, 45, 65, 205), on the clamp (195, 204, 205, 259, 400, 1000)
  wrap()                 loci deeper than 65535: the reference counts bases in uint16, the device hands such a locus
                         to the host, and the entries kept are counted without a wrap
  u32(shape)             17000 groups: ids that need the 32-bit id_base
  deep16()               loci of 330..1308 entries with 16-bit ids: two to six trips of the 256-entry vector loop
  tail(r)                a pileup of n_entries = r (mod 4), its last locus cut short
"""
import functools
import os

import numpy as np

from secedo_amd.pileup import FlatPileup
from tests.pileup_gen import from_rows, random_pileup

NO_POS = 16383
KAT_CELLS = 50
KAT_NAMED = ("Cov52OneDifferent", "Cov52TenDifferent", "Cov59TwoDifferent", "AtLimit", "Paradox")  # rows 0..4
KAT_NAMED_WANT = (0, 1, 0, 0, 0)


def counts_pileup(counts, n_cells, seed):
    """One locus per count vector at position index + 1: counts[b] entries of base b in a shuffled order, the groups
    dealt round-robin over n_cells from locus to locus."""
    rng = np.random.default_rng(seed)
    loci, rid = [], 0
    for l, c in enumerate(counts):
        bases = rng.permutation(np.repeat(np.arange(4), np.asarray(c, dtype=np.int64)))
        groups = (rid + np.arange(len(bases))) % n_cells
        loci.append((l + 1, list(zip(range(rid, rid + len(bases)), groups.tolist(), bases.tolist()))))
        rid += len(bases)
    return from_rows([loci])


@functools.lru_cache(maxsize=None)
def kat():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_kat.npz"))
    return z["counts"], z["theta"], z["cell_proportion"], z["significant"]


def kat_groups():
    _, theta, cp, _ = kat()
    return sorted(set(zip(theta.tolist(), cp.tolist())))


@functools.lru_cache(maxsize=None)
def kat_pileup(theta, cp):
    """-> (pileup, id_to_pos, rows of the file in locus order)"""
    counts, th, c, _ = kat()
    rows = np.flatnonzero((th == theta) & (c == cp))
    return counts_pileup(counts[rows], KAT_CELLS, 500 + cp), np.arange(KAT_CELLS, dtype=np.uint32), rows


def kat_kept_rows(theta, cp, kept_pos):
    """The file's rows that a filtered pileup of kat_pileup(theta, cp) kept."""
    return kat_pileup(theta, cp)[2][np.asarray(kept_pos, dtype=np.int64) - 1]


TIE_CLAMP_COVERAGE = (5, 15, 25, 45, 65, 195, 204, 205, 259, 400, 1000)
TIE_CLAMP_SETTINGS = ((0.01, 0), (0.01, 4), (0.05, 0), (0.05, 4))


@functools.lru_cache(maxsize=None)
def tie_clamp():
    """A minor allele of about 20 % (at least 5 entries from coverage 15 on: the integer pre-tests pass, the column's
    threshold decides)."""
    counts = [[cov - m, m, 0, 0] for cov in TIE_CLAMP_COVERAGE for m in [max(round(0.2 * cov), min(5, cov // 3))]]
    return counts_pileup(counts, KAT_CELLS, 510), np.arange(KAT_CELLS, dtype=np.uint32)


WRAP_COUNTS = ((65576, 12, 0, 0), (65588, 0, 0, 0), (40000, 30000, 0, 0), (60000, 5000, 600, 0), (45, 9, 0, 0),
               (52, 0, 0, 0))
WRAP_SETTINGS = ((0.01, 4), (0.05, 4))


@functools.lru_cache(maxsize=None)
def wrap(third_outside=False):
    i2p = np.arange(KAT_CELLS, dtype=np.uint32)
    if third_outside:  # the depth inside the cluster and the raw depth then lie on both sides of 65535
        i2p[::3] = NO_POS
    return counts_pileup(WRAP_COUNTS, KAT_CELLS, 520), i2p


U32_GROUPS = 17000
# name -> (arguments of random_pileup, theta, cell_proportion); the deep one has loci of more than 256 entries
U32_SHAPES = {"shallow": ((531, U32_GROUPS, 1, 300, 40, 500), 0.01, 4),
              "deep": ((532, U32_GROUPS, 1, 80, 300, 500), 0.05, 0)}


@functools.lru_cache(maxsize=None)
def u32(shape):
    """-> (pileup, id_to_pos, theta, cp): about half the groups outside, the others at positions below NO_POS."""
    args, theta, cp = U32_SHAPES[shape]
    p = random_pileup(*args, err=0.15)
    rng = np.random.default_rng(args[0])
    i2p = np.full(U32_GROUPS, NO_POS, dtype=np.uint32)
    inside = np.flatnonzero(rng.random(U32_GROUPS) < 0.5)
    i2p[inside] = np.arange(len(inside), dtype=np.uint32)
    return p, i2p, theta, cp


DEEP16_SETTINGS = ((0.01, 4), (0.001, 1), (0.05, 3))


@functools.lru_cache(maxsize=None)
def deep16():
    n = 200
    p = random_pileup(13, n, 2, 60, 700, 300, err=0.2)
    i2p = np.arange(n, dtype=np.uint32)
    i2p[np.random.default_rng(14).random(n) < 0.3] = NO_POS
    return p, i2p


@functools.lru_cache(maxsize=None)
def tail(r):
    """n_entries = r (mod 4) with the last locus cut short, still deep enough to be kept; the loci before it are
    whole."""
    n = 20
    p = counts_pileup([[30, 8, 0, 0], [25, 0, 0, 0], [9, 3, 0, 0], [64, 16, 0, 0]], n, 540)
    off = p.locus_entry_off.astype(np.int64)
    E = int(off[-1])
    while E % 4 != r:
        E -= 1
    off[-1] = E
    i2p = np.arange(n, dtype=np.uint32)
    i2p[3::4] = NO_POS
    return FlatPileup(p.chr_locus_off, p.locus_pos, off.astype(np.uint64), p.read_ids[:E], p.id_base[:E]), i2p


@functools.lru_cache(maxsize=None)
def expected(case, theta, cp, *key):
    """oracle_filter of a case, computed once and left unchanged. case: the name of a builder above, key: its
    arguments."""
    from oracle import bindings as ob
    p, i2p = globals()[case](*key)[:2]
    assert int(p.id_base.max() >> 2) < len(i2p)
    out = ob.oracle_filter(p, i2p, theta, cp)
    for a in out[:5]:
        a.setflags(write=False)
    return out
