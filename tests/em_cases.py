"""Inputs that put the EM refinement's kernels (secedo_amd/csrc/em_device.hip) on their edges, shared by the CPU
tests (tests/test_em_cpu.py: the conditions below) and the GPU tests (tests/test_gpu_em.py: parity with the oracle).

CASES maps a name to (pileup, id_to_pos, theta, start vector). The conditions every case must meet, asserted on the
CPU so that a badly chosen seed fails there: the oracle settles within MAX_ITER iterations, without a NaN, and the
high-precision restatement (tests/em_ref.py) stays MARGIN away from the edge of the "nothing moved by 1e-2" test in
every iteration, so the iteration count is a property of the input and the GPU owes it exactly.

  boundary_n<N>_<start>  two clones over three chromosomes (the middle one empty), locus depths DEPTHS: nothing, one
                         entry, a wave of 64 lanes less / exactly / more than full, two and four waves; every third
                         locus covered by the lower clone only. At most ACTIVE cells have entries: at N = 1023 and
                         1025 (the E-step's 1024 lanes, one short and one over) most cells have none.
                         Starts: exact 0 / 1 by clone, all ones, all zeros, all 0.5, 0 / 1 with every fifth cell 0.5.
  one_cell_*             n_cells = 1, with two entries and with an empty pileup
  perm16_*, perm32_*     id_to_pos a permutation of all positions, and one inside each clone, on a pileup with
                         16-bit ids and on one whose at most 100 groups have ids spread above 0xFFFF: the centres
                         weigh by prob[group id], the sums land at id_to_pos[group id]
"""
import numpy as np

from secedo_amd.pileup import FlatPileup
from tests.pileup_gen import from_rows, random_pileup

DEPTHS = (0, 1, 63, 64, 65, 0, 127, 128, 129, 2, 3, 256, 257, 40, 40, 40, 0)
BOUNDARY_N = (2, 7, 66, 1023, 1025)
STARTS = ("clones", "ones", "zeros", "half", "clones_fifth_half")
ACTIVE = 66
THETA = 1e-3
MAX_ITER, MARGIN = 40, 1e-6


def boundary_pileup(n_cells, seed=73):
    rng = np.random.default_rng(seed)
    half = n_cells // 2  # cells [0, half) are the lower clone
    lower = np.arange(min(half, ACTIVE // 2))
    upper = half + np.arange(min(n_cells - half, ACTIVE // 2))
    loci, rid = [], 0
    for l, depth in enumerate(DEPTHS):
        ref = int(rng.integers(0, 4))
        differs = rng.random() < 0.5  # the clones differ at about half the loci and 20 % of the bases are noise:
        cells = lower if l % 3 == 2 else np.concatenate([lower, upper])
        ents = []
        for g in rng.choice(cells, size=depth):
            b = ref if g < half or not differs else (ref + 1) & 3  # a clone-wise start takes up to 31 iterations
            if rng.random() < 0.2:
                b = int(rng.integers(0, 4))
            ents.append((rid, int(g), b))
            rid += 1
        loci.append((1000 + 10 * l, ents))
    return from_rows([loci[:9], [], loci[9:]])


def start_vector(kind, n_cells):
    clones = (np.arange(n_cells) >= n_cells // 2).astype(np.float64)
    if kind == "clones":
        return clones
    if kind == "ones":
        return np.ones(n_cells)
    if kind == "zeros":
        return np.zeros(n_cells)
    if kind == "half":
        return np.full(n_cells, 0.5)
    assert kind == "clones_fifth_half"
    clones[::5] = 0.5
    return clones


def _in_clone_permutation(rng, is_upper):
    perm = np.arange(len(is_upper), dtype=np.uint32)
    for side in (False, True):
        where = np.flatnonzero(is_upper == side)
        perm[where] = where[rng.permutation(len(where))]
    return perm


def _perm16(kind, seed=81):
    n = 60
    p = random_pileup(seed, n, 2, 150, 12, 300, err=0.1)
    rng = np.random.default_rng(seed + 1)
    is_upper = np.arange(n) >= n // 2
    i2p = rng.permutation(n).astype(np.uint32) if kind == "full" else _in_clone_permutation(rng, is_upper)
    prob = is_upper.astype(np.float64)
    prob[rng.random(n) < 0.2] = 0.5
    return p, i2p, THETA, prob


def _perm32(kind, seed=91):
    groups = 100
    p = random_pileup(seed, groups, 2, 150, 12, 300, err=0.1)
    rng = np.random.default_rng(seed + 1)
    ids = 0x10000 + 700 * np.arange(groups, dtype=np.uint32) + rng.integers(0, 700, groups).astype(np.uint32)
    n_cells = int(ids.max()) + 1 + 37
    p = FlatPileup(p.chr_locus_off, p.locus_pos, p.locus_entry_off, p.read_ids,
                   (ids[p.id_base >> 2] << np.uint32(2)) | (p.id_base & np.uint32(3)))
    is_upper = np.arange(n_cells) >= ids[groups // 2]  # ids ascend: random_pileup's upper clone is the upper half
    i2p = rng.permutation(n_cells).astype(np.uint32) if kind == "full" else _in_clone_permutation(rng, is_upper)
    return p, i2p, THETA, is_upper.astype(np.float64)


def _build():
    c = {}
    for n in BOUNDARY_N:
        p = boundary_pileup(n)
        for kind in STARTS:
            c["boundary_n%d_%s" % (n, kind)] = (p, np.arange(n, dtype=np.uint32), THETA, start_vector(kind, n))
    one = np.arange(1, dtype=np.uint32)
    c["one_cell_two_entries"] = (from_rows([[(5, [(0, 0, 1), (1, 0, 2)])]]), one, THETA, np.array([0.5]))
    c["one_cell_empty"] = (from_rows([[]]), one, THETA, np.array([0.5]))
    for kind in ("full", "in_clone"):
        c["perm16_" + kind] = _perm16(kind)
        c["perm32_" + kind] = _perm32(kind)
    for p, i2p, _, prob in c.values():
        for a in (p.chr_locus_off, p.locus_pos, p.locus_entry_off, p.read_ids, p.id_base, i2p, prob):
            a.setflags(write=False)
    return c


CASES = _build()
BOUNDARY = tuple(name for name in CASES if name.startswith("boundary_"))

_oracle = {}


def oracle(name):
    """oracle_em of a case, computed once: (probabilities, iterations)."""
    if name not in _oracle:
        from oracle import bindings as ob
        p, i2p, theta, prob = CASES[name]
        got, it = ob.oracle_em(p, i2p, theta, prob)
        got.setflags(write=False)
        _oracle[name] = (got, it)
    return _oracle[name]
