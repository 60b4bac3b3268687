"""The single-entry path of the device packing at the edges of its tables (pack_device.hip, stage 1).

The path finds the chromosome of an entry from the entry's INDEX (a table of the chromosomes' first entries), makes
the dense (chromosome, read id) number twice instead of storing it, numbers the entries of repeated ids ("M entries")
with a 64-bit mask and a prefix per 64 entries instead of a word per entry, and looks a locus up for the M entries only.
Every pileup here is written by hand (tests.pileup_gen.from_rows), small, and built so that one of those pieces meets
an edge: entry counts around 4, 64 and 4096 (a thread's quad, a mask word, a workgroup's block), M entries at the first
and last bit of a word and of a block, chromosome boundaries inside a quad and on a word, empty chromosomes and loci.

Every case checks: the accessor says the single-entry path ran; the work counters equal the oracle's; the finalized
matrix is within TOL (norm-wise) of the oracle's; finalize_raw is bit-identical between device and host packing.

A read belongs to one cell: the entries of one id in one chromosome carry one group here, as in every pileup the
pileup creation writes (the reference takes a read's cell from its first entry, the device packing from each entry).
Most cases choose max_fragment_length so small that reads complete and are flushed (only flushed reads are ever paired:
without a flush counters and matrix are zero on all sides); where that cuts a read of two distant entries in two, the
cut is part of what is compared.
"""
import numpy as np
import pytest

import secedo_amd
from oracle import bindings as ob
from tests import golden_util as gu
from tests.pileup_gen import from_rows

pytestmark = pytest.mark.gpu
TOL = 1e-9
RATES = (0.01, 0.5, 0.01)
N_CELLS = 60


def split(n_entries, cuts=(), locus=48):
    """Chromosomes as lists of locus sizes: n_entries entries in loci of `locus` entries, a new chromosome at every
    entry index of `cuts` (a repeated index, 0 or n_entries: a chromosome without loci)."""
    chroms, begin = [], 0
    for end in sorted(cuts) + [n_entries]:
        sizes = [min(locus, end - b) for b in range(begin, end, locus)]
        chroms.append(sizes)
        begin = end
    return chroms


def local_ids(chroms, seed):
    """A read id per entry, unique inside its chromosome, in no order; every chromosome draws from the same small
    range, so the same id stands for different reads in different chromosomes throughout."""
    rng = np.random.default_rng(seed)
    ids = []
    for sizes in chroms:
        k = sum(sizes)
        ids.extend((5 + 2 * rng.permutation(k)).tolist())
    return ids


def rows_of(chroms, ids, seed, n_cells=N_CELLS, positions=None):
    """from_rows input: positions 1000, 1001, ... in every chromosome (they start again at each boundary)."""
    rng = np.random.default_rng(seed + 1000)
    rows, e, l = [], 0, 0
    for sizes in chroms:
        chrom, cell_of = [], {}   # the cell of a read: that of its first entry in the chromosome
        for j, k in enumerate(sizes):
            ents = []
            for i in range(k):
                rid, cell = int(ids[e + i]), int(rng.integers(0, n_cells))
                ents.append((rid, cell_of.setdefault(rid, cell), int(rng.integers(0, 4))))
            chrom.append((1000 + j if positions is None else int(positions[l]), ents))
            e += k
            l += 1
        rows.append(chrom)
    assert e == len(ids)
    return rows


def pileup(n_entries, cuts=(), locus=48, repeats=(), seed=1, chroms=None):
    """repeats: pairs (i, j) of entry indices in one chromosome -- entry j takes the id of entry i."""
    chroms = split(n_entries, cuts, locus) if chroms is None else chroms
    ids = local_ids(chroms, seed)
    for i, j in repeats:
        ids[j] = ids[i]
    return from_rows(rows_of(chroms, ids, seed))


def run(plan, p, mfl, T, via=None):
    import torch
    if via is None:
        plan.prepare(p, N_CELLS, mfl, None, T)
    else:
        plan.prepare_resident(via, N_CELLS, mfl, T)
    acc = plan.new_acc()
    plan.accumulate(acc, *RATES)
    raw = plan.finalize_raw(acc).clone()
    got = plan.finalize(acc, "ADD_MIN").cpu().numpy()
    torch.cuda.synchronize()
    return raw, got, plan.last_counts()


_HOST = {}


def check(p, mfl, T, single=True, plan=None, key=None, via=None, empty_ok=False):
    """The four checks of this file for one prepare (on `plan`, or on a fresh one). empty_ok: the pileup is too small
    for a flush, so that nothing is paired and the matrix is zero."""
    import torch
    if key is None or key not in _HOST:  # the oracle and the host packing once per pileup
        ref = ob.oracle_compute(p, N_CELLS, mfl, None, *RATES, T, "ADD_MIN")
        counts = (ob.oracle_last_updates(), ob.oracle_last_read_pairs())
        with secedo_amd.SimilarityMatrixPlan(0) as host:
            host.set_packing("host")
            raw_host = run(host, p, mfl, T)[0]
            assert not host.used_device_packing and not host.used_single_entry_path
        _HOST[key if key is not None else "last"] = (ref, counts, raw_host)
    ref, counts, raw_host = _HOST[key if key is not None else "last"]
    own = plan is None
    plan = secedo_amd.SimilarityMatrixPlan(0) if own else plan
    try:
        plan.set_packing("device")
        raw, got, got_counts = run(plan, p, mfl, T, via)
        assert plan.used_device_packing
        assert plan.used_single_entry_path == single
    finally:
        if own:
            plan.close()
    assert got_counts == counts
    assert empty_ok or counts[0] > 0
    assert gu.normwise_err(got, ref) <= TOL
    assert torch.equal(raw, raw_host)


BIG_LOCUS = 320   # entries a locus where reads join entries 4100 apart: 13 loci, inside the records' 16-locus windows


def mfl_for(n_entries):
    # positions are one apart, so max_fragment_length counts loci. 8193 entries in loci of 320: 26 loci, no read spans
    # 20 of them and the reads of the first loci complete and are flushed in the last ones; around 4096 entries (13
    # loci) and below 129 (loci of 3) a read from the first to the last entry is cut by the flushes in between
    return 20 if n_entries > 8000 else 8 if n_entries > 4000 else 5


# ---- entry counts at the tables' edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_entries", [1, 3, 4, 5, 63, 64, 65, 127, 128, 4095, 4096, 4097, 8193])
def test_entry_counts_at_the_edges(n_entries):
    """A quad, a mask word and a block each short of, at and beyond its size; 64 and 4096 end on the closing chunk. The
    first and the last entry are one read wherever that leaves fewer than half of the entries repeated."""
    repeats = [(0, n_entries - 1)] if n_entries >= 4 else []
    if n_entries > 4200:
        repeats = [(0, 4100), (4200, n_entries - 1)]
    locus = BIG_LOCUS if n_entries > 128 else 3
    check(pileup(n_entries, locus=locus, repeats=repeats, seed=n_entries), mfl_for(n_entries), 1, empty_ok=n_entries < 63)


# ---- M entries at the edges ----------------------------------------------------------------------------------------
def test_m_entries_at_word_and_block_edges():
    """Repeated ids at the first and last bit of a mask word and of a 4096-entry block and at the last entry, each
    with its partner in another word and another block; a run of 64 M entries that fills a mask word and one of 65."""
    E = 8193
    repeats = [(0, 4100), (63, 4163), (64, 4164), (4095, 8191), (200, 4096), (4090, E - 1)]
    repeats += [(128 + i, 4224 + i) for i in range(64)]   # words 2 and 66, full
    repeats += [(1000 + i, 5200 + i) for i in range(65)]
    check(pileup(E, locus=BIG_LOCUS, repeats=repeats, seed=2), mfl_for(E), 1)


@pytest.mark.parametrize("n_entries", [65, 4097])
def test_no_m_entry_at_all(n_entries):
    check(pileup(n_entries, locus=BIG_LOCUS if n_entries > 128 else 3, seed=3), mfl_for(n_entries), 1)


# ---- chromosome boundaries -----------------------------------------------------------------------------------------
def test_chromosome_boundaries_inside_quads_words_and_blocks():
    """Boundaries between the entries 4k + 1 and 4k + 2, at 4k, inside a word, on 64 and on 4096; chromosomes of one
    entry; a chromosome without loci first, two in the middle, one last; chromosomes whose loci hold no entry."""
    E = 4300
    cuts = [0, 2, 8, 30, 64, 65, 65, 65, 130, 4096, 4097, E]
    chroms = split(E, cuts)
    assert [sum(c) for c in chroms] == [0, 2, 6, 22, 34, 1, 0, 0, 65, 3966, 1, 203, 0]
    chroms[6] = [0, 0]      # loci, but no entry
    chroms[12] = [0]
    # reads of two entries inside the long chromosomes, some across a quad that straddles a boundary's neighbourhood
    repeats = [(8, 29), (66, 129), (131, 4095), (140, 300), (4098, 4299), (4100, 4200)]
    check(pileup(E, repeats=repeats, seed=4, chroms=chroms), 30, 1)


def test_the_same_read_id_in_two_chromosomes():
    """Two single-entry reads with one id in two chromosomes; an id twice in A and once in B (an M read in A, an S
    entry in B); the smallest and the largest id of a chromosome as the repeated one."""
    chroms = [[5] * 20, [5] * 20, [5] * 4]
    ids = local_ids(chroms, 5)          # A, B and the third chromosome draw the same ids 5, 7, ...
    a = ids[:100]
    assert sorted(a) == sorted(ids[100:200])
    lo, hi = a.index(min(a)), a.index(max(a))
    ids[(lo + 37) % 100] = min(a)       # the smallest id of A twice (another locus: five entries a locus)
    ids[(hi + 41) % 100] = max(a)       # the largest
    b = ids[100:200]
    ids[100 + (b.index(max(b)) + 43) % 100] = max(b)
    p = from_rows(rows_of(chroms, ids, 5))
    check(p, 10, 1)


def test_more_chromosomes_than_the_lds_tables_hold():
    """1100 chromosomes of two loci with 0 to 5 entries each (the per-chromosome tables from global memory): boundaries
    at every offset inside a quad, empty chromosomes, chromosomes of one entry, reads across a chromosome's two loci."""
    rng = np.random.default_rng(6)
    chroms = [[int(rng.integers(0, 6)), int(rng.integers(0, 6))] for _ in range(1100)]
    chroms[0], chroms[1], chroms[500], chroms[501], chroms[1099] = [0, 0], [1, 0], [0, 0], [0, 1], [0, 0]
    ids = local_ids(chroms, 6)
    e = 0
    for c, (a, b) in enumerate(chroms):
        if c % 7 == 0 and a and b:
            ids[e + a] = ids[e]         # the first entry of both loci: one read
        e += a + b
    # (positions 1000 and 1002 in every chromosome: at its second locus the reads of the first are complete)
    check(from_rows(rows_of(chroms, ids, 6, positions=[1000, 1002] * len(chroms))), 2, 1)


# ---- empty loci ----------------------------------------------------------------------------------------------------
def test_loci_without_entries():
    """At the start, at the end, at a multiple of 64 loci and as a run of 70; in a second chromosome as well."""
    E = 4097
    first = [0] + [8] * 63 + [0] * 70 + [8] * 64 + [0] + [8] * 200
    n_first = sum(first)
    second = [0, 0] + split(E - n_first, locus=8)[0] + [0]
    repeats = [(0, 70), (500, 900), (n_first, n_first + 9), (n_first + 100, E - 1)]
    check(pileup(E, repeats=repeats, seed=7, chroms=[first, second]), 100, 1)


# ---- positions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("step", [0, -5])
def test_positions_that_do_not_increase_are_refused(where, step):
    """Equal or decreasing positions inside a chromosome raise the error they raised when k_entry_locus checked them,
    on a fresh plan (read-back 1) and on one that has packed before (read-back 1b); the same positions across a
    chromosome boundary are accepted."""
    chroms = split(400, cuts=[200], locus=5)
    n_loci = sum(len(c) for c in chroms)
    ids = local_ids(chroms, 8)
    good = from_rows(rows_of(chroms, ids, 8))   # (1000, 1001, ... in both chromosomes: a decrease at the boundary)
    pos = np.concatenate([1000 + 10 * np.arange(len(c)) for c in chroms])
    l = {"first": 0, "middle": len(chroms[0]) + 3, "last": n_loci - 2}[where]
    pos[l + 1] = pos[l] + step
    bad = from_rows(rows_of(chroms, ids, 8, positions=pos))
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        plan.set_packing("device")
        with pytest.raises(secedo_amd.SecedoError, match="strictly increasing"):
            plan.prepare(bad, N_CELLS, 1000, None, 1)
        check(good, 10, 1, plan=plan, key="positions")
        with pytest.raises(secedo_amd.SecedoError, match="strictly increasing"):
            plan.prepare(bad, N_CELLS, 1000, None, 1)
    # across the boundary alone: equal and decreasing positions are fine
    first = 1000 + 10 * np.arange(len(chroms[0]))
    pos = np.concatenate([first, first[-1] + step + 10 * np.arange(len(chroms[1]))])
    check(from_rows(rows_of(chroms, ids, 8, positions=pos)), 100, 1)


# ---- the route given up --------------------------------------------------------------------------------------------
def half_repeated(n_pairs):
    """200 entries in loci of 4, the first 2 * n_pairs of them reads of two entries (four loci apart)."""
    repeats = []
    for k in range(n_pairs):
        blk, i = divmod(k, 16)
        repeats.append((32 * blk + i, 32 * blk + 16 + i))
    chroms = split(200, locus=4)
    ids = local_ids(chroms, 9)
    for j, v in ((198, min(ids)), (199, max(ids))):   # the same id space whatever is repeated: no entry below takes
        i = ids.index(v)                             # the place of the smallest or the largest id
        ids[i], ids[j] = ids[j], ids[i]
    for i, j in repeats:
        ids[j] = ids[i]
    return from_rows(rows_of(chroms, ids, 9))


def test_exactly_half_of_the_entries_repeated_stays_on_the_path():
    check(half_repeated(50), 10, 1)


def test_more_than_half_repeated_takes_the_general_path():
    check(half_repeated(51), 10, 1, single=False)


def test_one_plan_sparse_clustered_sparse():
    """The entry -> locus table made late (the route given up behind read-back 1b), buffers the route never sized, a
    handle that has stopped trying (the table made up front) and tries again at its sixteenth call."""
    sparse, clustered = half_repeated(10), half_repeated(60)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        check(sparse, 10, 1, plan=plan, key="sparse")
        check(clustered, 10, 1, single=False, plan=plan, key="clustered")
        for _ in range(15):
            check(sparse, 10, 1, single=False, plan=plan, key="sparse")
        check(sparse, 10, 1, plan=plan, key="sparse")
    with secedo_amd.SimilarityMatrixPlan(0) as plan:   # a fresh plan meets the clustered pileup first
        check(clustered, 10, 1, single=False, plan=plan, key="clustered")
        check(sparse, 10, 1, single=False, plan=plan, key="sparse")


# ---- read ids that are not 16-byte aligned ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_entries,cuts", [(65, [2, 30]), (4097, [2, 64, 4096])])
def test_read_ids_off_the_16_byte_grid(n_entries, cuts):
    """prepare_resident takes whatever device pointer the caller has: the ids one word into an allocation (the
    one-by-one loads of k_id_range, k_id_store and k_id_check)."""
    import torch
    repeats = [(3, 28), (31, n_entries - 2)] if n_entries < 100 else [(70, 4000), (100, 4095)]
    p = pileup(n_entries, cuts=cuts, locus=3 if n_entries < 100 else 48, repeats=repeats, seed=10)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, None, N_CELLS)
        shifted = torch.empty(n_entries + 1, dtype=res["rid"].dtype, device=res["rid"].device)
        shifted[1:] = res["rid"]
        res["rid"] = shifted[1:]
        assert res["rid"].data_ptr() % 16 == 4
        check(p, 5 if n_entries < 100 else 30, 1, plan=plan, via=res)
