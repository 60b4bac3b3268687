"""The launch chain of the device packing's single-entry route (pack_device.hip) where a one-workgroup kernel or a fill
became part of the kernel in front of it: the id bases made by the last workgroup of k_id_range, read-back 1b published
by the first workgroup of k_compact_m (which also zeroes the M entries' counters), read-back 2 by the last workgroup
of k_read_info, pair bound, read-back 3 and the list blocks' scan in one kernel (k_records_tail); k_ranges_compact
copying all segments in one sweep on the side stream beside the placing pass; the ranks, the chromosomes' first ranks
and the per-read lists in one kernel (k_ranks_runs). "The last workgroup" draws tickets that must be back at zero for
the next launch, whatever grid that has: the cases on one handle are about that.

The yardstick of every case (check): the device packing must take the single-entry route in one counting attempt and
equal the host packing (pack_host.cpp) and its own serial twin (SECEDO_PACK_OVERLAP=0) in the work counters, the sizes,
the pair kernel and the raw matrix bit for bit; the two device routes also in the flagged entries' lists.

Pileups are written by hand: loci of one entry each (the raw entries are the loci) unless a case says otherwise, the M
entries -- entries of a read id that occurs more than once -- are placed where a case wants them. An id that repeats
has at least two entries, so one M entry cannot occur: where the request names n_m = 1 the cases take 0, 2 and 3.

rocPRIM's items per scan tile are not visible from here (no entry point of the library reports its scan config). The
cases that want a read across a tile boundary put a read across EVERY position instead: a leading three-entry read,
then two-entry reads (the reads stand in the sorted order in the order of their first entries) make every even
position the inside of a read, two-entry reads alone every odd one, up to 8200 M entries, so whatever the tile length,
even or odd, some case has a read across each of its boundaries; the all-triples layout adds triples across the
boundaries that are no multiple of three.

The locus ranges are compared with closed forms and with the serial twin, not with the host packing's range_off: the
host cuts greedily over the whole pileup with the geometry's limits, the device inside segments whose length the tile
plan may shorten, so the two legitimately differ in where they cut (and agree in every result, which is compared).
"""
import ctypes as C

import numpy as np
import pytest

import secedo_amd
from secedo_amd import _lib
from secedo_amd.pileup import FlatPileup
from secedo_amd.similarity_matrix import PackingRoute
from tests.pileup_gen import from_rows
from tests.test_gpu_pack_overlap import (SPECS, assert_lists_equal, assert_same, edge_pileup, host_result, pileup,
                                         result_of)

pytestmark = pytest.mark.gpu

ONE_COUNTING = PackingRoute(1, False, False, False)
CELLS = 128


def ranges_of(plan):
    """(num_ranges, max_range_span, cap_loci, range_off[0 .. num_ranges]) of the prepared pileup"""
    n, span, cap = C.c_uint32(), C.c_uint32(), C.c_uint32()
    off = np.zeros(plan.num_loci + 2, np.uint32)
    _lib.check(_lib.lib().secedo_simmat_debug_ranges(plan._h, C.byref(n), C.byref(span), C.byref(cap), _lib.ptr(off)))
    return n.value, span.value, cap.value, off[:n.value + 1].copy()


def pack(p, cells, mfl, threads, mode, plan=None, block=0):
    own = plan is None
    plan = secedo_amd.SimilarityMatrixPlan(0) if own else plan
    try:
        plan.set_packing(mode)
        plan.prepare(p, cells, mfl, None, threads, block_cells=block)
        out = dict(device=plan.used_device_packing, single=plan.used_single_entry_path, route=plan.packing_route,
                   ranges=ranges_of(plan))
        out["same"], out["lists"] = result_of(plan)
        return out
    finally:
        if own:
            plan.close()


def assert_ranges_sound(r, n_loci, what):
    n, span, cap, off = r
    assert n >= 1 and len(off) == n + 1, what
    assert off[0] == 0 and off[-1] == n_loci, (what, off[:4], off[-4:])
    d = np.diff(off.astype(np.int64))
    assert np.all(d > 0), what
    assert span == d.max(), (what, span, d.max())


def check(p, cells, mfl, threads, monkeypatch, single=True, plan=None, block=0, host=None, route=ONE_COUNTING):
    """The yardstick. Returns the device packing's result. route: what `plan` must report (a fresh handle, as the
    serial twin always is, takes one counting attempt)."""
    host = host or pack(p, cells, mfl, threads, "host", block=block)
    assert not host["device"]
    monkeypatch.delenv("SECEDO_PACK_OVERLAP", raising=False)
    dev = pack(p, cells, mfl, threads, "device", plan=plan, block=block)
    monkeypatch.setenv("SECEDO_PACK_OVERLAP", "0")
    twin = pack(p, cells, mfl, threads, "device", block=block)
    monkeypatch.delenv("SECEDO_PACK_OVERLAP", raising=False)
    for name, d in (("device", dev), ("serial twin", twin)):
        assert d["device"] and d["route"] == (route if name == "device" else ONE_COUNTING), (name, d["route"])
        assert d["single"] == single, name  # a case that falls to another route proves nothing
        assert_same(d["same"], host["same"], name)
        assert_ranges_sound(d["ranges"], p.n_loci, name)
    assert_lists_equal(dev["lists"], twin["lists"], "lists")
    assert dev["ranges"][:3] == twin["ranges"][:3] and np.array_equal(dev["ranges"][3], twin["ranges"][3])
    return dev


def chain_pileup(n, reads=(), chr_loci=24, cells=CELLS, empty_chr=(), extra=None):
    """n loci of one entry each, 10 positions apart in chromosomes of chr_loci loci; every entry a read of its own but
    for `reads`: tuples of loci that share one read id (and its cell). extra: locus -> bases of further entries of
    the locus' read AT that locus (mates: the duplicate-position rule). empty_chr: chromosome indices (in the final
    numbering) that hold no locus."""
    read_of, rid = {}, 0
    for loci in reads:
        for l in loci:
            assert l not in read_of and 0 <= l < n
            read_of[l] = ("r", loci[0])
    ids = {}
    rows = []
    for i in range(n):
        if i % chr_loci == 0:
            while len(rows) in empty_chr:
                rows.append([])
            rows.append([])
        key = read_of.get(i, ("s", i))
        if key not in ids:
            ids[key] = (3 + 5 * rid, (len(ids) * 37) % cells)
            rid += 1
        r, cell = ids[key]
        ents = [(r, cell, i & 3)] + [(r, cell, b) for b in (extra or {}).get(i, ())]
        rows[-1].append((10 * (i % chr_loci) + 1, ents))
    while len(rows) in empty_chr:
        rows.append([])
    return from_rows(rows)


def spread_pairs(n, k, chr_loci=24, first=1):
    """k two-locus reads (i, i + 1) spread over the loci first .. n - 1, inside their chromosomes"""
    out, step = [], max(3, (n - first - 2) // max(k, 1))
    i = first
    if not k:
        return out
    while len(out) < k:
        if i // chr_loci == (i + 1) // chr_loci:
            out.append((i, i + 1))
            i += step
        else:
            i += 1
    assert out[-1][1] < n
    return out


# ---- flag count + scan, the numbering of the M entries ------------------------------------------
@pytest.mark.parametrize("n_m", [0, 2, 3, 63, 64, 65, 66])
def test_m_entries_numbering_0_to_66(n_m, monkeypatch):
    """One flag block of 600 entries with n_m M entries (two-entry reads, an odd number with one three-entry read)."""
    reads = [(2, 3, 4)] if n_m % 2 else []
    reads += spread_pairs(600, (n_m - 3 * len(reads)) // 2, first=6)
    p = chain_pileup(600, reads)
    assert p.n_entries == 600
    dev = check(p, CELLS, 50, 1, monkeypatch)
    assert dev["same"]["num_reads"] == 600 - n_m + len(reads)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_flag_blocks_one_two_and_three(n, monkeypatch):
    """Raw entries of one, two and three 4096-entry flag blocks, the last block holding a single entry; M entries
    at the very end, across the 4096 boundary and one read in 192 loci (tests.test_gpu_pack_overlap.edge_pileup)."""
    p = edge_pileup(n)
    assert p.n_entries == n
    check(p, CELLS, 50, 1, monkeypatch, block=128)


def test_three_packings_on_one_handle_and_a_changing_grid(monkeypatch):
    """Nothing is left behind on a handle (the mailbox's sequence numbers, the counters k_compact_m zeroes): the same
    pileup three times on one handle, then a handle that alternates between a pileup of one flag block and one of
    three. The larger pileup behind the smaller one finds the handle's assumed id space too small: that attempt is
    void (read-back 1b says so) and is repeated without the assumption."""
    one, three = edge_pileup(4000), edge_pileup(8193)
    hosts = {4000: pack(one, CELLS, 50, 1, "host", block=128), 8193: pack(three, CELLS, 50, 1, "host", block=128)}
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        for _ in range(3):
            check(three, CELLS, 50, 1, monkeypatch, plan=plan, block=128, host=hosts[8193])
        for p in (one, three, one, three, one):
            check(p, CELLS, 50, 1, monkeypatch, plan=plan, block=128, host=hosts[p.n_entries],
                  route=PackingRoute(2, False, True, False) if p is three else ONE_COUNTING)


# ---- publishing: each read-back seen through what it decides, mailbox and plain copies -----------------------
def both_readbacks(monkeypatch, fn):
    monkeypatch.delenv("SECEDO_PACK_READBACK", raising=False)
    a = fn()
    monkeypatch.setenv("SECEDO_PACK_READBACK", "memcpy")
    try:
        b = fn()
    finally:
        monkeypatch.delenv("SECEDO_PACK_READBACK", raising=False)
    assert_same(a["same"], b["same"], "mailbox against memcpy")
    assert_lists_equal(a["lists"], b["lists"], "mailbox against memcpy")
    assert a["single"] == b["single"] and a["route"] == b["route"]
    return a


@pytest.mark.parametrize("n_m", [200, 202])
def test_read_back_1b_decides_whether_the_route_is_abandoned(n_m, monkeypatch):
    """400 entries: 202 M entries are more than half (n_m * 2 > E) and the route is given up for the general counting
    route, 200 are not. Both in one counting attempt, both equal to the host packing."""
    p = chain_pileup(400, spread_pairs(400, n_m // 2, chr_loci=400), chr_loci=400)
    assert p.n_entries == 400
    both_readbacks(monkeypatch, lambda: check(p, CELLS, 5000, 1, monkeypatch, single=n_m * 2 <= 400))


def test_read_back_2_sees_a_read_longer_than_max_fragment_length(monkeypatch):
    """`sparse` with max_fragment_length 60: reads span more, long_reads is raised and the cut iteration runs (the
    number of reads differs from that under 1000)."""
    p, cells = pileup("sparse"), SPECS["sparse"][0]
    host = host_result("sparse", 60, 0)[0]
    assert host["num_reads"] != host_result("sparse", 1000, 0)[0]["num_reads"]
    dev = both_readbacks(monkeypatch, lambda: check(p, cells, 60, 2, monkeypatch))
    assert_same(dev["same"], host, "host")


def deep_cell_pileup(deep=300, seed=5):
    """60 loci of 20 to 60 single-entry reads over 100 cells, and at locus 20 one cell with 300 entries: its sum of
    squares (90 000) is beyond the count tile's 65 536, so the ranges, cut for the count tile, are cut again.
    deep=0: the same without them (the count tile is taken)."""
    rng = np.random.default_rng(seed)
    rows, rid = [], 0
    for l in range(60):
        cellsl = [int(c) for c in rng.integers(0, 100, size=int(rng.integers(20, 60)))]
        if l == 20:
            cellsl += [7] * deep
        ents = []
        for c in cellsl:
            ents.append((rid, c, int(rng.integers(0, 4))))
            rid += 1
        rows.append((500 + 40 * l, ents))
    for k in range(4):
        rows.append((50000 + 3000 * k, [(rid + k, 0, 0)]))
    return from_rows([rows])


def test_read_back_3_sees_a_pair_bound_that_forbids_the_count_tile(monkeypatch):
    p = deep_cell_pileup()
    assert check(deep_cell_pileup(0), 100, 1000, 2, monkeypatch)["same"]["pair_kernel"] == "accumulate_counts"
    dev = both_readbacks(monkeypatch, lambda: check(p, 100, 1000, 2, monkeypatch))
    assert dev["same"]["pair_kernel"] != "accumulate_counts"
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        plan.set_packing("device")
        plan.prepare(p, 100, 1000, None, 2)
        assert plan.pair_bound >= 65536


# ---- k_ranges_compact ----------------------------------------------------------------------------------------------
def two_cell_pileup(n_loci, empty=(), cells=2):
    """two cells (or `cells`, taken in turn), one entry per locus (none at the loci of `empty`: half-open (begin, end)), every entry its own read:
    no entry limit ever binds, so the ranges are the segments"""
    has = np.ones(n_loci, bool)
    for a, b in empty:
        has[a:b] = False
    off = np.concatenate([[0], np.cumsum(has)]).astype(np.uint64)
    e = int(off[-1])
    cells = (np.arange(e) % cells).astype(np.uint32)
    return FlatPileup(np.array([0, n_loci], np.uint32), (1000 + 7 * np.arange(n_loci)).astype(np.uint32), off,
                      (11 + 3 * np.arange(e)).astype(np.uint32), (cells << 2) | (np.arange(e) % 4).astype(np.uint32))


def settled_two_cell_pileup(loci_of, empty_of=None):
    """The two-cell pileup of loci_of(segment length) loci, where the segment length is the one the tile plan chooses
    for that very pileup (it shortens the segments with the entries per locus and the number of loci: not a constant
    of the test). Packed until the two agree."""
    cap = 128
    for _ in range(6):
        p = two_cell_pileup(loci_of(cap), empty_of(cap) if empty_of else ())
        with secedo_amd.SimilarityMatrixPlan(0) as plan:
            plan.set_packing("device")
            plan.prepare(p, 2, 100, None, 1)
            got = ranges_of(plan)[2]
        if got == cap:
            return p, cap
        cap = got
    raise AssertionError("the segment length did not settle")


def check_segments_are_ranges(p, want_cap, monkeypatch, cells=2):
    dev = check(p, cells, 100, 1, monkeypatch)
    n, span, cap, off = dev["ranges"]
    assert cap == want_cap
    want = np.append(np.arange(0, p.n_loci, cap), p.n_loci).astype(np.uint32)
    assert n == len(want) - 1 and np.array_equal(off, want), (n, len(want) - 1, off[:4], off[-4:])
    assert span == min(cap, p.n_loci)
    return dev


@pytest.mark.parametrize("which", ["one segment", "one locus more", "two segments less one"])
def test_ranges_at_the_segment_edges(which, monkeypatch):
    loci_of = {"one segment": lambda cap: cap, "one locus more": lambda cap: cap + 1,
               "two segments less one": lambda cap: 2 * cap - 1}[which]
    p, cap = settled_two_cell_pileup(loci_of)
    dev = check_segments_are_ranges(p, cap, monkeypatch)
    assert dev["ranges"][0] == (1 if which == "one segment" else 2)


def test_ranges_over_a_stretch_of_loci_without_entries(monkeypatch):
    """A stretch of loci without entries, longer than a segment. A segment of loci always yields a range; the segments
    that yield none are the trailing ones of the limit set with the longer segments, which every case here has as soon
    as the two sets differ."""
    p, cap = settled_two_cell_pileup(lambda cap: 5 * cap - 3, lambda cap: [(cap - 5, 2 * cap + 9)])
    assert np.all(np.diff(p.locus_entry_off[cap - 5:2 * cap + 10].astype(np.int64)) == 0)
    check_segments_are_ranges(p, cap, monkeypatch)


def test_ranges_with_trailing_segments_of_no_range(monkeypatch):
    """Segments that yield zero ranges in the limit set k_ranges_compact picks. A segment that holds loci always yields
    a range, whatever its loci hold, so an empty segment in the middle (one that shares its begin with its successor)
    cannot occur; the empty ones are the trailing segments of the set with the LONGER segments, because the grid of
    k_ranges_segment is sized by the shorter. Here that is the picked set: 128 cells in one 128-cell block with one
    entry per locus keep the count tile's full 8190-locus segments (12288 staged entries are never reached) against
    2046 for the plain limits, so 2 * 8190 + 7 loci are cut in 9 segments of which the count tile's last 6 are empty."""
    p = two_cell_pileup(2 * 8190 + 7, cells=128)
    dev = check_segments_are_ranges(p, 8190, monkeypatch, cells=128)
    assert dev["same"]["block_cells"] == 128 and dev["same"]["pair_kernel"] == "accumulate_counts"
    assert dev["ranges"][0] == 3


def test_ranges_of_more_than_256_segments(monkeypatch):
    """a second sweep of the workgroup: 257 segments and five loci"""
    p, cap = settled_two_cell_pileup(lambda cap: 257 * cap + 5)
    dev = check_segments_are_ranges(p, cap, monkeypatch)
    assert dev["ranges"][0] == 258


def test_ranges_of_a_synthetic_pileup_are_sound(monkeypatch):
    """entry limits bind: several ranges per segment, none across a segment's edge"""
    p, cells = pileup("sparse"), SPECS["sparse"][0]
    dev = check(p, cells, 1000, 2, monkeypatch, host=dict(device=False, same=host_result("sparse", 1000, 0)[0]))
    n, span, cap, off = dev["ranges"]
    for a, b in zip(off[:-1], off[1:]):
        assert a // cap == (b - 1) // cap, (a, b, cap)


# ---- the fused ranks / runs kernel and the scans ---------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one", "two", "22 with empty ones"])
def test_chromosomes_first_ranks(layout, monkeypatch):
    """One chromosome, two, and 22 with an empty one in the middle and one at the end (rbeg, chr_entry)."""
    if layout == "one":
        p = chain_pileup(300, spread_pairs(300, 20, chr_loci=300), chr_loci=300)
    elif layout == "two":
        p = chain_pileup(300, spread_pairs(300, 20, chr_loci=150), chr_loci=150)
    else:
        p = chain_pileup(20 * 24, spread_pairs(480, 40), empty_chr=(9, 21))
        assert len(p.chr_locus_off) == 23 and p.chr_locus_off[9] == p.chr_locus_off[10]
        assert p.chr_locus_off[21] == p.chr_locus_off[22] == 480
    check(p, CELLS, 50, 1, monkeypatch)


def straddling_reads(n_m):
    """a leading three-entry read, two-entry reads, and a closing three-entry read if n_m is even: sorted positions
    3 + 2k, 4 + 2k hold one read, every even position is inside a read. As (size, first locus) in order."""
    sizes = [3] + [2] * ((n_m - 3) // 2 if n_m % 2 else (n_m - 6) // 2) + ([3] if n_m % 2 == 0 else [])
    assert sum(sizes) == n_m
    return sizes


def mates_pileup(sizes, kinds=3, gap=3):
    """Every read of `sizes` entries stands at ONE locus (mates at one position: the duplicate rule decides). Of the
    pairs every `kinds`-th has equal bases (the second is ignored), the others different ones (both go); a triple is
    base b, another base, a third (the first two go, the third is appended). Between the reads' loci `gap - 1` loci
    of single-entry reads, so that no more than half of the entries are M entries."""
    reads, extra, l = [], {}, 2
    for k, size in enumerate(sizes):
        b = l & 3
        if size == 3:
            extra[l] = [(b + 1) & 3, (b + 2) & 3]
        else:
            extra[l] = [b if k % kinds == 0 else (b + 1) & 3]
        l += gap
    n = l + 2
    p = chain_pileup(n, reads, chr_loci=n, extra=extra)
    n_m = sum(sizes)
    assert p.n_entries == n + n_m - len(sizes) and 2 * n_m <= p.n_entries
    return p


@pytest.mark.parametrize("n_m", [3, 254, 255, 256, 257, 258, 1023, 1024, 1025, 2049, 2561, 3073, 4097, 8200])
def test_duplicate_rule_across_every_even_scan_boundary(n_m, monkeypatch):
    """Reads of mates around multiples of 256 and 1024 M entries: the (read, locus) group that straddles a boundary is
    an equal pair, a different pair or a triple depending on the boundary."""
    p = mates_pileup(straddling_reads(n_m))
    dev = check(p, CELLS, 100000, 1, monkeypatch)
    assert dev["same"]["num_entries"] < p.n_entries  # the rule dropped entries


@pytest.mark.parametrize("n_m", [256, 1024, 2560, 4096, 8192])
def test_duplicate_rule_across_every_odd_scan_boundary(n_m, monkeypatch):
    """two-entry reads alone: every odd sorted position is inside a read (a tile length that is odd)"""
    dev = check(mates_pileup([2] * (n_m // 2)), CELLS, 100000, 1, monkeypatch)
    assert dev["same"]["num_entries"] < n_m * 2


@pytest.mark.parametrize("n_reads", [86, 342, 1366])
def test_triples_across_scan_boundaries(n_reads, monkeypatch):
    """all reads three mates: 258, 1026 and 4098 M entries; a boundary that is no multiple of three cuts a triple"""
    check(mates_pileup([3] * n_reads, gap=4), CELLS, 100000, 1, monkeypatch)


@pytest.mark.parametrize("n_m", [255, 1025, 4097])
def test_two_locus_reads_across_scan_boundaries(n_m, monkeypatch):
    """the same layouts with the reads' entries at neighbouring loci (kept entries, multi-locus reads)"""
    sizes, reads, l = straddling_reads(n_m), [], 1
    for s in sizes:
        reads.append(tuple(range(l, l + s)))
        l += s + 3
    n = l + 2
    p = chain_pileup(n, reads, chr_loci=n)
    assert 2 * n_m <= p.n_entries
    dev = check(p, CELLS, 100000, 1, monkeypatch)
    assert dev["same"]["num_reads"] == n - n_m + len(sizes)


def test_long_reads_every_m_entry_unmarked_but_the_heads(monkeypatch):
    """five reads of 40 entries at consecutive loci among 500: only a read's first entry is marked"""
    reads = [tuple(range(10 + 90 * k, 50 + 90 * k)) for k in range(5)]
    p = chain_pileup(500, reads, chr_loci=500)
    dev = check(p, CELLS, 100000, 1, monkeypatch)
    assert dev["same"]["num_reads"] == 500 - 200 + 5


def test_no_read_has_a_second_entry(monkeypatch):
    dev = check(chain_pileup(700), CELLS, 50, 1, monkeypatch)
    assert dev["same"]["num_reads"] == 700 and dev["same"]["num_entries"] == 700
