"""The decisions of the device packing (pack_device.hip): hand-over to the host, a voided attempt, a repeated one.

pack_pileup_device can hand over to the host emulation (Scalars::need_host, or a size limit seen before any attempt),
void a counting attempt and sort with radix (Scalars::regroup: RetryRadix) and start over without the previous call's
sizes (Scalars::id_exceeded: RetryPlain). The sibling files check what the packing produces; this one checks that each
decision is taken where it has to be, and only there: SimilarityMatrixPlan.packing_route says how many attempts ran,
whether the last sorted with radix, whether one was repeated plainly and whether the host was asked.

Every pileup is written by hand (tests.pileup_gen.from_rows). A case that stays on the device checks the route report
with the two older accessors, the work counters against the oracle's, the finalized matrix against the oracle's within
TOL (norm-wise), and finalize_raw bit for bit against the host packing's. A case that hands over runs twice: in auto
mode (no device packing, counters and matrix equal the oracle's) and in device mode (SecedoError, E_LIMIT).

A read belongs to one cell (the entries of one id carry one group), as in every pileup the pileup creation writes.
"""
import numpy as np
import pytest

import secedo_amd
from oracle import bindings as ob
from secedo_amd import _lib
from secedo_amd.pileup import FlatPileup
from secedo_amd.similarity_matrix import PackingRoute
from tests import golden_util as gu
from tests.pileup_gen import from_rows

pytestmark = pytest.mark.gpu
TOL = 1e-9
RATES = (0.01, 0.5, 0.01)
N_CELLS = 60

ONE_COUNTING = PackingRoute(1, False, False, False)
VOID_THEN_RADIX = PackingRoute(2, True, False, False)


def run(plan, p, n_cells, mfl, T, resident=False):
    import torch
    if resident:
        plan.prepare_resident(plan.upload(p, None, n_cells), n_cells, mfl, T)
    else:
        plan.prepare(p, n_cells, mfl, None, T)
    acc = plan.new_acc()
    plan.accumulate(acc, *RATES)
    raw = plan.finalize_raw(acc).clone()
    got = plan.finalize(acc, "ADD_MIN").cpu().numpy()
    torch.cuda.synchronize()
    return raw, got, plan.last_counts()


def oracle(p, n_cells, mfl, T):
    ref = ob.oracle_compute(p, n_cells, mfl, None, *RATES, T, "ADD_MIN")
    return ref, (ob.oracle_last_updates(), ob.oracle_last_read_pairs())


_REF = {}


def reference(key, p, n_cells, mfl, T, host_raw=True):
    """The oracle's matrix and counters and the host packing's raw matrix, once per pileup."""
    if key not in _REF:
        ref, counts = oracle(p, n_cells, mfl, T)
        raw_host = None
        if host_raw:
            with secedo_amd.SimilarityMatrixPlan(0) as host:
                host.set_packing("host")
                raw_host = run(host, p, n_cells, mfl, T)[0]
                assert not host.used_device_packing and not host.used_single_entry_path
                assert host.packing_route == PackingRoute(0, False, False, False)
        _REF[key] = (ref, counts, raw_host)
    return _REF[key]


def check_device(key, p, mfl, T, route, single, n_cells=N_CELLS, plan=None, resident=False):
    """The four checks of a case that stays on the device, on `plan` or on a fresh one. Returns finalize_raw."""
    import torch
    ref, counts, raw_host = reference(key, p, n_cells, mfl, T)
    own = plan is None
    plan = secedo_amd.SimilarityMatrixPlan(0) if own else plan
    try:
        plan.set_packing("device")
        raw, got, got_counts = run(plan, p, n_cells, mfl, T, resident)
        assert plan.packing_route == route
        assert plan.used_device_packing
        assert plan.used_single_entry_path == single
    finally:
        if own:
            plan.close()
    assert got_counts == counts
    assert counts[0] > 0
    assert gu.normwise_err(got, ref) <= TOL
    assert torch.equal(raw, raw_host)
    return raw


def check_handover(key, p, mfl, T, route, n_cells=N_CELLS, plan=None, resident=False):
    """A case that hands over: auto mode packs on the host and equals the oracle, device mode fails with E_LIMIT; the
    report says what the device packing did until it asked (`route`, asked_host set)."""
    assert route.asked_host
    ref, counts, _ = reference(key, p, n_cells, mfl, T, host_raw=False)
    own = plan is None
    plan = secedo_amd.SimilarityMatrixPlan(0) if own else plan
    try:
        plan.set_packing("auto")
        _, got, got_counts = run(plan, p, n_cells, mfl, T, resident)
        assert plan.packing_route == route
        assert not plan.used_device_packing and not plan.used_single_entry_path
        assert got_counts == counts
        assert counts[0] > 0
        assert gu.normwise_err(got, ref) <= TOL
        plan.set_packing("device")
        with pytest.raises(secedo_amd.SecedoError) as e:
            run(plan, p, n_cells, mfl, T, resident)
        assert e.value.code == _lib.E_LIMIT
        assert plan.packing_route == route
        assert not plan.used_device_packing and not plan.used_single_entry_path
    finally:
        if own:
            plan.close()


# ---- the 2^32 edge -------------------------------------------------------------------------------------------------
# start + max_fragment_length is a uint32 in the reference (similarity_matrix.cpp:348-352), in pack_host.cpp and in the
# oracle: beyond 2^32 - 1 it wraps and the read counts as complete at once. The device compares pos - mfl, which does
# not wrap, and hands over instead: k_read_info raises need_host per read of several entries (on the main stream, in
# front of read-back 2), k_completed per locus that has entries (on the side stream, beside read-back 2).
EDGE_LOCI, EDGE_DEPTH = 40, 6
VARIANTS = ("single", "quiet_pairs", "pair_past_edge", "pairs_general", "single_radix", "empty_past_edge")


def last_that_fits(mfl):
    return 2 ** 32 - 1 - mfl


def edge_tops(mfl):
    return [2 ** 32 - 2 - mfl, last_that_fits(mfl), 2 ** 32 - mfl, 2 ** 32 - 1]


def edge_pileup(variant, top, mfl, seed=11):
    """40 loci one position apart, the last at `top`, 6 entries per locus over 60 cells.
    single / single_radix: every read has one entry -- nothing but k_completed can see the edge.
    quiet_pairs: a first chromosome of 20 loci at low positions in front, 30 of its 120 reads with two entries (two
        loci apart): 60 of 360 entries repeat, the route stays single-entry, k_read_info runs and finds nothing.
    pair_past_edge: one read of two entries, at the loci 36 and 39: k_read_info sees `top` as a read's last position.
    pairs_general: every read has two entries, at the loci 2k and 2k + 1: the general route.
    empty_past_edge: a 41st locus WITHOUT entries at `top`, the 40 with entries end at the last position that fits (or
        below `top`): nothing that is there wraps, the device keeps it."""
    rng = np.random.default_rng(seed)
    n_loci = EDGE_LOCI
    end = min(top - 1, last_that_fits(mfl)) if variant == "empty_past_edge" else top
    ids = (5 + 2 * rng.permutation(n_loci * EDGE_DEPTH)).reshape(n_loci, EDGE_DEPTH)
    cells = rng.integers(0, N_CELLS, size=(n_loci, EDGE_DEPTH))
    bases = rng.integers(0, 4, size=(n_loci, EDGE_DEPTH))
    if variant == "pair_past_edge":
        ids[39, 2], cells[39, 2] = ids[36, 4], cells[36, 4]
    if variant == "pairs_general":
        ids[1::2], cells[1::2] = ids[0::2], cells[0::2]
    chrom = [(end - (n_loci - 1) + l, [(int(ids[l, i]), int(cells[l, i]), int(bases[l, i])) for i in range(EDGE_DEPTH)])
             for l in range(n_loci)]
    if variant == "empty_past_edge":
        chrom.append((top, []))
    rows = [chrom]
    if variant == "quiet_pairs":
        lids = (5 + 2 * rng.permutation(20 * EDGE_DEPTH)).reshape(20, EDGE_DEPTH)
        lcells = rng.integers(0, N_CELLS, size=(20, EDGE_DEPTH))
        lbases = rng.integers(0, 4, size=(20, EDGE_DEPTH))
        for k in range(30):
            l, i = 4 * (k // 12) + (k % 12) // EDGE_DEPTH, k % EDGE_DEPTH   # loci 4j, 4j + 1 pair with 4j + 2, 4j + 3
            lids[l + 2, i], lcells[l + 2, i] = lids[l, i], lcells[l, i]
        low = [(1000 + l, [(int(lids[l, i]), int(lcells[l, i]), int(lbases[l, i])) for i in range(EDGE_DEPTH)])
               for l in range(20)]
        rows = [low, chrom]
    return from_rows(rows)


def moved_down(p, by=2 ** 20):
    """the positions of the upper half 2^20 lower: the same pileup away from the edge"""
    pos = p.locus_pos.astype(np.int64)
    return FlatPileup(p.chr_locus_off, np.where(pos > 2 ** 31, pos - by, pos).astype(np.uint32), p.locus_entry_off,
                      p.read_ids, p.id_base)


def edge_expectation(variant, top, mfl):
    """(hands over, route, single-entry path)"""
    radix = variant == "single_radix"
    wraps = top > last_that_fits(mfl) and variant != "empty_past_edge"
    return wraps, PackingRoute(1, radix, False, wraps), variant not in ("pairs_general", "single_radix")


@pytest.mark.parametrize("mfl", [5, 8])
@pytest.mark.parametrize("variant", VARIANTS)
def test_positions_within_max_fragment_length_of_2_to_the_32(variant, mfl, monkeypatch):
    """The last position that fits (2^32 - 1 - mfl) and the one below stay on the device, the first that wraps
    (2^32 - mfl) and 2^32 - 1 hand over, on every route and through prepare and prepare_resident alike; an empty locus
    past the edge hands nothing over (k_completed looks at locus_entry_off). For 2^32 - 1 the wrap changes the result:
    the oracle's counters differ from those of the same pileup 2^20 lower (a wrap at the last locus alone does not:
    its reads are never flushed).

    With every read a single entry, k_completed is the only kernel that raises need_host, on the side stream; before
    the verdict behind the records honoured the flag, read-back 2 raced with it and the hand-over depended on which
    stream got there first. That made these cases timing-dependent at the parent commit, not certain to fail: what
    makes the hand-over certain is the stream order (the main stream waits for the side stream's ev_join in front of
    the records, and every ev_join is recorded behind k_completed), not this test having been seen red."""
    if variant == "single_radix":
        monkeypatch.setenv("SECEDO_PACK_GROUPING", "radix")
    for top in edge_tops(mfl):
        p = edge_pileup(variant, top, mfl)
        hands_over, route, single = edge_expectation(variant, top, mfl)
        if top == 2 ** 32 - 1 and hands_over:
            assert oracle(p, N_CELLS, mfl, 1)[1] != oracle(moved_down(p), N_CELLS, mfl, 1)[1]
        for resident in (False, True):
            key = ("edge", variant, top, mfl)
            if hands_over:
                check_handover(key, p, mfl, 1, route, resident=resident)
            else:
                check_device(key, p, mfl, 1, route, single, resident=resident)


def small_sparse(seed=21, n_entries=240, stride=2):
    """n_entries entries in loci of 4 at low positions, ten reads of two entries (four loci apart). With 240 entries
    and stride 2 the read-id space is that of the edge pileups: one handle sees the same sizes throughout."""
    rng = np.random.default_rng(seed)
    ids = 5 + stride * rng.permutation(n_entries)
    for j, v in ((n_entries - 2, ids.min()), (n_entries - 1, ids.max())):   # the extremes where no pair below takes
        i = int(np.flatnonzero(ids == v)[0])                               # their place: the id space is fixed
        ids[i], ids[j] = ids[j], ids[i]
    cells = rng.integers(0, N_CELLS, size=n_entries)
    for k in range(10):
        ids[8 * k + 16], cells[8 * k + 16] = ids[8 * k], cells[8 * k]
    assert ids.min() == 5 and ids.max() == 5 + stride * (n_entries - 1)
    chrom = [(1000 + e // 4, [(int(ids[i]), int(cells[i]), int(rng.integers(0, 4))) for i in range(e, e + 4)])
             for e in range(0, n_entries, 4)]
    return from_rows([chrom])


def test_late_need_host_on_a_handle_that_just_packed_on_the_device():
    """Single-entry reads at 2^32 - 1: five times on one plan, each after a device packing of a small pileup, the
    hand-over is taken in auto mode and device mode fails with E_LIMIT. The repeats sample the race between read-back
    2 and k_completed described above: at the parent commit each of them could go either way."""
    mfl, top = 5, 2 ** 32 - 1
    far, near = edge_pileup("single", top, mfl), small_sparse()
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        for _ in range(5):
            check_device("near", near, 10, 1, ONE_COUNTING, True, plan=plan)
            check_handover(("edge", "single", top, mfl), far, mfl, 1, PackingRoute(1, False, False, True), plan=plan)


def test_one_handle_across_hand_overs():
    """device -> hand-over -> device -> device-mode error -> device -> hand-over (resident) -> device on one plan. A
    hand-over leaves the handle's assumptions behind (id_space_hint, split_pays, the flag lists of the previous
    packing): every device step equals a fresh plan's finalize_raw bit for bit, takes one attempt and the single-entry
    path, and reports what a second plan reports that packs the same sequence with the far pileup 2^20 lower (the same
    sizes, no hand-over)."""
    import torch
    mfl, top = 5, 2 ** 32 - 1
    far, near = edge_pileup("single", top, mfl), small_sparse()
    far_key, asked = ("edge", "single", top, mfl), PackingRoute(1, False, False, True)
    fresh = check_device("near", near, 10, 1, ONE_COUNTING, True)
    steps = ["near", "auto", "near", "device", "near", "auto_resident", "near"]
    with secedo_amd.SimilarityMatrixPlan(0) as plan, secedo_amd.SimilarityMatrixPlan(0) as twin:
        for step in steps:
            if step == "near":
                raw = check_device("near", near, 10, 1, ONE_COUNTING, True, plan=plan)
                assert torch.equal(raw, fresh)
                check_device("near", near, 10, 1, plan.packing_route, plan.used_single_entry_path, plan=twin)
                continue
            check_device(("edge", "single", top, mfl, "lower"), moved_down(far), mfl, 1, ONE_COUNTING, True, plan=twin,
                         resident=step == "auto_resident")
            if step == "device":
                plan.set_packing("device")
                with pytest.raises(secedo_amd.SecedoError) as e:
                    run(plan, far, N_CELLS, mfl, 1)
                assert e.value.code == _lib.E_LIMIT and plan.packing_route == asked
            else:
                plan.set_packing("auto")
                ref, counts, _ = reference(far_key, far, N_CELLS, mfl, 1, host_raw=False)
                _, got, got_counts = run(plan, far, N_CELLS, mfl, 1, resident=step == "auto_resident")
                assert plan.packing_route == asked and not plan.used_device_packing
                assert got_counts == counts and gu.normwise_err(got, ref) <= TOL


# ---- the 8192 limit of the in-group ranking (kRankScanLimit), at its three sites -----------------------------------
LIMIT = 8192


def general_route_rows(deep_locus_cov, repeated_id_count, seed=91, n=40):
    """The generator of test_device_grouping_fallbacks (test_gpu_parity.py): 60 loci of 10 to 80 single-entry reads
    over 40 cells, `deep_locus_cov` of them at locus 20, and at locus 30 one read id `repeated_id_count` times."""
    rng = np.random.default_rng(seed)
    rows, rid, pos = [], 0, 500
    for l in range(60):
        pos += int(rng.integers(30, 300))
        cov = deep_locus_cov if l == 20 else int(rng.integers(10, 80))
        ents = []
        for _ in range(cov):
            ents.append((rid, int(rng.integers(0, n)), int(rng.integers(0, 4))))
            rid += 1
        if l == 30 and repeated_id_count:
            ents += [(rid, 3, int(rng.integers(0, 4))) for _ in range(repeated_id_count)]
            rid += 1
        rows.append((pos, ents))
    for k in range(4):  # far loci: everything above completes and is flushed
        pos += 3000
        rows.append((pos, [(rid + k, 0, 0)]))
    return from_rows([rows])


def long_read_rows(length, seed=83, n=40):
    """One id at `length` consecutive loci with two single-entry reads beside it at each: a third of the entries
    repeat, the route stays single-entry and the id is one read of the M entries (max_fragment_length covers it)."""
    rng = np.random.default_rng(seed)
    rows, rid, pos = [], 1, 5000
    for l in range(length):
        pos += 1
        ents = [(0, 3, l % 4 if l % 7 else (l + 1) % 4)]
        for _ in range(2):
            ents.append((rid, int(rng.integers(0, n)), int(rng.integers(0, 4)) if rng.random() < 0.2 else l % 4))
            rid += 1
        rows.append((pos, ents))
    for k in range(4):
        pos += 20000
        rows.append((pos, [(rid + k, 1, 0)]))
    return from_rows([rows])


@pytest.mark.parametrize("count", [LIMIT, LIMIT + 1])
@pytest.mark.parametrize("site", ["k_id_rank", "k_group_rank", "k_entry_records"])
def test_the_rank_scan_limit_at_8192_and_8193(site, count):
    """8192 members are ranked by the full-length scan in one counting attempt; 8193 void the attempt (every position
    of the void order still holds an entry: what follows stays inside its arrays) and the radix sorts take over.
    k_id_rank: a read id with that many entries on the general route (more than half of the entries repeat);
    k_group_rank: the same on the single-entry route; k_entry_records: a (cell block, locus) group of that many kept
    single-entry reads over 40 cells (some cell has two: the group is ranked)."""
    n, mfl, T = 40, 1000, 2
    if site == "k_id_rank":
        p = general_route_rows(50, count)
        assert 2 * count > p.n_entries
    elif site == "k_group_rank":
        p, mfl = long_read_rows(count), LIMIT + 8   # (the oracle's tables grow with its square)
        assert 2 * count < p.n_entries and p.n_entries == 3 * count + 4
    else:
        p = general_route_rows(count, 0)
    voided = count > LIMIT
    # (the radix attempt does not try the single-entry path)
    check_device(("limit", site, count), p, mfl, T, VOID_THEN_RADIX if voided else ONE_COUNTING,
                 site != "k_id_rank" and not voided, n_cells=n)


# ---- RetryPlain ----------------------------------------------------------------------------------------------------
def test_a_larger_id_space_than_the_previous_call_s_is_packed_again_without_it():
    """A handle assumes the read-id space of its previous call and skips read-back 1; k_id_bases finds the space of
    the second pileup larger (still within four times its entries: the counting scheme), the attempt is void and is
    repeated with the read-back. The third call, a smaller space again, takes one attempt."""
    small, large = small_sparse(), small_sparse(seed=22, n_entries=400, stride=3)
    retried = PackingRoute(2, False, True, False)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        check_device("near", small, 10, 1, ONE_COUNTING, True, plan=plan)
        check_device("large", large, 10, 1, retried, True, plan=plan)
        check_device("near", small, 10, 1, ONE_COUNTING, True, plan=plan)
        check_device("large", large, 10, 1, retried, True, plan=plan, resident=True)
    check_device("large", large, 10, 1, ONE_COUNTING, True)   # a fresh plan assumes nothing


# ---- size limits that need no large input ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2 ** 30, 2 ** 30 + 1])
def test_a_flush_threshold_beyond_32_bits_hands_over_before_any_attempt(T):
    """4 * num_threads >= 2^32 does not fit the device's flush threshold: no attempt is made. The reference multiplies
    in uint32 (similarity_matrix.cpp:354-356) and so do the oracle and the host packing: 2^30 threads flush at every
    locus (threshold 0), 2^30 + 1 are one thread (threshold 4)."""
    p = small_sparse()
    if T > 2 ** 30:
        wrapped, one = oracle(p, N_CELLS, 10, T), oracle(p, N_CELLS, 10, 1)
        assert wrapped[1] == one[1] and np.array_equal(wrapped[0], one[0])
    for resident in (False, True):
        check_handover(("threads", T), p, 10, T, PackingRoute(0, False, False, True), resident=resident)
