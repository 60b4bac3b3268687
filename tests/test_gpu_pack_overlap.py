"""The flagged entries' lists from the ballots of k_entry_records, enqueued behind the publishing kernel of the
packing's last read-back, against the serial twin (SECEDO_PACK_OVERLAP=0: the lists from entry32, behind the
read-back) and the host packing, on fresh handles and on handles that packed other pileups before.

Packed arrays, lists, counters and matrices must be bit for bit what the serial order gives. The makeup of the
synthetic inputs (entries, share on repeated ids, share in multi-locus reads; seed 7):
  sparse (130, 300, 3, 30000, 0.3): 11 863 entries (three 4096-blocks, the last partial; 11 863 mod 64 = 23), 1.6 %,
         0.9 % -- short cut, auto block_cells 128, count tile, lists built; 300 loci = four 64-locus tiles and one of 44
  mid    (130, 300, 3, 2000, 0.3): 14 136 entries, 31.9 %, 31.4 % -- short cut stays, clustered: auto 64, masks kernel
  dense  (130, 300, 3, 1000, 0.3): 16 695 entries, 53.7 % -- short cut abandoned at read-back 1b
  tiny   (70, 40, 1, 30000, 0.2): 532 entries, none on a repeated id (n_m == 0), one partial locus tile and flag block
"""
import ctypes as C

import numpy as np
import pytest

import secedo_amd
from secedo_amd import _lib
from secedo_amd.synth import synth_pileup
from tests.pileup_gen import from_rows

pytestmark = pytest.mark.gpu

RATES = (0.01, 0.5, 0.02)
SPECS = {
    "sparse": (130, 300, 3, 30000, 0.3),
    "mid": (130, 300, 3, 2000, 0.3),
    "dense": (130, 300, 3, 1000, 0.3),
    "tiny": (70, 40, 1, 30000, 0.2),
}
ENTRIES = {"sparse": 11863, "mid": 14136, "dense": 16695, "tiny": 532}
# auto block_cells -> (block_cells, pair kernel, lists built)
AUTO = {
    "sparse": (128, "accumulate_counts", True),
    "mid": (64, "accumulate_masks", False),
    "tiny": (128, "accumulate_counts", True),
}
_pileups = {}
_cache = {}


def pileup(name):
    if name not in _pileups:
        p = synth_pileup(*SPECS[name], seed=7)
        assert p.n_entries == ENTRIES[name], (name, p.n_entries)
        _pileups[name] = p
    return _pileups[name]


def flag_lists(plan):
    L = _lib.lib()
    n = C.c_uint64()
    if L.secedo_simmat_debug_flag_lists(plan._h, C.byref(n), None, None, None) != 0:
        return None
    nb = (plan.num_cells + plan.block_cells - 1) // plan.block_cells
    grp = np.zeros(nb * (plan.num_loci + 1), np.uint32)
    rec = np.zeros((max(n.value, 1), 4), np.uint32)
    idx = np.zeros(max(n.value, 1), np.uint32)
    _lib.check(L.secedo_simmat_debug_flag_lists(plan._h, C.byref(n), _lib.ptr(grp), _lib.ptr(rec), _lib.ptr(idx)))
    return grp, rec[:n.value], idx[:n.value]


def result_of(plan):
    """What a prepared plan gives: everything the routes must agree on, and its flagged entries' lists."""
    import torch
    lists = flag_lists(plan)  # (the packing's, before any accumulate)
    acc = plan.new_acc()
    plan.accumulate(acc, *RATES)
    torch.cuda.synchronize()
    same = dict(counts=plan.last_counts(), num_entries=plan.num_entries, num_reads=plan.num_reads,
                block_cells=plan.block_cells, pair_kernel=plan.pair_kernel,
                raw=plan.finalize_raw(acc).cpu().numpy().copy())
    return same, lists


def run(p, cells, mfl, threads, block, mode, twice=False):
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        plan.set_packing(mode)
        plan.prepare(p, cells, mfl, None, threads, block_cells=block)
        assert plan.used_device_packing == (mode == "device")
        out = [result_of(plan)]
        if twice:  # the same pileup again on the same handle: the assumed-geometry route
            plan.prepare(p, cells, mfl, None, threads, block_cells=block)
            out.append(result_of(plan))
    return out


def host_result(name, mfl, block):
    key = (name, mfl, block)
    if key not in _cache:
        _cache[key] = run(pileup(name), SPECS[name][0], mfl, 2, block, "host")[0]
    return _cache[key]


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if k == "raw":
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def assert_lists_equal(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        for x, y, k in zip(a, b, ("grp", "rec", "idx")):
            assert np.array_equal(x, y), (what, k)


def device_routes(monkeypatch, p, cells, mfl, threads, block, twice=False):
    monkeypatch.delenv("SECEDO_PACK_OVERLAP", raising=False)
    new = run(p, cells, mfl, threads, block, "device", twice)
    monkeypatch.setenv("SECEDO_PACK_OVERLAP", "0")
    old = run(p, cells, mfl, threads, block, "device", twice)
    monkeypatch.delenv("SECEDO_PACK_OVERLAP", raising=False)
    return new, old


@pytest.mark.parametrize("block", [0, 64, 128])
@pytest.mark.parametrize("name", ["sparse", "mid", "tiny"])
def test_routes_agree(name, block, monkeypatch):
    """Device packing, its serial twin and the host packing: same counters, sizes, block size, kernel and raw matrix;
    the two device routes also the same lists; and the same again on a second prepare of the handle."""
    p, cells = pileup(name), SPECS[name][0]
    new, old = device_routes(monkeypatch, p, cells, 1000, 2, block, twice=True)
    host = host_result(name, 1000, block)[0]
    for i in range(2):
        assert_same(new[i][0], host, (name, block, "overlap", i))
        assert_same(old[i][0], host, (name, block, "serial", i))
        assert_lists_equal(new[i][1], old[i][1], (name, block, i))
    same, lists = new[0]
    if block == 0:
        want_block, want_kernel, want_lists = AUTO[name]
        assert same["block_cells"] == want_block and same["pair_kernel"] == want_kernel
        assert (lists is not None) == want_lists
    else:
        assert same["block_cells"] == block
    assert (lists is not None) == (same["pair_kernel"] == "accumulate_counts")
    if lists is not None:
        assert len(lists[2]) > 0 and np.all(np.diff(lists[2].astype(np.int64)) > 0)


def test_reads_cut_by_flushes(monkeypatch):
    """max_fragment_length 60 on `sparse`: reads outlive it and are cut where a flush erases them (the k_split_update
    rounds)."""
    p, cells = pileup("sparse"), SPECS["sparse"][0]
    host = host_result("sparse", 60, 0)[0]
    assert host["num_reads"] != host_result("sparse", 1000, 0)[0]["num_reads"]  # the flushes cut reads here
    new, old = device_routes(monkeypatch, p, cells, 60, 2, 0)
    assert_same(new[0][0], host, "overlap")
    assert_same(old[0][0], host, "serial")
    assert_lists_equal(new[0][1], old[0][1], "lists")


def test_one_handle_changing_pileups():
    """One handle, auto block size, through pileups that change the block size (128 -> 64 -> 128), abandon the
    single-entry short cut (dense: no lists, the list buffers are released and come back), and have no M entry at
    all (tiny)."""
    import torch
    fresh = {}
    for name in ("sparse", "mid", "dense", "tiny"):
        fresh[name] = run(pileup(name), SPECS[name][0], 1000, 2, 0, "device")[0]
    assert fresh["sparse"][0]["block_cells"] == 128 and fresh["mid"][0]["block_cells"] == 64
    assert fresh["tiny"][0]["block_cells"] == 128
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        plan.set_packing("device")
        for step, name in enumerate(["sparse", "mid", "sparse", "dense", "tiny", "sparse"]):
            plan.prepare(pileup(name), SPECS[name][0], 1000, None, 2, block_cells=0)
            assert plan.used_device_packing
            same, lists = result_of(plan)
            assert_same(same, fresh[name][0], (step, name))
            assert_lists_equal(lists, fresh[name][1], (step, name))
    torch.cuda.synchronize()


CHR_LOCI = 24  # loci per chromosome: 4095 / 4096 and 8191 / 8192 lie inside one chromosome


def edge_pileup(n):
    """n loci of one entry each (so the packed order is the locus order), 128 cells, chromosomes of 24 loci 10
    positions apart: with max_fragment_length 50 and one thread a chromosome flushes every fourth completed read and
    leaves its last reads never flushed. Every entry is a read of its own except two-locus reads at the very end,
    across the 4096 boundary and one in 192 loci."""
    pairs = {n - 2}
    if n > 4096:
        pairs.add(4095)
    if n > 4000:
        pairs.update(i for i in range(5, n - 1, 192) if i + 1 not in pairs and i - 1 not in pairs)
    for i in pairs:
        assert i // CHR_LOCI == (i + 1) // CHR_LOCI, i
    assert 2 * len(pairs) < 0.05 * n
    rows, rid = [], 0
    read_of = {}
    for i in range(n):
        if i % CHR_LOCI == 0:
            rows.append([])
        if i - 1 in pairs:
            r = read_of[i - 1]
        else:
            r = rid
            rid += 1
        read_of[i] = r
        rows[-1].append((10 * (i % CHR_LOCI) + 1, [(r, (i * 37) % 128, i & 3)]))
    return from_rows(rows)


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097, 8193])
def test_list_edges(n, monkeypatch):
    """The lists at the edges of their 64-entry chunks and 4096-entry blocks."""
    p = edge_pileup(n)
    new, old = device_routes(monkeypatch, p, 128, 50, 1, 128)
    (same_new, lists_new), (same_old, lists_old) = new[0], old[0]
    assert_same(same_new, same_old, n)
    assert same_old["num_entries"] == n and same_old["block_cells"] == 128
    assert same_old["pair_kernel"] == "accumulate_counts"
    assert lists_old is not None and lists_new is not None
    assert_lists_equal(lists_new, lists_old, n)
    grp, rec, idx = lists_old
    assert np.all(np.diff(idx.astype(np.int64)) > 0)
    assert grp[-1] == len(idx) and 0 < len(idx) < n
    tail = ((rec[:, 0] >> 18) & 1).astype(bool)
    multi = (rec[:, 1] != 0) | ((rec[:, 0] & (3 << 19)) != 0)
    assert tail.any() and multi.any() and (tail | multi).all()
    assert idx[-1] >= (n - 1) // 64 * 64  # a flagged entry in the last chunk of the array
    if n > 4096:
        assert np.any((idx >= 4096) & (idx < 4096 + 64))  # ... and in the first chunk behind a block boundary
