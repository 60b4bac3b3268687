"""accumulate_counts where its counted LDS waits can go wrong. The pair loop reads the column words of an item by hand
and waits for them with s_waitcnt lgkmcnt(N), N the LDS instructions certainly issued behind the reads: the first item
of a thread, the middle ones and the last one have different counts, every GROUP has its own, a ring batch drained
between a load and its pair sits inside the count, and diagonal tiles wait in full. A wrong count is a stale column
word: a wrong count-tile address or base flag, hence wrong entries and usually wrong work counters, possibly different
from launch to launch. So per case: the un-normalised matrix against the oracle norm-wise to 1e-9 (against the direct
sums where a cell pair collects more than 1e4 pairs, as test_gpu_counts_items.py), both work counters exactly, the
kernel and its instance, and three further launches into fresh accumulators bit for bit the first.

The cases (entries per (locus, cell block) chosen, block_counts):
  ring_pressure_g4 / _g2  long stretches of exactly 9 and exactly 17 entries in every block: every primary step pushes
                          64 continuations, the ring passes 192 inside the primary loop and is drained between a load
                          and its pair, drained batches push again; overall density for GROUP 4 and for GROUP 2
  thin_a / _b / _c        one range whose blocks hold 1, 63, 64 / 65, 1023, 1024 / 12288, 12287, 1025 entries: threads
                          without an item, with the first item only, lanes past the row side, a full staging area
  group3                  density 2.8 (GROUP 3, a word per locus), loci of 0, 1, 3, 4 and 7 entries
  group3_offsets          the same in one range of 4200 loci: the instance with 16-bit offsets (380 cells: with a small
                          last block the packing cuts shorter ranges at this density)
  b64                     64-cell blocks (the 512-thread instance, eight items per thread; few multi-locus reads, or
                          the plan takes accumulate_masks)
  diagonal_only           100 cells: one tile, the C++ slots behind the wait-only statement

The GPU side of all cases runs in one child process per SECEDO_CORRECT_FUSED setting (read once per process)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bindings as ob
from tests import golden_util as gu
from tests.pileup_gen import from_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
MFL = 1000
T = 2
RATES = (0.01, 0.5, 0.01)

# case -> (cells, block_cells, GROUP by the density rule of choose_correction, a word per locus)
CASES = {
    "ring_pressure_g4": (280, 128, 4, True),
    "ring_pressure_g2": (280, 128, 2, True),
    "thin_a": (280, 128, 4, True),
    "thin_b": (280, 128, 4, True),
    "thin_c": (280, 128, 3, True),
    "group3": (280, 128, 3, True),
    "group3_offsets": (380, 128, 3, False),
    "b64": (280, 64, 4, False),
    "diagonal_only": (100, 128, 4, True),
}


def spread(total, L, at_least=0):
    """total entries over L loci, as evenly as it goes."""
    out = np.full(L, total // L, dtype=np.int64)
    out[: total - out.sum()] += 1
    assert out.sum() == total and out.min() >= at_least
    return out


def block_counts(case):
    """The case's entries per (locus, cell block): counts[L, nb]."""
    n, B, group, _ = CASES[case]
    nb = (n + B - 1) // B
    rng = np.random.default_rng(4000 + sum(map(ord, case)))
    ladder = (0, 1, group, group + 1, 2 * group + 1)
    if case == "ring_pressure_g4":
        counts = rng.poisson(3.8, size=(700, nb))
        counts[20:320, :] = 9
        counts[340:640, :] = 17
    elif case == "ring_pressure_g2":
        counts = rng.poisson(1.0, size=(4000, nb))
        counts[1000:1150, :] = 9
        counts[2500:2650, :] = 17
    elif case == "thin_a":
        counts = np.stack([spread(1, 10), spread(60, 10, 1), spread(64, 10)], axis=1)
    elif case == "thin_b":
        counts = np.stack([spread(65, 200), spread(1020, 200, 1), spread(1024, 200)], axis=1)
    elif case == "thin_c":
        counts = np.stack([spread(12288, 3072), spread(12284, 3072, 1), spread(1025, 3072)], axis=1)
    elif case == "group3":
        counts = rng.poisson(2.8, size=(1500, nb))
    elif case == "group3_offsets":
        # 4200 loci and at most 11900 entries in any block: one range (12288 are staged), longer than 4094 loci
        counts = np.minimum(rng.poisson(2.8, size=(4200, nb)), 7)
        for b in range(nb):
            while counts[:, b].sum() > 11900:
                counts[int(rng.integers(0, 4200)), b] = 1
    elif case == "b64":
        counts = rng.poisson(3.8, size=(600, nb))
        counts[50:200, :] = 9
        counts[310:460, :] = 17
    elif case == "diagonal_only":
        counts = rng.poisson(3.8, size=(800, nb))
        counts[100:250, :] = 9
        counts[420:570, :] = 17
    else:
        raise KeyError(case)
    L = counts.shape[0]
    if not case.startswith("thin"):
        # loci of 0, 1, GROUP, GROUP + 1 and 2 GROUP + 1 entries: every block the same, and mixed
        for k, v in enumerate(ladder):
            counts[3 + 2 * k, :] = v
            counts[L // 2 + 2 * k, :] = [ladder[(k + b) % len(ladder)] for b in range(nb)]
            counts[L - 12 + 2 * k, :] = v  # (a last ring batch of few items)
        counts[counts.sum(axis=1) == 0, 0] = 1  # (a locus holds an entry)
    # three last loci far away (everything before them is flushed), one entry each, in block 1: part of its total
    tail = np.zeros((3, nb), dtype=np.int64)
    tail[:, min(1, nb - 1)] = 1
    return np.concatenate([counts, tail])


@functools.lru_cache(maxsize=None)
def pileup(case):
    n, B, _, _ = CASES[case]
    counts = block_counts(case)
    rng = np.random.default_rng(5000 + sum(map(ord, case)))
    L, nb = counts.shape
    rows, rid, pos = [], 0, 1000
    # (64-cell blocks run accumulate_masks when more than 5 % of the entries are of multi-locus reads)
    p_multi = 0.015 if B == 64 else 0.3
    last = {}  # cell -> (read id, loci it has so far): some reads go on at the next locus
    for l in range(L):
        ref = int(rng.integers(0, 4))
        ents, now = [], {}
        for b in range(nb):
            cells_b = min(B, n - b * B)
            c = int(counts[l, b])
            cells = rng.choice(cells_b, size=c, replace=c > cells_b) + b * B
            for cell in cells.tolist():
                base = ref if rng.random() < 0.7 else int(rng.integers(0, 4))
                prev = last.get(cell)
                if prev is not None and prev[1] < 5 and cell not in now and rng.random() < p_multi:
                    r, k = prev[0], prev[1] + 1  # a multi-locus read (at most one entry per locus: nothing is dropped)
                else:
                    r, k = rid, 1
                    rid += 1
                now[cell] = (r, k)
                ents.append((r, cell, base))
        last = now
        pos += 5000 if l >= L - 3 else 40
        rows.append((pos, ents))
    return n, from_rows([rows])


@functools.lru_cache(maxsize=None)
def reference(case):
    n, p = pileup(case)
    _, raw = ob.oracle_compute(p, n, MFL, None, *RATES, T, "ADD_MIN", want_raw=True)
    counts = (ob.oracle_last_updates(), ob.oracle_last_read_pairs())
    ob.set_direct_llr_sum(True)
    try:
        _, direct = ob.oracle_compute(p, n, MFL, None, *RATES, T, "ADD_MIN", want_raw=True)
    finally:
        ob.set_direct_llr_sum(False)
    return raw, direct, counts


@pytest.mark.parametrize("case", sorted(CASES))
def test_generated_pileups_have_the_intended_counts(case):
    """CPU: the intended entries per (locus, cell block), the density of the intended GROUP, and no cell whose sum of
    squared entry counts reaches 65536 (another pair kernel would run)."""
    n, B, group, _ = CASES[case]
    counts = block_counts(case)
    _, p = pileup(case)
    L, nb = counts.shape
    assert p.n_loci == L
    cell = (p.id_base >> 2).astype(np.int64)
    locus = np.repeat(np.arange(L), np.diff(p.locus_entry_off.astype(np.int64)))
    got = np.zeros((L, nb), dtype=np.int64)
    np.add.at(got, (locus, cell // B), 1)
    assert np.array_equal(got, counts)
    density = p.n_entries / L / nb  # choose_correction's rule: 2 below 2.5, 3 below 3.2, else 4
    if B == 128:
        assert (2 if density < 2.5 else 3 if density < 3.2 else 4) == group, density
    if case.startswith("ring_pressure") or case in ("b64", "diagonal_only"):
        for v in (9, 17):
            assert np.sum(np.all(got == v, axis=1)) >= 150, v
    elif case == "thin_a":
        assert got.sum(axis=0).tolist() == [1, 63, 64]
    elif case == "thin_b":
        assert got.sum(axis=0).tolist() == [65, 1023, 1024]
    elif case == "thin_c":
        assert got.sum(axis=0).tolist() == [12288, 12287, 1025]
    if case.startswith("group3"):
        for v in (0, 1, 3, 4, 7):
            assert np.any(np.all(got == v, axis=1) if v else np.any(got == 0, axis=1)), v
        assert got.sum(axis=0).max() <= 12288
    per_cell = np.zeros((L, n), dtype=np.int64)
    np.add.at(per_cell, (locus, cell), 1)
    assert int((per_cell ** 2).sum(axis=0).max()) < 65536
    # (the oracle pairs them but for the reads that are never flushed: at most every pair of two cells at a locus)
    n_l = per_cell.sum(axis=1)
    pairs = int((n_l * (n_l - 1) // 2).sum() - (per_cell * (per_cell - 1) // 2).sum())
    updates, read_pairs = reference(case)[2]
    assert 0 < read_pairs <= updates <= pairs


SCRIPT = r'''
import sys
import numpy as np, torch
sys.path.insert(0, ROOT)
import secedo_amd
from secedo_amd import _lib
from tests.test_gpu_counts_waits import pileup, CASES, MFL, T, RATES

out = {}
L = _lib.lib()
for case, (n_cells, block, group, words) in sorted(CASES.items()):
    n, p = pileup(case)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        plan.prepare(p, n, MFL, None, T, block_cells=block)
        out[case + "/kernel"] = np.frombuffer(plan.pair_kernel.encode(), dtype=np.uint8)
        out[case + "/block"] = np.array([plan.block_cells])
        nt = plan.num_tiles
        tiles = np.arange(nt, dtype=np.uint32)
        # as a range of tiles (correct_tiles) ...
        acc = plan.new_acc()
        plan.accumulate(acc, *RATES)
        out[case + "/counts"] = np.asarray(plan.last_counts(), dtype=np.uint64)
        out[case + "/words"] = np.array([L.secedo_simmat_last_locus_words(plan._h)])
        out[case + "/raw"] = plan.finalize_raw(acc).cpu().numpy()
        same, same_counts = True, True
        for _ in range(3):
            again = plan.new_acc()
            plan.accumulate(again, *RATES)
            same_counts = same_counts and np.array_equal(np.asarray(plan.last_counts(), dtype=np.uint64), out[case + "/counts"])
            torch.cuda.synchronize()
            same = same and torch.equal(acc, again)
        # ... and as a stored list (the fused epilogue where every tile has one workgroup)
        for _ in range(4):
            again = plan.new_acc()
            again.fill_(-9)
            plan.accumulate_list(again, *RATES, tiles, overwrite=True)
            same_counts = same_counts and np.array_equal(np.asarray(plan.last_counts(), dtype=np.uint64), out[case + "/counts"])
            torch.cuda.synchronize()
            same = same and torch.equal(acc, again)
        out[case + "/list_words"] = np.array([L.secedo_simmat_last_locus_words(plan._h)])
        out[case + "/same"] = np.array([same])
        out[case + "/same_counts"] = np.array([same_counts])
np.savez(sys.argv[1], **out)
'''


@functools.lru_cache(maxsize=None)
def gpu_run(fused_env):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.npz")
        env = dict(os.environ, **({} if fused_env else {"SECEDO_CORRECT_FUSED": "0"}))
        subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SCRIPT, out], check=True, env=env, timeout=600)
        return dict(np.load(out))


@pytest.mark.gpu
@pytest.mark.parametrize("fused_env", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_counted_waits_match_the_oracle(case, fused_env):
    n, block, _, words = CASES[case]
    run = gpu_run(fused_env)
    raw, direct, counts = reference(case)
    assert bytes(run[case + "/kernel"]).decode() == "accumulate_counts"
    assert int(run[case + "/block"][0]) == block
    # the instance: a word per locus when no locus range of the packing is longer than 4094 loci (128-cell blocks)
    assert int(run[case + "/words"][0]) == int(words) and int(run[case + "/list_words"][0]) == int(words)
    assert tuple(int(c) for c in run[case + "/counts"]) == counts
    # three further launches of the tile range, four of the stored list: the first launch's accumulator and counters
    assert bool(run[case + "/same"][0]) and bool(run[case + "/same_counts"][0])
    got = run[case + "/raw"]
    err_direct, err_ref = gu.normwise_err(got, direct), gu.normwise_err(got, raw)
    print("%s: norm-wise %.2e against the direct sums, %.2e against the oracle" % (case, err_direct, err_ref))
    heavy = counts[1] / max(1.0, n * (n - 1) / 2) > 1e4  # (the oracle's own cancellation, test_gpu_parity.py)
    assert err_direct <= TOL
    assert err_ref <= (5e-8 if heavy else TOL)
    assert np.any(got != 0)
