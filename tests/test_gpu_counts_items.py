"""accumulate_counts at the boundaries of its items, groups and ring, in both of its 128-cell instances: the one that
stages a 32-bit word per locus (no locus range longer than 4094 loci) and the one with 16-bit offsets (ranges of up to
8190 loci). Pileups with a chosen number of entries per (cell block, locus), against the oracle: the un-normalised
matrix norm-wise to 1e-9 (test_gpu_parity.py's bar; for pileups with more than 1e4 pairs per cell pair against the
oracle's direct sums, as there), both work counters exactly.

The switch between the fused correction and correct_tiles is read once per process, so the GPU side of every case runs
in two child processes (default, SECEDO_CORRECT_FUSED=0); the oracle's side is computed once and shared."""
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
BLOCK = 128
MFL = 1000
T = 2
RATES = (0.01, 0.5, 0.01)
FORCED = (0, 1, 2, 3, 4, 5, 8, 9, 17)  # group and ring boundaries: GROUP is 2, 3 or 4; 9 and 17: two and four ring trips


def block_counts(case):
    """The case's entries per (locus, cell block): (n_cells, counts[L, nb])."""
    rng = np.random.default_rng(1000 + sum(map(ord, case)))
    if case in ("groups", "groups_host"):
        # one range of 2500 loci (9500 entries per block), 3.8 entries per block and locus: GROUP 4, the word instance,
        # one workgroup per tile
        n, L, lam = 300, 2500, 3.8
    elif case == "two_ranges":
        # 17500 entries per block: two ranges, workgroups that begin inside a range (row_begin, dsh)
        n, L, lam = 300, 3500, 5.0
    elif case == "span_4094":
        n, L, lam = 260, 4094, 1.5  # one range of exactly 4094 loci: still the word instance (GROUP 2)
    elif case == "span_4095":
        n, L, lam = 260, 4095, 1.5  # one locus more: the instance with 16-bit offsets
    elif case == "deep_unstaged":
        n, L, lam = 300, 1500, 2.8  # GROUP 3
    elif case == "full_diagonal_range":
        n, L, lam = 300, 3072, 3.0
    else:
        raise KeyError(case)
    nb = (n + BLOCK - 1) // BLOCK
    counts = rng.poisson(lam, size=(L, nb))
    # the forced loci: every block the same number, and mixed ones (an empty block beside a full one)
    for k, v in enumerate(FORCED):
        counts[100 + 7 * k, :] = v
        counts[300 + 7 * k, :] = [FORCED[(k + 3 * b) % len(FORCED)] for b in range(nb)]
        counts[L - 40 + 2 * k, :] = v  # ... and at the end of the last range: a last ring batch of few items
    if case == "two_ranges":
        counts[:1500, 2] = 0      # a block without entries in (nearly all of) the first range
        counts[700, :] = [300, 40, 33]   # wide items: c >= 32, and c >= 256 (beyond the staged word's 8 bits)
        counts[2900, :] = [31, 32, 260]  # (block 2 has 44 cells: many entries of one cell, skipped on the diagonal)
    if case in ("span_4094", "span_4095"):
        counts[2000, :] = [270, 35, 3]
    if case == "deep_unstaged":
        counts[640, :] = [12500, 20, 6]  # more than the 12288 entries a range stages: paired from HBM
        counts[641, :] = [40, 3, 0]
    if case == "full_diagonal_range":
        # block 0 has exactly 12288 entries in the one range: in tile (0, 0) the last entry's first column entry is the
        # end of the staging area (j0 == CAPJ, c == 0)
        counts[:, 0] = 4
        counts[:, 1:] = np.minimum(counts[:, 1:], 3)
    # the last three loci are far away (everything before them is flushed), one entry each, in block 1
    counts[L - 3:, :] = 0
    counts[L - 3:, 1] = 1
    if case == "full_diagonal_range":
        counts[0, 0] += 12288 - counts[:, 0].sum()
        assert counts[:, 0].sum() == 12288 and counts[0, 0] < 32
    return n, counts


@functools.lru_cache(maxsize=None)
def pileup(case):
    n, counts = block_counts(case)
    rng = np.random.default_rng(2000 + sum(map(ord, case)))
    L, nb = counts.shape
    rows, pos, rid = [], 1000, 0
    last = {}  # cell -> (read id, loci it has so far): some reads go on at the next locus
    for l in range(L):
        pos += 5000 if l >= L - 3 else 40
        ref = int(rng.integers(0, 4))
        ents, now = [], {}
        for b in range(nb):
            cells_b = min(BLOCK, n - b * BLOCK)
            c = int(counts[l, b])
            cells = rng.choice(cells_b, size=c, replace=c > cells_b) + b * BLOCK
            for cell in cells.tolist():
                base = ref if rng.random() < 0.7 else int(rng.integers(0, 4))
                prev = last.get(cell)
                if prev is not None and prev[1] < 5 and cell not in now and rng.random() < 0.3:
                    r, k = prev[0], prev[1] + 1  # a multi-locus read (at most one entry per locus: nothing is dropped)
                else:
                    r, k = rid, 1
                    rid += 1
                now[cell] = (r, k)
                ents.append((r, cell, base))
        last = now
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


# case -> (packing, runs the word instance, single range)
CASES = {
    "groups": ("auto", True, True),
    "groups_host": ("host", True, True),
    "two_ranges": ("auto", True, False),
    "span_4094": ("auto", True, True),
    "span_4095": ("auto", False, True),
    "deep_unstaged": ("auto", True, False),
    "full_diagonal_range": ("auto", True, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_generated_pileups_have_the_intended_counts(case):
    """CPU: the pileup holds the intended number of entries per (cell block, locus), and the oracle pairs exactly
    them: its update counter is the number of entry pairs of two different cells at a locus."""
    n, counts = block_counts(case)
    _, p = pileup(case)
    L, nb = counts.shape
    assert p.n_loci == L
    cell = (p.id_base >> 2).astype(np.int64)
    locus = np.repeat(np.arange(L), np.diff(p.locus_entry_off.astype(np.int64)))
    got = np.zeros((L, nb), dtype=np.int64)
    np.add.at(got, (locus, cell // BLOCK), 1)
    assert np.array_equal(got, counts)
    if case != "full_diagonal_range":  # (its block 0 has four entries everywhere)
        for v in FORCED:
            assert np.any(np.all(got == v, axis=1)), v
    per_cell = np.zeros((L, n), dtype=np.int64)
    np.add.at(per_cell, (locus, cell), 1)
    n_l = per_cell.sum(axis=1)
    pairs = int((n_l * (n_l - 1) // 2).sum() - (per_cell * (per_cell - 1) // 2).sum())
    _, _, (updates, read_pairs) = reference(case)
    assert updates == pairs
    assert 0 < read_pairs <= updates
    # 16-bit pair counters: no cell pair can collect 65536 pairs (else another pair kernel runs)
    assert int((per_cell.astype(np.int64) ** 2).sum(axis=0).max()) < 65536


SCRIPT = r'''
import sys
import numpy as np, torch
sys.path.insert(0, ROOT)
import secedo_amd
from secedo_amd import _lib
from tests.test_gpu_counts_items import pileup, CASES, MFL, T, RATES, BLOCK

out = {}
L = _lib.lib()
for case, (packing, words, single) in sorted(CASES.items()):
    n, p = pileup(case)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        plan.set_packing(packing)
        plan.prepare(p, n, MFL, None, T, block_cells=BLOCK)
        out[case + "/kernel"] = np.frombuffer(plan.pair_kernel.encode(), dtype=np.uint8)
        out[case + "/block"] = np.array([plan.block_cells])
        nt = plan.num_tiles
        acc = plan.new_acc()
        plan.accumulate(acc, *RATES)
        out[case + "/counts"] = np.asarray(plan.last_counts(), dtype=np.uint64)
        out[case + "/words"] = np.array([L.secedo_simmat_last_locus_words(plan._h)])
        out[case + "/fused"] = np.array([L.secedo_simmat_last_correction_fused(plan._h)])
        out[case + "/raw"] = plan.finalize_raw(acc).cpu().numpy()
        # every tile as a list, stored: one workgroup per tile when the pileup is one range -- the fused correction
        acc2 = plan.new_acc()
        acc2.fill_(-9)
        plan.accumulate_list(acc2, *RATES, np.arange(nt, dtype=np.uint32), overwrite=True)
        out[case + "/list_counts"] = np.asarray(plan.last_counts(), dtype=np.uint64)
        out[case + "/list_fused"] = np.array([L.secedo_simmat_last_correction_fused(plan._h)])
        out[case + "/list_words"] = np.array([L.secedo_simmat_last_locus_words(plan._h)])
        torch.cuda.synchronize()
        out[case + "/list_equal"] = np.array([torch.equal(acc, acc2)])
        # launches of few tiles: several workgroups per tile, shares of the row entries that begin inside a range
        acc3 = plan.new_acc()
        split = np.zeros(2, dtype=np.uint64)
        per_tile = []
        for lo, hi in ((0, 1), (1, 3), (3, nt)):
            plan.accumulate(acc3, *RATES, lo, hi)
            split += np.asarray(plan.last_counts(), dtype=np.uint64)
            per_tile.append(L.secedo_simmat_last_workgroups(plan._h) / (hi - lo))
        out[case + "/split_wg_per_tile"] = np.array(per_tile)
        torch.cuda.synchronize()
        out[case + "/split_counts"] = split
        out[case + "/split_equal"] = np.array([torch.equal(acc, acc3)])
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
def test_counts_items_match_the_oracle(case, fused_env):
    packing, words, single = CASES[case]
    run = gpu_run(fused_env)
    raw, direct, counts = reference(case)
    n, _ = pileup(case)
    assert bytes(run[case + "/kernel"]).decode() == "accumulate_counts"
    assert int(run[case + "/block"][0]) == BLOCK
    # the instance is chosen by the longest locus range of the packing
    assert int(run[case + "/words"][0]) == int(words) and int(run[case + "/list_words"][0]) == int(words)
    # a stored tile list is corrected in the pair kernel's epilogue where the plan gives every tile one workgroup (a
    # pileup the packing cut into one range: it may cut a short one in two); these few tiles as a range never are
    assert int(run[case + "/fused"][0]) == 0
    list_fused = int(run[case + "/list_fused"][0])
    if not fused_env or not single:
        assert list_fused == 0
    elif case == "full_diagonal_range":
        assert list_fused == 1
    for key in ("/counts", "/list_counts", "/split_counts"):
        assert tuple(int(c) for c in run[case + key]) == counts, key
    assert bool(run[case + "/list_equal"][0]) and bool(run[case + "/split_equal"][0])
    # the launches of one and two tiles did give a tile several workgroups (a tile gets at most one per locus range:
    # the pileups of several ranges; their later shares begin inside the row side, row_begin / dsh)
    if not single:
        assert np.all(run[case + "/split_wg_per_tile"][:2] > 1), run[case + "/split_wg_per_tile"]
    got = run[case + "/raw"]
    err_direct, err_ref = gu.normwise_err(got, direct), gu.normwise_err(got, raw)
    print("%s: norm-wise %.2e against the direct sums, %.2e against the oracle" % (case, err_direct, err_ref))
    heavy = counts[1] / max(1.0, n * (n - 1) / 2) > 1e4  # (the oracle's own cancellation, test_gpu_parity.py)
    assert err_direct <= TOL
    assert err_ref <= (5e-8 if heavy else TOL)
    assert np.any(got != 0)
