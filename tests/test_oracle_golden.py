"""The CPU oracle against the vectors generated from the compiled reference (CPU only)."""
import numpy as np
import pytest

from oracle import bindings as ob
from tests import golden_util as gu

TOL = 1e-9  # norm-wise; the oracle actually lands at <= 1e-13


@pytest.mark.parametrize("name", gu.fixture_names())
def test_oracle_matches_reference_vectors(name):
    p, cases = gu.load(name)
    assert cases
    for c in cases:
        got = ob.oracle_compute(p, c["num_cells"], c["mfl"], c["g2p"], c["eps"], c["h"], c["theta"],
                                c["T"], c["norm"])
        ref = c["out"]
        assert got.shape == ref.shape
        assert gu.normwise_err(got, ref) <= 1e-12, (name, c["T"], c["norm"])
        assert np.array_equal(got, got.T, equal_nan=True)
        assert np.all(np.diag(got) == 0)


def test_oracle_llr_kat_table():
    """D(x_s,x_d) read off reference matrices vs the oracle's restated formulas."""
    z = np.load(gu.GOLDEN + "/kat_llr_table.npz")
    for pi, (eps, h, theta) in enumerate(z["params"]):
        for ci, (xs, xd) in enumerate(z["combos"]):
            d = ob.oracle_log_prob_diff(int(xs), int(xd), eps, h, theta) \
                - ob.oracle_log_prob_same(int(xs), int(xd), eps, h, theta)
            assert abs(d - z["table"][pi, ci]) <= 1e-12 * max(1.0, abs(d)), (eps, h, theta, xs, xd)


def test_probe_facts():
    """tail drop, thread-count dependence, joint multi-locus term."""
    p, cases = gu.load("probe_single_locus")
    assert np.all(cases[0]["out"] == 0)  # ADD_MIN of an all-zero D
    assert np.all(cases[1]["out"][~np.eye(4, dtype=bool)] == 0.5)  # EXPONENTIATE
    p, cases = gu.load("probe_flush_T1_vs_T2")
    t1, t2 = cases[0]["out"], cases[3]["out"]
    assert np.any(t1 != 0) and np.all(t2 == 0)
    p, cases = gu.load("probe_multi_locus_pair")
    expo = cases[1]["out"]
    d01 = np.log(1.0 / expo[0, 1] - 1.0)
    assert abs(d01 - 0.0171106405755368) < 1e-9  # D(1,1), not D(1,0)+D(0,1)


def test_invalid_normalization():
    p, cases = gu.load("probe_single_locus")
    with pytest.raises(ValueError):
        ob.oracle_compute(p, 4, 1000, None, 0.01, 0.5, 0.01, 1, "BOGUS")


def test_oracle_refuses_read_pairs_beyond_the_reference_tables():
    """A read pair that shares >= max_fragment_length loci makes the reference index past its
    max_fragment_length-sized tables (similarity_matrix.cpp:314-317, :330): the oracle returns an error for
    such a pileup instead of following it out of bounds (it used to crash the test process)."""
    import pytest
    from oracle import bindings as ob
    from tests.pileup_gen import from_rows
    # two reads of different cells over 12 adjacent loci, then far loci of a third cell so that they flush
    rows = [(100 + l, [(1, 0, l & 3), (2, 1, (l + l // 5) & 3)]) for l in range(12)]
    rows += [(50000 + 5000 * k, [(10 + k, 2, 0)]) for k in range(6)]
    p = from_rows([rows])
    ob.oracle_compute(p, 3, 13, None, 0.01, 0.5, 0.01, 1, "ADD_MIN")  # 12 shared loci < 13 table rows: fine
    with pytest.raises(ValueError, match="max_fragment_length"):
        ob.oracle_compute(p, 3, 12, None, 0.01, 0.5, 0.01, 1, "ADD_MIN")


@pytest.mark.parametrize("name", ["clustered", "sparse", "deep", "deep_offdiag", "clustered_thin", "sparse_thin",
                                  "deep_thin"])
def test_pair_kernel_pileups_have_the_claimed_properties(name):
    """tests/pileup_gen.py: pair_kernel_pileup -- what decides the pair kernel of the GPU path (test_gpu_parity.py holds
    each of them to the oracle): the bound on the pairs of one cell pair (the 16-bit count tile below 65536), the share
    of entries that belong to multi-locus reads (the window masks are staged above 5 %), the entries per cell block
    (a locus range stages 2048 to 12288 of them), and for the deep locus what it was built for."""
    from tests.pileup_gen import pair_kernel_pileup
    p, n, block, kernel, tile_list = pair_kernel_pileup(name)
    block = block or (64 if n <= 200 else 128)
    L = p.n_loci
    cell = (p.id_base >> 2).astype(np.int64)
    locus = np.repeat(np.arange(L), np.diff(p.locus_entry_off.astype(np.int64)))
    per_cell = np.zeros((L, n), dtype=np.int64)
    np.add.at(per_cell, (locus, cell), 1)
    pair_bound = int((per_cell ** 2).sum(axis=0).max())
    key = p.read_ids.astype(np.int64) * (int(p.chr_locus_off.size)) + np.searchsorted(p.chr_locus_off[1:], locus, "right")
    reads, inverse = np.unique(key, return_inverse=True)
    loci_of_read = np.bincount(np.unique(np.stack([inverse, locus]), axis=1)[0], minlength=len(reads))
    multi_share = float(np.mean(loci_of_read[inverse] > 1))  # (entries of reads with entries at two or more loci)
    per_block = np.bincount(cell // block)
    ob.oracle_compute(p, n, 1000, None, 0.01, 0.5, 0.01, 2, "ADD_MIN")
    updates, read_pairs = ob.oracle_last_updates(), ob.oracle_last_read_pairs()
    assert 0 < read_pairs <= updates
    if name.endswith("_thin"):
        # the two entries of the last block, and their reads are flushed: the pair of the two is counted
        base_p, base_n, _, base_kernel, _ = pair_kernel_pileup(name[:-5])
        assert kernel == base_kernel and per_block[-1] == 2 and n == base_n // 64 * 64 + 64 + 2
        ob.oracle_compute(base_p, base_n, 1000, None, 0.01, 0.5, 0.01, 2, "ADD_MIN")
        assert updates == ob.oracle_last_updates() + 2 * int(per_cell[3].sum() - 2) + 1
    elif kernel == "accumulate_masks":
        assert multi_share > 0.2 and len(per_block) == 4 and per_block[:3].min() > 4 * 2048
        assert max(tile_list) == 4 * 5 // 2 - 1
    elif kernel == "accumulate_counts":
        assert multi_share < 0.04 and pair_bound < 65536
    else:
        assert multi_share < 0.04 and pair_bound >= 65536
        per_block_locus = np.zeros((L, 2), dtype=np.int64)
        np.add.at(per_block_locus, (locus, cell // 64), 1)
        deep = int(np.argmax(per_block_locus[:, 0]))
        assert tuple(per_block_locus[deep]) == (5000, 300 if name == "deep_offdiag" else 0) and 5000 > 4096
        assert np.all(np.delete(per_block_locus, deep, axis=0) == 60) and L == 41
        assert np.all(np.diff(p.locus_pos.astype(np.int64)) == 40)
        assert updates > 5000 * 4700 // 2 and read_pairs < updates  # its reads are flushed; some pairs are joint
        assert tile_list == [0, 2]
