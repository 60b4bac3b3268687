"""CPU tests of the EM refinement's oracle (oracle/em_oracle.c) against the vectors of the compiled
reference (tests/golden/em_cases.npz: the five cases of the reference's own
tests/test_expectation_maximization.cpp and three random pileups) and, when oracle/_ref is present,
live against the reference; of the high-precision restatement tests/em_ref.py against the oracle; and of the
conditions under which the edge cases of tests/em_cases.py have an iteration count the GPU must reproduce."""
import os

import numpy as np
import pytest

from oracle import bindings as ob
from secedo_amd.pileup import FlatPileup
from tests import em_cases as ec
from tests.em_ref import em_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def em_cases():
    z = np.load(os.path.join(GOLDEN, "em_cases.npz"), allow_pickle=False)
    names = sorted({k.split("__")[0] for k in z.files if "__" in k})
    out = []
    for n in names:
        g = lambda k: z[n + "__" + k]  # noqa: E731
        p = FlatPileup(g("chr_locus_off"), g("locus_pos"), g("locus_entry_off"), g("read_ids"), g("id_base"))
        out.append((n, p, g("id_to_pos"), g("prob_in"), g("prob_out"), int(g("iterations"))))
    return float(z["theta"]), out


THETA, CASES = em_cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_oracle_matches_reference_vectors(name):
    _, p, i2p, prob_in, prob_out, iters = next(c for c in CASES if c[0] == name)
    got, it = ob.oracle_em(p, i2p, THETA, prob_in)
    assert np.array_equal(got, prob_out) and it == iters


def test_reference_test_expectations_hold_for_the_vectors():
    """The assertions of tests/test_expectation_maximization.cpp:15-85, on the stored reference output."""
    out = {c[0]: c[4] for c in CASES}
    assert out["one_cell"][0] == 1.0
    assert abs(out["two_cells_same"][1] - out["two_cells_same"][0]) <= 1e-3
    assert abs(abs(out["two_cells_different"][0] - out["two_cells_different"][1]) - 1.0) <= 1e-3
    assert np.max(np.abs(out["four_cells_22"] - np.array([0, 0, 1, 1]))) <= 1e-3
    assert np.max(np.abs(out["four_cells_31"] - np.array([0, 1, 0, 0]))) <= 1e-3


def test_oracle_rejects_what_the_reference_cannot_index():
    _, p, i2p, prob_in, _, _ = next(c for c in CASES if c[0] == "random_40")
    with pytest.raises(RuntimeError):
        ob.oracle_em(p, i2p, THETA, prob_in[:20])  # group ids up to 39 index a 20-vector
    with pytest.raises(RuntimeError):
        ob.oracle_em(p, i2p[:10], THETA, prob_in)  # groups outside id_to_pos


REF_TOL = 1e-12  # em_ref (np.longdouble sums) against the oracle (double, sequential sums)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_em_ref_matches_oracle_on_reference_vectors(name):
    _, p, i2p, prob_in, prob_out, iters = next(c for c in CASES if c[0] == name)
    got, it, _ = em_ref(p, i2p, THETA, prob_in)
    assert it == iters and (len(prob_out) == 0 or np.max(np.abs(got - prob_out)) <= REF_TOL)


@pytest.mark.parametrize("name", list(ec.CASES))
def test_edge_case_conditions_and_em_ref(name):
    """What tests/test_gpu_em.py relies on: every case of tests/em_cases.py settles on the oracle within MAX_ITER
    iterations without a NaN, and no iteration of the high-precision run comes within MARGIN of the 1e-2 edge."""
    p, i2p, theta, prob_in = ec.CASES[name]
    want, iters = ec.oracle(name)
    assert not np.any(np.isnan(want)) and 1 <= iters <= ec.MAX_ITER
    got, it, margin = em_ref(p, i2p, theta, prob_in)
    print(name, "iterations", it, "margin", margin, "max |em_ref - oracle|", np.max(np.abs(got - want)))
    assert margin >= ec.MARGIN
    assert it == iters and np.max(np.abs(got - want)) <= REF_TOL


@pytest.mark.parametrize("n", ec.BOUNDARY_N)
def test_all_ones_and_all_zeros_are_fixed_points(n):
    for kind in ("ones", "zeros"):
        name = "boundary_n%d_%s" % (n, kind)
        got, it = ec.oracle(name)
        assert it == 1 and np.array_equal(got, ec.CASES[name][3])


def test_edge_cases_are_what_they_claim():
    p = ec.CASES["boundary_n66_clones"][0]
    assert p.n_chr == 3 and p.chr_locus_off.tolist() == [0, 9, 9, 17]
    assert np.diff(p.locus_entry_off.astype(np.int64)).tolist() == list(ec.DEPTHS)
    for l in range(2, p.n_loci, 3):  # every third locus: the lower clone only
        assert np.all(p.id_base[int(p.locus_entry_off[l]):int(p.locus_entry_off[l + 1])] >> 2 < 33)
    for n in (1023, 1025):  # most cells have no entry
        assert len(np.unique(ec.CASES["boundary_n%d_clones" % n][0].id_base >> 2)) <= ec.ACTIVE < n // 2
    for kind in ("full", "in_clone"):
        p16, i2p16 = ec.CASES["perm16_" + kind][:2]
        p32, i2p32 = ec.CASES["perm32_" + kind][:2]
        assert int(p16.id_base.max()) <= 0xFFFF < int(p32.id_base.min()) and len(np.unique(p32.id_base >> 2)) <= 100
        for p, i2p in ((p16, i2p16), (p32, i2p32)):
            used = np.unique(p.id_base >> 2)
            assert np.array_equal(np.sort(i2p), np.arange(len(i2p)))  # a permutation ...
            assert np.mean(i2p[used] != used) > 0.8  # ... that moves the cells which have entries


@pytest.mark.skipif(not ob.have_ref(), reason="oracle/_ref not built (no /root/reference here)")
def test_oracle_matches_reference_live():
    from tests.pileup_gen import random_pileup
    rng = np.random.default_rng(5)
    for seed, n in ((1, 30), (2, 90)):
        p = random_pileup(seed, n, 2, 250, 15, 300)
        prob = np.clip(rng.random(n), 0.02, 0.98)
        i2p = rng.permutation(n).astype(np.uint32)
        assert np.array_equal(ob.oracle_em(p, i2p, 1e-3, prob)[0], ob.ref_em(p, i2p, 1e-3, prob))
