"""Locus filter: the CPU oracle against the reference vectors and the compiled
reference, and the product's host-side significance test against both; and what the edge pileups of
tests/filter_cases.py do on the oracle, which tests/test_gpu_filter.py relies on. CPU only."""
import numpy as np
import pytest

import secedo_amd
from oracle import bindings as ob
from tests import filter_cases as fc
from tests import golden_util as gu
from tests.pileup_gen import random_pileup


def test_is_significant_reference_kats_and_vectors():
    """tests/golden/filter_kat.npz: the five known-answer strings of the reference's
    tests/test_is_significant.cpp:46-90 (as base counts) + 3000 decisions of the compiled reference."""
    z = np.load(gu.GOLDEN + "/filter_kat.npz")
    expect_first = [0, 1, 0, 0, 0]  # Cov52OneDifferent, Cov52TenDifferent, Cov59TwoDifferent, AtLimit, Paradox
    assert z["significant"][:5].tolist() == expect_first
    for c, th, cp, want in zip(z["counts"], z["theta"], z["cell_proportion"], z["significant"]):
        assert ob.oracle_is_significant(c, float(th), int(cp)) == bool(want)
        assert secedo_amd.Filter(float(th), int(cp)).is_significant(c) == bool(want)


@pytest.mark.parametrize("name", gu.filter_fixture_names())
def test_oracle_filter_matches_reference_vectors(name):
    p, i2p, theta, cp, expect = gu.load_filter(name)
    got = ob.oracle_filter(p, i2p, theta, cp)
    for a, b in zip(got[:5], expect[:5]):
        assert np.array_equal(a, b)
    assert got[5] == expect[5]


@pytest.mark.skipif(not ob.have_ref(), reason="oracle/_ref not built")
def test_oracle_filter_equals_reference_live():
    rng = np.random.default_rng(5)
    for seed in range(3):
        n = 50
        p = random_pileup(300 + seed, n, 2, 200, 30, 300, err=0.2)
        i2p = np.arange(n, dtype=np.uint32)
        drop = rng.random(n) < 0.4
        i2p[drop] = ob.NO_POS
        for cp in (0, 4):
            a = ob.oracle_filter(p, i2p, 0.01, cp)
            b = ob.ref_filter(p, i2p, 0.01, cp)
            assert all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5])) and a[5] == b[5]


def _kept_pos(expect):
    return expect[1].astype(np.int64)


@pytest.mark.parametrize("theta,cp", fc.kat_groups())
def test_kat_pileups_reproduce_the_reference_decisions(theta, cp):
    """The known answers as pileups (tests/filter_cases.py): oracle_filter keeps the loci the reference called
    significant, and every group both keeps and drops."""
    _, _, _, significant = fc.kat()
    rows = fc.kat_pileup(theta, cp)[2]
    kept = fc.kat_kept_rows(theta, cp, _kept_pos(fc.expected("kat_pileup", theta, cp, theta, cp)))
    assert np.array_equal(kept, rows[significant[rows] == 1]) and 0 < len(kept) < len(rows)


def test_kat_pileups_cover_the_file_and_every_threshold_column():
    counts, _, _, significant = fc.kat()
    groups = fc.kat_groups()
    rows = np.concatenate([fc.kat_pileup(th, cp)[2] for th, cp in groups])
    assert len(groups) == 15 and np.array_equal(np.sort(rows), np.arange(len(counts)))
    assert sum(fc.kat_pileup(th, cp)[0].n_entries for th, cp in groups) == int(counts.sum())
    assert significant[:5].tolist() == list(fc.KAT_NAMED_WANT)
    cov = counts.astype(np.int64).sum(1)[significant == 1]
    assert set(np.clip(np.rint(cov / 10.) - 1, 0, 19).astype(int)) == set(range(20))
    assert {25, 45, 205, 259} <= set(counts.astype(np.int64).sum(1).tolist())


def test_edge_pileups_both_keep_and_drop():
    """The conditions the GPU tests rely on, on the oracle."""
    n = len(fc.TIE_CLAMP_COVERAGE)
    depth = np.diff(fc.tie_clamp()[0].locus_entry_off.astype(np.int64))
    assert depth.tolist() == list(fc.TIE_CLAMP_COVERAGE)
    for theta, cp in fc.TIE_CLAMP_SETTINGS:
        assert 0 < len(fc.expected("tie_clamp", theta, cp)[1]) < n
    for shape, (_, theta, cp) in fc.U32_SHAPES.items():
        p, i2p = fc.u32(shape)[:2]
        assert int(p.id_base.max()) > 0xFFFF
        assert np.all((i2p == fc.NO_POS) | (i2p < fc.NO_POS)) and 0.4 < np.mean(i2p == fc.NO_POS) < 0.6
        assert 0 < len(fc.expected("u32", theta, cp, shape)[1]) < p.n_loci
    assert int(np.diff(fc.u32("deep")[0].locus_entry_off.astype(np.int64)).max()) > 256
    p, i2p = fc.deep16()
    depth = np.diff(p.locus_entry_off.astype(np.int64))
    assert int(p.id_base.max()) <= 0xFFFF and depth.min() > 256 and depth.max() > 1024 and p.n_entries > 90000
    assert len(set((p.locus_entry_off[:-1] & np.uint64(3)).tolist())) == 4  # every phase of the aligned start
    for theta, cp in fc.DEEP16_SETTINGS:
        assert 0 < len(fc.expected("deep16", theta, cp)[1]) < p.n_loci
    for r in (1, 2, 3):
        p, i2p = fc.tail(r)
        assert p.n_entries % 4 == r and 0 < len(fc.expected("tail", 0.01, 4, r)[1])
        assert int(fc.expected("tail", 0.01, 4, r)[1][-1]) == int(p.locus_pos[-1])  # the cut locus is kept


def test_wrap_pileup_decisions():
    """Loci deeper than 65535 (tests/filter_cases.py wrap): the reference's uint16 base counts wrap, the entries it
    keeps do not."""
    p, _ = fc.wrap()
    assert np.diff(p.locus_entry_off.astype(np.int64)).tolist() == [sum(c) for c in fc.WRAP_COUNTS]
    e = fc.expected("wrap", 0.01, 4)
    assert _kept_pos(e).tolist() == [1, 4, 5]  # (40, 12) after the wrap; the counts alone; the unwrapped twin
    assert np.diff(e[2].astype(np.int64)).tolist() == [65588, 65600, 54]
    assert secedo_amd.Filter(0.01, 4).is_significant([40000, 30000, 0, 0]) is False  # c3 < 1.5 c2 on the host
    assert _kept_pos(fc.expected("wrap", 0.05, 4)).tolist() == [1, 5]  # [60000, 5000, 600, 0] flips
    assert ob.oracle_is_significant([60000, 5000, 600, 0], 0.001, 4)
    p3, i2p3 = fc.wrap(True)
    inside = np.add.reduceat((i2p3[p3.id_base >> 2] != fc.NO_POS).astype(np.int64),
                             p3.locus_entry_off[:-1].astype(np.int64))
    assert (inside[:4] < 65536).all() and inside[2] > 40000  # raw depth above the line, depth inside below it
    for theta, cp in fc.WRAP_SETTINGS:
        kept = len(fc.expected("wrap", theta, cp, True)[1])
        print("a third of the cells outside, theta", theta, "kept", _kept_pos(fc.expected("wrap", theta, cp, True)))
        assert 0 < kept < len(fc.WRAP_COUNTS)


def test_filter_argument_errors():
    with pytest.raises(ValueError):
        secedo_amd.Filter(0.01, 7)
    with pytest.raises(ValueError):
        secedo_amd.Filter(0.01).is_significant([1, 2, 3])
