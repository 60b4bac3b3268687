"""Locus filter on the GPU (through the C-ABI) against the reference vectors and the CPU oracle:
exact equality of every output array (integer / index work) and of the average coverage."""
import numpy as np
import pytest

import secedo_amd
from oracle import bindings as ob
from tests import filter_cases as fc
from tests import golden_util as gu
from tests.pileup_gen import from_rows, random_pileup

pytestmark = pytest.mark.gpu


def _same(got_pileup, got_cov, expect):
    o_chr, o_pos, o_off, o_rid, o_idb, cov = expect
    assert np.array_equal(got_pileup.chr_locus_off, o_chr)
    assert np.array_equal(got_pileup.locus_pos, o_pos)
    assert np.array_equal(got_pileup.locus_entry_off, o_off)
    assert np.array_equal(got_pileup.read_ids, o_rid)
    assert np.array_equal(got_pileup.id_base, o_idb)
    assert got_cov == cov


@pytest.mark.parametrize("name", gu.filter_fixture_names())
def test_hip_filter_matches_reference_vectors(name):
    p, i2p, theta, cp, expect = gu.load_filter(name)
    got, cov = secedo_amd.Filter(theta, cp).filter(p, i2p, "", 1)
    _same(got, cov, expect)


@pytest.mark.parametrize("seed,n,theta,cp", [(401, 80, 0.01, 4), (402, 300, 0.001, 1), (403, 20, 0.05, 3)])
def test_hip_filter_matches_oracle_random(seed, n, theta, cp):
    rng = np.random.default_rng(seed)
    p = random_pileup(seed, n, 3, 400, 40, 500, err=0.15)
    i2p = np.arange(n, dtype=np.uint32)
    i2p[rng.random(n) < 0.35] = secedo_amd.NO_POS
    got, cov = secedo_amd.Filter(theta, cp).filter(p, i2p)
    _same(got, cov, ob.oracle_filter(p, i2p, theta, cp))


def test_filter_edge_cases():
    f = secedo_amd.Filter(0.01)
    # empty pileup and empty chromosomes (reference tests/test_is_significant.cpp:108-112 Filter.Empty)
    got, cov = f.filter(from_rows([[], []]), np.arange(4, dtype=np.uint32))
    assert got.n_loci == 0 and got.n_entries == 0 and cov == 0 and got.chr_locus_off.tolist() == [0, 0, 0]
    # every cell outside the sub-cluster: nothing survives
    p = random_pileup(404, 30, 1, 100, 30, 300, err=0.2)
    got, cov = f.filter(p, np.full(30, secedo_amd.NO_POS, dtype=np.uint32))
    assert got.n_loci == 0 and cov == 0


def test_filter_then_similarity_matrix_stays_in_hbm():
    """divide_cluster's first two steps (spectral_clustering.cpp:336-337, :354-356): filter, then the
    similarity matrix of the filtered pileup, with the pileup resident in HBM in between."""
    n = 120
    rng = np.random.default_rng(405)
    p = random_pileup(405, n, 2, 500, 40, 400, err=0.15)
    i2p = np.full(n, secedo_amd.NO_POS, dtype=np.uint32)
    inside = np.flatnonzero(rng.random(n) < 0.6)
    i2p[inside] = np.arange(len(inside), dtype=np.uint32)
    o_chr, o_pos, o_off, o_rid, o_idb, cov_ref = ob.oracle_filter(p, i2p, 0.01, 4)
    fp = secedo_amd.FlatPileup(o_chr, o_pos, o_off, o_rid, o_idb)
    ref = ob.oracle_compute(fp, len(inside), 1000, i2p, 0.01, 0.5, 0.01, 4, "ADD_MIN")
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, np.arange(n, dtype=np.uint32), n)
        filtered, cov = secedo_amd.filter_resident(plan, res, i2p, 0.01, 4)
        assert cov == cov_ref and filtered["n_loci"] == len(o_pos) and filtered["n_entries"] == len(o_rid)
        plan.prepare_resident(filtered, len(inside), 1000, 4)
        acc = plan.new_acc()
        plan.accumulate(acc, 0.01, 0.5, 0.01)
        got = plan.finalize(acc, "ADD_MIN").cpu().numpy()
    assert gu.normwise_err(got, ref) <= 1e-9


# ---- the kernels' edges (tests/filter_cases.py; what each case does on the oracle: tests/test_filter_cpu.py) ----

def _run(case, theta, cp, *key):
    p, i2p = getattr(fc, case)(*key)[:2]
    got, cov = secedo_amd.Filter(theta, cp).filter(p, i2p)
    _same(got, cov, fc.expected(case, theta, cp, *key))
    return got


_kat_kept = {}


def _kat_run(theta, cp):
    if (theta, cp) not in _kat_kept:
        got = _run("kat_pileup", theta, cp, theta, cp)
        _kat_kept[theta, cp] = fc.kat_kept_rows(theta, cp, got.locus_pos)
    return _kat_kept[theta, cp]


@pytest.mark.parametrize("theta,cp", fc.kat_groups())
def test_k_verdict_matches_the_reference_decisions(theta, cp):
    """The 3005 decisions of the compiled reference (coverage 2..259: every threshold column, the ties of the
    column choice, the clamp to the last one), each as a locus."""
    _, _, _, significant = fc.kat()
    rows = fc.kat_pileup(theta, cp)[2]
    assert np.array_equal(_kat_run(theta, cp), rows[significant[rows] == 1])


@pytest.mark.parametrize("row,name,want", [(i, n, w) for i, (n, w) in enumerate(zip(fc.KAT_NAMED, fc.KAT_NAMED_WANT))])
def test_k_verdict_on_the_reference_named_cases(row, name, want):
    """tests/test_is_significant.cpp:46-90 of the reference, through the device kernels."""
    _, theta, cp, _ = fc.kat()
    assert (row in _kat_run(float(theta[row]), int(cp[row]))) == bool(want)


@pytest.mark.parametrize("theta,cp", fc.TIE_CLAMP_SETTINGS)
def test_tie_and_clamp_coverages(theta, cp):
    _run("tie_clamp", theta, cp)


@pytest.mark.parametrize("third_outside", [False, True])
@pytest.mark.parametrize("theta,cp", fc.WRAP_SETTINGS)
def test_wrap_and_host_redecision(theta, cp, third_outside):
    """Loci of more than 65535 entries inside the cluster are decided on the host, on base counts that wrap in
    uint16 like the reference's, and keep all their entries; with a third of the cells outside, the same loci stay
    below the line and on the device."""
    _run("wrap", theta, cp, third_outside)


@pytest.mark.parametrize("shape", list(fc.U32_SHAPES))
def test_u32_ids(shape):
    p, _, theta, cp = fc.u32(shape)
    assert int(p.id_base.max()) > 0xFFFF
    got = _run("u32", theta, cp, shape)
    assert 0 < got.n_loci < p.n_loci


@pytest.mark.parametrize("theta,cp", fc.DEEP16_SETTINGS)
def test_deep_16bit_loci(theta, cp):
    _run("deep16", theta, cp)


def _same_resident(filtered, cov, expect):
    o_chr, o_pos, o_off, o_rid, o_idb, cov_ref = expect
    nl, ne = filtered["n_loci"], filtered["n_entries"]
    host = lambda t, n, view: t[:n].cpu().numpy().view(view)  # noqa: E731
    assert nl == len(o_pos) and ne == len(o_rid) and cov == cov_ref
    assert np.array_equal(host(filtered["chr"], len(o_chr), np.uint32), o_chr)
    assert np.array_equal(host(filtered["pos"], nl, np.uint32), o_pos)
    assert np.array_equal(host(filtered["off"], nl + 1, np.uint64), o_off)
    assert np.array_equal(host(filtered["rid"], ne, np.uint32), o_rid)
    assert np.array_equal(host(filtered["idb"], ne, np.uint16 if filtered["idb_is16"] else np.uint32), o_idb)


def test_unaligned_id_base_takes_the_scalar_path():
    """k_decide reads four 16-bit entries per lane only from an 8-byte aligned id_base; from any other address it
    reads them one by one. Both give the oracle's pileup."""
    import torch
    p, i2p = fc.deep16()
    theta, cp = fc.DEEP16_SETTINGS[0]
    expect = fc.expected("deep16", theta, cp)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, np.arange(len(i2p), dtype=np.uint32), len(i2p))
        assert res["idb_is16"] and res["idb"].data_ptr() % 8 == 0
        _same_resident(*secedo_amd.filter_resident(plan, res, i2p, theta, cp), expect)
        larger = torch.zeros(p.n_entries + 8, dtype=res["idb"].dtype, device=res["idb"].device)
        larger[1:p.n_entries + 1] = res["idb"]
        shifted = dict(res, idb=larger[1:p.n_entries + 1])
        assert shifted["idb"].data_ptr() % 8 == 2
        _same_resident(*secedo_amd.filter_resident(plan, shifted, i2p, theta, cp), expect)


@pytest.mark.parametrize("r", [1, 2, 3])
def test_last_entries_of_the_pileup(r):
    """n_entries = r (mod 4): the last lane's four entries end behind the array, in a tensor of exactly that size."""
    p, i2p = fc.tail(r)
    expect = fc.expected("tail", 0.01, 4, r)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, np.arange(len(i2p), dtype=np.uint32), len(i2p))
        assert res["idb"].numel() == p.n_entries and p.n_entries % 4 == r
        _same_resident(*secedo_amd.filter_resident(plan, res, i2p, 0.01, 4), expect)
    _run("tail", 0.01, 4, r)
