"""The clustering library (include/secedo_cluster.h) without a GPU: exports, string parsing, argument checks
that must fail before any device is touched, and the numpy KMeans::run restatement on hand-made cases."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from secedo_amd import _lib, cluster
from tests.kmeans_ref import block_sum, decide, gmm_learn, kmeans_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("secedo_")}


def _declared(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return set(re.findall(r"^(?:const\s+)?\w+\s*\*?\s*(secedo_\w+)\s*\(", text, re.M))


def test_simmat_exports_unchanged_and_cluster_exports_its_header():
    simmat = _exports(_lib.LIB_PATH)
    assert simmat == set(_lib.SIGNATURES)
    assert not any("cluster" in s for s in simmat)
    assert _exports(cluster.LIB_PATH) == _declared("secedo_cluster.h") == set(cluster.SIGNATURES)


def test_importing_the_package_does_not_load_the_cluster_library():
    import sys
    code = ("import secedo_amd, sys; from secedo_amd import cluster; "
            "assert cluster._cl is None; assert callable(secedo_amd.divide_cluster)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_parsers():
    assert [cluster.clustering_type(s) for s in ("FIEDLER", "SPECTRAL2", "SPECTRAL6")] == [0, 1, 2]
    with pytest.raises(_lib.SecedoError) as e:
        cluster.clustering_type("SPECTRAL3")
    assert e.value.code == _lib.E_INVALID_ARG and "SPECTRAL3" in str(e.value)
    # parse_termination: "AIC" is AIC, anything else BIC (spectral_clustering.cpp:30-32)
    assert cluster.termination("AIC") == 0 and cluster.termination("BIC") == 1 and cluster.termination("x") == 1


def _expect_invalid(fn, text):
    with pytest.raises(_lib.SecedoError) as e:
        fn()
    assert e.value.code == _lib.E_INVALID_ARG, str(e.value)
    assert text in str(e.value)


def test_invalid_arguments_fail_before_the_device():
    a = np.zeros((4, 4))
    _expect_invalid(lambda: cluster.spectral_clustering(a, "SPECTRAL2", "BIC", use_arma_kmeans=True), "use_arma_kmeans")
    _expect_invalid(lambda: cluster.spectral_clustering(a, "SPECTRAL6", "AIC", use_arma_kmeans=True), "use_arma_kmeans")
    _expect_invalid(lambda: cluster.spectral_clustering(a, "KMEANS"), "KMEANS")
    _expect_invalid(lambda: cluster.spectral_clustering(np.zeros((0, 0))), "no cells")
    from tests.clone_tree_gen import clone_tree
    p, _ = clone_tree(20, n_loci=50)
    ident = np.arange(20)
    args = (p, 500, ident.astype(np.uint16))
    rest = (0.01, 0.5, 0.05, 1, "", "ADD_MIN", "BIC", "SPECTRAL2")
    _expect_invalid(lambda: cluster.divide_cluster(*args, ident, ident[:0], *rest), "no cells")
    bad = ident.copy()
    bad[[3, 4]] = bad[[4, 3]]  # id_to_pos swapped against pos_to_id
    _expect_invalid(lambda: cluster.divide_cluster(*args, bad, ident, *rest), "inconsistent")
    _expect_invalid(lambda: cluster.divide_cluster(*args, ident, ident, 0.01, 0.5, 0.05, 1, "", "ADD_MIN", "BIC",
                                                   "SPECTRAL6", True), "use_arma_kmeans")


def test_fiedler_with_arma_kmeans_is_accepted_and_needs_the_gpu():
    # accepted (no effect with FIEDLER): without a GPU the call gets as far as the device check
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: covered by tests/test_gpu_cluster.py")
    except ImportError:
        pass
    with pytest.raises(_lib.SecedoError) as e:
        cluster.spectral_clustering(np.zeros((4, 4)), "FIEDLER", "AIC", use_arma_kmeans=True)
    assert e.value.code == _lib.E_NO_DEVICE


def test_kmeans_ref_empty_cluster_and_initial_zero_labels():
    # rows 0 and 1 coincide: both seed centroids are equal and every point goes to cluster 0 (first on ties).
    # That equals the initial all-zero labels, so pass 1 is already `done`; cluster 1 is empty and keeps the
    # zero centroid, and the inertia uses the centroid recomputed after that pass
    pts = np.array([[5.0, 5.0], [5.0, 5.0], [0.1, 0.0], [0.0, 0.1], [5.1, 5.0]])
    labels, inertia, passes = kmeans_run(pts, 2)
    assert list(labels) == [0, 0, 0, 0, 0] and passes == 1
    c0 = pts.sum(axis=0) / 5
    w = np.array([1.0, 1.2])
    assert math.isclose(inertia, sum(((p - c0) * w) @ ((p - c0) * w) for p in pts), rel_tol=1e-14)


def test_kmeans_ref_iteration_cap_recomputes_the_centroids():
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [10.0, 0.0], [11.0, 0.0]])
    labels1, inertia1, passes1 = kmeans_run(pts, 2, max_iter=1)
    # one pass: seeds rows 0, 1 -> labels [0, 1, 1, 1]; centroids recomputed from them, inertia uses those
    assert list(labels1) == [0, 1, 1, 1] and passes1 == 1
    c1 = pts[1:].mean(axis=0)
    assert math.isclose(inertia1, sum(((p - c1) ** 2).sum() for p in pts[1:]), rel_tol=1e-14)
    labels, inertia, _ = kmeans_run(pts, 2)
    assert list(labels) == [0, 0, 1, 1] and math.isclose(inertia, 1.0, rel_tol=1e-14)


def test_kmeans_ref_k_equals_n_and_beyond():
    pts = np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 7.0]])
    labels, inertia, _ = kmeans_run(pts, 3)
    assert list(labels) == [0, 1, 2] and inertia == 0
    assert kmeans_run(pts, 4)[1] == math.inf  # defined here: the reference never returns


def test_kmeans_ref_weights_coordinate_one():
    # equidistant in plain Euclid, not with coordinate 1 scaled by 1.2: the point joins the x-neighbour
    pts = np.array([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]])
    labels, _, _ = kmeans_run(pts, 2)
    assert labels[2] == 0


# ---- the restatement's trace / margin / sum order, and the gate of tests/cluster_cases.py ----

def _bits(v):
    if isinstance(v, dict):
        return {key: _bits(x) for key, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_bits(x) for x in v]
    return None if v is None else np.asarray(v, dtype=np.float64).tobytes()


def test_new_keyword_arguments_leave_the_default_results_bit_identical():
    """trace and margin only observe; sum_order and cache default to what decide and gmm_learn always did. On the
    hand-made cases above and on generic (inexact) points."""
    rng = np.random.default_rng(5)
    hand = [np.array([[5.0, 5.0], [5.0, 5.0], [0.1, 0.0], [0.0, 0.1], [5.1, 5.0]]),
            np.array([[0.0, 0.0], [1.0, 0.0], [10.0, 0.0], [11.0, 0.0]]),
            np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 7.0]]), np.array([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]])]
    for pts in hand + [rng.normal(size=(70, 3)), np.repeat(rng.normal(size=(2, 2)), 9, axis=0)]:
        for K in (1, 2, 3, 4):
            for cap in (1, 100):
                plain = kmeans_run(pts, K, max_iter=cap)
                assert _bits(plain) == _bits(kmeans_run(pts, K, max_iter=cap, trace=set(), margin=True)[:3])
            plain = gmm_learn(pts, K)
            assert _bits(plain) == _bits(gmm_learn(pts, K, trace=set())) == _bits(gmm_learn(pts, K, sum_order="sequential"))
            assert _bits(plain) == _bits(gmm_learn(pts, K, contract=False, pivots=[]))
    ev = rng.normal(size=(40, 7))
    for t in ("FIEDLER", "SPECTRAL2", "SPECTRAL6"):
        cache = {}
        plain = decide(ev, t, "BIC")
        assert _bits(plain) == _bits(decide(ev, t, "BIC", sum_order="sequential", cache=cache))
        assert _bits(plain) == _bits(decide(ev, t, "BIC", cache=cache))  # the second time from the cache
    # frozen values of the default path (the restatement before it learnt to say what it did gave these bits)
    pts = np.arange(24, dtype=np.float64).reshape(8, 3) ** 2 % 7 / 8
    assert kmeans_run(pts, 3)[1].hex() == KMEANS_FROZEN and gmm_learn(pts, 2)["avg_log_p"].hex() == GMM_FROZEN


KMEANS_FROZEN, GMM_FROZEN = "0x1.4fae147ae147bp-2", "0x1.11e51c2bf8ae9p+4"


def test_trace_names_the_branches():
    t = set()
    kmeans_run(np.array([[5.0, 5.0], [5.0, 5.0], [0.1, 0.0], [0.0, 0.1], [5.1, 5.0]]), 2, trace=t)
    assert t == {"km_empty"}
    t = set()
    kmeans_run(np.array([[0.0, 0.0], [1.0, 0.0], [10.0, 0.0], [11.0, 0.0]]), 2, max_iter=1, trace=t)
    assert t == {"iteration_cap"}
    t = set()
    assert gmm_learn(np.zeros((3, 2)), 4, trace=t)["status"] == 0 and t == {"fail_input"}
    t = set()
    assert gmm_learn(np.ones((9, 2)), 2, trace=t)["status"] == 1
    assert {"dead_mean", "donor", "var_floor", "km_converged"} <= t


def test_margin_ignores_identical_centroids_and_sees_a_bisector():
    # rows 0 and 1 coincide: pass 1 has one distinct centroid (no gap to speak of); pass 2 does not happen
    assert kmeans_run(np.array([[5.0, 5.0], [5.0, 5.0], [0.5, 0.0], [5.5, 5.0]]), 2, margin=True)[3] == math.inf
    # the third point lies on the bisector of the two seeds
    assert kmeans_run(np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 3.0], [9.0, 0.0]]), 2, margin=True)[3] == 0.0
    m = kmeans_run(np.array([[0.0, 0.0], [4.0, 0.0], [1.0, 0.0], [3.5, 0.0]]), 2, margin=True)[3]
    assert math.isclose(m, 2.0 / 3.0, rel_tol=1e-15)  # (3 - 1) / 3 at the third point, pass 1


def test_block_sum_is_the_kernels_order():
    """Thread partials over a stride of 256, the xor butterfly per wave, the waves left to right -- on values where
    the order shows (1e16 swallows a 1 unless the ones meet first)."""
    v = np.zeros(513)
    v[0], v[256], v[512] = 1e16, 1.0, 1.0  # thread 0 adds 1e16 + 1 + 1 one at a time: both ones are lost
    assert block_sum(v) == 1e16
    v = np.zeros(513)
    v[0], v[1], v[33] = 1e16, 1.0, 1.0  # lanes 1 and 33 meet at offset 32, before lane 0 joins: 1e16 + 2
    assert block_sum(v) == 1e16 + 2
    v = np.zeros(300)
    v[0], v[64], v[128] = 1.0, 1e16, -1e16  # waves left to right: ((1 + 1e16) - 1e16) + 0 = 0
    assert block_sum(v) == 0.0
    rng = np.random.default_rng(2)
    x = rng.integers(-99, 100, (1000, 3, 2)) / 64.0  # exact in any order
    assert np.array_equal(block_sum(x), x.sum(axis=0))


def test_case_table_is_exact_and_the_gate_admits_what_it_must():
    from tests import cluster_cases as cc
    for name, pts in cc.CASES.items():
        assert pts.shape[1] == 7 and np.array_equal(pts * 64, np.round(pts * 64)) and np.abs(pts).max() <= 64, name
    assert [len(cc.CASES["n%d" % n]) for n in cc.EDGE_N] == list(cc.EDGE_N)
    assert (cc.CASES["two_points_first3same"][:3] == cc.CASES["two_points_first3same"][0]).all()
    assert len(np.unique(cc.CASES["two_points"], axis=0)) == 2 and len(np.unique(cc.CASES["constant"], axis=0)) == 1
    assert cc.CASES["mostly_zero"].any(axis=1).sum() * 7 <= 300 + 6
    km = {(c, d, K): cc.kmeans_admitted(c, d, K) for c in cc.CASES for d, K in cc.kmeans_combos(c)}
    gm = {(c, d, K): cc.gmm_admitted(c, d, K) for c in cc.CASES for d, K in cc.gmm_combos(c)}
    print("k-means: %d admitted, %d dropped %s" % (sum(km.values()), len(km) - sum(km.values()),
                                                   [key for key, ok in km.items() if not ok]))
    print("GMM: %d admitted, %d dropped %s" % (sum(gm.values()), len(gm) - sum(gm.values()),
                                               [key for key, ok in gm.items() if not ok]))
    # 1. the cases that must be compared exactly are
    for table in (km, gm):
        assert [key for key, ok in table.items() if key[0] in cc.MUST_ADMIT and not ok] == []
    # 2. few are dropped
    assert len(km) - sum(km.values()) <= len(km) / 10 and len(gm) - sum(gm.values()) <= len(gm) / 4
    # 3. the admitted set still walks every branch that an input can reach
    seen = set().union(*(cc.gmm_ref(*key)["trace"] for key, ok in gm.items() if ok))
    print("GMM branches of the admitted set:", sorted(seen))
    assert seen == cc.REACHABLE_GMM  # chol_fallback and no_donor: unreachable, see the table's text
    assert set().union(*(cc.kmeans_ref(*key)["trace"] for key, ok in km.items() if ok)) == cc.REACHABLE_KMEANS
    assert "em_update_skipped" in cc.gmm_ref("two_points", 5, 1)["trace"] and gm["two_points", 5, 1]
    assert cc.gmm_ref("n3", 2, 4)["status"] == 0
    # the rank-1 covariance of two_points: pivots of exactly 0, with and without contraction
    assert set(cc.gmm_ref("two_points", 2, 1)["pivots"]) == {0.0} and not cc.gmm_admitted("n4", 4, 1)
    # every tolerance above the project's bound is 10 x a measured spread, and never above 1e-6
    for key, (spread, granted) in cc.TOLERANCE.items():
        assert gm[key] and cc.GMM_REL < granted <= 1e-6 and math.isclose(granted, min(10 * spread, 1e-6)), key
