"""The k-means, GMM and decision kernels (secedo_amd/csrc/cluster_kernels.hip) against the numpy restatements of
tests/kmeans_ref.py on the hard inputs of tests/cluster_cases.py: every template instance (k-means D = 2..7, GMM
D = 1..5), n below, at and past the 64 lanes and the 256 threads, duplicate rows, zero rows, constant columns.

A combination that passes the table's gate owes the restatement exact labels and passes and its values within the
project's bounds; one that the algorithm itself decides by rounding only has to run, give a finite or a failed
result, and give the same bits twice. Every combination is run twice."""
import math

import numpy as np
import pytest

from tests import cluster_cases as cc

pytestmark = pytest.mark.gpu
FAILED = dict(status=0, avg_log_p=-math.inf, aic=math.inf, bic=math.inf)
KEYS = ("status", "avg_log_p", "aic", "bic")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _rel(a, b):
    return 0.0 if a == b else abs(a - b) / max(abs(a), abs(b))


def _same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _gmm_values(m):
    return [m[key] for key in KEYS]


def _check_gmm(got, ref, fair, rel, where):
    """got against ref: exactly for a failed fit, within rel for status 1; only well-formed when not fair."""
    if got["status"] == 0:
        assert _gmm_values(got) == _gmm_values(FAILED), (where, got)
    else:
        assert got["status"] == 1 and all(math.isfinite(got[key]) for key in KEYS), (where, got)
    if not fair:
        return 0.0
    assert got["status"] == ref["status"], (where, got, ref)
    worst = 0.0
    if ref["status"]:
        worst = max(_rel(got[key], ref[key]) for key in KEYS[1:])
        for key in KEYS[1:]:
            assert math.isclose(got[key], ref[key], rel_tol=rel), (where, key, got[key], ref[key], worst)
    return worst


def _check_kmeans(got, ref, fair, where):
    labels, inertia, passes = got
    assert labels.min() >= 0 and math.isfinite(inertia) and inertia >= 0 and passes >= 1, where
    if not fair:
        return 0.0
    assert np.array_equal(labels, ref["labels"]), (where, int((labels != ref["labels"]).sum()))
    assert passes == ref["passes"], (where, passes, ref["passes"])
    if ref["inertia"] == 0:
        assert inertia == 0, (where, inertia)
    assert math.isclose(inertia, ref["inertia"], rel_tol=cc.KMEANS_REL, abs_tol=0.0), (where, inertia, ref["inertia"])
    return _rel(inertia, ref["inertia"])


@pytest.mark.parametrize("case", list(cc.CASES))
def test_kmeans_every_dims_against_the_restatement(case):
    from secedo_amd import cluster
    pts = _dev(cc.CASES[case])
    worst, fair_n = 0.0, 0
    for dims, K in cc.kmeans_combos(case):
        got = cluster.kmeans_device(pts[:, :dims], K)
        again = cluster.kmeans_device(pts[:, :dims], K)
        assert np.array_equal(got[0], again[0]) and _same_bits(got[1], again[1]) and got[2] == again[2]
        assert got[0].max() < K
        fair = cc.kmeans_admitted(case, dims, K)
        fair_n += fair
        worst = max(worst, _check_kmeans(got, cc.kmeans_ref(case, dims, K), fair, (case, dims, K)))
    print("kmeans %s: %d combinations, %d compared exactly, largest rel error of the inertia %.3g"
          % (case, len(cc.kmeans_combos(case)), fair_n, worst))


@pytest.mark.parametrize("max_iter", [1, 2])
def test_kmeans_iteration_cap_recomputes_the_centroids(max_iter):
    """The restatement needs more than 9 passes here; at the cap the centroids are still recomputed from the last
    labels and the inertia uses them."""
    from secedo_amd import cluster
    pts = _dev(cc.CASES["blob"])
    for dims, K in ((3, 3), (4, 4), (7, 2)):
        assert cc.kmeans_ref("blob", dims, K)["passes"] > 9
        ref = cc.kmeans_ref("blob", dims, K, max_iter)
        assert ref["margin"] > cc.MARGIN and ref["passes"] == max_iter and "iteration_cap" in ref["trace"]
        got = cluster.kmeans_device(pts[:, :dims], K, max_iter)
        err = _check_kmeans(got, ref, True, ("blob", dims, K, max_iter))
        print("cap %d, dims %d, K %d: rel error of the inertia %.3g" % (max_iter, dims, K, err))


@pytest.mark.parametrize("case", list(cc.CASES))
def test_gmm_every_dims_against_the_restatement(case):
    """K > n (status 0, nothing seeded) is part of every case with n < 4."""
    from secedo_amd import cluster
    pts = _dev(cc.CASES[case])
    worst, fair_n = 0.0, 0
    for dims, K in cc.gmm_combos(case):
        got = cluster.gmm_device(pts[:, :dims], K)
        again = cluster.gmm_device(pts[:, :dims], K)
        assert _same_bits(_gmm_values(got), _gmm_values(again)), (case, dims, K, got, again)
        fair = cc.gmm_admitted(case, dims, K)
        fair_n += fair
        err = _check_gmm(got, cc.gmm_ref(case, dims, K), fair, cc.gmm_tolerance(case, dims, K), (case, dims, K))
        worst = max(worst, err)
    print("gmm %s: %d combinations, %d compared, largest rel error %.3g"
          % (case, len(cc.gmm_combos(case)), fair_n, worst))


def test_gmm_more_components_than_points_fails():
    from secedo_amd import cluster
    for n in (1, 2, 3):
        pts = _dev(cc.CASES["blob"][:n])
        for dims in cc.GMM_DIMS:
            for K in range(n + 1, 5):
                assert _gmm_values(cluster.gmm_device(pts[:, :dims], K)) == _gmm_values(FAILED), (n, dims, K)


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_gmm_non_finite_entry_past_the_first_trip_fails(bad):
    """Row 257 is read on the second trip of thread 1; learn() fails on any non-finite input."""
    from secedo_amd import cluster
    from tests.kmeans_ref import gmm_learn
    for dims in cc.GMM_DIMS:
        x = cc.CASES["blob"][:, :dims].copy()
        x[257, dims - 1] = bad
        for K in cc.KS:
            assert gmm_learn(x, K)["status"] == 0
            assert _gmm_values(cluster.gmm_device(_dev(x), K)) == _gmm_values(FAILED), (dims, K)


@pytest.mark.parametrize("k", cc.DECISION_K)
@pytest.mark.parametrize("case", list(cc.DECISION_CASES))
def test_decision_step_against_the_restatement(case, k):
    from secedo_amd import cluster
    from secedo_amd._lib import SecedoError
    ev = _dev(cc.DECISION_CASES[case][:, :k])
    n = ev.shape[0]
    if k > n:  # n cells have at most n eigenvectors: the entry point refuses the block and launches nothing
        for t in cc.TYPES:
            for term in cc.TERMINATIONS:
                with pytest.raises(SecedoError, match="n_vectors"):
                    cluster.spectral_clustering_device(ev, t, term)
        return
    ref, fair = cc.decision_ref(case, k)
    worst = 0.0
    for t in cc.TYPES:
        for term in cc.TERMINATIONS:
            where = (case, k, t, term)
            nc, c, rec = cluster.spectral_clustering_device(ev, t, term)
            nc2, c2, rec2 = cluster.spectral_clustering_device(ev, t, term)
            assert nc == nc2 and rec == rec2 and _same_bits(c.cpu().numpy(), c2.cpu().numpy()), where
            rnc, rlab, rrec = ref[t, term]
            c = c.cpu().numpy()
            assert rec["cluster_count"] in (2, 3, 4) and nc in (1, rec["cluster_count"]), where
            assert ((c >= 0) & (c < max(2, min(rec["cluster_count"], n))) & (c == np.floor(c))).all(), where
            for K in cc.KS:
                got = rec["inertia"][K - 1]
                if K > n:
                    assert got == math.inf, (where, K, got)
                elif fair["kmeans"]:
                    want = rrec["inertia"][K - 1]
                    assert math.isclose(got, want, rel_tol=cc.KMEANS_REL, abs_tol=0.0), (where, K, got, want)
                model = dict(status=rec["gmm_status"][K - 1], avg_log_p=rec["avg_log_p"][K - 1], aic=rec["aic"][K - 1],
                             bic=rec["bic"][K - 1])
                worst = max(worst, _check_gmm(model, rrec["gmm"][K - 1], fair["gmm"][K - 1], cc.GMM_REL, (where, K)))
            if fair["kmeans"]:
                assert rec["cluster_count"] == rrec["cluster_count"], where
            if fair["labels"][t]:
                assert np.array_equal(c, rlab), (where, int((c != rlab).sum()))
            if fair["kmeans"] and all(fair["gmm"]):
                assert nc == rnc, where
    print("decision %s k=%d: exact parts %s, largest rel error of a GMM record %.3g" % (case, k, fair, worst))


def test_fiedler_threshold_cases_are_what_they_claim():
    """Column 1 of the two FIEDLER cases has the minimum 0.0 / -0.0, and the rows at it get label 0."""
    from secedo_amd import cluster
    for name, sign in (("fiedler_zero", 0.0), ("fiedler_negzero", 1.0)):
        col = cc.DECISION_CASES[name][:, 1]
        assert col.min() == 0 and float(np.signbit(col[col == 0]).mean()) == sign
        _, c, _ = cluster.spectral_clustering_device(_dev(cc.DECISION_CASES[name]), "FIEDLER", "BIC")
        assert np.array_equal(c.cpu().numpy(), (col > 0).astype(np.float64))
