"""Hard inputs for the k-means, GMM and decision kernels of secedo_amd/csrc/cluster_kernels.hip, with the gate that
says on which of them the numpy restatement (tests/kmeans_ref.py) is a fair exact reference.

Every coordinate is a multiple of 1/64 of small magnitude, so every hard-assignment sum (k-means centroids, the
GMM's k-means and initial covariances) is exact in any order, and the kernel owes the restatement the same labels
and passes. Every case has 7 columns; a model of `dims` dimensions reads the first `dims` of them.

The gate (computed, and its conditions asserted in tests/test_cluster_cpu.py):
  k-means (case, dims, K)  admitted when the margin of kmeans_run -- the smallest relative gap between the nearest
                           and the second-nearest centroid of distinct coordinates -- is above 1e-9;
  GMM (case, dims, K)      admitted when gmm_learn with sequential sums and with the kernel's order of sums agree
                           in status and trace and, for status 1, in avg_log_p, AIC and BIC to rel 1e-10; and
                           when, besides, no EM update meets a Cholesky pivot of 0 +- eps. Sums of exact terms
                           (weights of exactly 0 and 1, as for K = 1) are the same in every order, so the order
                           of the sums cannot show such a pivot. Two things do: the kernel's order with every
                           multiply-subtract of the covariance and of the factorisation rounded once, as a
                           compiler that contracts them does (gmm_learn(contract=True)), must agree in the same
                           way; and no pivot may be nonzero and below PIVOT = 1e-6 of its diagonal entry. A
                           pivot of exactly 0 under both roundings comes from exact arithmetic and is fair.
A combination that fails it is one the algorithm itself decides by rounding (a point on the bisector of two
centroids; a handful of points in D >= 2, or points on a line, whose covariance has a Cholesky pivot of 0 +- eps).
On the device such a combination gave, at K = 1, an avg_log_p of 19.06 against the restatement's 19.03
(two rows repeated 143 and 157 times, dims 2) and of 1.9e15 against 0.19 (dims 3): noise accepted as a variance.
Those still run on the GPU, for "no error, finite or failed, twice the same bits".

Branches of gmm_learn that no finite input reaches, shown from the restatement:
  chol_fallback  init_constants factorises either the initial covariance, which is diagonal with every entry in
                 [1e-10, DBL_MAX] after em_fix_params, or a covariance that em_update_params accepted because
                 this same factorisation succeeded on these same bits (em_fix_params changes nothing of it: its
                 diagonal is already floored and finite). Armadillo reaches its fallback only where LAPACK's
                 inv_sympd and log_det disagree; one deterministic Cholesky cannot disagree with itself.
  no_donor       needs a dead mean and no mean with >= 2 points: then at most K - 1 means hold one point each,
                 n <= K - 1, and learn() has already failed on n < K.
fail_means / fail_progress / fail_params need sums that overflow (|x| near DBL_MAX); not in this table.

TOLERANCE holds every admitted GMM combination that is compared above the project's rel 1e-9, as
(case, dims, K) -> (measured spread of the restatement, granted tolerance = 10 x spread, capped at 1e-6).
"""
import functools
import math

import numpy as np

from tests.kmeans_ref import decide, gmm_learn, kmeans_run, normalised_rows

EDGE_N = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513)
KMEANS_DIMS, GMM_DIMS, KS = tuple(range(2, 8)), tuple(range(1, 6)), (1, 2, 3, 4)
MARGIN, GMM_GATE_REL = 1e-9, 1e-10
# A Cholesky pivot is a diagonal entry A_jj minus squares of its size, each rounded to eps / 2: it carries an error
# of about D * eps * A_jj = 1e-15 * A_jj, whatever the order of the sums. Relative to a pivot of r * A_jj that is
# 1e-15 / r, and it goes straight into the log-determinant: r >= 1e-6 keeps it at the project's 1e-9.
PIVOT = 1e-6
GMM_REL, KMEANS_REL = 1e-9, 1e-12  # the project's bounds (tests/test_gpu_cluster.py)
TOLERANCE = {}

# the cases whose every (dims, K) must pass the gate
MUST_ADMIT = ("blob", "three_blobs", "outlier", "plane_axis", "two_points", "constant") + tuple(
    "n%d" % n for n in EDGE_N if n >= 63)
REACHABLE_GMM = frozenset(("dead_mean", "donor", "random_resample", "km_converged", "heft_dedupe", "var_floor",
                           "em_update_skipped", "em_converged", "fail_input"))
REACHABLE_KMEANS = frozenset(("km_empty",))  # iteration_cap: blob with max_iter 1 and 2


def _grid(seed, n, half=32):
    return np.random.default_rng(seed).integers(-half, half + 1, (n, 7)) / 64.0


def _build():
    c = {}
    c["blob"] = _grid(11, 1000, 128)
    rng = np.random.default_rng(12)
    shift = np.array([np.zeros(7), np.full(7, 0.75), 0.75 * (-1.0) ** np.arange(1, 8)])
    three = np.concatenate([_grid(13 + b, m, 8) + shift[b] for b, m in enumerate((370, 370, 371))])
    c["three_blobs"] = three[rng.permutation(len(three))]
    c["outlier"] = _grid(16, 600, 64)
    c["outlier"][300] = 64.0
    c["plane_axis"] = _grid(17, 1000)
    c["plane_axis"][:, 2:] = 0.0
    rng = np.random.default_rng(18)
    pair = np.array([[8, -16, 24, 4, -12, 20, -28], [-24, 12, -4, 28, 16, -8, 2]]) / 64.0
    # 150 rows of each, so that the mean (p + q) / 2 and the covariance of all 300, the outer product of (p - q) / 2
    # with itself, are exact: the second Cholesky pivot of the rank-1 covariance is 0, not 0 +- eps
    c["two_points"] = pair[np.concatenate([(0, 1), rng.permutation(np.arange(298) % 2)])]
    c["two_points_first3same"] = pair[np.concatenate([(0, 0, 0), rng.permutation((np.arange(297) < 150).astype(int))])]
    c["constant"] = np.repeat(pair[:1], 257, axis=0)
    c["mostly_zero"] = np.zeros((300, 7))
    c["mostly_zero"][3::7] = _grid(19, len(range(3, 300, 7)))
    for n in EDGE_N:
        c["n%d" % n] = c["blob"][:n].copy()
    for a in c.values():
        a.setflags(write=False)
    return c


CASES = _build()


def _decision_cases():
    c = {"n%d" % n: CASES["blob"][:n] for n in (2, 3, 4, 5, 64, 257, 1000)}
    c["three_blobs"] = CASES["three_blobs"]  # separated groups: the GMMs with K > 1 win
    z = CASES["blob"][:257].copy()
    z[[0, 5, 100, 256]] = 0.0  # rows of norm 0 stay as they are
    c["zero_rows"] = z
    for name, zero in (("fiedler_zero", 0.0), ("fiedler_negzero", -0.0)):
        f = CASES["blob"][:257].copy()
        f[:, 1] = np.abs(f[:, 1])
        f[f[:, 1] == 0, 1] = 1 / 64.0
        f[[1, 70, 256], 1] = zero  # the minimum of column 1: the threshold becomes DBL_MIN
        c[name] = f
    for a in c.values():
        a.setflags(write=False)
    return c


DECISION_CASES = _decision_cases()
DECISION_K = tuple(range(2, 8))
TYPES, TERMINATIONS = ("FIEDLER", "SPECTRAL2", "SPECTRAL6"), ("AIC", "BIC")


@functools.lru_cache(maxsize=None)
def kmeans_ref(case, dims, K, max_iter=100):
    trace = set()
    labels, inertia, passes, margin = kmeans_run(CASES[case][:, :dims], K, max_iter, trace=trace, margin=True)
    if labels is not None:
        labels.setflags(write=False)
    return dict(labels=labels, inertia=inertia, passes=passes, margin=margin, trace=frozenset(trace))


@functools.lru_cache(maxsize=None)
def gmm_ref(case, dims, K, sum_order="kernel"):
    return gmm_traced(CASES[case][:, :dims], K, sum_order)


@functools.lru_cache(maxsize=None)
def _gmm_contracted(case, dims, K):
    return gmm_traced(CASES[case][:, :dims], K, "kernel", True)


def gmm_traced(points, K, sum_order, contract=False):
    trace, pivots = set(), []
    r = gmm_learn(points, K, trace=trace, sum_order=sum_order, contract=contract, pivots=pivots)
    return dict(r, trace=frozenset(trace), pivots=tuple(pivots))


def gmm_pivots_are_sound(pivots):
    return all(p == 0 or abs(p) >= PIVOT for p in pivots)


def _close(a, b, rel):
    return a == b or math.isclose(a, b, rel_tol=rel)


def gmm_agree(a, b, rel=GMM_GATE_REL):
    return a["status"] == b["status"] and a["trace"] == b["trace"] and all(
        _close(a[key], b[key], rel) for key in ("avg_log_p", "aic", "bic"))


def kmeans_admitted(case, dims, K):
    return kmeans_ref(case, dims, K)["margin"] > MARGIN


def gmm_admitted(case, dims, K):
    plain = gmm_ref(case, dims, K, "kernel")
    return (gmm_agree(gmm_ref(case, dims, K, "sequential"), plain) and gmm_agree(_gmm_contracted(case, dims, K), plain)
            and gmm_pivots_are_sound(_gmm_contracted(case, dims, K)["pivots"] + plain["pivots"]))


def kmeans_combos(case):
    n = len(CASES[case])
    return [(dims, K) for dims in KMEANS_DIMS for K in KS if K <= n]


def gmm_combos(case):
    return [(dims, K) for dims in GMM_DIMS for K in KS]  # K > n included: status 0


def gmm_tolerance(case, dims, K):
    return TOLERANCE.get((case, dims, K), (0.0, GMM_REL))[1]


@functools.lru_cache(maxsize=None)
def decision_ref(case, k):
    """The restatement's decisions on the first k columns, for every type and termination, and which parts of
    them pass the gate: 'kmeans' (the four inertias and cluster_count), 'gmm' (per K), 'labels' (per type)."""
    ev = DECISION_CASES[case][:, :k]
    n = len(ev)
    cache, out = {}, {}
    for t in TYPES:
        for term in TERMINATIONS:
            out[t, term] = decide(ev, t, term, sum_order="kernel", cache=cache)
    km = ev[:, :min(2, k - 1) + 1]
    gm = ev[:, 1:min(5, k - 1) + 1]
    fair = dict(kmeans=all(kmeans_run(km, K, margin=True)[3] > MARGIN for K in KS if K <= n), gmm=[], labels={})
    for K in KS:
        a, b, c = gmm_traced(gm, K, "sequential"), gmm_traced(gm, K, "kernel"), gmm_traced(gm, K, "kernel", True)
        fair["gmm"].append(gmm_agree(a, b) and gmm_agree(c, b) and gmm_pivots_are_sound(b["pivots"] + c["pivots"]))
    count = out["FIEDLER", "AIC"][2]["cluster_count"]
    for t in TYPES:
        fair["labels"][t] = t == "FIEDLER" or (
            fair["kmeans"] and kmeans_run(normalised_rows(ev, t), count, margin=True)[3] > MARGIN)
    return out, fair
