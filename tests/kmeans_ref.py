"""numpy restatements of the decision step's models, as secedo_amd/csrc/cluster_kernels.hip documents them.

kmeans_run: the reference's KMeans::run (util/kmeans.cpp) with all of its tries, quirks included -- centroids
seeded from the first K rows, labels declared once outside the tries (try 1 starts from zeros), empty clusters
get the zero centroid, centroids recomputed after the last pass (also at the cap), coordinate 1 scaled by 1.2,
short sums in Armadillo's interleaved order. K > n -> inertia +inf (the reference never returns).

gmm_learn: arma::gmm_full::learn(X, K, eucl_dist, random_subset, 10, 5, 1e-10) with the seeding the kernel
documents (splitmix64 keyed by (K << 32) | n), followed by avg_log_p, AIC and BIC.

Both can say what they did. `trace`: a set that receives the name of every special branch taken (GMM:
dead_mean, donor, random_resample, no_donor, km_converged, heft_dedupe, var_floor, em_update_skipped,
chol_fallback, em_converged, fail_*; k-means: km_empty, iteration_cap). kmeans_run(margin=True) also returns
the smallest relative gap, over all passes and points, between the distances to the nearest and the
second-nearest centroid of distinct coordinates (identical centroids are a true tie, broken "first wins" by
every implementation). gmm_learn(sum_order="kernel") takes every sum over points in the order of
cluster_kernels.hip's block_sum -- one partial per thread over i = t, t + 256, ..., the xor butterfly over the 64
lanes of a wave, the four waves left to right -- so that only libm and FMA contraction separate it from the
kernel. gmm_learn(contract=True) rounds the multiply-subtracts that decide whether an EM update is accepted -- the
initial variances, the new covariance and the Cholesky factorisation, in the kernel's loop order -- once, as a
compiler that contracts them into fused multiply-adds does; gmm_learn(pivots=list) records every pivot past the
first of the Cholesky factorisations of the EM updates, relative to its diagonal entry. A pivot that is rounding
noise around 0 shows in both. The defaults leave every result as it was.
"""
import math
from fractions import Fraction

import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
DBL_EPS = np.finfo(np.float64).eps
MASK = (1 << 64) - 1


def sumsq(t):
    """Armadillo's two interleaved accumulators over the last axis (a vector, or one vector per row)."""
    t = np.asarray(t)
    m = t.shape[-1]
    a1 = a2 = 0.0
    i, j = 0, 1
    while j < m:
        a1 = a1 + t[..., i] * t[..., i]
        a2 = a2 + t[..., j] * t[..., j]
        i += 2
        j += 2
    if i < m:
        a1 = a1 + t[..., i] * t[..., i]
    return a1 + a2


def _wdist2(P, c):
    """weighted_dist2 of every row of P to c (one centroid, or one per row)."""
    t = P - c
    t[..., 1] *= 1.2
    return sumsq(t)


def _margin(d, cen):
    """Smallest relative gap between the nearest and the second-nearest distance, centroids of equal coordinates
    counted once. d: n x K distances."""
    _, first = np.unique(np.stack(cen), axis=0, return_index=True)
    if len(first) < 2:
        return math.inf
    s = np.sort(d[:, np.sort(first)], axis=1)
    return float(((s[:, 1] - s[:, 0]) / s[:, 1]).min())


def kmeans_run(points, K, max_iter=100, num_tries=10, trace=None, margin=False):
    """-> (labels, inertia, passes of the last try), with margin=True also the margin (see the module text)."""
    X = np.asarray(points, dtype=np.float64)
    n = X.shape[0]
    if K > n:
        return (None, math.inf, 0, math.inf) if margin else (None, math.inf, 0)
    labels = np.zeros(n, dtype=np.int64)
    best, best_inertia, passes, gap = None, np.finfo(np.float64).max, 0, math.inf
    for _ in range(num_tries):
        cen = [X[i].copy() for i in range(K)]
        it, done = 0, False
        for it in range(1, max_iter + 1):
            d = np.sqrt(np.stack([_wdist2(X, c) for c in cen], axis=1))
            if margin:
                gap = min(gap, _margin(d, cen))
            b = np.argmin(d, axis=1)  # the first of equal distances
            done = bool((b == labels).all())
            labels = b
            sums = np.zeros((K, X.shape[1]))
            np.add.at(sums, labels, X)  # row after row, as the reference adds them
            counts = np.bincount(labels, minlength=K)
            if trace is not None and (counts == 0).any():
                trace.add("km_empty")
            cen = [c / counts[g] if counts[g] > 0 else c for g, c in enumerate(sums)]
            if done:
                break
        if trace is not None and not done:
            trace.add("iteration_cap")
        inertia = sum(_wdist2(X, np.stack(cen)[labels]).tolist())
        if inertia < best_inertia:
            best, best_inertia, passes = labels.copy(), inertia, it
    return (best, best_inertia, passes, gap) if margin else (best, best_inertia, passes)


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return state, z ^ (z >> 31)


def _fma(a, b, c):
    """a * b + c with one rounding, as a contracted multiply-add gives it."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _chol(A, contract=False, pivots=None):
    """pivots: a list that receives every pivot past the first, relative to its diagonal entry. contract: the
    kernel's loop (one term subtracted after the other) with every multiply-subtract rounded once."""
    D = A.shape[0]
    L = np.zeros_like(A)
    for j in range(D):
        if contract:
            s = A[j, j]
            for k in range(j):
                s = _fma(-L[j, k], L[j, k], s)
        else:
            s = A[j, j] - sum(L[j, k] ** 2 for k in range(j))
        if pivots is not None and j and math.isfinite(s) and A[j, j] > 0:
            pivots.append(float(s / A[j, j]))
        if not (s > 0) or not math.isfinite(s):
            return None
        L[j, j] = math.sqrt(s)
        for i in range(j + 1, D):
            if contract:
                t = A[i, j]
                for k in range(j):
                    t = _fma(-L[i, k], L[j, k], t)
                L[i, j] = t / L[j, j]
            else:
                L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    return L


def _note(trace, name):
    if trace is not None:
        trace.add(name)


def _fix_params(means, fcov, hefts, K, trace=None):
    for g in range(K):
        for d in range(fcov.shape[1]):
            v = fcov[g, d, d]
            if v < 1e-10:
                fcov[g, d, d] = 1e-10
                _note(trace, "var_floor")
            elif v > np.finfo(np.float64).max:
                fcov[g, d, d] = np.finfo(np.float64).max
            elif math.isnan(v):
                fcov[g, d, d] = 1.0
    for g1 in range(K):
        if hefts[g1] > 0:
            for g2 in range(g1 + 1, K):
                if hefts[g2] > 0 and abs(hefts[g1] - hefts[g2]) <= DBL_EPS and sumsq(means[g1] - means[g2]) == 0:
                    hefts[g2] = 0
                    _note(trace, "heft_dedupe")
    for g in range(K):
        h = hefts[g]
        if h < DBL_MIN:
            hefts[g] = DBL_MIN
        elif h > 1:
            hefts[g] = 1
        elif math.isnan(h):
            hefts[g] = 1.0 / K
    s = hefts.sum()
    if s < 1 - DBL_EPS or s > 1 + DBL_EPS:
        hefts /= s


def _constants(fcov, hefts, K, D, trace=None, contract=False):
    tmp = (D / 2.0) * math.log(2 * math.pi)
    inv = np.zeros_like(fcov)
    lde = np.zeros(K)
    for g in range(K):
        L = _chol(fcov[g], contract)
        if L is not None:
            Li = np.linalg.inv(L)
            inv[g] = Li.T @ Li
            ld = 2 * sum(math.log(L[d, d]) for d in range(D))
        else:
            _note(trace, "chol_fallback")
            v = np.maximum(np.diag(fcov[g]), DBL_MIN)
            inv[g] = np.diag(1 / v)
            ld = float(np.log(v).sum())
        lde[g] = -(tmp + 0.5 * ld)
    np.maximum(hefts, DBL_MIN, out=hefts)
    return inv, lde, np.log(hefts)


def _log_add_exp(a, b):
    if a < b:
        a, b = b, a
    nd = b - a
    if nd < math.log(DBL_MIN) or not math.isfinite(nd):
        return a
    return a + math.log1p(math.exp(nd))


def _log_p(X, means, inv, lde, K):
    diff = X[:, None, :] - means[None, :K, :]
    q = np.einsum("ngd,gde,nge->ng", diff, inv[:K], diff)
    return -0.5 * q + lde[None, :K]


def _log_sum(gl):
    out = np.empty(gl.shape[0])
    for i in range(gl.shape[0]):
        s = gl[i, 0]
        for g in range(1, gl.shape[1]):
            s = _log_add_exp(s, gl[i, g])
        out[i] = s
    return out


THREADS, LANES = 256, 64


def block_sum(v):
    """Sum over axis 0 in the order of the kernel's block_sum: thread t adds rows t, t + 256, ... from zero, every
    wave runs the xor butterfly (offsets 32 .. 1; all lanes end with the same bits), the four waves add left to
    right."""
    v = np.asarray(v, dtype=np.float64)
    trips = -(-v.shape[0] // THREADS)
    pad = np.zeros((trips * THREADS,) + v.shape[1:])  # a thread past the end adds nothing: + 0.0 changes no sum
    pad[:v.shape[0]] = v
    pad = pad.reshape((trips, THREADS) + v.shape[1:])
    x = np.zeros((THREADS,) + v.shape[1:])
    for r in range(trips):
        x = x + pad[r]
    x = x.reshape((THREADS // LANES, LANES) + v.shape[1:])
    lane = np.arange(LANES)
    o = LANES // 2
    while o:
        x = x + x[:, lane ^ o]
        o //= 2
    w = x[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def _nearest(X, means, K):
    d2 = np.stack([sumsq(X - means[g]) for g in range(K)], axis=1)
    return np.argmin(d2, axis=1)  # the first of equal distances


def gmm_learn(points, K, trace=None, sum_order="sequential", contract=False, pivots=None):
    """-> dict(status, avg_log_p, aic, bic). contract and pivots: see the module text."""
    if sum_order not in ("sequential", "kernel"):
        raise ValueError(sum_order)
    kernel = sum_order == "kernel"
    X = np.asarray(points, dtype=np.float64)
    n, D = X.shape
    failed = dict(status=0, avg_log_p=-math.inf, aic=math.inf, bic=math.inf)
    if n < K or not np.isfinite(X).all():
        _note(trace, "fail_input")
        return failed
    state = (K << 32) | n
    idx = []
    while len(idx) < K:
        state, z = splitmix64(state)
        c = z % n
        if c not in idx:
            idx.append(c)
    means = X[idx].copy()
    for _ in range(10):  # km_iterate
        best = _nearest(X, means, K)
        cnt = np.bincount(best, minlength=K)
        if kernel:
            tot = block_sum(X[:, None, :] * (best[:, None] == np.arange(K))[:, :, None])
            new = np.stack([tot[g] / cnt[g] if cnt[g] else np.zeros(D) for g in range(K)])
        else:
            new = np.stack([X[best == g].sum(axis=0) / cnt[g] if cnt[g] else np.zeros(D) for g in range(K)])
        last = [int(np.nonzero(best == g)[0].max()) if cnt[g] else 0 for g in range(K)]
        live = [g for g in range(K - 1, -1, -1) if cnt[g] >= 2]
        used = 0
        for g in range(K):
            if cnt[g]:
                continue
            _note(trace, "dead_mean")
            if not live:
                _note(trace, "no_donor")
                _note(trace, "fail_no_donor")
                return failed
            if used < len(live):
                prop = last[live[used]]
                used += 1
                _note(trace, "donor")
            else:
                state, z = splitmix64(state)
                prop = z % n
                _note(trace, "random_resample")
            new[g] = X[prop]
        rs = 0.0
        for g in range(K):
            dd = sumsq(means[g] - new[g])
            rs = dd if g == 0 else rs + (dd - rs) / (g + 1)
        means = new
        if rs <= DBL_EPS:
            _note(trace, "km_converged")
            break
    if not np.isfinite(means).all():
        _note(trace, "fail_means")
        return failed
    best = _nearest(X, means, K)
    fcov = np.zeros((K, D, D))
    hefts = np.zeros(K)
    if kernel:
        mask = (best[:, None] == np.arange(K))[:, :, None]
        tot, tot2 = block_sum(X[:, None, :] * mask), block_sum((X * X)[:, None, :] * mask)
    for g in range(K):
        sel = X[best == g]
        h = len(sel)
        with np.errstate(invalid="ignore", divide="ignore"):
            if kernel:
                tmp, sq = tot[g] / np.float64(h), tot2[g] / np.float64(h)
            else:
                tmp = sel.sum(axis=0) / h if h else np.full(D, np.nan)
                sq = [(sel[:, d] ** 2).sum() / h if h else math.nan for d in range(D)]
        means[g] = tmp if h >= 1 else 0
        for d in range(D):
            if contract and h >= 2:
                fcov[g, d, d] = _fma(-tmp[d], tmp[d], sq[d])
            else:
                fcov[g, d, d] = sq[d] - tmp[d] ** 2 if h >= 2 else 1e-10
        if h < 2:
            _note(trace, "var_floor")
        hefts[g] = h / n
    _fix_params(means, fcov, hefts, K, trace)
    old = -math.inf
    for _ in range(5):
        inv, lde, lh = _constants(fcov, hefts, K, D, trace, contract)
        gl = _log_p(X, means, inv, lde, K) + lh[None, :]
        ls = _log_sum(gl)
        w = np.exp(gl - ls[:, None])
        if kernel:
            acc_w = block_sum(w)
            acc_x = block_sum(X[:, None, :] * w[:, :, None])
            acc_xx = block_sum(w[:, :, None, None] * (X[:, :, None] * X[:, None, :])[:, None, :, :])
        for g in range(K):
            an = max(acc_w[g] if kernel else w[:, g].sum(), DBL_MIN)
            if not math.isfinite(an):
                _note(trace, "em_update_skipped")
                continue
            if kernel:
                mu = acc_x[g] / an
                m2 = acc_xx[g] / an
            else:
                mu = (X * w[:, g:g + 1]).sum(axis=0) / an
                m2 = (X.T * w[:, g]) @ X / an
            if contract:
                cov = np.array([[_fma(-mu[d], mu[e], m2[d, e]) for e in range(D)] for d in range(D)])
            else:
                cov = m2 - np.outer(mu, mu)
            for d in range(D):
                if cov[d, d] < 1e-10:
                    _note(trace, "var_floor")
                cov[d, d] = max(cov[d, d], 1e-10)
            if not np.isfinite(cov).all() or _chol(cov, contract, pivots) is None:
                _note(trace, "em_update_skipped")
                continue
            hefts[g] = an / n
            means[g] = mu
            fcov[g] = cov
        _fix_params(means, fcov, hefts, K, trace)
        new = (block_sum(ls) if kernel else ls.sum()) / n
        if not math.isfinite(new):
            _note(trace, "fail_progress")
            return failed
        if abs(old - new) <= DBL_EPS:
            _note(trace, "em_converged")
            break
        old = new
    if any((np.diag(fcov[g]) <= 0).any() for g in range(K)) or not (
            np.isfinite(means).all() and np.isfinite(fcov).all() and np.isfinite(hefts).all()):
        _note(trace, "fail_params")
        return failed
    inv, lde, lh = _constants(fcov, hefts, K, D, trace, contract)
    ls = _log_sum(_log_p(X, means, inv, lde, K) + lh[None, :])
    avg = (block_sum(ls) if kernel else ls.sum()) / n
    npar = K * D * (D + 1) // 2 + K * D + K - 1
    return dict(status=1, avg_log_p=avg, aic=2 * npar - 2 * n * avg, bic=npar * math.log(n) - 2 * n * avg)


def _memo(cache, key, fn):
    if cache is None:
        return fn()
    if key not in cache:
        cache[key] = fn()
    return cache[key]


def decide(ev, clustering_type, termination, sum_order="sequential", cache=None):
    """The rules of spectral_clustering.cpp:182-298 on an n x k eigenvector block -> (num_clusters, labels, record).
    cache: a dict of the caller's, one per block, that keeps the models between calls on the same block."""
    ev = np.asarray(ev, dtype=np.float64)
    n, k = ev.shape
    if k < 2:
        return 1, np.zeros(n), {}
    inertia = [_memo(cache, ("kmeans", K), lambda: kmeans_run(ev[:, :min(2, k - 1) + 1], K))[1] for K in range(1, 5)]
    gmms = [_memo(cache, ("gmm", K, sum_order), lambda: gmm_learn(ev[:, 1:min(5, k - 1) + 1], K, sum_order=sum_order))
            for K in range(1, 5)]
    gaps = [inertia[i - 1] - inertia[i] for i in range(1, 4)]
    count = 2
    for i in range(1, 3):
        if gaps[i] > 0.75 * gaps[i - 1]:
            count = i + 2
        else:
            break
    if clustering_type == "FIEDLER":
        thr = DBL_MIN if ev[:, 1].min() == 0 else 0.0
        labels = (ev[:, 1] >= thr).astype(np.float64)
    else:
        y = normalised_rows(ev, clustering_type)
        labels = _memo(cache, ("labels", clustering_type, count), lambda: kmeans_run(y, count))[0].astype(np.float64)
    st = [g["status"] for g in gmms]
    aic = [g["aic"] for g in gmms]
    bic = [g["bic"] for g in gmms]
    if (not st[1] and not st[2] and not st[3]) or termination == "AIC":
        done = aic[0] < min(aic[1:])
    else:
        done = bic[0] < min(bic[1:])
    return (1 if done else count), labels, dict(inertia=inertia, gmm=gmms, cluster_count=count)


def normalised_rows(ev, clustering_type):
    """The rows that SPECTRAL2 / SPECTRAL6 cluster: columns 0..min(2 | 6, k-1), every row of norm > 0 normalised."""
    k = ev.shape[1]
    y = ev[:, :min(2 if clustering_type == "SPECTRAL2" else 6, k - 1) + 1].copy()
    for i in range(len(y)):
        nr = math.sqrt(sumsq(y[i]))
        if nr > 0:
            y[i] = y[i] / nr
    return y
