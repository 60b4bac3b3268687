// cluster_kernels.hip -- the decision step of spectral clustering on the device (gfx950).
//
// Restates what the reference's spectral_clustering() does after eig_sym (spectral_clustering.cpp:140-298)
// on the n x k eigenvector block the spectral step leaves in HBM (column-major, k = min(7, n)):
//
//   how many clusters   KMeans::run (util/kmeans.cpp) on columns 0..min(2, k-1), K = 1..4, 100 iterations,
//                       then the gap rule of :193-205 -> cluster_count in {2, 3, 4}
//   whether to stop     arma::gmm_full::learn on columns 1..min(5, k-1), 1..4 components, eucl_dist,
//                       random_subset, 10 k-means + 5 EM iterations, variance floor 1e-10; avg_log_p,
//                       AIC, BIC (:55-115, :182-191) and the termination rule of :286-288
//   labels              FIEDLER: column 1 cut at 0 (DBL_MIN when its minimum is 0, :215-228);
//                       SPECTRAL2 / SPECTRAL6: columns 0..min(2 | 6, k-1), every row of norm > 0
//                       normalised, KMeans::run with K = cluster_count (:229-282)
//
// KMeans::run is deterministic although it draws random indices. Every try sets centroids[i] =
// points.row(i) -- the first K rows; the random index only feeds used_pointIds. The label vector is
// declared outside the tries, so try 1 starts from all-zero labels and try t > 1 from the labels try t-1
// ended with. Labels and centroids after the first assignment pass of a try depend on the centroids alone,
// so every try runs the trajectory of try 1; the only difference is the `done` test of pass 1, which in
// try t > 1 may stop at once -- exactly when pass 1's labels equal try 1's final labels, and then the
// centroids recomputed from them equal try 1's final centroids. All tries end with the same labels and
// inertia, and since a later try replaces the best only on a strictly smaller inertia, one try is what ten
// return. Kept quirks: initial labels all 0; an empty cluster's centroid is the zero vector; centroids are
// recomputed after the last assignment, also when the cap of 100 passes ends the loop, and the inertia uses
// them; coordinate 1 of a difference is scaled by 1.2 (weighted_dist, weighted_dist2). Norms and dot
// products of short vectors add in Armadillo's order (two interleaved accumulators). With K > n the
// reference loops forever or reads past the matrix; here that model's inertia is +inf, so the gap rule
// (a gap with an infinite term is -inf or NaN and never exceeds 0.75 x the previous one) never chooses it.
//
// gmm_full::learn follows gmm_full_meat.hpp (Armadillo 10.3) step by step -- seeding, the k-means with its
// dead-mean recovery and mean-delta stop, the diagonal initial covariances, EM with the per-component update
// that is skipped when the new covariance is not positive definite, em_fix_params, the failure checks --
// with two documented departures. Seeding: Armadillo draws the subset from its own RNG stream, which cannot
// be reproduced, so the K distinct indices come from splitmix64 seeded with (K << 32) | n, each draw taken
// modulo n and redrawn when already chosen; the last-resort random sample of the dead-mean recovery draws
// from the same stream. Reductions: sums over points (accumulators, the EM progress, avg_log_p) are
// plain sums in a fixed order divided by n, where Armadillo keeps running means per thread. inv_sympd +
// log_det succeed together iff the Cholesky factorisation does (positive pivots); log_det is then
// 2 sum log L_dd. A failed fit (learn() == false) leaves an empty model in the reference, whose AIC / BIC
// are +inf; here status 0, avg_log_p -inf, AIC and BIC +inf.
//
// Shape: the data is n x <= 7 doubles and stays in L2, so this is a latency problem. Launch 1 runs eight
// independent workgroups (4 k-means, 4 GMMs), each streaming the points from global memory on every pass.
// Launch 2 (one workgroup) reads the eight results, applies the rules and labels the cells. Every sum goes
// per-thread over a fixed stride, then a shuffle butterfly per wave and the four waves in order: no float
// atomics, two runs give bit-identical labels and criteria.
#include "cluster_kernels.hpp"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace secedo {
namespace cluster {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = (int)kMaxClusters;
constexpr uint32_t kKmeansIter = 100;  // spectral_clustering.cpp:189, :279
constexpr int kGmmKmIter = 10, kGmmEmIter = 5;
constexpr double kVarFloor = 1e-10;

// Deterministic block-wide sum of NV values per thread; every thread receives the sums.
template <int NV>
__device__ void block_sum(double (&v)[NV], double *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        double x = v[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        v[j] = x;
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) lds[wave * NV + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = ((lds[j] + lds[NV + j]) + lds[2 * NV + j]) + lds[3 * NV + j];
    __syncthreads();
}

__device__ double block_max(double v, double *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    v = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
    __syncthreads();
    return v;
}

// Armadillo's sum of squares of a short vector (op_norm / op_dot / distance<eT,1>): two interleaved accumulators.
template <int D>
__device__ inline double sumsq(const double (&t)[D]) {
    double a1 = 0, a2 = 0;
    int i = 0, j = 1;
    for (; j < D; i += 2, j += 2) {
        a1 += t[i] * t[i];
        a2 += t[j] * t[j];
    }
    if (i < D) a1 += t[i] * t[i];
    return a1 + a2;
}

template <int D>
__device__ inline void load_point(const double *X, uint32_t n, uint32_t i, double (&p)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) p[d] = X[(size_t)d * n + i];
}

// weighted_dist2 (util/kmeans.cpp): coordinate 1 of the difference scaled by 1.2
template <int D>
__device__ inline double wdist2(const double (&p)[D], const double *c) {
    double t[D];
#pragma unroll
    for (int d = 0; d < D; ++d) t[d] = p[d] - c[d];
    t[1] *= 1.2;
    return sumsq<D>(t);
}

// KMeans::run(points, K, max_iter, tries) -- one try (see the header comment). cen: LDS, kMaxK * D.
// Labels in lab[n] (global). Returns the inertia; *iters = assignment passes.
template <int D>
__device__ double kmeans_block(const double *X, uint32_t n, uint32_t K, uint32_t max_iter, uint32_t *lab,
                               double *cen, double *lds, uint32_t *iters) {
    static_assert(D >= 2 && D <= 7, "k-means dims");
    constexpr int NV = kMaxK * (D + 1);
    if (threadIdx.x < (uint32_t)(kMaxK * D)) {
        const int g = threadIdx.x / D, d = threadIdx.x % D;
        cen[threadIdx.x] = (uint32_t)g < K ? X[(size_t)d * n + g] : 0.0;
    }
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) lab[i] = 0;
    __syncthreads();
    uint32_t it = 0;
    while (it < max_iter) {
        ++it;
        int changed = 0;
        double acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = 0;
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
            double p[D];
            load_point<D>(X, n, i, p);
            // nearest_cluster: the smallest weighted_dist (a norm: sqrt of the sum), first on ties
            double best_d = sqrt(wdist2<D>(p, cen));
            uint32_t best = 0;
            for (uint32_t g = 1; g < K; ++g) {
                const double dd = sqrt(wdist2<D>(p, cen + g * D));
                if (dd < best_d) {
                    best_d = dd;
                    best = g;
                }
            }
            if (best != lab[i]) changed = 1;
            lab[i] = best;
#pragma unroll
            for (int g = 0; g < kMaxK; ++g) {
                if ((uint32_t)g == best) {
#pragma unroll
                    for (int d = 0; d < D; ++d) acc[g * (D + 1) + d] += p[d];
                    acc[g * (D + 1) + D] += 1.0;
                }
            }
        }
        block_sum<NV>(acc, lds);
        if (threadIdx.x < (uint32_t)(kMaxK * D)) {
            const int g = threadIdx.x / D, d = threadIdx.x % D;
            const double cnt = acc[g * (D + 1) + D];
            double s = 0;
#pragma unroll
            for (int gg = 0; gg < kMaxK; ++gg)
#pragma unroll
                for (int dd = 0; dd < D; ++dd)
                    if (gg == g && dd == d) s = acc[gg * (D + 1) + dd];
            cen[threadIdx.x] = cnt > 0 ? s / cnt : 0.0;  // c.zeros(), then no division for an empty cluster
        }
        if (!__syncthreads_or(changed)) break;
    }
    double in[1] = {0};
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
        double p[D];
        load_point<D>(X, n, i, p);
        in[0] += wdist2<D>(p, cen + lab[i] * D);
    }
    block_sum<1>(in, lds);
    *iters = it;
    return in[0];
}

// ---------------------------------------------------------------------------------------------------------
// gmm_full::learn
// ---------------------------------------------------------------------------------------------------------

__device__ inline uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// distance<eT,1>::eval: squared Euclidean distance, interleaved accumulators
template <int D>
__device__ inline double eucl2(const double *a, const double *b) {
    double t[D];
#pragma unroll
    for (int d = 0; d < D; ++d) t[d] = a[d] - b[d];
    return sumsq<D>(t);
}

template <int D>
__device__ inline double eucl2p(const double (&a)[D], const double *b) {
    double t[D];
#pragma unroll
    for (int d = 0; d < D; ++d) t[d] = a[d] - b[d];
    return sumsq<D>(t);
}

// Cholesky of a D x D SPD matrix (row-major in, lower factor out). false when a pivot is not > 0 or not finite.
template <int D>
__device__ bool cholesky(const double *A, double *L) {
    for (int i = 0; i < D * D; ++i) L[i] = 0;
    for (int j = 0; j < D; ++j) {
        double s = A[j * D + j];
        for (int k = 0; k < j; ++k) s -= L[j * D + k] * L[j * D + k];
        if (!(s > 0) || !isfinite(s)) return false;
        const double ljj = sqrt(s);
        L[j * D + j] = ljj;
        for (int i = j + 1; i < D; ++i) {
            double t = A[i * D + j];
            for (int k = 0; k < j; ++k) t -= L[i * D + k] * L[j * D + k];
            L[i * D + j] = t / ljj;
        }
    }
    return true;
}

// inverse from the lower Cholesky factor: A^-1 = L^-T L^-1
template <int D>
__device__ void chol_inverse(const double *L, double *inv) {
    double Li[D * D];
    for (int i = 0; i < D * D; ++i) Li[i] = 0;
    for (int c = 0; c < D; ++c) {  // solve L y = e_c
        for (int i = 0; i < D; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= L[i * D + k] * Li[k * D + c];
            Li[i * D + c] = s / L[i * D + i];
        }
    }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            double s = 0;
            for (int k = 0; k < D; ++k) s += Li[k * D + i] * Li[k * D + j];
            inv[i * D + j] = s;
        }
}

struct GmmShared {
    double means[kMaxK * 5];
    double fcov[kMaxK * 25];
    double inv[kMaxK * 25];
    double hefts[kMaxK];
    double log_det_etc[kMaxK];
    double log_hefts[kMaxK];
    double new_means[kMaxK * 5];
    int fail;
};

// init_constants(): inverse + log-det (Cholesky, diagonal fallback), floored hefts. Thread 0.
template <int D>
__device__ void init_constants(GmmShared &m, uint32_t K) {
    const double tmp = (double(D) / 2.0) * log(2.0 * M_PI);
    for (uint32_t g = 0; g < K; ++g) {
        double L[D * D];
        double log_det = 0;
        if (cholesky<D>(m.fcov + g * D * D, L)) {
            chol_inverse<D>(L, m.inv + g * D * D);
            for (int d = 0; d < D; ++d) log_det += log(L[d * D + d]);
            log_det *= 2.0;
        } else {
            for (int i = 0; i < D * D; ++i) m.inv[g * D * D + i] = 0;
            for (int d = 0; d < D; ++d) {
                const double v = fmax(m.fcov[g * D * D + d * D + d], DBL_MIN);
                m.inv[g * D * D + d * D + d] = 1.0 / v;
                log_det += log(v);
            }
        }
        m.log_det_etc[g] = -1.0 * (tmp + 0.5 * log_det);
    }
    for (uint32_t g = 0; g < K; ++g) {
        m.hefts[g] = fmax(m.hefts[g], DBL_MIN);
        m.log_hefts[g] = log(m.hefts[g]);
    }
}

// em_fix_params(). Thread 0.
template <int D>
__device__ void em_fix_params(GmmShared &m, uint32_t K) {
    for (uint32_t g = 0; g < K; ++g)
        for (int d = 0; d < D; ++d) {
            double &v = m.fcov[g * D * D + d * D + d];
            if (v < kVarFloor) v = kVarFloor;
            else if (v > DBL_MAX) v = DBL_MAX;
            else if (isnan(v)) v = 1.0;
        }
    for (uint32_t g1 = 0; g1 < K; ++g1) {
        if (m.hefts[g1] > 0) {
            for (uint32_t g2 = g1 + 1; g2 < K; ++g2) {
                if (m.hefts[g2] > 0 && fabs(m.hefts[g1] - m.hefts[g2]) <= DBL_EPSILON) {
                    if (eucl2<D>(m.means + g1 * D, m.means + g2 * D) == 0) m.hefts[g2] = 0;
                }
            }
        }
    }
    double sum = 0;
    for (uint32_t g = 0; g < K; ++g) {
        double &h = m.hefts[g];
        if (h < DBL_MIN) h = DBL_MIN;
        else if (h > 1.0) h = 1.0;
        else if (isnan(h)) h = 1.0 / double(K);
        sum += h;
    }
    if (sum < 1.0 - DBL_EPSILON || sum > 1.0 + DBL_EPSILON)
        for (uint32_t g = 0; g < K; ++g) m.hefts[g] /= sum;
}

// internal_scalar_log_p(x, g)
template <int D>
__device__ inline double log_p_g(const double (&x)[D], const GmmShared &m, uint32_t g) {
    const double *mu = m.means + g * D;
    const double *inv = m.inv + g * D * D;
    double outer = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double inner = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) inner += (x[j] - mu[j]) * inv[i * D + j];  // column i of a symmetric matrix
        outer += inner * (x[i] - mu[i]);
    }
    return -0.5 * outer + m.log_det_etc[g];
}

__device__ inline double log_add_exp(double a, double b) {
    if (a < b) {
        const double t = a;
        a = b;
        b = t;
    }
    const double negdelta = b - a;
    if (negdelta < log(DBL_MIN) || !isfinite(negdelta)) return a;
    return a + log1p(exp(negdelta));
}

template <int D>
__device__ void gmm_block(const double *X, uint32_t n, uint32_t K, GmmShared &m, double *lds, ModelResult *out) {
    static_assert(D >= 1 && D <= 5, "GMM dims");
    constexpr int NVK = 1 + D + D * (D + 1) / 2;  // per component: weight, mean sums, upper covariance sums
    const uint32_t t = threadIdx.x;
    bool ok = n >= K;
    // learn(): a non-finite input fails
    {
        double bad = 0;
        for (uint32_t i = t; ok && i < n; i += kThreads)
            for (int d = 0; d < D; ++d)
                if (!isfinite(X[(size_t)d * n + i])) bad = 1;
        ok = ok && block_max(bad, lds) == 0;
    }
    uint64_t rng = ((uint64_t)K << 32) | n;
    if (ok) {
        // generate_initial_means, random_subset: K distinct indices
        uint32_t idx[kMaxK];
        for (uint32_t g = 0; g < K; ++g) {
            for (;;) {
                const uint32_t c = (uint32_t)(splitmix64(rng) % n);
                bool dup = false;
                for (uint32_t h = 0; h < g; ++h) dup = dup || idx[h] == c;
                if (!dup) {
                    idx[g] = c;
                    break;
                }
            }
        }
        if (t == 0) {
            m.fail = 0;
            for (uint32_t g = 0; g < K; ++g)
                for (int d = 0; d < D; ++d) m.means[g * D + d] = X[(size_t)d * n + idx[g]];
        }
        __syncthreads();
        // km_iterate<1>(X, 10)
        for (int iter = 1; iter <= kGmmKmIter; ++iter) {
            constexpr int NV = kMaxK * (D + 1);
            double acc[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[j] = 0;
            double last[kMaxK] = {-1, -1, -1, -1};
            for (uint32_t i = t; i < n; i += kThreads) {
                double p[D];
                load_point<D>(X, n, i, p);
                double min_d = INFINITY;
                uint32_t best = 0;
                for (uint32_t g = 0; g < K; ++g) {
                    const double dd = eucl2p<D>(p, m.means + g * D);
                    if (dd < min_d) {
                        min_d = dd;
                        best = g;
                    }
                }
#pragma unroll
                for (int g = 0; g < kMaxK; ++g)
                    if ((uint32_t)g == best) {
#pragma unroll
                        for (int d = 0; d < D; ++d) acc[g * (D + 1) + d] += p[d];
                        acc[g * (D + 1) + D] += 1.0;
                        last[g] = (double)i;
                    }
            }
            block_sum<NV>(acc, lds);
#pragma unroll
            for (int g = 0; g < kMaxK; ++g) last[g] = block_max(last[g], lds);
            if (t == 0) {
                for (uint32_t g = 0; g < K; ++g) {
                    double cnt = 0;
                    for (int gg = 0; gg < kMaxK; ++gg)
                        if ((uint32_t)gg == g) cnt = acc[gg * (D + 1) + D];
                    for (int d = 0; d < D; ++d) {
                        double s = 0;
                        for (int gg = 0; gg < kMaxK; ++gg)
                            if ((uint32_t)gg == g) s = acc[gg * (D + 1) + d];
                        m.new_means[g * D + d] = cnt >= 1 ? s / cnt : 0.0;
                    }
                }
                // heuristics to resurrect dead means: donors are the live means with >= 2 points, highest index first
                uint32_t live[kMaxK], n_live = 0, used = 0;
                for (int g = kMaxK - 1; g >= 0; --g)
                    if ((uint32_t)g < K && acc[g * (D + 1) + D] >= 2) live[n_live++] = (uint32_t)g;
                for (uint32_t g = 0; g < K && !m.fail; ++g) {
                    if (acc[g * (D + 1) + D] != 0) continue;
                    if (n_live == 0) {
                        m.fail = 1;
                        break;
                    }
                    uint32_t proposed;
                    if (used < n_live) {
                        const uint32_t donor = live[used++];
                        proposed = last[donor] >= 0 ? (uint32_t)last[donor] : 0;
                    } else {
                        proposed = (uint32_t)(splitmix64(rng) % n);
                    }
                    for (int d = 0; d < D; ++d) m.new_means[g * D + d] = X[(size_t)d * n + proposed];
                }
                // running mean of the distances old -> new, then swap
                double rs = 0;
                for (uint32_t g = 0; g < K; ++g) {
                    const double dd = eucl2<D>(m.means + g * D, m.new_means + g * D);
                    rs = g == 0 ? dd : rs + (dd - rs) / double(g + 1);
                }
                for (uint32_t j = 0; j < K * D; ++j) m.means[j] = m.new_means[j];
                if (rs <= DBL_EPSILON) m.fail |= 2;  // converged: stop flag
            }
            __syncthreads();
            const int f = m.fail;
            __syncthreads();
            if (f & 1) break;
            if (f & 2) {
                if (t == 0) m.fail = 0;
                __syncthreads();
                break;
            }
        }
        if (t == 0 && !m.fail)
            for (uint32_t j = 0; j < K * D; ++j)
                if (!isfinite(m.means[j])) m.fail = 1;
        __syncthreads();
        ok = !m.fail;
        __syncthreads();
    }
    if (ok) {
        // generate_initial_params<1>: hard assignment, diagonal covariances
        constexpr int NV = kMaxK * (2 * D + 1);
        double acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = 0;
        for (uint32_t i = t; i < n; i += kThreads) {
            double p[D];
            load_point<D>(X, n, i, p);
            double min_d = INFINITY;
            uint32_t best = 0;
            for (uint32_t g = 0; g < K; ++g) {
                const double dd = eucl2p<D>(p, m.means + g * D);
                if (dd < min_d) {
                    min_d = dd;
                    best = g;
                }
            }
#pragma unroll
            for (int g = 0; g < kMaxK; ++g)
                if ((uint32_t)g == best) {
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        acc[g * (2 * D + 1) + d] += p[d];
                        acc[g * (2 * D + 1) + D + d] += p[d] * p[d];
                    }
                    acc[g * (2 * D + 1) + 2 * D] += 1.0;
                }
        }
        block_sum<NV>(acc, lds);
        if (t == 0) {
            for (int g = 0; g < kMaxK; ++g) {
                if ((uint32_t)g >= K) continue;
                const double heft = acc[g * (2 * D + 1) + 2 * D];
                for (int i = 0; i < D * D; ++i) m.fcov[g * D * D + i] = 0;
                for (int d = 0; d < D; ++d) {
                    const double tmp = acc[g * (2 * D + 1) + d] / heft;
                    m.means[g * D + d] = heft >= 1 ? tmp : 0.0;
                    m.fcov[g * D * D + d * D + d] =
                            heft >= 2 ? (acc[g * (2 * D + 1) + D + d] / heft) - tmp * tmp : kVarFloor;
                }
                m.hefts[g] = heft / double(n);
            }
            em_fix_params<D>(m, K);
        }
        __syncthreads();
        // em_iterate(X, 5)
        double old_avg = -INFINITY;
        int em_it = 0;
        for (int iter = 1; iter <= kGmmEmIter; ++iter) {
            em_it = iter;
            if (t == 0) init_constants<D>(m, K);
            __syncthreads();
            constexpr int NV2 = kMaxK * NVK + 1;
            double acc2[NV2];
#pragma unroll
            for (int j = 0; j < NV2; ++j) acc2[j] = 0;
            for (uint32_t i = t; i < n; i += kThreads) {
                double x[D];
                load_point<D>(X, n, i, x);
                double gl[kMaxK];
#pragma unroll
                for (int g = 0; g < kMaxK; ++g) gl[g] = (uint32_t)g < K ? log_p_g<D>(x, m, g) + m.log_hefts[g] : 0.0;
                double lsum = gl[0];
#pragma unroll
                for (int g = 1; g < kMaxK; ++g)
                    if ((uint32_t)g < K) lsum = log_add_exp(lsum, gl[g]);
                acc2[kMaxK * NVK] += lsum;
#pragma unroll
                for (int g = 0; g < kMaxK; ++g) {
                    if ((uint32_t)g >= K) continue;
                    const double w = exp(gl[g] - lsum);
                    double *a = acc2 + g * NVK;
                    a[0] += w;
#pragma unroll
                    for (int d = 0; d < D; ++d) a[1 + d] += x[d] * w;
                    int o = 1 + D;
#pragma unroll
                    for (int d = 0; d < D; ++d)
#pragma unroll
                        for (int e = d; e < D; ++e) a[o++] += w * (x[d] * x[e]);
                }
            }
            block_sum<NV2>(acc2, lds);
            if (t == 0) {
                // em_update_params: per component, skipped when the new covariance fails the checks
                for (int g = 0; g < kMaxK; ++g) {
                    if ((uint32_t)g >= K) continue;
                    const double *a = acc2 + g * NVK;
                    const double an = fmax(a[0], DBL_MIN);
                    if (!isfinite(an)) continue;
                    double mu[D], cov[D * D];
                    for (int d = 0; d < D; ++d) mu[d] = a[1 + d] / an;
                    int o = 1 + D;
                    for (int d = 0; d < D; ++d)
                        for (int e = d; e < D; ++e, ++o) {
                            cov[d * D + e] = a[o] / an - mu[d] * mu[e];
                            cov[e * D + d] = a[o] / an - mu[e] * mu[d];
                        }
                    bool fin = true;
                    for (int d = 0; d < D; ++d)
                        if (cov[d * D + d] < kVarFloor) cov[d * D + d] = kVarFloor;
                    for (int j = 0; j < D * D; ++j) fin = fin && isfinite(cov[j]);
                    if (!fin) continue;
                    double L[D * D];
                    if (!cholesky<D>(cov, L)) continue;
                    m.hefts[g] = an / double(n);
                    for (int d = 0; d < D; ++d) m.means[g * D + d] = mu[d];
                    for (int j = 0; j < D * D; ++j) m.fcov[g * D * D + j] = cov[j];
                }
                em_fix_params<D>(m, K);
                const double new_avg = acc2[kMaxK * NVK] / double(n);
                m.fail = !isfinite(new_avg) ? 1 : (fabs(old_avg - new_avg) <= DBL_EPSILON ? 2 : 0);
                lds[0] = new_avg;
            }
            __syncthreads();
            const int f = m.fail;
            old_avg = lds[0];
            __syncthreads();
            if (f) break;
        }
        if (t == 0) {
            if (m.fail == 2) m.fail = 0;
            for (uint32_t g = 0; g < K; ++g) {
                for (int d = 0; d < D; ++d)
                    if (!(m.fcov[g * D * D + d * D + d] > 0)) m.fail = 1;
                for (int j = 0; j < D; ++j) m.fail |= !isfinite(m.means[g * D + j]);
                for (int j = 0; j < D * D; ++j) m.fail |= !isfinite(m.fcov[g * D * D + j]);
                m.fail |= !isfinite(m.hefts[g]);
            }
            if (!m.fail) init_constants<D>(m, K);
            out->iterations = (uint32_t)em_it;
        }
        __syncthreads();
        ok = !m.fail;
        __syncthreads();
    }
    if (!ok) {
        if (t == 0) {
            out->status = 0;
            out->avg_log_p = -INFINITY;
            out->aic = INFINITY;
            out->bic = INFINITY;
        }
        return;
    }
    // avg_log_p over the data, then aic() / bic() with num_params()
    double s[1] = {0};
    for (uint32_t i = t; i < n; i += kThreads) {
        double x[D];
        load_point<D>(X, n, i, x);
        double lsum = log_p_g<D>(x, m, 0) + m.log_hefts[0];
        for (uint32_t g = 1; g < K; ++g) lsum = log_add_exp(lsum, log_p_g<D>(x, m, g) + m.log_hefts[g]);
        s[0] += lsum;
    }
    block_sum<1>(s, lds);
    if (t == 0) {
        const double avg = s[0] / double(n);
        const uint32_t np = K * D * (D + 1) / 2 + K * D + K - 1;
        out->status = 1;
        out->avg_log_p = avg;
        out->aic = double(2u * np) - 2.0 * double(n) * avg;
        out->bic = double(np) * log(double(n)) - 2.0 * double(n) * avg;
    }
}

template <int D>
__device__ void kmeans_dispatch_inertia(const double *X, uint32_t n, uint32_t K, uint32_t *lab, double *cen,
                                        double *lds, ModelResult *out) {
    uint32_t it = 0;
    const double in = kmeans_block<D>(X, n, K, kKmeansIter, lab, cen, lds, &it);
    if (threadIdx.x == 0) {
        out->inertia = in;
        out->iterations = it;
    }
}

__device__ void kmeans_any(const double *X, uint32_t n, uint32_t dims, uint32_t K, uint32_t max_iter, uint32_t *lab,
                           double *cen, double *lds, ModelResult *out) {
    uint32_t it = 0;
    double in = 0;
    switch (dims) {
        case 2: in = kmeans_block<2>(X, n, K, max_iter, lab, cen, lds, &it); break;
        case 3: in = kmeans_block<3>(X, n, K, max_iter, lab, cen, lds, &it); break;
        case 4: in = kmeans_block<4>(X, n, K, max_iter, lab, cen, lds, &it); break;
        case 5: in = kmeans_block<5>(X, n, K, max_iter, lab, cen, lds, &it); break;
        case 6: in = kmeans_block<6>(X, n, K, max_iter, lab, cen, lds, &it); break;
        default: in = kmeans_block<7>(X, n, K, max_iter, lab, cen, lds, &it); break;
    }
    if (threadIdx.x == 0) {
        out->inertia = in;
        out->iterations = it;
    }
}

__device__ void gmm_any(const double *X, uint32_t n, uint32_t dims, uint32_t K, GmmShared &m, double *lds,
                        ModelResult *out) {
    if (threadIdx.x == 0) {
        out->inertia = 0;
        out->iterations = 0;
    }
    switch (dims) {
        case 1: gmm_block<1>(X, n, K, m, lds, out); break;
        case 2: gmm_block<2>(X, n, K, m, lds, out); break;
        case 3: gmm_block<3>(X, n, K, m, lds, out); break;
        case 4: gmm_block<4>(X, n, K, m, lds, out); break;
        default: gmm_block<5>(X, n, K, m, lds, out); break;
    }
}

constexpr int kLdsDoubles = kWaves * (kMaxK * (1 + 5 + 15) + 1);  // the widest block_sum (EM, D = 5)

// Launch 1: blocks 0..3 the k-means of the cluster count (K = block + 1), blocks 4..7 the GMMs.
__global__ __launch_bounds__(kThreads) void k_models(const double *ev, uint32_t n, uint32_t k, uint32_t *lab_scratch,
                                                     Decision *dec) {
    __shared__ double lds[kLdsDoubles];
    __shared__ double cen[kMaxK * 7];
    __shared__ GmmShared m;
    const uint32_t b = blockIdx.x;
    if (b < kMaxClusters) {
        const uint32_t K = b + 1;
        ModelResult *out = &dec->kmeans[b];
        if (K > n) {  // the reference loops forever here: define +inf, never chosen
            if (threadIdx.x == 0) {
                *out = ModelResult{INFINITY, 0, 0, 0, 0, 0};
            }
            return;
        }
        if (threadIdx.x == 0) {
            out->avg_log_p = out->aic = out->bic = 0;
            out->status = 0;
        }
        const uint32_t dims = (k - 1 < 2 ? k - 1 : 2) + 1;  // columns 0..min(2, k-1)
        kmeans_any(ev, n, dims, K, kKmeansIter, lab_scratch + (size_t)b * n, cen, lds, out);
    } else {
        const uint32_t K = b - kMaxClusters + 1;
        const uint32_t dims = k - 1 < 5 ? k - 1 : 5;  // columns 1..min(5, k-1)
        gmm_any(ev + n, n, dims, K, m, lds, &dec->gmm[b - kMaxClusters]);
    }
}

// Launch 2: rules, labels.
__global__ __launch_bounds__(kThreads) void k_labels(const double *ev, uint32_t n, uint32_t k, int type, int termination,
                                                     double *cluster, uint32_t *lab, double *Y, Decision *dec) {
    __shared__ double lds[kLdsDoubles];
    __shared__ double cen[kMaxK * 7];
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0) {
        // gap rule (:193-205)
        double gaps[kMaxK - 1];
        for (int i = 1; i < kMaxK; ++i) gaps[i - 1] = dec->kmeans[i - 1].inertia - dec->kmeans[i].inertia;
        uint32_t count = 2;
        for (int i = 1; i < kMaxK - 1; ++i) {
            if (gaps[i] > 0.75 * gaps[i - 1]) count = i + 2;
            else break;
        }
        // termination (:286-288), the precedence of the reference kept: (all failed || AIC) ? AIC test : BIC test
        const ModelResult *g = dec->gmm;
        bool done;
        if ((!g[1].status && !g[2].status && !g[3].status) || termination == 0)
            done = g[0].aic < fmin(fmin(g[1].aic, g[2].aic), g[3].aic);
        else
            done = g[0].bic < fmin(fmin(g[1].bic, g[2].bic), g[3].bic);
        dec->cluster_count = count;
        dec->num_clusters = done ? 1 : count;
        dec->label_iterations = 0;
        dec->reserved = 0;
        s_count = count;
    }
    __syncthreads();
    const uint32_t count = s_count < n ? s_count : n;  // cluster_count <= n by the gap rule; kept in bounds anyway
    if (type == 0) {  // FIEDLER
        double mn = INFINITY;
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) mn = fmin(mn, ev[n + i]);
        mn = -block_max(-mn, lds);
        const double threshold = mn == 0 ? DBL_MIN : 0.0;
        for (uint32_t i = threadIdx.x; i < n; i += kThreads) cluster[i] = ev[n + i] >= threshold ? 1.0 : 0.0;
        return;
    }
    const uint32_t last = type == 1 ? 2u : 6u;
    const uint32_t dims = (k - 1 < last ? k - 1 : last) + 1;
    // normalise every row of norm > 0 into Y (column-major n x dims)
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
        double r[7];
        double a1 = 0, a2 = 0;
        uint32_t a = 0, b = 1;
        for (uint32_t d = 0; d < dims; ++d) r[d] = ev[(size_t)d * n + i];
        for (; b < dims; a += 2, b += 2) {
            a1 += r[a] * r[a];
            a2 += r[b] * r[b];
        }
        if (a < dims) a1 += r[a] * r[a];
        const double norm = sqrt(a1 + a2);
        for (uint32_t d = 0; d < dims; ++d) Y[(size_t)d * n + i] = norm > 0 ? r[d] / norm : r[d];
    }
    __syncthreads();
    __threadfence_block();
    ModelResult res;
    kmeans_any(Y, n, dims, count, kKmeansIter, lab, cen, lds, &res);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) cluster[i] = (double)lab[i];
    if (threadIdx.x == 0) dec->label_iterations = res.iterations;
}

__global__ __launch_bounds__(kThreads) void k_kmeans(const double *X, uint32_t n, uint32_t dims, uint32_t K,
                                                     uint32_t max_iter, uint32_t *lab, ModelResult *out) {
    __shared__ double lds[kLdsDoubles];
    __shared__ double cen[kMaxK * 7];
    ModelResult res;
    kmeans_any(X, n, dims, K, max_iter, lab, cen, lds, &res);
    if (threadIdx.x == 0) *out = ModelResult{res.inertia, 0, 0, 0, 0, res.iterations};
}

__global__ __launch_bounds__(kThreads) void k_gmm(const double *X, uint32_t n, uint32_t dims, uint32_t K,
                                                  ModelResult *out) {
    __shared__ double lds[kLdsDoubles];
    __shared__ GmmShared m;
    gmm_any(X, n, dims, K, m, lds, out);
}

__device__ inline int child_of(double v, uint32_t num_clusters) {
    for (uint32_t c = 0; c < num_clusters; ++c)
        if (fabs(v - (double)c) < 0.05) return (int)c;
    return -1;
}

// One workgroup: ordered compaction of the positions into the children (wave ballots + LDS wave offsets).
__global__ __launch_bounds__(kThreads) void k_partition(const double *cluster, uint32_t n_sub, uint32_t num_clusters,
                                                        const uint32_t *p2i, uint32_t n_groups, uint32_t *child_i2p,
                                                        uint32_t *child_p2i, uint32_t *info) {
    __shared__ uint32_t wave_cnt[kWaves][kMaxK];
    __shared__ uint32_t base[kMaxK];
    __shared__ uint32_t maxg[kMaxK];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t j = threadIdx.x; j < (size_t)num_clusters * n_groups; j += kThreads) child_i2p[j] = kNoPos;
    if (threadIdx.x < kMaxK) {
        base[threadIdx.x] = 0;
        maxg[threadIdx.x] = 0;
    }
    __syncthreads();
    for (uint32_t start = 0; start < n_sub; start += kThreads) {
        const uint32_t i = start + threadIdx.x;
        const int c = i < n_sub ? child_of(cluster[i], num_clusters) : -1;
        uint32_t rank = 0;
        for (int cc = 0; cc < kMaxK; ++cc) {
            const uint64_t mask = __ballot(c == cc);
            if (c == cc) rank = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wave_cnt[wave][cc] = __popcll(mask);
        }
        __syncthreads();
        if (c >= 0) {
            uint32_t pos = base[c] + rank;
            for (uint32_t w = 0; w < wave; ++w) pos += wave_cnt[w][c];
            const uint32_t g = p2i[i];
            child_p2i[(size_t)c * n_sub + pos] = g;
            if (g < n_groups) child_i2p[(size_t)c * n_groups + g] = pos;
            atomicMax(&maxg[c], g);
        }
        __syncthreads();
        if (threadIdx.x < kMaxK)
            for (uint32_t w = 0; w < kWaves; ++w) base[threadIdx.x] += wave_cnt[w][threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < kMaxK) {
        info[threadIdx.x] = base[threadIdx.x];
        info[kMaxK + threadIdx.x] = maxg[threadIdx.x];
    }
}

__global__ void k_label_cells(const double *cluster, uint32_t n_sub, uint32_t num_clusters, const uint16_t *id_to_group,
                              uint32_t n_cells, const uint32_t *id_to_pos, uint32_t n_groups, uint32_t cluster_idx,
                              uint16_t *clusters) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_cells) return;
    const uint32_t g = id_to_group[cell];
    if (g >= n_groups) return;
    const uint32_t p = id_to_pos[g];
    if (p == kNoPos || p >= n_sub) return;
    const int c = child_of(cluster[p], num_clusters);
    clusters[cell] = c >= 0 ? (uint16_t)(cluster_idx + (uint32_t)c) : (uint16_t)0;
}

}  // namespace

static size_t labels_words(uint32_t n) { return ((size_t)n * 5 + 1) / 2 * 2; }  // keeps the doubles aligned

size_t decide_scratch_bytes(uint32_t n) {
    // count k-means labels (4 n), label k-means labels (n), normalised rows (7 n doubles)
    return labels_words(n) * sizeof(uint32_t) + (size_t)n * 7 * sizeof(double);
}

hipError_t decide(const double *d_ev, uint32_t n, uint32_t k, int clustering_type, int termination,
                  double *d_cluster, Decision *d_decision, void *d_scratch, hipStream_t stream) {
    uint32_t *lab = static_cast<uint32_t *>(d_scratch);
    double *Y = reinterpret_cast<double *>(lab + labels_words(n));
    hipLaunchKernelGGL(k_models, dim3(2 * kMaxClusters), dim3(kThreads), 0, stream, d_ev, n, k, lab, d_decision);
    hipLaunchKernelGGL(k_labels, dim3(1), dim3(kThreads), 0, stream, d_ev, n, k, clustering_type, termination,
                       d_cluster, lab + (size_t)n * 4, Y, d_decision);
    return hipGetLastError();
}

hipError_t kmeans(const double *d_points, uint32_t n, uint32_t dims, uint32_t K, uint32_t max_iter, uint32_t *d_labels,
                  ModelResult *d_result, hipStream_t stream) {
    hipLaunchKernelGGL(k_kmeans, dim3(1), dim3(kThreads), 0, stream, d_points, n, dims, K, max_iter, d_labels,
                       d_result);
    return hipGetLastError();
}

hipError_t gmm(const double *d_points, uint32_t n, uint32_t dims, uint32_t K, ModelResult *d_result,
               hipStream_t stream) {
    hipLaunchKernelGGL(k_gmm, dim3(1), dim3(kThreads), 0, stream, d_points, n, dims, K, d_result);
    return hipGetLastError();
}

hipError_t partition(const double *d_cluster, uint32_t n_sub, uint32_t num_clusters, const uint32_t *d_pos_to_id,
                     uint32_t n_groups, uint32_t *d_child_i2p, uint32_t *d_child_p2i, uint32_t *d_child_info,
                     const uint16_t *d_id_to_group, uint32_t n_cells, const uint32_t *d_id_to_pos,
                     uint32_t cluster_idx, uint16_t *d_clusters, hipStream_t stream) {
    hipLaunchKernelGGL(k_partition, dim3(1), dim3(kThreads), 0, stream, d_cluster, n_sub, num_clusters, d_pos_to_id,
                       n_groups, d_child_i2p, d_child_p2i, d_child_info);
    if (n_cells)
        hipLaunchKernelGGL(k_label_cells, dim3((n_cells + 255) / 256), dim3(256), 0, stream, d_cluster, n_sub,
                           num_clusters, d_id_to_group, n_cells, d_id_to_pos, n_groups, cluster_idx, d_clusters);
    return hipGetLastError();
}

}  // namespace cluster
}  // namespace secedo
