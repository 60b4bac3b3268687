// cluster_kernels.hpp -- launch wrappers of cluster_kernels.hip (gfx950): the decision step of the
// reference's spectral_clustering() after eig_sym (spectral_clustering.cpp:140-298) and the partition
// of divide_cluster() (:379-433). See cluster_kernels.hip for the rules they restate.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace secedo {
namespace cluster {

constexpr uint32_t kMaxClusters = 4;  // spectral_clustering.cpp:174
constexpr uint32_t kNoPos = 16383;    // NO_POS, util/is_significant.hpp:11

// One fitted model: a KMeans::run (inertia) or an arma::gmm_full::learn (status, avg_log_p, aic, bic).
struct ModelResult {
    double inertia;    // k-means; +inf when K > n
    double avg_log_p;  // GMM; -inf when the fit failed
    double aic;        // GMM; +inf when the fit failed
    double bic;        // GMM; +inf when the fit failed
    uint32_t status;   // GMM: 1 = learn() returned true
    uint32_t iterations;  // k-means: assignment passes; GMM: EM iterations run
};

// What crosses to the host per level.
struct Decision {
    ModelResult kmeans[kMaxClusters];
    ModelResult gmm[kMaxClusters];
    uint32_t cluster_count;  // gap rule, :193-205
    uint32_t num_clusters;   // 1 when the termination rule says done, else cluster_count
    uint32_t label_iterations;  // passes of the label k-means (0 for FIEDLER)
    uint32_t reserved;
};

// Launch 1 + launch 2: d_ev column-major n x k (k = min(7, n) >= 2), d_cluster[n] out (labels as doubles),
// d_decision out. d_scratch: decide_scratch_bytes(n).
size_t decide_scratch_bytes(uint32_t n);
hipError_t decide(const double *d_ev, uint32_t n, uint32_t k, int clustering_type, int termination,
                  double *d_cluster, Decision *d_decision, void *d_scratch, hipStream_t stream);

// KMeans::run on d_points (column-major n x dims, 2 <= dims <= 7, 1 <= K <= 4, K <= n): labels, result.
hipError_t kmeans(const double *d_points, uint32_t n, uint32_t dims, uint32_t K, uint32_t max_iter,
                  uint32_t *d_labels, ModelResult *d_result, hipStream_t stream);
// gmm_full::learn (+ avg_log_p, aic, bic) on d_points (column-major n x dims, 1 <= dims <= 5, 1 <= K <= 4).
hipError_t gmm(const double *d_points, uint32_t n, uint32_t dims, uint32_t K, ModelResult *d_result,
               hipStream_t stream);

// Partition (:379-416) of the n_sub positions into num_clusters children: a position joins child c iff
// |cluster - c| < 0.05 (first such c). d_child_i2p[num_clusters * n_groups] (NO_POS outside the child),
// d_child_p2i[num_clusters * n_sub] (the reference's order), d_child_info[2 * kMaxClusters]: sizes, then the
// largest group id of every child (0 when empty). Then every cell whose group lies in the sub-cluster gets
// cluster_idx + c, or 0 when unassigned.
hipError_t partition(const double *d_cluster, uint32_t n_sub, uint32_t num_clusters, const uint32_t *d_pos_to_id,
                     uint32_t n_groups, uint32_t *d_child_i2p, uint32_t *d_child_p2i, uint32_t *d_child_info,
                     const uint16_t *d_id_to_group, uint32_t n_cells, const uint32_t *d_id_to_pos,
                     uint32_t cluster_idx, uint16_t *d_clusters, hipStream_t stream);

}  // namespace cluster
}  // namespace secedo
