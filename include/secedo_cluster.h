/*
 * secedo_cluster.h -- C-ABI of the clustering that consumes the eigenvectors: the decision step of the
 * reference's spectral_clustering() and the recursion of divide_cluster()
 * (spectral_clustering.cpp:117-299, :311-434). Library libsecedo_cluster.so, linked against
 * libsecedo_simmat.so and calling only its public C-ABI (secedo_simmat.h, secedo_spectral.h, secedo_em.h).
 *
 * Everything after eig_sym runs on the GPU (secedo_amd/csrc/cluster_kernels.hip, which documents how the
 * reference's k-means and Armadillo's gmm_full::learn are restated): one small struct of scalars crosses to
 * the host per level. Error codes are those of secedo_simmat.h; secedo_cluster_last_error() holds the
 * message, which is secedo_simmat_last_error()'s when a wrapped call failed. No CPU fallback.
 */
#ifndef SECEDO_CLUSTER_H
#define SECEDO_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SECEDO_CLUSTER_FIEDLER 0
#define SECEDO_CLUSTER_SPECTRAL2 1
#define SECEDO_CLUSTER_SPECTRAL6 2
#define SECEDO_TERMINATION_AIC 0
#define SECEDO_TERMINATION_BIC 1

#define SECEDO_CLUSTER_MAX 4u        /* models of 1..4 clusters (spectral_clustering.cpp:174) */
#define SECEDO_CLUSTER_EIGENVALUES 20u /* eigenvalues a level records (:141-143) */
#define SECEDO_CLUSTER_MARKER 64u     /* bytes of a level's marker, NUL included */

/* parse_clustering_type (:19-28): "FIEDLER" / "SPECTRAL2" / "SPECTRAL6", else SECEDO_E_INVALID_ARG. */
int secedo_cluster_type_from_string(const char *name);
/* parse_termination (:30-32): "AIC" -> AIC, anything else -> BIC (the reference's rule). */
int secedo_termination_from_string(const char *name);
const char *secedo_cluster_last_error(void);

/* One fitted model: KMeans::run (inertia, iterations = assignment passes) or gmm_full::learn (status,
 * avg_log_p, aic, bic, iterations = EM iterations). A k-means with K > n has inertia +inf; a failed GMM fit
 * has status 0, avg_log_p -inf, aic = bic = +inf. */
typedef struct secedo_cluster_model {
    double inertia;
    double avg_log_p;
    double aic;
    double bic;
    uint32_t status;
    uint32_t iterations;
} secedo_cluster_model;

/* The decision of one spectral_clustering() call. */
typedef struct secedo_cluster_decision {
    secedo_cluster_model kmeans[SECEDO_CLUSTER_MAX]; /* K = 1..4 on eigenvector columns 0..min(2, k-1) */
    secedo_cluster_model gmm[SECEDO_CLUSTER_MAX];    /* 1..4 components on columns 1..min(5, k-1) */
    uint32_t cluster_count;    /* gap rule (:193-205); 0 when fewer than 2 eigenvectors */
    uint32_t num_clusters;     /* what spectral_clustering returns: 1, or cluster_count */
    uint32_t label_iterations; /* passes of the SPECTRAL* label k-means */
    uint32_t n_vectors;        /* k = min(7, n) */
} secedo_cluster_decision;

/* Decision step on eigenvectors resident in HBM: d_eigenvectors column-major n x n_vectors (the output of
 * secedo_spectral_eigs_device with n_vectors = min(7, n)); d_cluster[n] out: labels as doubles (0/1 for
 * FIEDLER, 0..cluster_count-1 for SPECTRAL*, all 0 with fewer than 2 vectors). use_arma_kmeans is accepted
 * with FIEDLER only, where the reference ignores it; SECEDO_E_INVALID_ARG otherwise. Synchronises `stream`. */
int secedo_spectral_clustering_device(int device_id, const double *d_eigenvectors, uint32_t n, uint32_t n_vectors,
                                      int clustering_type, int termination, int use_arma_kmeans, double *d_cluster,
                                      uint32_t *num_clusters, secedo_cluster_decision *decision, void *stream);

/* spectral_clustering(const Matd &similarity, ...) on a host matrix (n x n row-major, symmetric, zero
 * diagonal): eigenpairs on the GPU, then the decision step. cluster[n] host out; eigenvalues (may be NULL)
 * receives min(20, n) values. */
int secedo_spectral_clustering(int device_id, const double *similarity, uint32_t n, int clustering_type,
                               int termination, int use_arma_kmeans, double *cluster, uint32_t *num_clusters,
                               secedo_cluster_decision *decision, double *eigenvalues);

/* KMeans::run(points, K, max_iter, tries) of util/kmeans.cpp on the device (tries make no difference, see
 * cluster_kernels.hip): d_points column-major n x dims (2 <= dims <= 7), 1 <= K <= min(4, n); d_labels[n] out. */
int secedo_cluster_kmeans_device(int device_id, const double *d_points, uint32_t n, uint32_t dims, uint32_t K,
                                 uint32_t max_iter, uint32_t *d_labels, secedo_cluster_model *model, void *stream);
/* gmm_full::learn(data, K, eucl_dist, random_subset, 10, 5, 1e-10) + avg_log_p / aic / bic on the device:
 * d_points column-major n x dims (1 <= dims <= 5), 1 <= K <= 4. */
int secedo_cluster_gmm_device(int device_id, const double *d_points, uint32_t n, uint32_t dims, uint32_t K,
                              secedo_cluster_model *model, void *stream);

/* What one level of divide_cluster() logs. */
#define SECEDO_STOP_SPLIT 0       /* partitioned; children visited per child_state */
#define SECEDO_STOP_COVERAGE 1    /* filtered coverage < 9 (:342-345) */
#define SECEDO_STOP_ONE_CLUSTER 2 /* spectral_clustering returned 1 */
#define SECEDO_CHILD_RECURSED 0
#define SECEDO_CHILD_TOO_SMALL 1  /* size < min_cluster_size (:421-423) */
#define SECEDO_CHILD_TOO_LARGE 2  /* n - size < min_cluster_size (:424-426) */
#define SECEDO_EM_NOT_RUN 0       /* not asked for, or not 2 clusters */
#define SECEDO_EM_RUN 1
#define SECEDO_EM_SKIPPED 2       /* a group id >= the sub-cluster size: the reference reads past its vector */

typedef struct secedo_cluster_level {
    char marker[SECEDO_CLUSTER_MARKER];
    uint32_t n_cells;        /* pos_to_id.size() */
    uint32_t stop_reason;    /* SECEDO_STOP_* */
    uint64_t kept_loci;      /* loci the filter kept */
    double coverage;         /* average coverage of the kept loci */
    double eigenvalues[SECEDO_CLUSTER_EIGENVALUES];
    uint32_t n_eigenvalues;  /* min(20, n) when the matrix was built, else 0 */
    uint32_t num_clusters;   /* spectral_clustering's return value (0 when not reached) */
    secedo_cluster_decision decision;
    uint32_t em_state;       /* SECEDO_EM_* */
    uint32_t em_iterations;
    uint32_t cluster_idx;    /* *cluster_idx before this level's children were numbered */
    uint32_t child_size[SECEDO_CLUSTER_MAX];
    uint32_t child_state[SECEDO_CLUSTER_MAX]; /* SECEDO_CHILD_* */
    /* wall time of the level's steps in ms, each ended by a stream synchronisation: filter, matrix (prepare +
     * accumulate + finalize), eigenpairs, decision, EM, partition */
    double step_ms[6];
} secedo_cluster_level;

/* divide_cluster(pds, max_read_length, id_to_group, id_to_pos, pos_to_id, mutation_rate, homozygous_rate,
 * seq_error_rate, num_threads, out_dir, normalization, termination, clustering_type, use_arma_kmeans,
 * use_expectation_maximization, min_cluster_size, cell_proportion, marker, &clusters, &cluster_idx)
 * with the raw flat pileup resident in HBM (the layout of secedo_simmat_set_pileup_device; group ids in
 * id_base). Host: id_to_group[n_cells], id_to_pos[n_groups], pos_to_id[n_pos] (consistent: id_to_pos[
 * pos_to_id[p]] == p, every other entry NO_POS = 16383), clusters[n_cells] in/out, *cluster_idx in/out.
 * normalization: SECEDO_NORM_*. cell_proportion is accepted and ignored as in the reference (:336).
 * One record per visited level, depth-first, into records[capacity]; *n_records = levels visited
 * (SECEDO_E_LIMIT when more than capacity). Synchronises `stream`. */
int secedo_divide_cluster_device(int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                                 const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                                 const uint32_t *d_read_ids, const uint16_t *d_id_base16, const uint32_t *d_id_base32,
                                 uint32_t n_loci, uint64_t n_entries, uint32_t max_read_length,
                                 const uint16_t *id_to_group, uint32_t n_cells, const uint32_t *id_to_pos,
                                 uint32_t n_groups, const uint32_t *pos_to_id, uint32_t n_pos, double mutation_rate,
                                 double homozygous_rate, double seq_error_rate, int normalization, int termination,
                                 int clustering_type, int use_arma_kmeans, int use_expectation_maximization,
                                 uint32_t min_cluster_size, uint32_t cell_proportion, const char *marker,
                                 uint16_t *clusters, uint16_t *cluster_idx, secedo_cluster_level *records,
                                 uint32_t capacity, uint32_t *n_records, void *stream);

/* Same with the flat pileup in host memory (uploaded once). */
int secedo_divide_cluster(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                          const uint64_t *locus_entry_off, const uint32_t *read_ids, const uint16_t *id_base16,
                          const uint32_t *id_base32, uint32_t max_read_length, const uint16_t *id_to_group,
                          uint32_t n_cells, const uint32_t *id_to_pos, uint32_t n_groups, const uint32_t *pos_to_id,
                          uint32_t n_pos, double mutation_rate, double homozygous_rate, double seq_error_rate,
                          int normalization, int termination, int clustering_type, int use_arma_kmeans,
                          int use_expectation_maximization, uint32_t min_cluster_size, uint32_t cell_proportion,
                          const char *marker, uint16_t *clusters, uint16_t *cluster_idx,
                          secedo_cluster_level *records, uint32_t capacity, uint32_t *n_records);

/* The same two recursions writing the reference's output files into out_dir (created when missing), per level
 * (spectral_clustering.cpp:141-143, :236-279, :336-417):
 *   <out_dir>/significant_positions<marker>   every level, before the coverage stop: id_to_chromosome(slot) TAB
 *                                             position per kept locus, slot order
 *   out_dir + "sim_mat_eigenvalues" + marker + ".csv"        every level that built a matrix
 *   out_dir + "sim_mat_eigenvectors_norm" + marker + ".csv"  SPECTRAL2 / SPECTRAL6 with >= 2 eigenvectors:
 *                                             columns 0..min(col_idx, k - 1) (col_idx 2 resp. 6), each row divided
 *                                             by its norm when non-zero, space separated
 *   <out_dir>/spectral_clustering<marker>      num_clusters > 1: per cell NO_POS (16383) when its group is outside
 *                                             the sub-cluster, else uint16(cluster[pos]), comma separated
 *   <out_dir>/expectation_maximization<marker> the same on the post-EM values, when EM ran (SECEDO_EM_RUN)
 *   <out_dir>/clustering                       after every split: the clusters of all cells so far
 * (the two eigen files are a plain concatenation of out_dir and the name, as in the reference). Departures: the
 * eigenvalue file holds the min(20, n) recorded eigenvalues (the reference's cols(0, min(20, n_cols - 1)) of a
 * column vector writes all n, against its own comment); numbers are written with %.17g, not Armadillo's layout;
 * no expectation_maximization file when EM is SECEDO_EM_SKIPPED (the reference reads past its vector there);
 * n_chr > 24 is SECEDO_E_INVALID_ARG, as slots are named by chromosome id. */
int secedo_divide_cluster_files_device(int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                                       const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                                       const uint32_t *d_read_ids, const uint16_t *d_id_base16,
                                       const uint32_t *d_id_base32, uint32_t n_loci, uint64_t n_entries,
                                       uint32_t max_read_length, const uint16_t *id_to_group, uint32_t n_cells,
                                       const uint32_t *id_to_pos, uint32_t n_groups, const uint32_t *pos_to_id,
                                       uint32_t n_pos, double mutation_rate, double homozygous_rate,
                                       double seq_error_rate, int normalization, int termination, int clustering_type,
                                       int use_arma_kmeans, int use_expectation_maximization,
                                       uint32_t min_cluster_size, uint32_t cell_proportion, const char *marker,
                                       uint16_t *clusters, uint16_t *cluster_idx, secedo_cluster_level *records,
                                       uint32_t capacity, uint32_t *n_records, void *stream, const char *out_dir);

int secedo_divide_cluster_files(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr,
                                const uint32_t *locus_pos, const uint64_t *locus_entry_off, const uint32_t *read_ids,
                                const uint16_t *id_base16, const uint32_t *id_base32, uint32_t max_read_length,
                                const uint16_t *id_to_group, uint32_t n_cells, const uint32_t *id_to_pos,
                                uint32_t n_groups, const uint32_t *pos_to_id, uint32_t n_pos, double mutation_rate,
                                double homozygous_rate, double seq_error_rate, int normalization, int termination,
                                int clustering_type, int use_arma_kmeans, int use_expectation_maximization,
                                uint32_t min_cluster_size, uint32_t cell_proportion, const char *marker,
                                uint16_t *clusters, uint16_t *cluster_idx, secedo_cluster_level *records,
                                uint32_t capacity, uint32_t *n_records, const char *out_dir);

#ifdef __cplusplus
}
#endif

#endif /* SECEDO_CLUSTER_H */
