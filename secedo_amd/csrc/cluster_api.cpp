// cluster_api.cpp -- host side of include/secedo_cluster.h: the decision step around the kernels of
// cluster_kernels.hip, and the recursion of the reference's divide_cluster() (spectral_clustering.cpp:311-434)
// with the pileup resident in HBM. Calls libsecedo_simmat.so through its public C-ABI only.
//
// One level: secedo_filter_device on the original pileup with the level's id_to_pos -> stop below coverage 9 ->
// the matrix of the filtered pileup through one reused simmat handle -> 20 eigenvalues, 7 eigenvectors ->
// decision -> EM when asked and 2 clusters -> partition -> children depth-first. The matrix and the
// eigenvectors of a level are freed before its children run; id_to_pos / pos_to_id of the children stay on the
// device, only their sizes (and largest group ids, for the EM rule) come back. The labels live on the device
// until the top-level call returns.
#include "secedo_cluster.h"
#include "secedo_em.h"
#include "secedo_simmat.h"
#include "secedo_spectral.h"
#include "cluster_kernels.hpp"
#include "host_util.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

namespace {

using secedo::cluster::Decision;
using secedo::cluster::kNoPos;
using secedo::cluster::ModelResult;
using namespace secedo::host;

// Host threads secedo_simmat_prepare may use when a level's pileup needs the host packing path (a read split at
// a flush; the device path ignores it). The reference's num_threads has no counterpart in this C-ABI, which
// takes no thread count: a fixed, moderate width.
constexpr uint32_t kPrepareThreads = 8;

// a wrapped libsecedo_simmat call failed: forward its message
int forward(int code, const char *what) {
    const char *m = secedo_simmat_last_error();
    return fail(code, std::string(what) + ": " + (m ? m : ""));
}

#define CL_CALL(expr)                                  \
    do {                                               \
        int rc_ = (expr);                              \
        if (rc_ != SECEDO_OK) return forward(rc_, #expr); \
    } while (0)

int check_device(int device_id) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(SECEDO_E_NO_DEVICE, "no HIP device is visible: the clustering step has no CPU fallback");
    if (device_id < 0 || device_id >= n_dev) return fail(SECEDO_E_NO_DEVICE, "device id out of range");
    SECEDO_TRY(hipSetDevice(device_id));
    return SECEDO_OK;
}

int check_options(int clustering_type, int termination, int use_arma_kmeans) {
    if (clustering_type < SECEDO_CLUSTER_FIEDLER || clustering_type > SECEDO_CLUSTER_SPECTRAL6)
        return fail(SECEDO_E_INVALID_ARG, "unknown clustering type");
    if (termination != SECEDO_TERMINATION_AIC && termination != SECEDO_TERMINATION_BIC)
        return fail(SECEDO_E_INVALID_ARG, "unknown termination");
    if (use_arma_kmeans && clustering_type != SECEDO_CLUSTER_FIEDLER)
        return fail(SECEDO_E_INVALID_ARG,
                    "use_arma_kmeans (Armadillo's randomly seeded k-means) is not provided; it is accepted with FIEDLER "
                    "only, where the reference ignores it");
    return SECEDO_OK;
}

void copy_model(const ModelResult &m, secedo_cluster_model *out) {
    out->inertia = m.inertia;
    out->avg_log_p = m.avg_log_p;
    out->aic = m.aic;
    out->bic = m.bic;
    out->status = m.status;
    out->iterations = m.iterations;
}

// the decision step; d_cluster is written in full. Synchronises the stream.
int decide(const double *d_ev, uint32_t n, uint32_t k, int type, int termination, double *d_cluster,
           uint32_t *num_clusters, secedo_cluster_decision *out, hipStream_t stream) {
    secedo_cluster_decision dec;
    std::memset(&dec, 0, sizeof(dec));
    dec.n_vectors = k;
    if (k < 2) {  // "Perfect decomposition, all cells in same cluster" (:160-163)
        if (n) SECEDO_TRY(hipMemsetAsync(d_cluster, 0, (size_t)n * sizeof(double), stream));
        SECEDO_TRY(hipStreamSynchronize(stream));
        dec.num_clusters = 1;
        if (num_clusters) *num_clusters = 1;
        if (out) *out = dec;
        return SECEDO_OK;
    }
    Buf scratch, d_dec;
    SECEDO_TRY(scratch.alloc(secedo::cluster::decide_scratch_bytes(n)));
    SECEDO_TRY(d_dec.alloc(sizeof(Decision)));
    SECEDO_TRY(secedo::cluster::decide(d_ev, n, k, type, termination, d_cluster, d_dec.as<Decision>(), scratch.p, stream));
    Decision h;
    SECEDO_TRY(hipMemcpyAsync(&h, d_dec.p, sizeof(Decision), hipMemcpyDeviceToHost, stream));
    SECEDO_TRY(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < SECEDO_CLUSTER_MAX; ++i) {
        copy_model(h.kmeans[i], &dec.kmeans[i]);
        copy_model(h.gmm[i], &dec.gmm[i]);
    }
    dec.cluster_count = h.cluster_count;
    dec.num_clusters = h.num_clusters;
    dec.label_iterations = h.label_iterations;
    if (num_clusters) *num_clusters = h.num_clusters;
    if (out) *out = dec;
    return SECEDO_OK;
}

struct Params {
    int device_id;
    const uint32_t *d_chr, *d_pos, *d_rid;
    const uint64_t *d_off;
    const uint16_t *d_b16;
    const uint32_t *d_b32;
    uint32_t n_chr, n_loci;
    uint64_t n_entries;
    uint32_t max_read_length;
    const uint16_t *d_id_to_group;
    uint32_t n_cells, n_groups;
    double mutation_rate, homozygous_rate, seq_error_rate;
    int normalization, termination, type, use_em;
    uint32_t min_cluster_size;
    uint16_t *d_clusters;
    secedo_simmat_t *handle;
    hipStream_t stream;
    secedo_cluster_level *records;
    uint32_t capacity, n_records;
    // the reference's output files (spectral_clustering.cpp:141-143, :236-279, :336-417) when `write` is set
    bool write;
    std::string out_dir;
    const uint16_t *id_to_group;  // host
};

// --- the files divide_cluster writes -------------------------------------------------------------------------

std::string id_to_chromosome(uint32_t c) {
    if (c < 22) return std::to_string(c + 1);
    return c == 22 ? "X" : "Y";
}

std::string in_dir(const std::string &dir, const std::string &name) {
    return (std::filesystem::path(dir) / name).string();
}

int open_out(const std::string &path, FILE **f) {
    *f = std::fopen(path.c_str(), "w");
    return *f ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, "cannot write " + path);
}

// write_vec (util.hpp:49-60): comma-joined values and a newline; an empty vector leaves an empty file
int write_vec(const std::string &path, const std::vector<uint16_t> &v) {
    FILE *f;
    if (int rc = open_out(path, &f)) return rc;
    for (size_t i = 0; i < v.size(); ++i) std::fprintf(f, i + 1 < v.size() ? "%u," : "%u\n", (unsigned)v[i]);
    std::fclose(f);
    return SECEDO_OK;
}

template <class T>
int download(std::vector<T> *out, const void *d, size_t n, hipStream_t s) {
    out->resize(n);
    if (n) SECEDO_TRY(hipMemcpyAsync(out->data(), d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    return SECEDO_OK;
}

// significant_positions<marker>: id_to_chromosome(slot) TAB position per kept locus, slot order
int write_positions(const Params &P, const std::string &marker, const uint32_t *d_chr, const uint32_t *d_pos,
                    uint64_t kept_loci) {
    std::vector<uint32_t> chr, pos;
    if (int rc = download(&chr, d_chr, P.n_chr + 1, P.stream)) return rc;
    if (int rc = download(&pos, d_pos, kept_loci, P.stream)) return rc;
    FILE *f;
    if (int rc = open_out(in_dir(P.out_dir, "significant_positions" + marker), &f)) return rc;
    for (uint32_t c = 0; c < P.n_chr; ++c) {
        const std::string name = id_to_chromosome(c);
        for (uint32_t i = chr[c]; i < chr[c + 1]; ++i) std::fprintf(f, "%s\t%u\n", name.c_str(), pos[i]);
    }
    std::fclose(f);
    return SECEDO_OK;
}

// sim_mat_eigenvalues<marker>.csv: the recorded eigenvalues, one per line (the reference's path is a plain
// concatenation of out_dir and the name)
int write_eigenvalues(const Params &P, const std::string &marker, const double *vals, uint32_t n) {
    FILE *f;
    if (int rc = open_out(P.out_dir + "sim_mat_eigenvalues" + marker + ".csv", &f)) return rc;
    for (uint32_t i = 0; i < n; ++i) std::fprintf(f, "%.17g\n", vals[i]);
    std::fclose(f);
    return SECEDO_OK;
}

// sim_mat_eigenvectors_norm<marker>.csv: eigenvector columns 0..min(col_idx, k - 1), rows scaled to unit norm
// when non-zero (:240-249); d_ev column-major n x k
int write_eigenvectors(const Params &P, const std::string &marker, const double *d_ev, uint32_t n, uint32_t k) {
    std::vector<double> ev;
    if (int rc = download(&ev, d_ev, (size_t)n * k, P.stream)) return rc;
    const uint32_t col_idx = P.type == SECEDO_CLUSTER_SPECTRAL2 ? 2 : 6;
    const uint32_t cols = std::min(col_idx, k - 1) + 1;
    FILE *f;
    if (int rc = open_out(P.out_dir + "sim_mat_eigenvectors_norm" + marker + ".csv", &f)) return rc;
    std::vector<double> row(cols);
    for (uint32_t i = 0; i < n; ++i) {
        double sq = 0;
        for (uint32_t c = 0; c < cols; ++c) {
            row[c] = ev[(size_t)c * n + i];
            sq += row[c] * row[c];
        }
        const double norm = std::sqrt(sq);
        for (uint32_t c = 0; c < cols; ++c) {
            const double v = norm > 0 ? row[c] / norm : row[c];
            std::fprintf(f, c + 1 < cols ? "%.17g " : "%.17g\n", v);
        }
    }
    std::fclose(f);
    return SECEDO_OK;
}

// spectral_clustering<marker> / expectation_maximization<marker>: per cell, NO_POS when its group is outside the
// sub-cluster, else uint16(cluster[pos]) (:356-371)
int write_id_to_cluster(const Params &P, const std::string &name, const uint32_t *d_i2p, const double *d_cluster,
                        uint32_t n_sub) {
    std::vector<uint32_t> i2p;
    std::vector<double> cl;
    if (int rc = download(&i2p, d_i2p, P.n_groups, P.stream)) return rc;
    if (int rc = download(&cl, d_cluster, n_sub, P.stream)) return rc;
    std::vector<uint16_t> out(P.n_cells);
    for (uint32_t c = 0; c < P.n_cells; ++c) {
        const uint32_t pos = i2p[P.id_to_group[c]];
        out[c] = pos == kNoPos ? (uint16_t)kNoPos : (uint16_t)cl[pos];
    }
    return write_vec(in_dir(P.out_dir, name), out);
}

// One level of divide_cluster. d_i2p[n_groups], d_p2i[n_sub] on the device; max_group = largest id in d_p2i.
int level(Params &P, const uint32_t *d_i2p, const uint32_t *d_p2i, uint32_t n_sub, uint32_t max_group,
          const std::string &marker, uint16_t *cluster_idx) {
    const uint32_t rec_id = P.n_records++;
    secedo_cluster_level scratch_rec;
    secedo_cluster_level &rec = rec_id < P.capacity ? P.records[rec_id] : scratch_rec;
    std::memset(&rec, 0, sizeof(rec));
    std::snprintf(rec.marker, sizeof(rec.marker), "%s", marker.c_str());
    rec.n_cells = n_sub;
    rec.cluster_idx = *cluster_idx;
    if (marker.size() >= SECEDO_CLUSTER_MARKER) return fail(SECEDO_E_LIMIT, "recursion deeper than the marker holds");
    Clock::time_point t0 = Clock::now();

    // Filter filter(seq_error_rate): cell_proportion is the default 4 whatever the caller passed (:336)
    Buf f_chr, f_pos, f_off, f_rid, f_idb;
    const uint64_t L = P.n_loci, E = P.n_entries;
    SECEDO_TRY(f_chr.alloc((size_t)(P.n_chr + 1) * 4));
    SECEDO_TRY(f_pos.alloc((size_t)std::max<uint64_t>(L, 1) * 4));
    SECEDO_TRY(f_off.alloc((size_t)(L + 1) * 8));
    SECEDO_TRY(f_rid.alloc((size_t)std::max<uint64_t>(E, 1) * 4));
    SECEDO_TRY(f_idb.alloc((size_t)std::max<uint64_t>(E, 1) * (P.d_b16 ? 2 : 4)));
    uint64_t kept_loci = 0, kept_entries = 0;
    double coverage = 0;
    CL_CALL(secedo_filter_device(P.d_chr, P.n_chr, P.d_pos, P.d_off, P.d_rid, P.d_b16, P.d_b32, d_i2p, P.n_groups,
                                 P.n_loci, P.n_entries, P.seq_error_rate, 4, f_chr.as<uint32_t>(), f_pos.as<uint32_t>(),
                                 f_off.as<uint64_t>(), f_rid.as<uint32_t>(), f_idb.p, &kept_loci, &kept_entries,
                                 &coverage, P.stream));
    rec.step_ms[0] = ms_lap(t0);  // secedo_filter_device synchronises the stream
    rec.kept_loci = kept_loci;
    rec.coverage = coverage;
    if (P.write) {
        if (int rc = write_positions(P, marker, f_chr.as<uint32_t>(), f_pos.as<uint32_t>(), kept_loci)) return rc;
        t0 = Clock::now();
    }
    if (coverage < 9) {
        rec.stop_reason = SECEDO_STOP_COVERAGE;
        return SECEDO_OK;
    }

    // computeSimilarityMatrix on the filtered pileup, n_sub cells
    Buf sim, ev, d_cluster;
    SECEDO_TRY(sim.alloc((size_t)n_sub * n_sub * 8));
    {
        const uint16_t *b16 = P.d_b16 ? f_idb.as<uint16_t>() : nullptr;
        const uint32_t *b32 = P.d_b16 ? nullptr : f_idb.as<uint32_t>();
        CL_CALL(secedo_simmat_set_pileup_device(P.handle, f_chr.as<uint32_t>(), P.n_chr, f_pos.as<uint32_t>(),
                                                f_off.as<uint64_t>(), f_rid.as<uint32_t>(), b16, b32, d_i2p, P.n_groups,
                                                (uint32_t)kept_loci, kept_entries));
        CL_CALL(secedo_simmat_prepare(P.handle, n_sub, P.max_read_length, kPrepareThreads, 0, P.stream));
        Buf acc;
        SECEDO_TRY(acc.alloc((size_t)secedo_simmat_acc_elems(P.handle) * 8));
        CL_CALL(secedo_simmat_assign_finalize(P.handle, P.mutation_rate, P.homozygous_rate, P.seq_error_rate,
                                              P.normalization, acc.as<int64_t>(), sim.as<double>(), P.stream));
        SECEDO_TRY(hipStreamSynchronize(P.stream));
        rec.step_ms[1] = ms_lap(t0);
    }
    // laplacian + eig_sym: the 20 smallest eigenvalues, the eigenvectors of the 7 smallest
    const uint32_t n_values = std::min<uint32_t>(SECEDO_CLUSTER_EIGENVALUES, n_sub);
    const uint32_t k = std::min<uint32_t>(7, n_sub);
    SECEDO_TRY(ev.alloc((size_t)n_sub * std::max<uint32_t>(k, 1) * 8));
    SECEDO_TRY(d_cluster.alloc((size_t)std::max<uint32_t>(n_sub, 1) * 8));
    if (n_sub > 0) {
        secedo_spectral_info info;
        CL_CALL(secedo_spectral_eigs_device(P.device_id, sim.as<double>(), n_sub, n_values, k, 0, 0, rec.eigenvalues,
                                            ev.as<double>(), &info, P.stream));
        rec.n_eigenvalues = n_values;
    }
    rec.step_ms[2] = ms_lap(t0);
    if (P.write && n_sub > 0) {
        if (int rc = write_eigenvalues(P, marker, rec.eigenvalues, n_values)) return rc;
        if (P.type != SECEDO_CLUSTER_FIEDLER && k >= 2)
            if (int rc = write_eigenvectors(P, marker, ev.as<double>(), n_sub, k)) return rc;
        t0 = Clock::now();
    }
    sim.reset();
    uint32_t num_clusters = 1;
    CL_CALL(decide(ev.as<double>(), n_sub, k, P.type, P.termination, d_cluster.as<double>(), &num_clusters,
                   &rec.decision, P.stream));
    rec.step_ms[3] = ms_lap(t0);  // decide() synchronises the stream
    ev.reset();
    rec.num_clusters = num_clusters;
    if (num_clusters == 1) {
        rec.stop_reason = SECEDO_STOP_ONE_CLUSTER;
        return SECEDO_OK;
    }
    if (P.write) {
        if (int rc = write_id_to_cluster(P, "spectral_clustering" + marker, d_i2p, d_cluster.as<double>(), n_sub))
            return rc;
        t0 = Clock::now();
    }

    if (P.use_em && num_clusters == 2) {
        // expectation_maximization reads prob_cluster_b[group id]: past the vector when a group id >= n_sub
        if (max_group >= n_sub) {
            rec.em_state = SECEDO_EM_SKIPPED;
        } else {
            uint32_t iters = 0;
            const uint16_t *b16 = P.d_b16 ? f_idb.as<uint16_t>() : nullptr;
            const uint32_t *b32 = P.d_b16 ? nullptr : f_idb.as<uint32_t>();
            CL_CALL(secedo_em_refine_device(P.device_id, f_off.as<uint64_t>(), (uint32_t)kept_loci, kept_entries, b16,
                                            b32, d_i2p, P.n_groups, P.seq_error_rate, d_cluster.as<double>(), n_sub, 0,
                                            &iters, P.stream));
            rec.em_state = SECEDO_EM_RUN;
            rec.em_iterations = iters;
        }
    }
    SECEDO_TRY(hipStreamSynchronize(P.stream));
    rec.step_ms[4] = ms_lap(t0);
    if (P.write && rec.em_state == SECEDO_EM_RUN) {
        if (int rc = write_id_to_cluster(P, "expectation_maximization" + marker, d_i2p, d_cluster.as<double>(), n_sub))
            return rc;
        t0 = Clock::now();
    }
    f_chr.reset();
    f_pos.reset();
    f_off.reset();
    f_rid.reset();
    f_idb.reset();

    // partition (:379-416) and the labels of the cells
    Buf c_i2p, c_p2i, c_info;
    SECEDO_TRY(c_i2p.alloc((size_t)num_clusters * P.n_groups * 4));
    SECEDO_TRY(c_p2i.alloc((size_t)num_clusters * std::max<uint32_t>(n_sub, 1) * 4));
    SECEDO_TRY(c_info.alloc(2 * SECEDO_CLUSTER_MAX * 4));
    SECEDO_TRY(secedo::cluster::partition(d_cluster.as<double>(), n_sub, num_clusters, d_p2i, P.n_groups, c_i2p.as<uint32_t>(),
                                      c_p2i.as<uint32_t>(), c_info.as<uint32_t>(), P.d_id_to_group, P.n_cells, d_i2p,
                                      *cluster_idx, P.d_clusters, P.stream));
    uint32_t info[2 * SECEDO_CLUSTER_MAX];
    SECEDO_TRY(hipMemcpyAsync(info, c_info.p, sizeof(info), hipMemcpyDeviceToHost, P.stream));
    SECEDO_TRY(hipStreamSynchronize(P.stream));
    rec.step_ms[5] = ms_lap(t0);
    if (P.write) {
        std::vector<uint16_t> cells;
        if (int rc = download(&cells, P.d_clusters, P.n_cells, P.stream)) return rc;
        if (int rc = write_vec(in_dir(P.out_dir, "clustering"), cells)) return rc;
    }
    d_cluster.reset();
    *cluster_idx = (uint16_t)(*cluster_idx + num_clusters);
    rec.stop_reason = SECEDO_STOP_SPLIT;
    for (uint32_t c = 0; c < num_clusters; ++c) {
        rec.child_size[c] = info[c];
        if (info[c] < P.min_cluster_size) rec.child_state[c] = SECEDO_CHILD_TOO_SMALL;
        else if (n_sub - info[c] < P.min_cluster_size) rec.child_state[c] = SECEDO_CHILD_TOO_LARGE;
        else rec.child_state[c] = SECEDO_CHILD_RECURSED;
    }
    for (uint32_t c = 0; c < num_clusters; ++c) {
        if (rec.child_state[c] != SECEDO_CHILD_RECURSED) continue;
        const int rc = level(P, c_i2p.as<uint32_t>() + (size_t)c * P.n_groups, c_p2i.as<uint32_t>() + (size_t)c * n_sub,
                             info[c], info[SECEDO_CLUSTER_MAX + c], marker + static_cast<char>('A' + c), cluster_idx);
        if (rc) return rc;
    }
    return SECEDO_OK;
}

}  // namespace

extern "C" {

const char *secedo_cluster_last_error(void) { return g_error.c_str(); }

int secedo_cluster_type_from_string(const char *name) {
    const std::string s = name ? name : "";
    if (s == "FIEDLER") return SECEDO_CLUSTER_FIEDLER;
    if (s == "SPECTRAL2") return SECEDO_CLUSTER_SPECTRAL2;
    if (s == "SPECTRAL6") return SECEDO_CLUSTER_SPECTRAL6;
    return fail(SECEDO_E_INVALID_ARG, "unknown clustering type '" + s + "' (FIEDLER, SPECTRAL2 or SPECTRAL6)");
}

int secedo_termination_from_string(const char *name) {
    return name && std::string(name) == "AIC" ? SECEDO_TERMINATION_AIC : SECEDO_TERMINATION_BIC;
}

int secedo_spectral_clustering_device(int device_id, const double *d_eigenvectors, uint32_t n, uint32_t n_vectors,
                                      int clustering_type, int termination, int use_arma_kmeans, double *d_cluster,
                                      uint32_t *num_clusters, secedo_cluster_decision *decision, void *stream) {
    if (int rc = check_options(clustering_type, termination, use_arma_kmeans)) return rc;
    if (n == 0) return fail(SECEDO_E_INVALID_ARG, "no cells");
    if (n_vectors > 7 || n_vectors > n) return fail(SECEDO_E_INVALID_ARG, "n_vectors must be <= min(7, n)");
    if ((n_vectors && !d_eigenvectors) || !d_cluster) return fail(SECEDO_E_INVALID_ARG, "null device buffer");
    if (int rc = check_device(device_id)) return rc;
    return decide(d_eigenvectors, n, n_vectors, clustering_type, termination, d_cluster, num_clusters, decision,
                  static_cast<hipStream_t>(stream));
}

int secedo_spectral_clustering(int device_id, const double *similarity, uint32_t n, int clustering_type,
                               int termination, int use_arma_kmeans, double *cluster, uint32_t *num_clusters,
                               secedo_cluster_decision *decision, double *eigenvalues) {
    if (int rc = check_options(clustering_type, termination, use_arma_kmeans)) return rc;
    if (n == 0) return fail(SECEDO_E_INVALID_ARG, "no cells");
    if (!similarity || !cluster) return fail(SECEDO_E_INVALID_ARG, "null host buffer");
    if (int rc = check_device(device_id)) return rc;
    const uint32_t n_values = std::min<uint32_t>(SECEDO_CLUSTER_EIGENVALUES, n), k = std::min<uint32_t>(7, n);
    Buf a, ev, c;
    SECEDO_TRY(a.alloc((size_t)n * n * 8));
    SECEDO_TRY(ev.alloc((size_t)n * k * 8));
    SECEDO_TRY(c.alloc((size_t)n * 8));
    SECEDO_TRY(hipMemcpy(a.p, similarity, (size_t)n * n * 8, hipMemcpyHostToDevice));
    double vals[SECEDO_CLUSTER_EIGENVALUES];
    secedo_spectral_info info;
    CL_CALL(secedo_spectral_eigs_device(device_id, a.as<double>(), n, n_values, k, 0, 0, vals, ev.as<double>(), &info,
                                        nullptr));
    if (eigenvalues) std::memcpy(eigenvalues, vals, n_values * sizeof(double));
    a.reset();
    if (int rc = decide(ev.as<double>(), n, k, clustering_type, termination, c.as<double>(), num_clusters, decision,
                        nullptr))
        return rc;
    SECEDO_TRY(hipMemcpy(cluster, c.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return SECEDO_OK;
}

int secedo_cluster_kmeans_device(int device_id, const double *d_points, uint32_t n, uint32_t dims, uint32_t K,
                                 uint32_t max_iter, uint32_t *d_labels, secedo_cluster_model *model, void *stream) {
    if (n == 0) return fail(SECEDO_E_INVALID_ARG, "no points");
    if (dims < 2 || dims > 7) return fail(SECEDO_E_INVALID_ARG, "dims must be in 2..7");
    if (K < 1 || K > SECEDO_CLUSTER_MAX || K > n) return fail(SECEDO_E_INVALID_ARG, "K must be in 1..min(4, n)");
    if (!d_points || !d_labels || !model) return fail(SECEDO_E_INVALID_ARG, "null buffer");
    if (int rc = check_device(device_id)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Buf r;
    SECEDO_TRY(r.alloc(sizeof(ModelResult)));
    SECEDO_TRY(secedo::cluster::kmeans(d_points, n, dims, K, max_iter, d_labels, r.as<ModelResult>(), s));
    ModelResult h;
    SECEDO_TRY(hipMemcpyAsync(&h, r.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    copy_model(h, model);
    return SECEDO_OK;
}

int secedo_cluster_gmm_device(int device_id, const double *d_points, uint32_t n, uint32_t dims, uint32_t K,
                              secedo_cluster_model *model, void *stream) {
    if (n == 0) return fail(SECEDO_E_INVALID_ARG, "no points");
    if (dims < 1 || dims > 5) return fail(SECEDO_E_INVALID_ARG, "dims must be in 1..5");
    if (K < 1 || K > SECEDO_CLUSTER_MAX) return fail(SECEDO_E_INVALID_ARG, "K must be in 1..4");
    if (!d_points || !model) return fail(SECEDO_E_INVALID_ARG, "null buffer");
    if (int rc = check_device(device_id)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Buf r;
    SECEDO_TRY(r.alloc(sizeof(ModelResult)));
    SECEDO_TRY(secedo::cluster::gmm(d_points, n, dims, K, r.as<ModelResult>(), s));
    ModelResult h;
    SECEDO_TRY(hipMemcpyAsync(&h, r.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    copy_model(h, model);
    return SECEDO_OK;
}

static int divide_device(int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                         const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off, const uint32_t *d_read_ids,
                         const uint16_t *d_id_base16, const uint32_t *d_id_base32, uint32_t n_loci, uint64_t n_entries,
                         uint32_t max_read_length, const uint16_t *id_to_group, uint32_t n_cells,
                         const uint32_t *id_to_pos, uint32_t n_groups, const uint32_t *pos_to_id, uint32_t n_pos,
                         double mutation_rate, double homozygous_rate, double seq_error_rate, int normalization,
                         int termination, int clustering_type, int use_arma_kmeans, int use_expectation_maximization,
                         uint32_t min_cluster_size, uint32_t cell_proportion, const char *marker, uint16_t *clusters,
                         uint16_t *cluster_idx, secedo_cluster_level *records, uint32_t capacity,
                         uint32_t *n_records, void *stream, const char *out_dir) {
    (void)cell_proportion;  // Filter filter(seq_error_rate) (:336)
    if (int rc = check_options(clustering_type, termination, use_arma_kmeans)) return rc;
    if (normalization < SECEDO_NORM_ADD_MIN || normalization > SECEDO_NORM_SCALE_MAX_1)
        return fail(SECEDO_E_INVALID_NORMALIZATION, "unknown normalization");
    if (n_pos == 0) return fail(SECEDO_E_INVALID_ARG, "no cells: pos_to_id is empty");
    if (!id_to_group || !id_to_pos || !pos_to_id || !clusters || !cluster_idx || !n_records || (capacity && !records))
        return fail(SECEDO_E_INVALID_ARG, "null host buffer");
    if ((d_id_base16 == nullptr) == (d_id_base32 == nullptr))
        return fail(SECEDO_E_INVALID_ARG, "exactly one of id_base16 / id_base32 must be given");
    if (n_groups >= 65536u || n_cells >= 65536u) return fail(SECEDO_E_INVALID_ARG, "more than 65535 groups or cells");
    // id_to_pos and pos_to_id must describe the same sub-cluster
    uint32_t in_sub = 0, max_group = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t p = id_to_pos[g];
        if (p == kNoPos) continue;
        if (p >= n_pos || pos_to_id[p] != g)
            return fail(SECEDO_E_INVALID_ARG, "id_to_pos and pos_to_id are inconsistent at group " + std::to_string(g));
        ++in_sub;
    }
    for (uint32_t p = 0; p < n_pos; ++p) max_group = std::max(max_group, pos_to_id[p]);
    if (in_sub != n_pos) return fail(SECEDO_E_INVALID_ARG, "id_to_pos and pos_to_id are inconsistent");
    if (n_pos >= kNoPos) return fail(SECEDO_E_INVALID_ARG, "a sub-cluster holds at most 16382 cells (NO_POS)");
    for (uint32_t c = 0; c < n_cells; ++c)
        if (id_to_group[c] >= n_groups) return fail(SECEDO_E_INVALID_ARG, "id_to_group names a group past id_to_pos");
    if (out_dir && n_chr > 24)
        return fail(SECEDO_E_INVALID_ARG, "more than 24 chromosome slots: significant_positions names slots by chromosome");
    if (int rc = check_device(device_id)) return rc;
    if (out_dir && *out_dir) {
        std::error_code ec;
        std::filesystem::create_directories(out_dir, ec);
        if (ec) return fail(SECEDO_E_INVALID_ARG, std::string("cannot create ") + out_dir + ": " + ec.message());
    }

    Params P{};
    P.device_id = device_id;
    P.d_chr = d_chr_locus_off;
    P.d_pos = d_locus_pos;
    P.d_rid = d_read_ids;
    P.d_off = d_locus_entry_off;
    P.d_b16 = d_id_base16;
    P.d_b32 = d_id_base32;
    P.n_chr = n_chr;
    P.n_loci = n_loci;
    P.n_entries = n_entries;
    P.max_read_length = max_read_length;
    P.n_cells = n_cells;
    P.n_groups = n_groups;
    P.mutation_rate = mutation_rate;
    P.homozygous_rate = homozygous_rate;
    P.seq_error_rate = seq_error_rate;
    P.normalization = normalization;
    P.termination = termination;
    P.type = clustering_type;
    P.use_em = use_expectation_maximization;
    P.min_cluster_size = min_cluster_size;
    P.stream = static_cast<hipStream_t>(stream);
    P.records = records;
    P.capacity = capacity;
    P.write = out_dir != nullptr;
    P.out_dir = out_dir ? out_dir : "";
    P.id_to_group = id_to_group;

    Buf d_g, d_i2p, d_p2i, d_cl;
    SECEDO_TRY(d_g.alloc((size_t)n_cells * 2));
    SECEDO_TRY(d_i2p.alloc((size_t)n_groups * 4));
    SECEDO_TRY(d_p2i.alloc((size_t)n_pos * 4));
    SECEDO_TRY(d_cl.alloc((size_t)n_cells * 2));
    SECEDO_TRY(hipMemcpyAsync(d_g.p, id_to_group, (size_t)n_cells * 2, hipMemcpyHostToDevice, P.stream));
    SECEDO_TRY(hipMemcpyAsync(d_i2p.p, id_to_pos, (size_t)n_groups * 4, hipMemcpyHostToDevice, P.stream));
    SECEDO_TRY(hipMemcpyAsync(d_p2i.p, pos_to_id, (size_t)n_pos * 4, hipMemcpyHostToDevice, P.stream));
    SECEDO_TRY(hipMemcpyAsync(d_cl.p, clusters, (size_t)n_cells * 2, hipMemcpyHostToDevice, P.stream));
    P.d_id_to_group = d_g.as<uint16_t>();
    P.d_clusters = d_cl.as<uint16_t>();

    secedo_simmat_t *h = nullptr;
    CL_CALL(secedo_simmat_create(&h, device_id));
    P.handle = h;
    uint16_t idx = *cluster_idx;
    const int rc = level(P, d_i2p.as<uint32_t>(), d_p2i.as<uint32_t>(), n_pos, max_group, marker ? marker : "", &idx);
    secedo_simmat_destroy(h);
    *n_records = P.n_records;
    if (rc) return rc;
    SECEDO_TRY(hipMemcpyAsync(clusters, d_cl.p, (size_t)n_cells * 2, hipMemcpyDeviceToHost, P.stream));
    SECEDO_TRY(hipStreamSynchronize(P.stream));
    *cluster_idx = idx;
    if (P.n_records > capacity)
        return fail(SECEDO_E_LIMIT, "more levels (" + std::to_string(P.n_records) + ") than record capacity");
    return SECEDO_OK;
}

static int divide_host(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                       const uint64_t *locus_entry_off, const uint32_t *read_ids, const uint16_t *id_base16,
                       const uint32_t *id_base32, uint32_t max_read_length, const uint16_t *id_to_group,
                       uint32_t n_cells, const uint32_t *id_to_pos, uint32_t n_groups, const uint32_t *pos_to_id,
                       uint32_t n_pos, double mutation_rate, double homozygous_rate, double seq_error_rate,
                       int normalization, int termination, int clustering_type, int use_arma_kmeans,
                       int use_expectation_maximization, uint32_t min_cluster_size, uint32_t cell_proportion,
                       const char *marker, uint16_t *clusters, uint16_t *cluster_idx, secedo_cluster_level *records,
                       uint32_t capacity, uint32_t *n_records, const char *out_dir) {
    if (int rc = check_options(clustering_type, termination, use_arma_kmeans)) return rc;
    if (n_pos == 0) return fail(SECEDO_E_INVALID_ARG, "no cells: pos_to_id is empty");
    if (!chr_locus_off || (!locus_pos && n_chr) || !locus_entry_off)
        return fail(SECEDO_E_INVALID_ARG, "null pileup buffer");
    if ((id_base16 == nullptr) == (id_base32 == nullptr))
        return fail(SECEDO_E_INVALID_ARG, "exactly one of id_base16 / id_base32 must be given");
    if (!id_to_pos || !pos_to_id) return fail(SECEDO_E_INVALID_ARG, "null host buffer");
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t p = id_to_pos[g];
        if (p != kNoPos && (p >= n_pos || pos_to_id[p] != g))
            return fail(SECEDO_E_INVALID_ARG, "id_to_pos and pos_to_id are inconsistent at group " + std::to_string(g));
    }
    if (int rc = check_device(device_id)) return rc;
    const uint32_t L = chr_locus_off[n_chr];
    const uint64_t E = locus_entry_off[L];
    Buf chr, pos, off, rid, idb;
    SECEDO_TRY(chr.alloc((size_t)(n_chr + 1) * 4));
    SECEDO_TRY(pos.alloc((size_t)std::max<uint32_t>(L, 1) * 4));
    SECEDO_TRY(off.alloc((size_t)(L + 1) * 8));
    SECEDO_TRY(rid.alloc((size_t)std::max<uint64_t>(E, 1) * 4));
    SECEDO_TRY(idb.alloc((size_t)std::max<uint64_t>(E, 1) * (id_base16 ? 2 : 4)));
    SECEDO_TRY(hipMemcpy(chr.p, chr_locus_off, (size_t)(n_chr + 1) * 4, hipMemcpyHostToDevice));
    if (L) SECEDO_TRY(hipMemcpy(pos.p, locus_pos, (size_t)L * 4, hipMemcpyHostToDevice));
    SECEDO_TRY(hipMemcpy(off.p, locus_entry_off, (size_t)(L + 1) * 8, hipMemcpyHostToDevice));
    if (E) {
        SECEDO_TRY(hipMemcpy(rid.p, read_ids, (size_t)E * 4, hipMemcpyHostToDevice));
        if (id_base16) SECEDO_TRY(hipMemcpy(idb.p, id_base16, (size_t)E * 2, hipMemcpyHostToDevice));
        else SECEDO_TRY(hipMemcpy(idb.p, id_base32, (size_t)E * 4, hipMemcpyHostToDevice));
    }
    return divide_device(device_id, chr.as<uint32_t>(), n_chr, pos.as<uint32_t>(), off.as<uint64_t>(),
                         rid.as<uint32_t>(), id_base16 ? idb.as<uint16_t>() : nullptr,
                         id_base16 ? nullptr : idb.as<uint32_t>(), L, E, max_read_length, id_to_group, n_cells,
                         id_to_pos, n_groups, pos_to_id, n_pos, mutation_rate, homozygous_rate, seq_error_rate,
                         normalization, termination, clustering_type, use_arma_kmeans, use_expectation_maximization,
                         min_cluster_size, cell_proportion, marker, clusters, cluster_idx, records, capacity,
                         n_records, nullptr, out_dir);
}

#define DEVICE_ARGS                                                                                                  \
    device_id, d_chr_locus_off, n_chr, d_locus_pos, d_locus_entry_off, d_read_ids, d_id_base16, d_id_base32, n_loci, \
        n_entries, max_read_length, id_to_group, n_cells, id_to_pos, n_groups, pos_to_id, n_pos, mutation_rate,      \
        homozygous_rate, seq_error_rate, normalization, termination, clustering_type, use_arma_kmeans,               \
        use_expectation_maximization, min_cluster_size, cell_proportion, marker, clusters, cluster_idx, records,     \
        capacity, n_records, stream
#define HOST_ARGS                                                                                                     \
    device_id, chr_locus_off, n_chr, locus_pos, locus_entry_off, read_ids, id_base16, id_base32, max_read_length,     \
        id_to_group, n_cells, id_to_pos, n_groups, pos_to_id, n_pos, mutation_rate, homozygous_rate, seq_error_rate, \
        normalization, termination, clustering_type, use_arma_kmeans, use_expectation_maximization, min_cluster_size, \
        cell_proportion, marker, clusters, cluster_idx, records, capacity, n_records

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
                                 uint32_t capacity, uint32_t *n_records, void *stream) {
    return divide_device(DEVICE_ARGS, nullptr);
}

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
                                       uint32_t capacity, uint32_t *n_records, void *stream, const char *out_dir) {
    if (!out_dir) return fail(SECEDO_E_INVALID_ARG, "null out_dir");
    return divide_device(DEVICE_ARGS, out_dir);
}

int secedo_divide_cluster(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                          const uint64_t *locus_entry_off, const uint32_t *read_ids, const uint16_t *id_base16,
                          const uint32_t *id_base32, uint32_t max_read_length, const uint16_t *id_to_group,
                          uint32_t n_cells, const uint32_t *id_to_pos, uint32_t n_groups, const uint32_t *pos_to_id,
                          uint32_t n_pos, double mutation_rate, double homozygous_rate, double seq_error_rate,
                          int normalization, int termination, int clustering_type, int use_arma_kmeans,
                          int use_expectation_maximization, uint32_t min_cluster_size, uint32_t cell_proportion,
                          const char *marker, uint16_t *clusters, uint16_t *cluster_idx,
                          secedo_cluster_level *records, uint32_t capacity, uint32_t *n_records) {
    return divide_host(HOST_ARGS, nullptr);
}

int secedo_divide_cluster_files(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr,
                                const uint32_t *locus_pos, const uint64_t *locus_entry_off, const uint32_t *read_ids,
                                const uint16_t *id_base16, const uint32_t *id_base32, uint32_t max_read_length,
                                const uint16_t *id_to_group, uint32_t n_cells, const uint32_t *id_to_pos,
                                uint32_t n_groups, const uint32_t *pos_to_id, uint32_t n_pos, double mutation_rate,
                                double homozygous_rate, double seq_error_rate, int normalization, int termination,
                                int clustering_type, int use_arma_kmeans, int use_expectation_maximization,
                                uint32_t min_cluster_size, uint32_t cell_proportion, const char *marker,
                                uint16_t *clusters, uint16_t *cluster_idx, secedo_cluster_level *records,
                                uint32_t capacity, uint32_t *n_records, const char *out_dir) {
    if (!out_dir) return fail(SECEDO_E_INVALID_ARG, "null out_dir");
    return divide_host(HOST_ARGS, out_dir);
}

}  // extern "C"
