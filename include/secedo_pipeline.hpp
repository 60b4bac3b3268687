// secedo_pipeline.hpp -- header-only C++ host side of the two consumers next to the similarity matrix,
// with the reference's own signatures on top of the C-ABI (secedo_em.h, secedo_spectral.h). Templates
// over the caller's types, like secedo_simmat.hpp, so that this repository contains none of the
// reference's headers.
//
//   void expectation_maximization(pos_data, id_to_pos, num_threads, theta, &prob_cluster_b)
//        reference: expectation_maximization.hpp:26-30 (caller spectral_clustering.cpp:375-377)
//   void smallest_eigenpairs(similarity, n_values, n_vectors, &eigenvalues, &eigenvectors)
//        replaces laplacian() + arma::eig_sym in spectral_clustering() (spectral_clustering.cpp:127-138);
//        eigenvectors column-major n x n_vectors (arma::mat layout)
//   uint32_t spectral_clustering(similarity, clustering, termination, out_dir, marker, use_arma_kmeans, &cluster)
//        reference: spectral_clustering.cpp:117-299; clustering and termination as the strings the reference
//        parses (parse_clustering_type / parse_termination), so that no reference header is needed
//   void divide_cluster(pds, max_read_length, id_to_group, id_to_pos, pos_to_id, mutation_rate, homozygous_rate,
//                       seq_error_rate, num_threads, out_dir, normalization, termination, clustering_type,
//                       use_arma_kmeans, use_expectation_maximization, min_cluster_size, cell_proportion, marker,
//                       &clusters, &cluster_idx)
//        reference: spectral_clustering.cpp:311-434
//   void variant_calling(pos_data, clusters, reference_genome, map_file, hetero_prior, theta, out_dir)
//        reference: variant_calling.cpp:323-461; writes the same files (needs libsecedo_variant.so,
//        include/secedo_variant.h, at link time)
// divide_cluster and spectral_clustering need libsecedo_cluster.so (include/secedo_cluster.h) at link time. num_threads and out_dir are
// accepted and unused: the GPU path needs no thread count and writes no files (the optional `levels` output
// carries what the reference logs and writes per level).
//
// A failure of the library throws std::runtime_error with the library's message; the reference has no
// error path at these places (it asserts, or reads out of bounds).
#pragma once

#include "secedo_cluster.h"
#include "secedo_em.h"
#include "secedo_simmat.h"
#include "secedo_spectral.h"
#include "secedo_variant.h"

#include <cstdint>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <vector>

namespace secedo_amd {

// vector<vector<PosData>> -> the structure-of-arrays pileup of secedo_simmat.h
struct FlatPileupHost {
    std::vector<uint32_t> chr_locus_off{0}, locus_pos, read_ids;
    std::vector<uint64_t> locus_entry_off{0};
    std::vector<uint16_t> id_base;
    uint32_t n_loci() const { return static_cast<uint32_t>(locus_pos.size()); }
};

template <class PosDataT>
FlatPileupHost flatten(const std::vector<std::vector<PosDataT>> &pos_data) {
    FlatPileupHost flat;
    uint64_t n_loci = 0, n_entries = 0;
    for (const auto &chromosome : pos_data) {
        n_loci += chromosome.size();
        for (const PosDataT &pd : chromosome) n_entries += pd.read_ids.size();
    }
    flat.locus_pos.reserve(n_loci);
    flat.locus_entry_off.reserve(n_loci + 1);
    flat.read_ids.reserve(n_entries);
    flat.id_base.reserve(n_entries);
    for (const auto &chromosome : pos_data) {
        for (const PosDataT &pd : chromosome) {
            flat.locus_pos.push_back(pd.position);
            flat.read_ids.insert(flat.read_ids.end(), pd.read_ids.begin(), pd.read_ids.end());
            flat.id_base.insert(flat.id_base.end(), pd.group_ids_bases.begin(), pd.group_ids_bases.end());
            flat.locus_entry_off.push_back(flat.read_ids.size());
        }
        flat.chr_locus_off.push_back(static_cast<uint32_t>(flat.locus_pos.size()));
    }
    return flat;
}

template <class PosDataT>
void expectation_maximization(const std::vector<std::vector<PosDataT>> &pos_data,
                              const std::vector<uint32_t> &id_to_pos, uint32_t /*num_threads*/, double theta,
                              std::vector<double> *prob_cluster_b) {
    const FlatPileupHost flat = flatten(pos_data);
    const int rc = secedo_em_refine(0, flat.locus_entry_off.data(), flat.n_loci(), flat.id_base.data(), nullptr,
                                    id_to_pos.data(), static_cast<uint32_t>(id_to_pos.size()), theta,
                                    prob_cluster_b->data(), static_cast<uint32_t>(prob_cluster_b->size()), 0,
                                    nullptr);
    if (rc != SECEDO_OK) throw std::runtime_error(std::string("secedo_em: ") + secedo_simmat_last_error());
}

// MatdT: rows(), and contiguous row-major storage reachable through `data()` (the reference's
// Mat<double>) -- the matrix is symmetric, so row-major and column-major coincide.
// The iteration stops at residuals <= 1e-9 or after its cycle limit; pairs that did not get there are not
// handed out silently: without `info_out` an unconverged solve throws, with it the caller decides
// (info_out->converged, max_residual_vectors / _values).
template <class MatdT>
void smallest_eigenpairs(const MatdT &similarity, uint32_t n_values, uint32_t n_vectors,
                         std::vector<double> *eigenvalues, std::vector<double> *eigenvectors,
                         secedo_spectral_info *info_out = nullptr) {
    const uint32_t n = similarity.rows();
    n_values = n_values < n ? n_values : n;
    n_vectors = n_vectors < n_values ? n_vectors : n_values;
    eigenvalues->assign(n_values, 0.0);
    eigenvectors->assign(static_cast<size_t>(n) * n_vectors, 0.0);
    secedo_spectral_info info;
    const int rc = secedo_spectral_eigs(0, similarity.data(), n, n_values, n_vectors, 0.0, 0, eigenvalues->data(),
                                        eigenvectors->data(), &info);
    if (rc != SECEDO_OK) throw std::runtime_error(std::string("secedo_spectral: ") + secedo_simmat_last_error());
    if (info_out) *info_out = info;
    else if (!info.converged)
        throw std::runtime_error("secedo_spectral: the eigensolver did not converge (residual "
                                 + std::to_string(info.max_residual_vectors) + " after "
                                 + std::to_string(info.cycles) + " cycles)");
}

// MatdT as for smallest_eigenpairs. Returns the number of clusters (1 = stop), cluster[n] the labels.
// An unknown clustering type throws std::invalid_argument, as parse_clustering_type does.
template <class MatdT>
uint32_t spectral_clustering(const MatdT &similarity, const std::string &clustering, const std::string &termination,
                             const std::string & /*out_dir*/, const std::string & /*marker*/, bool use_arma_kmeans,
                             std::vector<double> *cluster, secedo_cluster_decision *decision = nullptr) {
    const int type = secedo_cluster_type_from_string(clustering.c_str());
    if (type < 0) throw std::invalid_argument(clustering);
    const uint32_t n = similarity.rows();
    cluster->assign(n, 0.0);
    uint32_t num_clusters = 0;
    const int rc = secedo_spectral_clustering(0, similarity.data(), n, type,
                                              secedo_termination_from_string(termination.c_str()), use_arma_kmeans,
                                              cluster->data(), &num_clusters, decision, nullptr);
    if (rc != SECEDO_OK) throw std::runtime_error(std::string("secedo_cluster: ") + secedo_cluster_last_error());
    return num_clusters;
}

// PosDataT as for flatten (group ids in group_ids_bases). clusters[id] and *cluster_idx in/out as in the reference.
template <class PosDataT>
void divide_cluster(const std::vector<std::vector<PosDataT>> &pds, uint32_t max_read_length,
                    const std::vector<uint16_t> &id_to_group, const std::vector<uint32_t> &id_to_pos,
                    const std::vector<uint32_t> &pos_to_id, double mutation_rate, double homozygous_rate,
                    double seq_error_rate, const uint32_t /*num_threads*/, const std::string & /*out_dir*/,
                    const std::string &normalization, const std::string &termination_str,
                    const std::string &clustering_type_str, bool use_arma_kmeans, bool use_expectation_maximization,
                    uint32_t min_cluster_size, uint8_t cell_proportion, const std::string marker,
                    std::vector<uint16_t> *clusters, uint16_t *cluster_idx,
                    std::vector<secedo_cluster_level> *levels = nullptr) {
    const int norm = secedo_simmat_normalization_from_string(normalization.c_str());
    if (norm < 0) throw std::logic_error("Invalid normalization: " + normalization);
    const int type = secedo_cluster_type_from_string(clustering_type_str.c_str());
    if (type < 0) throw std::invalid_argument(clustering_type_str);
    const FlatPileupHost flat = flatten(pds);
    std::vector<secedo_cluster_level> records(4 * pos_to_id.size() + 16);
    uint32_t n_records = 0;
    const int rc = secedo_divide_cluster(
            0, flat.chr_locus_off.data(), static_cast<uint32_t>(flat.chr_locus_off.size() - 1), flat.locus_pos.data(),
            flat.locus_entry_off.data(), flat.read_ids.data(), flat.id_base.data(), nullptr, max_read_length,
            id_to_group.data(), static_cast<uint32_t>(id_to_group.size()), id_to_pos.data(),
            static_cast<uint32_t>(id_to_pos.size()), pos_to_id.data(), static_cast<uint32_t>(pos_to_id.size()),
            mutation_rate, homozygous_rate, seq_error_rate, norm, secedo_termination_from_string(termination_str.c_str()),
            type, use_arma_kmeans, use_expectation_maximization, min_cluster_size, cell_proportion, marker.c_str(),
            clusters->data(), cluster_idx, records.data(), static_cast<uint32_t>(records.size()), &n_records);
    if (rc != SECEDO_OK) throw std::runtime_error(std::string("secedo_cluster: ") + secedo_cluster_last_error());
    if (levels) levels->assign(records.begin(), records.begin() + n_records);
}

// variant_calling (variant_calling.cpp:323-461): cluster_<i>.vcf, common.vcf, variant and scores under out_dir.
// Nothing is written for empty clusters, as in the reference.
template <class PosDataT>
void variant_calling(const std::vector<std::vector<PosDataT>> &pos_data, const std::vector<uint16_t> &clusters,
                     const std::string &reference_genome, const std::string &map_file, double hetero_prior,
                     double theta, const std::filesystem::path &out_dir) {
    if (clusters.empty()) return;
    const FlatPileupHost flat = flatten(pos_data);
    const int rc = secedo_variant_calling(
            0, flat.chr_locus_off.data(), static_cast<uint32_t>(flat.chr_locus_off.size() - 1), flat.locus_pos.data(),
            flat.locus_entry_off.data(), flat.id_base.data(), nullptr, clusters.data(),
            static_cast<uint32_t>(clusters.size()), reference_genome.c_str(), map_file.c_str(), hetero_prior, theta,
            out_dir.c_str(), nullptr);
    if (rc != SECEDO_OK) throw std::runtime_error(secedo_variant_last_error());
}

}  // namespace secedo_amd
