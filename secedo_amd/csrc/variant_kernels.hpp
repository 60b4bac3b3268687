// variant_kernels.hpp -- launch wrappers of variant_kernels.hip (gfx950): the per-locus genotype calls of the
// reference's variant_calling() (variant_calling.cpp:366-455). See variant_kernels.hip for the layout and the
// exactness argument.
#pragma once

#include "secedo_variant.h"

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace secedo {
namespace variant {

constexpr uint32_t kNoGenotype = SECEDO_NO_GENOTYPE;
constexpr uint32_t kThresholds = 65536;  // likely_homozygous threshold per u16 coverage
constexpr uint32_t kLociPerWave = 32;    // loci one wave walks in order (its records are contiguous)
constexpr uint32_t kLdsGroups = 16384;   // groups whose counted-entry counters fit one workgroup's LDS (64 KiB)

// Host-computed constants: the logarithms with glibc, so that the device's libm does not enter the decisions.
struct Logs {
    double log_theta;       // log(theta / 3)
    double log_one_minus;   // log(1 - theta)
    double log_half_minus;  // log(0.5 - theta / 3)
    double log_prior;       // log(hetero_prior)
};

struct CallsIn {
    const uint32_t *chr_locus_off;  // device [n_chr + 1]
    const uint32_t *chr_locus_end;  // device [n_chr]
    uint32_t n_chr;
    const uint64_t *locus_entry_off;
    const uint16_t *id_base16;
    const uint32_t *id_base32;
    uint32_t n_loci;
    const uint16_t *clusters;  // per group id
    uint32_t n_groups;
    const uint8_t *locus_ref;
    const double *threshold;  // [kThresholds], host-computed
    Logs logs;
};

// Workspace sizes for n_loci loci.
uint32_t num_ranges(uint32_t n_loci);

// Pass 1: per-group counters (d_mismatch, d_loci, zeroed here), records per wave range (d_range_count
// [ranges + 1]), a flag per locus with records, *d_error = 1 on a group id >= n_groups. Then the exclusive scan
// into d_range_off[ranges + 1] (d_range_off[ranges] = the total). scan_tmp: hipcub workspace. lds_counters:
// privatise the counted entries per workgroup in LDS (taken when n_groups <= kLdsGroups); max_blocks bounds the
// grid (the waves loop over the ranges).
hipError_t count_calls(const CallsIn &in, uint32_t *d_mismatch, uint32_t *d_loci, uint32_t *d_range_count,
                       uint32_t *d_range_off, uint8_t *d_locus_flag, uint32_t *d_error, void *scan_tmp,
                       size_t scan_bytes, bool lds_counters, uint32_t max_blocks, hipStream_t stream);
size_t scan_workspace(uint32_t n_loci);

// Pass 2: the records of the flagged loci at their scanned offsets.
hipError_t write_calls(const CallsIn &in, const uint32_t *d_range_off, const uint8_t *d_locus_flag,
                       secedo_variant_record *d_records, hipStream_t stream);

// likely_homozygous / most_likely_genotype of n count vectors (u16 x 4 each), one thread per vector.
hipError_t genotypes(const uint16_t *d_counts, uint32_t n, int likely_homozygous_total, const double *d_threshold,
                     Logs logs, uint8_t *d_homozygous, uint8_t *d_genotype, hipStream_t stream);

// ---- The VCF text, formatted in HBM (the bgzf output route) -----------------------------------------------------
//
// The files are cluster_0 .. cluster_<num_clusters - 1>, then common: num_clusters + 1 of them. Their texts stand
// back to back in that order in one buffer, each file's preamble (made by the host; common has none) first.
struct FormatIn {
    const secedo_variant_record *records;  // device, in write order
    uint32_t n_records;
    const uint32_t *chr_locus_off;  // device [n_chr + 1]
    uint32_t n_chr;
    const uint32_t *locus_pos;  // device
    const uint8_t *locus_ref;   // device
    uint32_t num_clusters;
    const uint8_t *preamble;       // device: the preambles back to back
    const uint64_t *preamble_off;  // device [num_clusters + 2]: file f's preamble is bytes [off[f], off[f + 1])
};

constexpr uint32_t kMaxLineBytes = 82;  // "22\t4294967295\t.\tA\tCG" + the fixed columns + "1/1\t" + 4 x "65535 " + "\n"

// Bytes of workspace format_measure and format_write share for n_records records.
size_t format_workspace(uint32_t n_records);

// Step 1: each record's destination file and text length, the stable partition by file (records keep their write
// order within a file), the u64 scan of the lengths. d_file_off[num_clusters + 2] receives each file's first byte in
// the buffer, the last entry the total.
hipError_t format_measure(const FormatIn &in, void *workspace, size_t workspace_bytes, uint64_t *d_file_off,
                          hipStream_t stream);

// Step 2: the lines and the preambles into d_text (d_file_off's total bytes), from the workspace step 1 left.
hipError_t format_write(const FormatIn &in, const void *workspace, size_t workspace_bytes, const uint64_t *d_file_off,
                        uint8_t *d_text, hipStream_t stream);

}  // namespace variant
}  // namespace secedo
