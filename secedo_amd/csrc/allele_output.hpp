// allele_output.hpp -- the host side of the per-cell allele counts (include/secedo_variant.h): the setting, the cell
// names, the run of allele_kernels.hip's passes and the files under <out_dir>/allele_counts/. Internal to
// libsecedo_variant.so; the C entry points of the feature are defined in allele_output.cpp.
#pragma once

#include "allele_kernels.hpp"

#include <filesystem>

namespace secedo {
namespace allele {

// The selection of this call: secedo_variant_set_allele_counts, else SECEDO_ALLELE_COUNTS (unset or empty: none). An
// unknown value of the variable is SECEDO_E_INVALID_ARG.
int selection_kind(int *selection);

// What the last call of this thread did (secedo_variant_allele_stats).
secedo_variant_allele_info &info();

// SECEDO_E_INVALID_ARG when cell names are set and are not n_cells of them.
int check_cell_names(uint32_t n_cells);

// Everything under out_dir/allele_counts from the records where write_calls left them and the tables in HBM; bgzf as
// the VCF output of the call. Sets info(). Synchronises s.
int write_outputs(const std::filesystem::path &out_dir, int selection, bool bgzf, const Pileup &pileup,
                  const secedo_variant_record *d_records, uint32_t n_records, const uint8_t *d_locus_ref,
                  const uint32_t *d_chr_locus_off, uint32_t n_chr, const uint32_t *d_locus_pos, hipStream_t s);

}  // namespace allele
}  // namespace secedo
