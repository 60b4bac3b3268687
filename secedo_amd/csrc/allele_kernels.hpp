// allele_kernels.hpp -- launch wrappers of allele_kernels.hip (gfx950): the per-cell allele counts at the called
// variants (include/secedo_variant.h, "Per-cell allele counts") and their Matrix Market / VCF text. The mask rule
// itself stands here once, for the device and for the host-only secedo_variant_allele_masks. See allele_kernels.hip
// for the layout.
#pragma once

#include "secedo_variant.h"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SECEDO_ALLELE_HD __host__ __device__ inline
#else
#define SECEDO_ALLELE_HD inline
#endif

namespace secedo {
namespace allele {

constexpr uint32_t kWaveEntries = 128;   // a locus of at most this many entries is sorted in one wave's registers
constexpr uint32_t kMaxMtxLine = 33;     // "4294967295\t4294967295\t4294967295\n"
constexpr uint32_t kMaxVcfLine = 96;     // "22\t4294967295\t.\tA,C\tA,C,G,T\t.\tPASS\tAD=..;DP=..;OTH=..\n" with 10-digit numbers
constexpr uint32_t kFiles = 4;           // AD, DP, OTH, the base VCF: the order of the texts in a range's buffer

// the bits of {code & 7, code >> 3} that are bases: an N (5) or anything past T adds nothing
SECEDO_ALLELE_HD uint32_t genotype_bits(uint32_t code) {
    const uint32_t a = code & 7, b = code >> 3;
    return (a < 4 ? 1u << a : 0u) | (b < 4 ? 1u << b : 0u);
}

// ref_mask | alt_mask << 4 of a locus with reference genotype `ref` whose records' genotypes OR to the bits g
SECEDO_ALLELE_HD uint32_t site_masks(uint32_t ref, uint32_t g) {
    const uint32_t rf = genotype_bits(ref);
    uint32_t alt = g & ~rf, rm = rf;
    if (alt == 0) {  // the calls only lose a reference allele
        alt = g;
        rm = rf & ~g;
    }
    return rm | alt << 4;
}

// per site, what the count pass leaves
struct SiteCounts {
    uint32_t pairs, nnz_ad, nnz_dp, nnz_oth;  // distinct groups; those with ad > 0, ad + rd > 0, oth > 0
    uint32_t ad, rd, oth, reserved;           // the site's totals
};

// sums over the sites, u64 each
struct Totals {
    unsigned long long entries, nnz_ad, nnz_dp, nnz_oth, deep_sites, error;  // error: a group id >= n_cells was seen
};

struct Pileup {
    const uint64_t *locus_entry_off;
    const uint16_t *id_base16;
    const uint32_t *id_base32;
    uint32_t n_cells;
};

// Site pass, step 1: per record, flag = 1 at the first record of a selected locus and mask = its ref_mask | alt_mask << 4;
// d_flag[n_records + 1] (the last 0) is then scanned into d_index[n_records + 1] (d_index[n_records] = the sites).
hipError_t site_flags(const secedo_variant_record *d_records, uint32_t n_records, const uint8_t *d_locus_ref,
                      int selection, uint32_t *d_flag, uint8_t *d_mask, uint32_t *d_index, void *scan_tmp,
                      size_t scan_bytes, hipStream_t stream);
size_t site_scan_workspace(uint32_t n_records);

// Site pass, step 2: the sites compacted (d_site_locus, d_site_mask [n_sites]) and each one's entries where it is deep
// (d_deep_len[n_sites + 1] u64, 0 for a site of at most kWaveEntries entries), scanned into d_deep_off[n_sites + 1].
hipError_t site_compact(const secedo_variant_record *d_records, uint32_t n_records, const uint32_t *d_flag,
                        const uint8_t *d_mask, const uint32_t *d_index, const Pileup &p, uint32_t n_sites,
                        uint32_t *d_site_locus, uint8_t *d_site_mask, uint64_t *d_deep_len, uint64_t *d_deep_off,
                        void *scan_tmp, size_t scan_bytes, hipStream_t stream);
size_t pair_scan_workspace(uint32_t n_sites);

// The deep sites' entries as keys site << 32 | group << 2 | class at d_deep_off, sorted (hipcub radix sort, n_deep < 2^31)
// into d_keys_sorted: a site's keys stay in its own span.
size_t deep_sort_workspace(uint64_t n_deep);
hipError_t deep_sort(const Pileup &p, const uint32_t *d_site_locus, const uint8_t *d_site_mask, uint32_t n_sites,
                     const uint64_t *d_deep_off, uint64_t n_deep, uint64_t *d_keys, uint64_t *d_keys_sorted,
                     void *sort_tmp, size_t sort_bytes, hipStream_t stream);

struct Sites {
    const uint32_t *locus;
    const uint8_t *mask;
    uint32_t n;
    const uint64_t *deep_off;     // [n + 1]
    const uint64_t *keys_sorted;  // the deep sites' sorted keys
};

// Count pass: d_counts[n_sites], *d_totals (zeroed here), d_pair_len[n_sites + 1] u64 scanned into d_pair_off[n_sites + 1].
hipError_t count_pairs(const Pileup &p, const Sites &s, SiteCounts *d_counts, Totals *d_totals, uint64_t *d_pair_len,
                       uint64_t *d_pair_off, void *scan_tmp, size_t scan_bytes, hipStream_t stream);

// Write pass: d_pairs[d_pair_off[n_sites]] (zeroed here), site then group ascending.
hipError_t write_pairs(const Pileup &p, const Sites &s, const uint64_t *d_pair_off, uint64_t n_pairs,
                       secedo_allele_pair *d_pairs, hipStream_t stream);

// ---- The text of sites [s0, s1), pairs [p0, p1) ------------------------------------------------------------------
//
// The four texts stand back to back: AD, DP, OTH, base VCF, each with its header bytes first (hdr_len; 0 but in the
// first range). One item per header and per line: file f < 3 has items f * (np + 1) .. with np = p1 - p0, the VCF's
// follow, one per site, and a last item of length 0 closes the scan.
struct FormatIn {
    const secedo_allele_pair *pairs;  // device, all pairs
    const SiteCounts *counts;         // device, all sites
    const uint32_t *site_locus;
    const uint8_t *site_mask;
    const uint32_t *chr_locus_off;  // device [n_chr + 1]
    uint32_t n_chr;
    const uint32_t *locus_pos;  // device
    uint32_t s0, s1;
    uint64_t p0, p1;
    uint32_t hdr_len[kFiles];
};
inline uint64_t format_items(const FormatIn &in) { return 3 * (in.p1 - in.p0 + 1) + (in.s1 - in.s0) + 2; }
size_t format_scan_workspace(uint64_t items);
// d_len / d_off [items] u64; d_file_off[kFiles + 1]: each text's first byte, the last entry the total
hipError_t format_measure(const FormatIn &in, uint64_t *d_len, uint64_t *d_off, uint64_t *d_file_off, void *scan_tmp,
                          size_t scan_bytes, hipStream_t stream);
// d_hdr: the four headers back to back (hdr_len each)
hipError_t format_write(const FormatIn &in, const uint64_t *d_off, const uint8_t *d_hdr, uint8_t *d_text,
                        hipStream_t stream);

}  // namespace allele
}  // namespace secedo
