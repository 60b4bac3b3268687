// vcf_output.hpp -- the files a variant calling leaves: the VCF text of the reference's variant_calling()
// (variant_calling.cpp:226-321, :395-442), `variant` and `scores`, by two routes. PLAIN builds the text on the host
// from downloaded records and writes cluster_<i>.vcf / common.vcf. BGZF formats the same text in HBM from the records
// where write_calls left them (variant_kernels.hip), deflates it there (bgzf_deflate_kernels.hip) and writes
// cluster_<i>.vcf.gz / common.vcf.gz; only compressed bytes come to the host. Under SECEDO_VCF_INDEX_TBI the BGZF route
// also writes <file>.tbi beside each (tabix_host.hpp). Internal to libsecedo_variant.so.
#pragma once

#include "bam_index_build.hpp"  // Member: a BGZF member for virtual offsets
#include "secedo_variant.h"

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <filesystem>
#include <string>
#include <vector>

namespace secedo {
namespace bgzf { struct EncoderCounts; }  // bgzf_encoder.hpp
namespace vcf {

// The output kind of this call: secedo_variant_set_vcf_output, else SECEDO_VCF (unset or empty: plain). An unknown
// value of the variable is SECEDO_E_INVALID_ARG.
int output_kind(int *kind);
void set_output(int kind);
int get_output();

// What the last file-writing call of this thread did (secedo_variant_vcf_stats).
secedo_variant_vcf_info &info();

// The texts of the PLAIN route: vcfs[i] = cluster_<i>.vcf with `preambles[i]` first, *common = common.vcf.
void build_texts(const std::vector<std::string> &preambles, const secedo_variant_record *records, size_t n_records,
                 const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos, const uint8_t *locus_ref,
                 std::vector<std::string> *vcfs, std::string *common);

// write_vcf_preamble of every cluster file, made now (##fileDate)
std::vector<std::string> preambles(const std::string &reference, uint32_t num_clusters);

// PLAIN: everything under out_dir. Resets info().
int write_outputs(const std::filesystem::path &out_dir, const std::string &reference, uint32_t num_clusters,
                  const std::vector<secedo_variant_record> &records, const uint32_t *chr_locus_off, uint32_t n_chr,
                  const uint32_t *locus_pos, const uint8_t *locus_ref, const std::vector<uint32_t> &mismatch,
                  const std::vector<uint32_t> &loci);

// The files' texts back to back in HBM, as the BGZF route compresses them.
struct DeviceText {
    unsigned char *alloc = nullptr;    // hipMalloc'ed; the text starts kDeflateInSlack bytes in
    std::vector<uint64_t> file_off;    // [files + 1], from the text's start
    ~DeviceText();
    const uint8_t *text() const;
};

// The formatter alone on records and tables resident in HBM. Synchronises s.
int format_device(const std::vector<std::string> &preambles, const secedo_variant_record *d_records,
                  uint32_t n_records, const uint32_t *d_chr_locus_off, uint32_t n_chr, const uint32_t *d_locus_pos,
                  const uint8_t *d_locus_ref, DeviceText *out, hipStream_t s);

// The encoder alone: every file [file_off[f], file_off[f + 1]) of d_text (kDeflateInSlack readable bytes before and
// after the whole) cut into members of at most 0xFF00 bytes, deflated, and closed with the EOF member. *out receives
// the BGZF files back to back, out_off[files + 1] their bounds (the loop around the kernels is bgzf_encoder.hpp's).
// Adds the encoder's counts to info(), or gives them in *counts (the index bodies are not VCF files). Synchronises s.
// *table (may be null) receives what was laid out: the members of file f are m[first[f], first[f + 1]), the EOF
// member last, each with its byte in the file and the text bytes of the file it holds.
struct MemberTable {
    std::vector<bamindexbuild::Member> m;
    std::vector<size_t> first;  // [files + 1]
};
int deflate_device(const uint8_t *d_text, const std::vector<uint64_t> &file_off, std::vector<uint8_t> *out,
                   std::vector<uint64_t> *out_off, hipStream_t s, MemberTable *table = nullptr,
                   bgzf::EncoderCounts *counts = nullptr);

// BGZF: everything under out_dir, the records and tables in HBM. Resets info(). Synchronises s.
int write_outputs_bgzf(const std::filesystem::path &out_dir, const std::string &reference, uint32_t num_clusters,
                       const secedo_variant_record *d_records, uint32_t n_records, const uint32_t *d_chr_locus_off,
                       uint32_t n_chr, const uint32_t *d_locus_pos, const uint8_t *d_locus_ref,
                       const std::vector<uint32_t> &mismatch, const std::vector<uint32_t> &loci, hipStream_t s);

}  // namespace vcf
}  // namespace secedo
