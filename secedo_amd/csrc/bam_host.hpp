// bam_host.hpp -- what the two host files of include/secedo_bam.h share: bam_input.cpp reads the BAM and SAM files
// into one ChrInput per requested chromosome, bam_pileup.cpp turns those into the pileup. Internal, nothing exported.
#pragma once

#include "host_util.hpp"
#include "secedo_bam.h"

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace secedo {
namespace bam_host __attribute__((visibility("hidden"))) {

using namespace secedo::host;

inline uint32_t rd32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint16_t rd16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }

// Layout of a BAM record body c (after block_size): 32 fixed bytes, read name, CIGAR, packed SEQ, QUAL, aux fields.
inline uint32_t rec_l_name(const uint8_t *c) { return c[8]; }
inline uint32_t rec_n_cigar(const uint8_t *c) { return rd16(c + 12); }
inline uint32_t rec_l_seq(const uint8_t *c) { return rd32(c + 16); }
inline uint64_t rec_aux_off(const uint8_t *c) {
    return 32 + uint64_t(rec_l_name(c)) + 4ull * rec_n_cigar(c) + (uint64_t(rec_l_seq(c)) + 1) / 2 + rec_l_seq(c);
}

// the records of one chromosome, file after file in input order
struct ChrInput {
    uint32_t chromosome;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> file_base;          // [n_files] start of each file's run in bytes
    std::vector<std::vector<uint64_t>> roff;  // per file: record offsets (relative to its run)
    std::vector<std::vector<int32_t>> rpos;
    std::vector<std::vector<uint64_t>> ridx;  // record index in the file (messages)
};

// what one call read
struct Inputs {
    std::vector<std::string> paths;  // [n_files] (messages)
    std::vector<uint64_t> line0;     // [n_files] SAM: the line of record 0 (1-based); BAM: 0
    std::vector<ChrInput> chrs;      // [n_chr]
};

// Where record idx of file f is, for messages:
//   SAM (line0 != 0):        "file f (path), line line0 + idx"
//   BAM while loading:       "path: record idx"
//   BAM in the device stage: "file f, record idx"
// Known wart: the two BAM wordings name the same record differently. Both are kept as callers know them.
enum class Stage { kLoad, kDevice };
std::string record_where(const std::string &path, size_t f, uint64_t line0, uint64_t idx, Stage stage = Stage::kLoad);

// Reads the files (BAM or SAM, told apart by their first bytes) and keeps the records of the requested chromosomes.
// t: stage times are added to it; may be null.
int load_inputs(const std::vector<std::string> &files, const uint32_t *chromosome_ids, uint32_t n_chr,
                uint32_t threads, Inputs *in, secedo_bam_times *t);

// Frees the device memory of the last secedo_bgzf_inflate result of this thread (secedo_bam_release calls it).
void release_inflated();

}  // namespace bam_host
}  // namespace secedo
