// tabix_host.hpp -- the host side of the .tbi indexes (include/secedo_variant.h): the setting, the statistics, and the
// two steps both routes share: the line pass over texts in HBM feeding one tabix_build.hpp builder per file, and the
// compression of the index bodies by the encoder of the .vcf.gz files. tabix_api.cpp holds them and the stand-alone
// route; vcf_output.cpp's BGZF writer calls them on the text it has. Internal to libsecedo_variant.so.
#pragma once

#include "bam_index_build.hpp"
#include "secedo_variant.h"

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

namespace secedo {
namespace tabix_host {

// The index kind of this call: secedo_variant_set_vcf_index, else SECEDO_VCF_INDEX (unset or empty: none). An unknown
// value of the variable is SECEDO_E_INVALID_ARG.
int index_kind(int *kind);
void set_index(int kind);
int get_index();

// What the last index-writing call of this thread did (secedo_variant_tabix_stats).
secedo_variant_tabix_info &info();

// One compressed file as its index needs it: what to call it in a message, its BGZF members (the EOF member included)
// and its size.
struct IndexedFile {
    std::string label;
    std::vector<bamindexbuild::Member> members;
    uint64_t file_bytes = 0;
};

// The uncompressed .tbi of every file: file f is text bytes [file_off[f], file_off[f + 1]) of d_text (kTextSlack readable
// bytes before and after the whole). On an error of file k, *n_good = k and raw[0, k) are whole; else *n_good = files.
// Adds to info(). Synchronises s.
int build_raw(const uint8_t *d_text, const std::vector<uint64_t> &file_off, const std::vector<IndexedFile> &files,
              std::vector<std::vector<uint8_t>> *raw, size_t *n_good, hipStream_t s);

// raw[0, n) compressed as BGZF files and written to paths[k], each through a temporary name. Adds to info(), not to
// vcf::info(). Synchronises s.
int compress_and_write(const std::vector<std::vector<uint8_t>> &raw, size_t n, const std::vector<std::string> &paths,
                       hipStream_t s);

}  // namespace tabix_host
}  // namespace secedo
