// fasta_source.hpp -- the reference genome as a file of one of three kinds, told apart by content as secedo_bam.h
// does: plain text, BGZF (gzip members with the BC subfield) and plain gzip. fasta_source.cpp opens and classifies the
// file and inflates on the host (zlib); fasta_device.cpp is the device route of include/secedo_variant.h: the text
// (BGZF: the compressed members) uploaded in ranges, parsed and gathered in HBM. Internal, nothing exported.
#pragma once

#include "bgzf_members.hpp"
#include "host_util.hpp"
#include "secedo_variant.h"

#include <cstdint>
#include <string>
#include <vector>

namespace secedo {
namespace fasta_host __attribute__((visibility("hidden"))) {

using namespace secedo::host;

namespace bm = secedo::bgzf_members;  // the member list of a BGZF file, its descriptors and its error words
using bm::Member;

// "<path>: BGZF block <k>: <why>", from either route
inline int bad_member(const std::string &path, uint64_t k, const std::string &why) {
    return fail(SECEDO_E_INVALID_ARG, path + ": " + bm::block_where(k) + ": " + why);
}

struct Source {
    std::string path;
    uint32_t kind = SECEDO_FASTA_KIND_TEXT;
    const uint8_t *file = nullptr;  // the mapped file
    size_t file_bytes = 0;
    std::vector<uint8_t> inflated;  // plain gzip: its text; BGZF: its text once a host function or the map needed it
    std::vector<Member> members;    // BGZF, in file order
    uint64_t members_text = 0;      // BGZF: the sum of ISIZE
    bool has_text = false;          // text() is the whole FASTA text

    Source() = default;
    Source(const Source &) = delete;
    Source &operator=(const Source &) = delete;
    ~Source();
    const uint8_t *text() const { return kind == SECEDO_FASTA_KIND_TEXT ? file : inflated.data(); }
    size_t text_bytes() const { return kind == SECEDO_FASTA_KIND_TEXT ? file_bytes : inflated.size(); }
};

// What the last FASTA-reading call of this thread did (secedo_variant_fasta_stats).
secedo_variant_fasta_info &info();

// The route of this call: secedo_variant_set_fasta_route, else SECEDO_FASTA (unset or empty: host). An unknown value of
// the variable is SECEDO_E_INVALID_ARG.
int fasta_route(bool *device);
void set_route(int route);
int get_route();

// Text bytes per range of the device route: SECEDO_FASTA_BATCH_BYTES, else 256 MiB; at least 64.
uint64_t batch_bytes();

// Maps and classifies the file; plain gzip is inflated here (every member's CRC32 and ISIZE checked by zlib), the
// members of a BGZF file are listed by following BSIZE. Resets info().
int open_source(const char *path, Source *src);

// BGZF: every member inflated with zlib into src->inflated, ISIZE and CRC32 checked; the lowest bad member k is
// "<path>: BGZF block <k>: inflate failed or ISIZE mismatch" or "... CRC32 mismatch".
int inflate_bgzf_host(Source *src);

// check_is_diploid on a text
bool first_word_has_maternal(const uint8_t *p, size_t n);
// the same for a BGZF file whose text is not on the host: leading members are inflated with zlib until the first word
// is whole
int bgzf_is_diploid(const Source &src, bool *diploid);

// ---- fasta_device.cpp

// The device route: locus_ref in HBM and chr_locus_end on the host, as the host route computes them. src has no map.
int device_genotypes(const Source &src, bool diploid, const uint32_t *d_chr_locus_off, const uint32_t *chr_locus_off,
                     uint32_t n_chr, const uint32_t *d_locus_pos, uint32_t n_loci, uint8_t *d_locus_ref,
                     uint32_t *chr_locus_end, hipStream_t s);

// BGZF with a map file: the members inflated on the GPU, the text downloaded into src->inflated for the host route.
int download_bgzf_text(Source *src, hipStream_t s);

}  // namespace fasta_host
}  // namespace secedo
