// sam_kernels.hpp -- launch wrappers of sam_kernels.hip (gfx950): SAM text lines -> the BAM records bam_kernels.hip
// reads. See sam_kernels.hip for the conversion rules.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace bam {

// error codes of the SAM passes, reported for the lowest line that has one (u64 min of line << 8 | code)
enum SamErr : uint32_t {
    kSamOk = 0,
    kSamFields = 1,     // fewer than 11 tab-separated mandatory fields, or an empty one
    kSamName = 2,       // QNAME longer than 254 characters
    kSamFlag = 3,       // FLAG not a decimal integer in [0, 65535]
    kSamRname = 4,      // RNAME not '*' and not an @SQ name
    kSamPos = 5,        // POS not a decimal integer in [0, 2^31 - 1]
    kSamMapq = 6,       // MAPQ not a decimal integer in [0, 255]
    kSamCigar = 7,      // CIGAR not '*' and not ops MIDNSHP=X with lengths in [1, 2^28)
    kSamRnext = 8,      // RNEXT not '*', '=' or an @SQ name
    kSamPnext = 9,      // PNEXT not a decimal integer in [0, 2^31 - 1]
    kSamTlen = 10,      // TLEN not a decimal integer in [-(2^31 - 1), 2^31 - 1]
    kSamQual = 11,      // QUAL not '*', of another length than SEQ, or a character outside '!'..'~'
    kSamCigarSeq = 12,  // CIGAR query length (M/I/S/=/X) differs from the SEQ length
    kSamAux = 13,       // a malformed optional field
    kSamHeader = 14,    // an '@' line after the first alignment line
    kSamEmpty = 15,     // an empty line that does not end the file
    kSamManyOps = 16,   // more than 65535 CIGAR ops (SECEDO_E_LIMIT)
    kSamTooLong = 17,   // a record of 2^31 bytes or more (SECEDO_E_LIMIT)
    kSamCodes = 18,
};

// RefID of a line that is no record (the empty line that ends a file)
constexpr int32_t kSamNoRecord = -2147483647 - 1;

// 64-bit FNV-1a of a reference name; the host hashes the @SQ names with it, the device the RNAME / RNEXT fields
__host__ __device__ inline uint64_t sam_name_hash(const uint8_t *p, uint32_t n) {
    uint64_t h = 1469598103934665603ull;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// the @SQ names of one file: packed bytes (off[n + 1] by RefID), their hashes sorted and the RefID of each;
// sel[RefID] = 1 for the chromosomes whose records are encoded
struct SamRefs {
    const uint8_t *bytes;
    const uint32_t *off;
    const uint64_t *hash;
    const uint32_t *id;
    const uint8_t *sel;
    uint32_t n;
};

// One range of SAM text (whole lines, the last one ending the range), uploaded into d_text padded with zeros to a
// multiple of 16 bytes plus 16. Line k spans [d_start[k], d_start[k + 1] - 1).
// newline_count: d_cnt[i] = the '\n' bytes of the 16-byte vector i (n16 vectors)
hipError_t sam_newline_count(const uint8_t *d_text, uint64_t n16, uint32_t *d_cnt, hipStream_t s);
// line starts from the exclusive scan of d_cnt; n_lines = newlines + (no_trailing_newline ? 1 : 0); the range
// length len closes the last line when it has no '\n'
hipError_t sam_line_starts(const uint8_t *d_text, uint64_t n16, const uint32_t *d_scan, uint32_t n_lines,
                           uint32_t len, bool no_trailing_newline, uint32_t *d_start, hipStream_t s);
// size pass: per line its RefID, 0-based POS, and the bytes of its BAM record (block_size field included) when its
// RefID is selected, else 0. line_base: the file's line index (0 = first line after the header) of line 0;
// ends_file: the range ends the file (its last line may be empty). d_err: u64 min of (line_base + k) << 8 | code
hipError_t sam_size(const uint8_t *d_text, const uint32_t *d_start, uint32_t n_lines, uint64_t line_base,
                    bool ends_file, const SamRefs &refs, uint64_t *d_size, int32_t *d_ref, int32_t *d_pos,
                    unsigned long long *d_err, hipStream_t s);
// encode pass: the records of the lines [0, n_lines) with a selected RefID at d_out + d_off[k] (the exclusive scan
// of d_size); every line below n_lines must have passed the size pass
hipError_t sam_encode(const uint8_t *d_text, const uint32_t *d_start, uint32_t n_lines, const SamRefs &refs,
                      const uint64_t *d_off, uint8_t *d_out, hipStream_t s);

}  // namespace bam
}  // namespace secedo
