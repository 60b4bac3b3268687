// sam_kernels.hpp -- launch wrappers of sam_kernels.hip (gfx950): SAM text lines -> the BAM records bam_kernels.hip
// reads. See sam_kernels.hip for the conversion rules.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "sam_parse.hpp"  // SamErr, kSamNoRecord, sam_name_hash, SamRefs

namespace secedo {
namespace bam {

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
