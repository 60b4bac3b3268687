// fasta_kernels.hpp -- launch wrappers of fasta_kernels.hip (gfx950): the FASTA text of one range, resident in HBM,
// parsed into one code byte per base and a small table of the header lines, and the per-locus gather of the reference
// genotypes from those codes. See fasta_lines.hpp for the line roles and fasta_kernels.hip for the passes.
#pragma once

#include "fasta_lines.hpp"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace fasta {

constexpr uint32_t kChunk = 16;            // text bytes per lane: one 16-byte vector load
constexpr uint32_t kMaxRange = 1u << 30;   // offsets inside a range are u32

inline uint32_t num_chunks(uint32_t len) { return (len + kChunk - 1) / kChunk; }

// What the passes of one range need beside the text, sized for ranges of up to max_len bytes and `cap` header slots.
struct RangeWork {
    Transfer *tf, *tf_in;        // [chunks] per chunk: its transfer function; the composition of all chunks before it
    uint64_t *cnt, *cnt_before;  // [chunks] sequence bytes | header starts << 32 of the chunk; of all chunks before it
    uint8_t *codes;              // [max_len] one code per base of the range, in text order
    RangeTotals *totals;         // followed by HeaderSlot[cap]: read back in one copy
    uint32_t cap;
    void *scan_tmp;
    size_t scan_bytes;
};
SECEDO_FASTA_HD inline HeaderSlot *slots_of(RangeTotals *t) { return reinterpret_cast<HeaderSlot *>(t + 1); }
inline size_t table_bytes(uint32_t cap) { return sizeof(RangeTotals) + size_t(cap) * sizeof(HeaderSlot); }

// temporary storage of the two scans over num_chunks(max_len) elements
size_t scan_workspace(uint32_t max_len);

// The passes of one range: d_text[0, len), 16-byte aligned, entered in `state`. Leaves w.codes, w.totals and the slots.
// len may be 0 (the totals then say so). Asynchronous on s.
hipError_t parse_range(const uint8_t *d_text, uint32_t len, uint32_t state, const RangeWork &w, hipStream_t s);

// The last pass alone, over the tf_in and cnt_before that parse_range left for this same range: the totals and the
// slots again, for a caller that found w.cap too small (RangeTotals.headers >= cap) and comes back with a table that
// fits. w.codes may be null here and in parse_range: the codes are then not written.
hipError_t emit_range(const uint8_t *d_text, uint32_t len, uint32_t state, const RangeWork &w, hipStream_t s);

// d_dst[l] = d_codes[code_off + (p - q0)] for the loci l of [l0, l1) with p = d_pos[l] - 1 in [q0, q0 + count)
hipError_t gather(const uint8_t *d_codes, uint32_t code_off, uint32_t count, uint64_t q0, const uint32_t *d_pos,
                  uint32_t l0, uint32_t l1, uint8_t *d_dst, hipStream_t s);

// d_end[c] = the first locus of chromosome c with d_pos - 1 >= d_len[c], else d_chr_off[c + 1]; d_locus_ref[l] = the
// genotype from d_mat / d_pat (d_hap[c]: maternal twice) in front of it, 0 from it on.
hipError_t finish(const uint32_t *d_chr_off, uint32_t n_chr, const uint32_t *d_pos, uint32_t n_loci,
                  const uint64_t *d_len, const uint8_t *d_hap, const uint8_t *d_mat, const uint8_t *d_pat,
                  uint8_t *d_locus_ref, uint32_t *d_end, hipStream_t s);

}  // namespace fasta
}  // namespace secedo
