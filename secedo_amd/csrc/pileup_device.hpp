// pileup_device.hpp -- launch wrappers of pileup_device.hip (gfx950): the per-record and per-entry passes of
// the binary pileup loader of include/secedo_pileup.h. See pileup_device.hip for the restated semantics.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace pileup {

// Per-file state the passes update with atomics; zeroed (err_key set to kNoError) before a file.
struct FileState {
    uint32_t max_cell_plus1;  // largest kept raw cell id + 1, 0 without kept entries
    uint32_t max_rid;         // largest kept read id
    uint32_t stopped;         // a coverage-passing record found the position list exhausted
    uint32_t pad;
    uint64_t err_key;         // min over bad kept entries of record << 30 | entry << 14 | cell
    uint32_t max_span;        // largest read span (the span passes)
    uint32_t pad2;
};
constexpr uint64_t kNoError = ~0ull;

// Sizes at the end of a chunk: its kept loci and entries, and the last value of its position max-scan.
struct ChunkTail {
    uint32_t loci;
    uint32_t max_pos;
    uint64_t entries;
};

// One chunk of complete records: bytes (2-byte aligned device copy), rec_off[n] record starts in bytes (a chunk
// holds less than 4 GiB).
struct Chunk {
    const uint16_t *bytes;
    const uint32_t *rec_off;
    uint32_t n;
    uint64_t rec_base;  // index in the file of the chunk's first record
};

// Scratch of one chunk, n_cap records.
struct ChunkScratch {
    uint32_t *pos, *cov, *mval, *mscan, *keep, *lidx;
    uint64_t *cnt, *eoff;
    void *tmp;
    size_t tmp_bytes;
};

size_t scan_bytes(uint64_t n);
size_t sort_bytes(uint64_t n);

// heads + max-scan + keep flags + the locus / entry scans + gather + tail, all in stream s.
// carry_max: running maximum of the coverage-passing positions before the chunk (valid when have_carry).
hipError_t decode_chunk(const Chunk &c, const ChunkScratch &w, uint32_t max_coverage, const uint32_t *d_positions,
                        uint64_t n_positions, uint32_t carry_max, uint64_t l_base, uint64_t e_base,
                        const uint16_t *d_id_to_group, uint32_t n_ids, uint32_t *pos_out, uint64_t *off_out,
                        uint32_t *rid_out, uint16_t *idb_out, FileState *st, ChunkTail *tail, hipStream_t s);

// Read spans of one file's output: loci [l0, l0 + n_loci), entries off[l0] .. off[l0 + n_loci].
// Dense: first/last tables of table_n = max_rid + 1 u32 each. Sparse: keys[2 * n_entries] u64 + sort scratch.
hipError_t spans_dense(const uint32_t *pos, const uint64_t *off, const uint32_t *rid, uint64_t l0, uint32_t n_loci,
                       uint32_t *first, uint32_t *last, uint32_t table_n, FileState *st, hipStream_t s);
hipError_t spans_sparse(const uint32_t *pos, const uint64_t *off, const uint32_t *rid, uint64_t l0, uint32_t n_loci,
                        uint64_t e0, uint64_t n_entries, uint64_t *keys, void *tmp, size_t tmp_bytes,
                        FileState *st, hipStream_t s);

}  // namespace pileup
}  // namespace secedo
