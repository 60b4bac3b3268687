// bam_index_kernels.hpp -- launch wrappers of bam_index_kernels.hip (gfx950): what a .bai index needs of the records of
// one batch of the device walk, after walk_records. See bam_index_kernels.hip for the passes and bam_index_build.hpp
// for what the host makes of the results.
#pragma once

#include "bam_walk_kernels.hpp"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace bam {

// error codes of the index pass, min of (record of the file << 8 | code) per file
constexpr uint32_t kIndexErrRef = 1;   // a RefID at or past the header's n_ref
constexpr uint32_t kIndexErrEnd = 2;   // the record ends past 2^29
constexpr uint32_t kIndexErrSize = 3;  // the CIGAR does not lie inside the record (the walk reports it first)

// IndexFile, one file of the batch: bam_batch.hpp, which fills it

// the first record of a run of consecutive records of one file with the same (RefID, bin, flag 0x4)
struct IndexHead {
    uint64_t lin;  // its file-linear offset
    uint64_t ord;  // its ordinal in the file
    int32_t ref;
    uint32_t bin, file, unmapped;
};

// a 16 kb window and the first record of this batch that overlaps it
struct IndexWin {
    uint64_t lin;
    uint32_t file;
    int32_t ref;
    uint32_t w, pad;
};

// per record of the batch
struct IndexRecords {
    uint32_t *meta;                   // [n] bin | flag 0x4 << 31; 0 for RefID -1
    uint64_t *key, *key_max;          // [n] (the RefID's number << 16 | last window); its inclusive max scan
    uint32_t *head, *head_scan;       // [n + 1] 1 = a run starts here; exclusive sum
    uint64_t *n_win, *n_win_scan;     // [n + 1] windows this record is the first to overlap; exclusive sum
};

size_t index_scan_bytes(uint64_t n);
// per record end, bin and key, then key_max; tmp: index_scan_bytes(r.n)
hipError_t index_records(const WalkBatch &b, const WalkRecords &r, const IndexRecords &x, IndexFile *d_files, void *tmp,
                         size_t tmp_bytes, hipStream_t s);
// head[] and n_win[], the scans' last element included (the caller scans both)
hipError_t index_flags(const WalkBatch &b, const WalkRecords &r, const IndexRecords &x, hipStream_t s);
// after the scans: the heads and windows, each in record order
hipError_t index_emit(const WalkBatch &b, const WalkRecords &r, const IndexRecords &x, const IndexFile *d_files,
                      IndexHead *d_heads, IndexWin *d_wins, hipStream_t s);

}  // namespace bam
}  // namespace secedo
