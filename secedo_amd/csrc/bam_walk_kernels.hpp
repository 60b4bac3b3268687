// bam_walk_kernels.hpp -- launch wrappers of bam_walk_kernels.hip (gfx950): the BAM record walk over bytes that
// bgzf_kernels.hip inflated in HBM. See bam_walk_kernels.hip for the passes and bam_walk.hpp for the decisions.
#pragma once

#include "bam_batch.hpp"
#include "bam_walk.hpp"
#include "bgzf_kernels.hpp"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace bam {

// kWalkWindow, WalkFile, WalkRun, SpanCheck and the kSpan* flags: bam_batch.hpp, which fills them

// the arrays of one batch
struct WalkBatch {
    uint8_t *buf;               // inflated bytes; buf_bytes (a multiple of 16) are allocated
    uint64_t buf_bytes;
    const bamwalk::Seg *segs;   // [n_seg]
    WalkFile *files;            // [n_files]
    uint32_t n_seg, n_files;
    uint32_t *lists, *rewalk;   // [n_list] each
    bamwalk::SegWalk *walk;     // [n_seg]
    bamwalk::SegJoin *join;     // [n_seg]
    uint32_t *seg_cnt;          // [n_seg + 1] accepted records per segment, then their exclusive sum in seg_base
    uint32_t *seg_base;
};

// per accepted record of a batch
struct WalkRecords {
    uint32_t n;
    uint32_t *off, *file;       // [n] offset in buf, file of the batch
    int32_t *ref, *pos;         // [n]
    uint32_t *sel;              // [n + 1] 1 = taken (a requested chromosome's first run)
    uint64_t *size;             // [n + 1] its bytes if taken
    uint32_t *sel_scan;         // [n + 1] exclusive sums
    uint64_t *size_scan;
};

// the carries into place, then per bad member the file's limit and `bad` (status[] as bgzf_inflate left it)
// for the first n_members segments, which are the batch's members in the order of d_desc
hipError_t walk_prepare(const WalkBatch &b, const uint8_t *d_in, const BgzfDesc *d_desc, const uint32_t *d_status,
                        uint32_t n_members, hipStream_t s);
// speculative segment walk, join, records per segment (seg_cnt; the caller scans it into seg_base)
hipError_t walk_segments(const WalkBatch &b, hipStream_t s);
// per record: offset, file, RefID, Position, the structural check, sortedness, run starts; d_per_ref (may be null):
// records per RefID < n_ref, d_per_ref[n_ref] = the unmapped ones. Then the run ends and the selection with its checks.
hipError_t walk_records(const WalkBatch &b, const WalkRecords &r, const uint32_t *d_chr, uint32_t n_chr,
                        WalkRun *d_runs, unsigned long long *d_per_ref, uint32_t n_ref, hipStream_t s);
// after walk_records: the consistency pass over the spans of indexed files, d_checks[n_files * n_chr]
hipError_t walk_span_check(const WalkBatch &b, const WalkRecords &r, uint32_t n_chr, SpanCheck *d_checks,
                           hipStream_t s);
// after the scans of sel and size: the runs' extents; d_totals[0] = records taken, [1] = their bytes
hipError_t walk_runs(const WalkBatch &b, const WalkRecords &r, uint32_t n_chr, WalkRun *d_runs, uint64_t *d_totals,
                     hipStream_t s);
// the taken records' bytes to d_out in record order; per taken record its offset there, Position and file index
hipError_t walk_gather(const WalkBatch &b, const WalkRecords &r, uint8_t *d_out, uint64_t *d_sel_off,
                       int32_t *d_sel_pos, uint64_t *d_sel_idx, hipStream_t s);

}  // namespace bam
}  // namespace secedo
