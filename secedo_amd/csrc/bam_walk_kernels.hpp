// bam_walk_kernels.hpp -- launch wrappers of bam_walk_kernels.hip (gfx950): the BAM record walk over bytes that
// bgzf_kernels.hip inflated in HBM. See bam_walk_kernels.hip for the passes and bam_walk.hpp for the decisions.
#pragma once

#include "bam_walk.hpp"
#include "bgzf_kernels.hpp"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace bam {

// bytes the walk may read past the last inflated byte of the buffer (its LDS window is staged in whole vectors)
constexpr uint32_t kWalkWindow = 4096;

// One file of a batch (or one range of a file): set by the host, updated by the passes, read back whole.
struct WalkFile {
    // in
    uint32_t first_seg, n_seg;  // its segments, one per BGZF member of the batch, in file order
    uint32_t data_end;          // the end of its bytes in the buffer (they start at its first segment's start)
    uint32_t final;             // the bytes end the file
    uint64_t carry_src;         // carry_len bytes at d_in + carry_src go in front of its first member's bytes
    uint32_t carry_len, has_prev;
    uint64_t rec_base;          // records of the file before this range
    int32_t prev_ref, prev_pos; // of the last of them (has_prev)
    // out
    uint32_t limit;             // in: data_end; the start of the first member that did not inflate, if lower
    uint32_t stop_off;          // where the chain stopped: the bytes from here on are carried into the next range
    unsigned long long bad;     // in: ~0; min of (member of the batch << 8 | its bgzf status) over bad members
    unsigned long long err;     // in: ~0; min of (record of the file << 8 | bamwalk::Code)
    unsigned long long unsorted;  // in: ~0; the lowest record that sorts before its predecessor
    uint64_t n_rec;             // records in these bytes
    uint32_t first_rec;         // the batch's index of the first of them
    uint32_t rewalked;          // segments joined by a walk of their own
    int32_t last_ref, last_pos; // of the last record (n_rec > 0)
};

// the first run of requested chromosome u in file f, entry f * n_chr + u
struct WalkRun {
    uint32_t first, last;  // in and out: bam_walk.hpp's started / done rule (kNoRun, kNoRun for a fresh file)
    uint32_t j0, j1;       // out: its records among the batch's selected ones
    uint64_t b0, b1;       // out: its bytes among the gathered ones
};

// One requested chromosome u of file f of a batch whose bytes are a span of an indexed file (or a range of one),
// entry f * n_chr + u: what the index says of it, as offsets of the batch's buffer, against the records the walk found.
// The offsets are signed: a chromosome may start or end in another range of the span.
constexpr uint32_t kSpanOn = 1;     // the chromosome lies in this span
constexpr uint32_t kSpanEntry = 2;  // beg is where the walk enters the span: the RefID there is read before the walk's
                                    // results are believed (when those 8 bytes lie below the file's limit)
constexpr uint32_t kSpanTail = 4;   // end is the span's limit and the 8 bytes at it are inflated: the RefID there
struct SpanCheck {
    // in
    long long beg, end;
    uint32_t flags;
    int32_t ref;
    // out
    uint32_t start;      // 0: beg is no record start of this range's; 1: the record there has RefID ref; 2: none has
    uint32_t entry_bad;  // kSpanEntry: the RefID at beg is not ref
    uint32_t tail_bad;   // kSpanTail: the RefID at end is ref
    uint32_t reserved;
    uint64_t count;      // records of this range that start in [beg, end)
};

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
