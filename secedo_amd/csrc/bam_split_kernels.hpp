// bam_split_kernels.hpp -- launch wrappers of bam_split_kernels.hip (gfx950): the device passes of
// secedo_bam_split_clusters between the chromosome's records in HBM and the BGZF encoder. The rules that
// decide bytes are in bam_split.hpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "bam_split.hpp"

namespace secedo {
namespace bamsplit {

// Keys, one thread per uploaded record o < n (input order: file, record): d_key[o] = cluster << 32 | Position and
// d_sel[o] = 1 for a record with a cell. Per-file mode (d_tag_key null): the cell is d_file[o]. Tag mode: d_tag_key /
// d_tag_sel are what bam::cells (rule 3b of bam_kernels.hip, flag filter off) gave for the same records, and the cell
// is the one in its key; records it did not select get d_sel 0. d_cell_cluster[n_cells]; a cell at or past n_cells
// gets d_sel 0 (the host has refused such input before).
hipError_t split_keys(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, const uint16_t *d_file,
                      const uint64_t *d_tag_key, const uint32_t *d_tag_sel, const uint16_t *d_cell_cluster,
                      uint32_t n_cells, uint64_t *d_key, uint32_t *d_sel, hipStream_t s);

// stable radix sort of (key, input ordinal) over key bits [0, end_bit)
size_t split_sort_bytes(uint32_t n);
hipError_t split_sort(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in,
                      uint32_t *v_out, uint32_t n, int end_bit, hipStream_t s);

// Sorted record j < m is input ordinal d_val[j]: d_src[j] = its byte offset in d_bytes, d_len[j] = 4 + block_size.
// d_len[m] = 0, so that an exclusive sum over m + 1 entries ends with the total.
hipError_t split_lengths(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                         uint64_t *d_src, uint64_t *d_len, hipStream_t s);

// d_beg[c] = d_dst[j] for the first sorted record j of cluster c; other entries of d_beg are left as they are
hipError_t split_extents(const uint64_t *d_key, const uint64_t *d_dst, uint32_t m, uint64_t *d_beg, hipStream_t s);

// The gather: output bytes [0, total) of the one stream, record j's bytes at d_dst[j] (d_dst[m] = total), written to
// d_out as whole 16-byte vectors (d_out 16-byte aligned, room for total rounded up to 16; the bytes past total are
// zero). d_bytes is read as aligned dwords: it needs 8 bytes of room behind its last record. marks: d_src went through
// split_mark, and a marked record is written with 0x400 set in its FLAG (the kMark instantiation).
hipError_t split_gather(const uint8_t *d_bytes, const uint64_t *d_src, const uint64_t *d_dst, uint32_t m,
                        uint64_t total, uint8_t *d_out, hipStream_t s, bool marks = false);

// ---- read groups (secedo_bam_split_clusters_rg); RecordPlan and the rules are bam_split.hpp's

// The plan, one thread per sorted record j < m (input ordinal d_val[j]): d_src[j] as split_lengths gives it, d_plan[j]
// = the hole of the strict aux walk, the record's length and its cell (d_file / d_tag_key as for split_keys), d_len[j]
// = the edited length, d_len[m] = 0. d_suf_off[n_cells + 1]: where each cell's suffix starts in the suffix table.
// d_cnt[0..3] += records with a hole, records whose walk failed, appended bytes, removed bytes (zero them first).
hipError_t split_plan(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                      const uint16_t *d_file, const uint64_t *d_tag_key, const uint32_t *d_suf_off, uint64_t *d_src,
                      uint64_t *d_len, RecordPlan *d_plan, uint64_t *d_cnt, hipStream_t s);

// split_gather over edited records: record j's edited bytes at d_dst[j]. d_bytes and d_out as for split_gather; d_suf
// is read byte by byte. marks as for split_gather.
hipError_t split_gather_rg(const uint8_t *d_bytes, const uint64_t *d_src, const uint64_t *d_dst,
                           const RecordPlan *d_plan, const uint32_t *d_suf_off, const uint8_t *d_suf, uint32_t m,
                           uint64_t total, uint8_t *d_out, hipStream_t s, bool marks = false);

// ---- record selection (secedo_bam_split_clusters_select)

// per-file mode's flag filter: d_sel[o] = 0 where d_keep[o] == 0 (bam::flag_test over the input order)
hipError_t split_and(uint32_t *d_sel, const uint32_t *d_keep, uint32_t n, hipStream_t s);
// The bam::Records view of the sorted records for rule 3d's passes: d_off[j] = d_in_off[d_val[j]], d_cell[j] = the
// cell of sorted record j (d_file / d_tag_key as for split_keys).
hipError_t split_view(const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m, const uint16_t *d_file,
                      const uint64_t *d_tag_key, uint64_t *d_off, uint16_t *d_cell, hipStream_t s);
// remove: the sorted pairs with d_keep[j] != 0 at d_scan[j] (the exclusive sum of d_keep), order kept
hipError_t split_compact(const uint64_t *d_key, const uint32_t *d_val, const uint32_t *d_keep, const uint32_t *d_scan,
                         uint32_t m, uint64_t *d_key_out, uint32_t *d_val_out, hipStream_t s);
// mark: d_src[j] = pack_src(d_src[j], d_keep[j] == 0)
hipError_t split_mark(uint64_t *d_src, const uint32_t *d_keep, uint32_t m, hipStream_t s);

}  // namespace bamsplit
}  // namespace secedo
