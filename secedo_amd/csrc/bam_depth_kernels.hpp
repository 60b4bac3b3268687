// bam_depth_kernels.hpp -- launch wrappers of bam_depth_kernels.hip (gfx950): the device passes of secedo_bam_depth
//  between a chromosome's records in HBM and the reduced (bin, cell, value) pairs, the summaries over the
// pairs and the text of the output files. The rules that decide numbers and bytes are in bam_depth.hpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "bam_depth.hpp"

namespace secedo {
namespace bamdepth {

// slots of the device counters behind secedo_bam_depth_info
enum Stat : uint32_t {
    kStatBarcode = 0, kStatRequire, kStatExclude, kStatDuplicate, kStatMapq, kStatRange, kStatRecords, kStatCounted,
    kStatSlots
};

// one reduced pair, in output order (bin, then cell)
struct Pair {
    uint32_t bin, cell;
    uint64_t value;
};
static_assert(sizeof(Pair) == 16, "one 16-byte load per pair");

// Front, one thread per uploaded record o < n (input order): the cell (d_file[o], or in tag mode the cell of
// bam::cells' key where d_tag_sel[o]), steps 1 and 2 of the selection. d_cell[o] = the cell (0xFFFF without one),
// d_sel[o] = 1 for a record with a cell whose FLAG passes, d_key[o] = its Position (the duplicate rule's sort key).
// d_cell_records[cell] += 1 for every record with a cell; d_stat takes kStatBarcode, kStatRecords, kStatRequire,
// kStatExclude.
hipError_t depth_front(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, const uint16_t *d_file,
                       const uint64_t *d_tag_key, const uint32_t *d_tag_sel, uint32_t n_cells, uint32_t require,
                       uint32_t exclude, uint16_t *d_cell, uint32_t *d_sel, uint64_t *d_key,
                       unsigned long long *d_cell_records, unsigned long long *d_stat, hipStream_t s);

// Steps 3 to 5, one thread per selected record j < m (input ordinal d_val[j]): d_keep (null: step 3 is off) is rule
// 3d's choice, then MapQuality >= min_mapq, then 0 <= Position < ln. d_pieces[j] = the record's pieces (0 for a
// dropped record; 1 in `reads` mode; touched_bins in `bases` mode), d_pieces[m] = 0. d_cell_counted[cell] += 1 for a
// survivor; d_stat takes kStatDuplicate, kStatMapq, kStatRange, kStatCounted.
hipError_t depth_count(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                       const uint16_t *d_cell, const uint32_t *d_keep, uint32_t min_mapq, uint32_t ln, uint32_t S,
                       int mode, uint64_t *d_pieces, unsigned long long *d_cell_counted, unsigned long long *d_stat,
                       hipStream_t s);

// Emit, one lane per piece p < n_pieces: its record is the j with d_piece_off[j] <= p < d_piece_off[j + 1]
// (d_piece_off = the exclusive sum of d_pieces, m + 1 entries). d_key[p] = (bin_base + bin) * n_cells + cell,
// d_value[p] = 1 (`reads`) or piece_covered (`bases`, may be 0).
hipError_t depth_emit(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                      const uint16_t *d_cell, const uint64_t *d_piece_off, uint32_t n_pieces, uint32_t ln, uint32_t S,
                      int mode, uint64_t bin_base, uint32_t n_cells, uint64_t *d_key, uint32_t *d_value, hipStream_t s);

// stable radix sort of (key, value) over key bits [0, end_bit); n up to 2^32 - 1 (bamsplit::split_sort counts its items
// as an int)
size_t depth_sort_bytes(uint32_t n);
hipError_t depth_sort(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in,
                      uint32_t *v_out, uint32_t n, int end_bit, hipStream_t s);

// Reduce over the n sorted pieces. heads: d_head[p] = 1 where a run of equal keys starts, d_wide[p] = d_value[p] as
// u64; both have n + 1 entries, the last 0.
hipError_t depth_heads(const uint64_t *d_key, const uint32_t *d_value, uint32_t n, uint32_t *d_head, uint64_t *d_wide,
                       hipStream_t s);
// d_start[r] = the first piece of run r (d_run = the exclusive sum of d_head, n_runs = d_run[n]); d_start[n_runs] = n
hipError_t depth_run_starts(const uint32_t *d_head, const uint32_t *d_run, uint32_t n, uint32_t *d_start,
                            hipStream_t s);
// run r's pair: the key's bin and cell, value = d_sum[d_start[r + 1]] - d_sum[d_start[r]] (d_sum = the exclusive sum
// of d_wide). d_keep[r] = value > 0, d_keep[n_runs] = 0.
hipError_t depth_run_sums(const uint64_t *d_key, const uint32_t *d_start, const uint64_t *d_sum, uint32_t n_runs,
                          uint32_t n_cells, Pair *d_pair, uint32_t *d_keep, hipStream_t s);
// the pairs with d_keep at d_at (its exclusive sum), order kept
hipError_t depth_compact(const Pair *d_pair, const uint32_t *d_keep, const uint32_t *d_at, uint32_t n_runs,
                         Pair *d_out, hipStream_t s);

// Summaries over all n pairs of the call: d_rows[cell].sum / nonzero_bins / max_value (records and counted are left
// as they are), and with d_cluster (the cluster of each cell) d_table[bin * n_clusters + cluster] += value. At most
// one atomic per pair and target, all integer sums and maxima.
hipError_t depth_summaries(const Pair *d_pair, uint64_t n, CellRow *d_rows, const uint16_t *d_cluster,
                           uint32_t n_clusters, uint64_t *d_table, hipStream_t s);

// ---- text, count then store (text_sink.hpp). The items [i0, i0 + n) of one file; measure gives d_len[k] (n + 1
// entries, the last 0), write stores item k's line at d_out + d_off[k] (d_off = the exclusive sum of d_len). The host
// loop over the ranges of a file is text_out.hpp's Formatter; Names is bam_depth.hpp's.

// depth.counts.mtx: item = pair
hipError_t mtx_measure(const Pair *d_pair, uint64_t i0, uint32_t n, uint64_t *d_len, hipStream_t s);
hipError_t mtx_write(const Pair *d_pair, uint64_t i0, uint32_t n, const uint64_t *d_off, uint8_t *d_out,
                     hipStream_t s);
// depth.cells.tsv: item = cell
hipError_t cells_measure(const CellRow *d_rows, Names names, uint32_t i0, uint32_t n, uint64_t *d_len, hipStream_t s);
hipError_t cells_write(const CellRow *d_rows, Names names, uint32_t i0, uint32_t n, const uint64_t *d_off,
                       uint8_t *d_out, hipStream_t s);
// depth.clusters.tsv: item = global bin; d_base[n_chr + 1] and d_len_chr[n_chr] are the layout's, chr_names those of
// the requested chromosomes
struct BinTable {
    const uint64_t *base;
    const uint32_t *len;
    uint32_t n_chr, S;
    Names chr_names;
    const uint64_t *table;
    uint32_t n_clusters;
};
hipError_t clusters_measure(const BinTable &t, uint64_t i0, uint32_t n, uint64_t *d_len, hipStream_t s);
hipError_t clusters_write(const BinTable &t, uint64_t i0, uint32_t n, const uint64_t *d_off, uint8_t *d_out,
                          hipStream_t s);

}  // namespace bamdepth
}  // namespace secedo
