// bam_depth_kernels.hip -- the device passes of secedo_bam_depth (include/secedo_bam.h), gfx950: per-cell
// read depth in fixed genomic bins, the bins x cells count matrix copy-number tools start from.
//
// The contract, restated (include/secedo_bam.h holds it; bam_depth.hpp decides every number and byte):
//  A. Bins. Chromosome id c is @SQ index c; with bin size S >= 1 it has ceil(LN_c / S) bins and bin b covers
//     [b S, min((b + 1) S, LN_c)). Global bin numbers run over the requested chromosomes in ascending id.
//  B. Cells. The file index, or in tag mode the index of the record's barcode in the list (rule 3b of
//     bam_kernels.hip).
//  C. Selection, in this order, per call and never from the process-wide pileup settings: 1. the barcode (3b);
//     2. the flag masks (3c): (flag & require) == require and (flag & exclude) == 0, require counted first; 3. the
//     per-cell duplicate removal (3d, bam_host.hpp: duplicate_keep); 4. MapQuality >= min_map_quality; 5. the range:
//     a Position < 0 or >= LN_c is dropped and counted.
//  D. What is counted. `reads`: each survivor adds 1 to the bin of its 0-based Position. `bases`: each survivor adds,
//     to every bin it touches, the reference positions in that bin that an M, = or X op of its CIGAR covers; D and N
//     advance the position and add nothing, I, S, H and P do neither, positions >= LN_c add nothing, a record without
//     a CIGAR adds nothing and is still a counted record.
//  E. Values are u64, only integer sums and maxima exist: no result depends on an execution order, two runs are
//     byte-identical. Zeros never reach the outputs.
//
// Passes, per requested chromosome (its records in HBM in input order: file, record):
//   k_front        one thread per record: cell, steps 1 and 2, the per-cell `records` counter
//   (scan, compaction of the passing records: bam_kernels.hip's; with duplicates=remove the stable sort by Position
//    and rule 3d's passes, as secedo_bam_split_clusters_select runs them)
//   k_count        one thread per passing record: steps 3 to 5, the per-cell `counted` counter, the record's pieces
//                  (`reads`: 1; `bases`: the bins its reference span touches)
//   (exclusive sum of the pieces)
//   k_emit         one lane per piece: its record by the lookup of bam_split.hpp's record_of, then key =
//                  global_bin * n_cells + cell and value = 1 or the CIGAR walk to the piece; a 70 kb read over 1 kb
//                  bins is 70 lanes, not one thread's 70 steps
//   (stable radix sort of the pieces over the key bits in use: hipcub)
//   k_heads, k_run_starts, k_run_sums, k_compact   run heads, the runs' first pieces, each run's sum as a difference
//                  of the values' exclusive sum, and the runs with a sum above 0 compacted: the pairs in output order
// and once per call over all pairs: k_summaries (per-cell sum, nonzero_bins, max_value and the dense n_bins x K
// cluster table: at most one atomic per pair and target, neighbouring lanes on different cells), then the text of
// depth.counts.mtx, depth.cells.tsv and depth.clusters.tsv by count-then-store sinks (text_sink.hpp), one thread per
// line.
//
// No record adds into a bins x cells table: within a cell the records are position-sorted, so whole waves would hit
// one address, and the dense table would not fit. The per-cell counters of k_front and k_count have the same shape
// (in per-file mode a wave's records are one cell's), so a wave first groups its lanes by cell with ballots and adds
// once per distinct cell. Plain C++ stores only.
#include "bam_depth_kernels.hpp"
#include "bam_split.hpp"
#include "text_sink.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

namespace secedo {
namespace bamdepth {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNoCell = 0xFFFF;

inline uint32_t grid(uint64_t n) { return uint32_t((n + kBlock - 1) / kBlock); }

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}
__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }

// Block-wide count of `yes` into *slot, one atomic per block. Every thread of the block calls it.
__device__ __forceinline__ void block_count(bool yes, unsigned long long *slot) {
    const int c = __syncthreads_count(yes ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(slot, (unsigned long long)c);
}

// table[cell] += 1 for every lane with `yes`, one atomic per distinct cell of the wave. Every lane of the wave calls
// it; the loop's condition is the same in all of them.
__device__ __forceinline__ void wave_cell_add(bool yes, uint32_t cell, unsigned long long *table) {
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long left = __ballot(yes);
    while (left) {
        const int leader = __ffsll(left) - 1;
        const uint32_t c = __shfl(cell, leader, 64);
        const unsigned long long same = __ballot(yes && cell == c);
        if (lane == uint32_t(leader)) atomicAdd(&table[c], (unsigned long long)__popcll(same));
        left &= ~same;
    }
}

__global__ void __launch_bounds__(kBlock) k_front(const uint8_t *__restrict__ bytes,
                                                  const uint64_t *__restrict__ in_off, uint32_t n,
                                                  const uint16_t *__restrict__ file,
                                                  const uint64_t *__restrict__ tag_key,
                                                  const uint32_t *__restrict__ tag_sel, uint32_t n_cells,
                                                  uint32_t require, uint32_t exclude, uint16_t *__restrict__ cell_out,
                                                  uint32_t *__restrict__ sel, uint64_t *__restrict__ key,
                                                  unsigned long long *__restrict__ cell_records,
                                                  unsigned long long *__restrict__ stat) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    const bool in = o < n;
    uint32_t cell = kNoCell;
    bool has = false, req = false, exc = false;
    if (in) {
        if (tag_key) {
            if (tag_sel[o]) cell = uint32_t(tag_key[o] >> 32) & 0x3FFF;  // chunk << 46 | cell << 32 | Position
        } else {
            cell = file[o];
        }
        has = cell < n_cells;
        if (!has) cell = kNoCell;
        const uint8_t *rec = bytes + in_off[o];
        const uint32_t flag = ld16(rec + 4 + 14);
        req = has && (flag & require) != require;
        exc = has && !req && (flag & exclude) != 0;
        cell_out[o] = uint16_t(cell);
        sel[o] = (has && !req && !exc) ? 1 : 0;
        key[o] = ld32(rec + 4 + 4);
    }
    wave_cell_add(has, cell, cell_records);
    block_count(in && !has, stat + kStatBarcode);
    block_count(has, stat + kStatRecords);
    block_count(req, stat + kStatRequire);
    block_count(exc, stat + kStatExclude);
}

__global__ void __launch_bounds__(kBlock) k_count(const uint8_t *__restrict__ bytes,
                                                  const uint64_t *__restrict__ in_off,
                                                  const uint32_t *__restrict__ val, uint32_t m,
                                                  const uint16_t *__restrict__ cell_in,
                                                  const uint32_t *__restrict__ keep, uint32_t min_mapq, uint32_t ln,
                                                  uint32_t S, int mode, uint64_t *__restrict__ pieces,
                                                  unsigned long long *__restrict__ cell_counted,
                                                  unsigned long long *__restrict__ stat) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool dup = false, low = false, out = false, ok = false;
    uint32_t cell = kNoCell;
    if (j < m) {
        const uint32_t o = val[j];
        const uint8_t *core = bytes + in_off[o] + 4;
        cell = cell_in[o];
        const int32_t pos = int32_t(ld32(core + 4));
        dup = keep && keep[j] == 0;
        low = !dup && uint32_t(core[9]) < min_mapq;
        out = !dup && !low && (pos < 0 || uint32_t(pos) >= ln);
        ok = !dup && !low && !out;
        uint64_t np = 0;
        if (ok) {
            if (mode == kModeReads) {
                np = 1;
            } else {
                const uint32_t n_cigar = ld16(core + 12);
                const uint8_t *cigar = core + 32 + core[8];
                np = touched_bins(uint32_t(pos), ref_span(cigar, n_cigar), ln, S);
            }
        }
        pieces[j] = np;
    }
    if (j == m) pieces[m] = 0;
    wave_cell_add(ok, cell, cell_counted);
    block_count(dup, stat + kStatDuplicate);
    block_count(low, stat + kStatMapq);
    block_count(out, stat + kStatRange);
    block_count(ok, stat + kStatCounted);
}

__global__ void __launch_bounds__(kBlock) k_emit(const uint8_t *__restrict__ bytes,
                                                 const uint64_t *__restrict__ in_off,
                                                 const uint32_t *__restrict__ val, uint32_t m,
                                                 const uint16_t *__restrict__ cell_in,
                                                 const uint64_t *__restrict__ piece_off, uint32_t n_pieces,
                                                 uint32_t ln, uint32_t S, int mode, uint64_t bin_base,
                                                 uint32_t n_cells, uint64_t *__restrict__ key,
                                                 uint32_t *__restrict__ value) {
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n_pieces) return;
    const uint32_t j = bamsplit::record_of(piece_off, 0, m, p);  // piece_off[j] <= p < piece_off[j + 1]
    const uint32_t q = uint32_t(p - piece_off[j]);
    const uint32_t o = val[j];
    const uint8_t *core = bytes + in_off[o] + 4;
    const uint32_t pos = ld32(core + 4);  // in [0, ln): k_count gave this record pieces
    uint32_t v = 1;
    if (mode != kModeReads) v = piece_covered(core + 32 + core[8], ld16(core + 12), pos, ln, S, q);
    key[p] = pack_key(bin_base + bin_of(pos, S) + q, cell_in[o], n_cells);
    value[p] = v;
}

__global__ void __launch_bounds__(kBlock) k_heads(const uint64_t *__restrict__ key,
                                                  const uint32_t *__restrict__ value, uint32_t n,
                                                  uint32_t *__restrict__ head, uint64_t *__restrict__ wide) {
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p > n) return;
    if (p == n) {
        head[n] = 0;
        wide[n] = 0;
        return;
    }
    head[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
    wide[p] = value[p];
}

__global__ void __launch_bounds__(kBlock) k_run_starts(const uint32_t *__restrict__ head,
                                                       const uint32_t *__restrict__ run, uint32_t n,
                                                       uint32_t *__restrict__ start) {
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p > n) return;
    if (p == n) start[run[n]] = n;
    else if (head[p]) start[run[p]] = uint32_t(p);
}

__global__ void __launch_bounds__(kBlock) k_run_sums(const uint64_t *__restrict__ key,
                                                     const uint32_t *__restrict__ start,
                                                     const uint64_t *__restrict__ sum, uint32_t n_runs,
                                                     uint32_t n_cells, Pair *__restrict__ pair,
                                                     uint32_t *__restrict__ keep) {
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r > n_runs) return;
    if (r == n_runs) {
        keep[n_runs] = 0;
        return;
    }
    const uint32_t a = start[r], z = start[r + 1];
    const uint64_t k = key[a], v = sum[z] - sum[a];
    pair[r] = Pair{key_bin(k, n_cells), key_cell(k, n_cells), v};
    keep[r] = v > 0 ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_compact(const Pair *__restrict__ pair, const uint32_t *__restrict__ keep,
                                                    const uint32_t *__restrict__ at, uint32_t n_runs,
                                                    Pair *__restrict__ out) {
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r >= n_runs || !keep[r]) return;
    out[at[r]] = pair[r];
}

__global__ void __launch_bounds__(kBlock) k_summaries(const Pair *__restrict__ pair, uint64_t n,
                                                      CellRow *__restrict__ rows,
                                                      const uint16_t *__restrict__ cluster, uint32_t n_clusters,
                                                      uint64_t *__restrict__ table) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const Pair p = pair[i];
    CellRow *row = rows + p.cell;
    atomicAdd(reinterpret_cast<unsigned long long *>(&row->sum), (unsigned long long)p.value);
    atomicAdd(reinterpret_cast<unsigned long long *>(&row->nonzero_bins), 1ull);
    atomicMax(reinterpret_cast<unsigned long long *>(&row->max_value), (unsigned long long)p.value);
    if (cluster)
        atomicAdd(reinterpret_cast<unsigned long long *>(table + uint64_t(p.bin) * n_clusters + cluster[p.cell]),
                  (unsigned long long)p.value);
}

// ---- text: one thread per line, the same put_* once into a CountSink and once into a ByteSink

template <class Sink>
__device__ __forceinline__ void cell_line(Sink &s, const CellRow *rows, const Names &names, uint32_t c) {
    put_cell_line(s, c, names.bytes + names.off[c], names.off[c + 1] - names.off[c], rows[c]);
}

template <class Sink>
__device__ __forceinline__ void cluster_line(Sink &s, const BinTable &t, uint64_t g) {
    const uint32_t k = chr_of_bin(t.base, t.n_chr, g);
    const uint32_t b = uint32_t(g - t.base[k]);
    put_cluster_line(s, t.chr_names.bytes + t.chr_names.off[k], t.chr_names.off[k + 1] - t.chr_names.off[k],
                     bin_start(b, t.S), bin_end(b, t.S, t.len[k]), t.table + g * t.n_clusters, t.n_clusters);
}

__global__ void __launch_bounds__(kBlock) k_mtx_measure(const Pair *__restrict__ pair, uint64_t i0, uint32_t n,
                                                        uint64_t *__restrict__ len) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k > n) return;
    text::CountSink s;
    if (k < n) {
        const Pair p = pair[i0 + k];
        put_mtx_line(s, p.bin, p.cell, p.value);
    }
    len[k] = s.n;
}

__global__ void __launch_bounds__(kBlock) k_mtx_write(const Pair *__restrict__ pair, uint64_t i0, uint32_t n,
                                                      const uint64_t *__restrict__ off, uint8_t *__restrict__ out) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= n) return;
    const Pair p = pair[i0 + k];
    text::ByteSink s{out + off[k]};
    put_mtx_line(s, p.bin, p.cell, p.value);
}

__global__ void __launch_bounds__(kBlock) k_cells_measure(const CellRow *__restrict__ rows, Names names, uint32_t i0,
                                                          uint32_t n, uint64_t *__restrict__ len) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k > n) return;
    text::CountSink s;
    if (k < n) cell_line(s, rows, names, i0 + uint32_t(k));
    len[k] = s.n;
}

__global__ void __launch_bounds__(kBlock) k_cells_write(const CellRow *__restrict__ rows, Names names, uint32_t i0,
                                                        uint32_t n, const uint64_t *__restrict__ off,
                                                        uint8_t *__restrict__ out) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= n) return;
    text::ByteSink s{out + off[k]};
    cell_line(s, rows, names, i0 + uint32_t(k));
}

__global__ void __launch_bounds__(kBlock) k_clusters_measure(BinTable t, uint64_t i0, uint32_t n,
                                                             uint64_t *__restrict__ len) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k > n) return;
    text::CountSink s;
    if (k < n) cluster_line(s, t, i0 + k);
    len[k] = s.n;
}

__global__ void __launch_bounds__(kBlock) k_clusters_write(BinTable t, uint64_t i0, uint32_t n,
                                                           const uint64_t *__restrict__ off,
                                                           uint8_t *__restrict__ out) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= n) return;
    text::ByteSink s{out + off[k]};
    cluster_line(s, t, i0 + k);
}

}  // namespace

hipError_t depth_front(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, const uint16_t *d_file,
                       const uint64_t *d_tag_key, const uint32_t *d_tag_sel, uint32_t n_cells, uint32_t require,
                       uint32_t exclude, uint16_t *d_cell, uint32_t *d_sel, uint64_t *d_key,
                       unsigned long long *d_cell_records, unsigned long long *d_stat, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_front<<<grid(n), kBlock, 0, s>>>(d_bytes, d_in_off, n, d_file, d_tag_key, d_tag_sel, n_cells, require, exclude,
                                       d_cell, d_sel, d_key, d_cell_records, d_stat);
    return hipGetLastError();
}

hipError_t depth_count(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                       const uint16_t *d_cell, const uint32_t *d_keep, uint32_t min_mapq, uint32_t ln, uint32_t S,
                       int mode, uint64_t *d_pieces, unsigned long long *d_cell_counted, unsigned long long *d_stat,
                       hipStream_t s) {
    k_count<<<grid(uint64_t(m) + 1), kBlock, 0, s>>>(d_bytes, d_in_off, d_val, m, d_cell, d_keep, min_mapq, ln, S, mode,
                                                     d_pieces, d_cell_counted, d_stat);
    return hipGetLastError();
}

hipError_t depth_emit(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                      const uint16_t *d_cell, const uint64_t *d_piece_off, uint32_t n_pieces, uint32_t ln, uint32_t S,
                      int mode, uint64_t bin_base, uint32_t n_cells, uint64_t *d_key, uint32_t *d_value,
                      hipStream_t s) {
    if (n_pieces == 0 || m == 0) return hipSuccess;
    k_emit<<<grid(n_pieces), kBlock, 0, s>>>(d_bytes, d_in_off, d_val, m, d_cell, d_piece_off, n_pieces, ln, S, mode,
                                             bin_base, n_cells, d_key, d_value);
    return hipGetLastError();
}

size_t depth_sort_bytes(uint32_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                             (const uint32_t *)nullptr, (uint32_t *)nullptr, n);
    return b;
}

hipError_t depth_sort(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in,
                      uint32_t *v_out, uint32_t n, int end_bit, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k_in, k_out, v_in, v_out, n, 0, end_bit, s);
}

hipError_t depth_heads(const uint64_t *d_key, const uint32_t *d_value, uint32_t n, uint32_t *d_head, uint64_t *d_wide,
                       hipStream_t s) {
    k_heads<<<grid(uint64_t(n) + 1), kBlock, 0, s>>>(d_key, d_value, n, d_head, d_wide);
    return hipGetLastError();
}

hipError_t depth_run_starts(const uint32_t *d_head, const uint32_t *d_run, uint32_t n, uint32_t *d_start,
                            hipStream_t s) {
    k_run_starts<<<grid(uint64_t(n) + 1), kBlock, 0, s>>>(d_head, d_run, n, d_start);
    return hipGetLastError();
}

hipError_t depth_run_sums(const uint64_t *d_key, const uint32_t *d_start, const uint64_t *d_sum, uint32_t n_runs,
                          uint32_t n_cells, Pair *d_pair, uint32_t *d_keep, hipStream_t s) {
    k_run_sums<<<grid(uint64_t(n_runs) + 1), kBlock, 0, s>>>(d_key, d_start, d_sum, n_runs, n_cells, d_pair, d_keep);
    return hipGetLastError();
}

hipError_t depth_compact(const Pair *d_pair, const uint32_t *d_keep, const uint32_t *d_at, uint32_t n_runs,
                         Pair *d_out, hipStream_t s) {
    if (n_runs == 0) return hipSuccess;
    k_compact<<<grid(n_runs), kBlock, 0, s>>>(d_pair, d_keep, d_at, n_runs, d_out);
    return hipGetLastError();
}

hipError_t depth_summaries(const Pair *d_pair, uint64_t n, CellRow *d_rows, const uint16_t *d_cluster,
                           uint32_t n_clusters, uint64_t *d_table, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if ((n + kBlock - 1) / kBlock > 0x7FFFFFFFull) return hipErrorInvalidValue;
    k_summaries<<<grid(n), kBlock, 0, s>>>(d_pair, n, d_rows, d_cluster, n_clusters, d_table);
    return hipGetLastError();
}

hipError_t mtx_measure(const Pair *d_pair, uint64_t i0, uint32_t n, uint64_t *d_len, hipStream_t s) {
    k_mtx_measure<<<grid(uint64_t(n) + 1), kBlock, 0, s>>>(d_pair, i0, n, d_len);
    return hipGetLastError();
}
hipError_t mtx_write(const Pair *d_pair, uint64_t i0, uint32_t n, const uint64_t *d_off, uint8_t *d_out,
                     hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_mtx_write<<<grid(n), kBlock, 0, s>>>(d_pair, i0, n, d_off, d_out);
    return hipGetLastError();
}
hipError_t cells_measure(const CellRow *d_rows, Names names, uint32_t i0, uint32_t n, uint64_t *d_len, hipStream_t s) {
    k_cells_measure<<<grid(uint64_t(n) + 1), kBlock, 0, s>>>(d_rows, names, i0, n, d_len);
    return hipGetLastError();
}
hipError_t cells_write(const CellRow *d_rows, Names names, uint32_t i0, uint32_t n, const uint64_t *d_off,
                       uint8_t *d_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_cells_write<<<grid(n), kBlock, 0, s>>>(d_rows, names, i0, n, d_off, d_out);
    return hipGetLastError();
}
hipError_t clusters_measure(const BinTable &t, uint64_t i0, uint32_t n, uint64_t *d_len, hipStream_t s) {
    k_clusters_measure<<<grid(uint64_t(n) + 1), kBlock, 0, s>>>(t, i0, n, d_len);
    return hipGetLastError();
}
hipError_t clusters_write(const BinTable &t, uint64_t i0, uint32_t n, const uint64_t *d_off, uint8_t *d_out,
                          hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_clusters_write<<<grid(n), kBlock, 0, s>>>(t, i0, n, d_off, d_out);
    return hipGetLastError();
}

}  // namespace bamdepth
}  // namespace secedo
