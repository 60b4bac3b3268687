// bam_split_kernels.hip -- the device passes of secedo_bam_split_clusters (include/secedo_bam.h), gfx950.
//
// Per requested chromosome the records lie in HBM in input order (file, record), with the byte offset of each. The
// passes turn them into one output stream, cluster after cluster, each cluster's records in (Position, file, record)
// order, byte for byte as they came:
//   k_split_keys     one thread per record: cell -> cluster, key = cluster << 32 | Position, sel = the record has a cell
//   (scan, compaction: bam_kernels.hip's; stable radix sort of (key, ordinal) over the key bits in use: hipcub)
//   k_split_lengths  one thread per sorted record: where it lies and how long it is (4 + block_size)
//   (exclusive sum of the lengths: each record's destination, the total last)
//   k_split_extents  one thread per sorted record: a cluster's first record gives where the cluster starts
//   k_split_gather   one thread per 16 output bytes: the bandwidth pass
// secedo_bam_split_clusters_rg runs k_split_plan in place of k_split_lengths (the aux walk, the hole of
// the record's own RG field, the edited length) and k_split_gather_rg in place of k_split_gather (the same tiles over
// edited records); both stand behind the plain call's kernels below. secedo_bam_split_clusters_select
// adds, only when asked: k_split_and (per-file mode's flag test joins the selection), k_split_view (the sorted records
// as the bam::Records that rule 3d's passes of bam_kernels.hip take), k_split_compact (remove: the chosen records
// leave the order) and k_split_mark (mark: the choice goes into the top bit of src[j]); the two gathers are templates
// whose <true> instantiation sets 0x04 in byte 19 of a marked record, and whose <false> one is the code they were.
//
// The gather is balanced over output bytes, not over records: lane i of a workgroup writes bytes [16 i, 16 i + 16) of
// the workgroup's 4 KiB tile with one aligned 16-byte store, so a wave's store instruction covers 1 KiB contiguous
// bytes, and a 70 KB record is spread over 18 workgroups like any other bytes. Which record holds an output byte is a
// binary search in the destination offsets: lane 0 searches all of them once for the tile's first byte, every lane then
// searches only the records that can start inside the tile (bam_split.hpp: kTileRecords, at most 7 steps, L1/L2 hits).
// The source side is at arbitrary byte alignment: a lane whose 16 bytes lie in one record reads the five aligned dwords
// that cover them and shifts (consecutive lanes read consecutive dwords, so the loads coalesce as the stores do); a
// lane on a record boundary, and the stream's last lane, assemble their dwords byte by byte.
#include "bam_split.hpp"
#include "bam_split_kernels.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

namespace secedo {
namespace bamsplit {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

__global__ void __launch_bounds__(kBlock) k_split_keys(const uint8_t *__restrict__ bytes,
                                                       const uint64_t *__restrict__ in_off, uint32_t n,
                                                       const uint16_t *__restrict__ file,
                                                       const uint64_t *__restrict__ tag_key,
                                                       const uint32_t *__restrict__ tag_sel,
                                                       const uint16_t *__restrict__ cell_cluster, uint32_t n_cells,
                                                       uint64_t *__restrict__ key, uint32_t *__restrict__ sel) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= n) return;
    uint32_t cell = ~0u;
    if (tag_key) {
        if (tag_sel[o]) cell = uint32_t(tag_key[o] >> 32) & 0x3FFF;  // chunk << 46 | cell << 32 | Position
    } else {
        cell = file[o];
    }
    const bool ok = cell < n_cells;
    const uint32_t pos = ld32(bytes + in_off[o] + 4 + 4);  // >= 0: the input layer refuses negative positions
    key[o] = ok ? pack_key(cell_cluster[cell], pos) : 0;
    sel[o] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_split_lengths(const uint8_t *__restrict__ bytes,
                                                          const uint64_t *__restrict__ in_off,
                                                          const uint32_t *__restrict__ val, uint32_t m,
                                                          uint64_t *__restrict__ src, uint64_t *__restrict__ len) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j > m) return;
    if (j == m) {
        len[m] = 0;
        return;
    }
    const uint64_t off = in_off[val[j]];
    src[j] = off;
    len[j] = 4ull + ld32(bytes + off);
}

__global__ void __launch_bounds__(kBlock) k_split_extents(const uint64_t *__restrict__ key,
                                                          const uint64_t *__restrict__ dst, uint32_t m,
                                                          uint64_t *__restrict__ beg) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t c = key_cluster(key[j]);
    if (j == 0 || key_cluster(key[j - 1]) != c) beg[c] = dst[j];
}

// the dword at byte address p + s of an array whose base p is dword-aligned: two aligned loads and a shift
__device__ __forceinline__ uint32_t dword_at(const uint32_t *__restrict__ w, uint64_t s) {
    const uint64_t k = s >> 2;
    const uint64_t pair = uint64_t(w[k + 1]) << 32 | w[k];
    return uint32_t(pair >> (8 * uint32_t(s & 3)));
}

// kMark: src[j] carries the record's duplicate mark in its top bit (bam_split.hpp: pack_src); the lane
// that holds byte 19 of a marked record sets 0x04 in it. Without kMark src[j] is the offset and nothing is tested.
template <bool kMark>
__global__ void __launch_bounds__(kGatherLanes) k_split_gather(const uint8_t *__restrict__ bytes,
                                                               const uint64_t *__restrict__ src,
                                                               const uint64_t *__restrict__ dst, uint32_t m,
                                                               uint64_t total, uint8_t *__restrict__ out) {
    __shared__ uint32_t s_first;
    const uint64_t tile = uint64_t(blockIdx.x) * kTileBytes;
    if (threadIdx.x == 0) s_first = record_of(dst, 0, m, tile);
    __syncthreads();
    const uint64_t b = tile + uint64_t(threadIdx.x) * kGatherVec;
    if (b >= total) return;
    const uint32_t lo = s_first;
    const uint32_t hi = uint64_t(lo) + kTileRecords < m ? lo + kTileRecords : m;
    uint32_t j = record_of(dst, lo, hi, b);
    uint64_t d0 = dst[j], d1 = dst[j + 1], s0 = src[j];
    const bool marked = kMark && src_marked(s0);
    if (kMark) s0 = src_off(s0);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(bytes);
    uint32_t v[4];
    if (b + kGatherVec <= d1) {  // all 16 bytes in record j: five aligned dwords cover them
        const uint64_t s = s0 + (b - d0);
        const uint64_t k = s >> 2;
        const uint32_t sh = 8 * uint32_t(s & 3);
        uint32_t x[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = w[k + i];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = uint32_t((uint64_t(x[i + 1]) << 32 | x[i]) >> sh);
        if (marked) mark_vector(v, b - d0);
    } else {  // a record boundary or the stream's end: never byte 19 of a record (bam_split.hpp)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t p = b + 4 * i;
            while (p < total && p >= d1) {  // p < total = dst[m]: j + 1 <= m stays inside dst
                ++j;
                d0 = d1, d1 = dst[j + 1], s0 = kMark ? src_off(src[j]) : src[j];
            }
            if (p + 4 <= d1) {
                v[i] = dword_at(w, s0 + (p - d0));
                continue;
            }
            uint32_t x = 0;
            for (uint32_t q = 0; q < 4 && p + q < total; ++q) {
                while (p + q >= d1) {
                    ++j;
                    d0 = d1, d1 = dst[j + 1], s0 = kMark ? src_off(src[j]) : src[j];
                }
                x |= uint32_t(bytes[s0 + (p + q - d0)]) << (8 * q);
            }
            v[i] = x;
        }
    }
    *reinterpret_cast<uint4 *>(out + b) = make_uint4(v[0], v[1], v[2], v[3]);
}

// ---- read groups

// One thread per sorted record: where it lies, its cell (as k_split_keys found it), the strict aux walk of
// bam_split.hpp and the edited length. cnt[0..3] += records with a hole, records whose walk failed, appended bytes,
// removed bytes: summed per workgroup in LDS, one global atomic per counter and workgroup.
__global__ void __launch_bounds__(kBlock) k_split_plan(const uint8_t *__restrict__ bytes,
                                                       const uint64_t *__restrict__ in_off,
                                                       const uint32_t *__restrict__ val, uint32_t m,
                                                       const uint16_t *__restrict__ file,
                                                       const uint64_t *__restrict__ tag_key,
                                                       const uint32_t *__restrict__ suf_off,
                                                       uint64_t *__restrict__ src, uint64_t *__restrict__ len,
                                                       RecordPlan *__restrict__ plan,
                                                       unsigned long long *__restrict__ cnt) {
    __shared__ unsigned long long s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j == m) len[m] = 0;
    if (j < m) {
        const uint32_t o = val[j];
        const uint64_t off = in_off[o];
        const uint32_t cell = tag_key ? uint32_t(tag_key[o] >> 32) & 0x3FFF : file[o];
        const uint32_t n = 4u + ld32(bytes + off);
        const AuxHole h = aux_walk(bytes + off, n);
        const uint32_t suf = suf_off[cell + 1] - suf_off[cell];
        src[j] = off;
        plan[j] = RecordPlan{h.hole_off, h.hole_len, n, cell};
        len[j] = uint64_t(n) - h.hole_len + suf;
        if (h.hole_len) {
            atomicAdd(&s_cnt[0], 1ull);
            atomicAdd(&s_cnt[3], (unsigned long long)h.hole_len);
        }
        if (!h.parsed) atomicAdd(&s_cnt[1], 1ull);
        atomicAdd(&s_cnt[2], (unsigned long long)suf);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
}

// The sorted record a lane of the editing gather stands in: its extent in the stream, its source, its edit and its
// cell's suffix.
struct Cursor {
    uint64_t d0, d1, s0;
    Edit e;
    const uint8_t *suffix;
    bool marked;
    template <bool kMark>
    __device__ __forceinline__ void load(const uint64_t *__restrict__ src, const uint64_t *__restrict__ dst,
                                         const RecordPlan *__restrict__ plan, const uint32_t *__restrict__ suf_off,
                                         const uint8_t *__restrict__ suf, uint32_t j) {
        d0 = dst[j], d1 = dst[j + 1], s0 = src[j];
        marked = kMark && src_marked(s0);
        if (kMark) s0 = src_off(s0);
        const RecordPlan p = plan[j];
        const uint32_t so = suf_off[p.cell];
        e = Edit{p.len, p.hole_off, p.hole_len, suf_off[p.cell + 1] - so};
        suffix = suf + so;
    }
};

// k_split_gather over edited records: the same tiles, lanes and stores. An edited record is the patched block_size
// word, the bytes before the hole, the bytes after it and the cell's suffix. A lane whose 16 bytes lie in one of the
// two copied segments keeps the five-dword path; any other lane (a record's first bytes, a hole, a suffix, a record
// boundary, the stream's end) takes whole dwords where a dword lies in a copied segment and edited_byte's rule for the
// rest. The tile bound is the plain gather's (bam_split.hpp says why it holds for edited records). kMark as in
// k_split_gather: byte 19 lies in front of any hole, in a lane of the five-dword path (bam_split.hpp).
template <bool kMark>
__global__ void __launch_bounds__(kGatherLanes) k_split_gather_rg(const uint8_t *__restrict__ bytes,
                                                                  const uint64_t *__restrict__ src,
                                                                  const uint64_t *__restrict__ dst,
                                                                  const RecordPlan *__restrict__ plan,
                                                                  const uint32_t *__restrict__ suf_off,
                                                                  const uint8_t *__restrict__ suf, uint32_t m,
                                                                  uint64_t total, uint8_t *__restrict__ out) {
    __shared__ uint32_t s_first;
    const uint64_t tile = uint64_t(blockIdx.x) * kTileBytes;
    if (threadIdx.x == 0) s_first = record_of(dst, 0, m, tile);
    __syncthreads();
    const uint64_t b = tile + uint64_t(threadIdx.x) * kGatherVec;
    if (b >= total) return;
    const uint32_t lo = s_first;
    const uint32_t hi = uint64_t(lo) + kTileRecords < m ? lo + kTileRecords : m;
    uint32_t j = record_of(dst, lo, hi, b);
    Cursor c;
    c.template load<kMark>(src, dst, plan, suf_off, suf, j);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(bytes);
    uint32_t v[4];
    const uint64_t r = b - c.d0;  // < 2^32: inside record j
    const uint32_t kept = c.e.len - c.e.hole_len;
    const bool before = r >= 4 && r + kGatherVec <= c.e.hole_off;
    const bool after = r >= c.e.hole_off && r + kGatherVec <= kept;  // hole_off >= 36 > 4
    if (b + kGatherVec <= c.d1 && (before || after)) {
        const uint64_t s = c.s0 + r + (after ? c.e.hole_len : 0u);
        const uint64_t k = s >> 2;
        const uint32_t sh = 8 * uint32_t(s & 3);
        uint32_t x[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = w[k + i];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = uint32_t((uint64_t(x[i + 1]) << 32 | x[i]) >> sh);
        if (c.marked) mark_vector(v, r);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t p = b + 4 * i;
            // j <= m - 1: p < dst[m]
            while (p < total && p >= c.d1) c.template load<kMark>(src, dst, plan, suf_off, suf, ++j);
            const uint64_t q = p - c.d0;
            const uint32_t keep = c.e.len - c.e.hole_len;
            if (p + 4 <= c.d1 && q >= 4 && q + 4 <= c.e.hole_off) {
                v[i] = dword_at(w, c.s0 + q);
                continue;
            }
            if (p + 4 <= c.d1 && q >= c.e.hole_off && q + 4 <= keep) {
                v[i] = dword_at(w, c.s0 + q + c.e.hole_len);
                continue;
            }
            uint32_t x = 0;
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                if (p + t >= total) break;
                while (p + t >= c.d1) c.template load<kMark>(src, dst, plan, suf_off, suf, ++j);
                x |= uint32_t(edited_byte(bytes + c.s0, c.e, c.suffix, uint32_t(p + t - c.d0))) << (8 * t);
            }
            v[i] = x;
        }
    }
    *reinterpret_cast<uint4 *>(out + b) = make_uint4(v[0], v[1], v[2], v[3]);
}

// ---- record selection

// per-file mode's flag filter: the selection of k_split_keys ANDed with bam::flag_test's keep, in front of the scan
__global__ void __launch_bounds__(kBlock) k_split_and(uint32_t *__restrict__ sel, const uint32_t *__restrict__ keep,
                                                      uint32_t n) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o < n && !keep[o]) sel[o] = 0;
}

// The bam::Records view of the sorted records, one thread per sorted record j: where it lies and its cell (as
// k_split_keys found it). Within a cell the sorted order is the pileup's global order, so rule 3d's passes over this
// view choose the pileup's set.
__global__ void __launch_bounds__(kBlock) k_split_view(const uint64_t *__restrict__ in_off,
                                                       const uint32_t *__restrict__ val, uint32_t m,
                                                       const uint16_t *__restrict__ file,
                                                       const uint64_t *__restrict__ tag_key,
                                                       uint64_t *__restrict__ off, uint16_t *__restrict__ cell) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t o = val[j];
    off[j] = in_off[o];
    cell[j] = tag_key ? uint16_t((tag_key[o] >> 32) & 0x3FFF) : file[o];
}

// remove: the sorted (key, ordinal) pairs with keep[j] at scan[j] (keep's exclusive sum), order kept
__global__ void __launch_bounds__(kBlock) k_split_compact(const uint64_t *__restrict__ key,
                                                          const uint32_t *__restrict__ val,
                                                          const uint32_t *__restrict__ keep,
                                                          const uint32_t *__restrict__ scan, uint32_t m,
                                                          uint64_t *__restrict__ key_out,
                                                          uint32_t *__restrict__ val_out) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m || !keep[j]) return;
    key_out[scan[j]] = key[j];
    val_out[scan[j]] = val[j];
}

// mark: the chosen records (keep[j] == 0) get the top bit of their source offset set
__global__ void __launch_bounds__(kBlock) k_split_mark(uint64_t *__restrict__ src, const uint32_t *__restrict__ keep,
                                                       uint32_t m) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < m) src[j] = pack_src(src[j], keep[j] == 0);
}

inline uint32_t grid(uint64_t n) { return uint32_t((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t split_and(uint32_t *d_sel, const uint32_t *d_keep, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_split_and<<<grid(n), kBlock, 0, s>>>(d_sel, d_keep, n);
    return hipGetLastError();
}

hipError_t split_view(const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m, const uint16_t *d_file,
                      const uint64_t *d_tag_key, uint64_t *d_off, uint16_t *d_cell, hipStream_t s) {
    if (m == 0) return hipSuccess;
    k_split_view<<<grid(m), kBlock, 0, s>>>(d_in_off, d_val, m, d_file, d_tag_key, d_off, d_cell);
    return hipGetLastError();
}

hipError_t split_compact(const uint64_t *d_key, const uint32_t *d_val, const uint32_t *d_keep, const uint32_t *d_scan,
                         uint32_t m, uint64_t *d_key_out, uint32_t *d_val_out, hipStream_t s) {
    if (m == 0) return hipSuccess;
    k_split_compact<<<grid(m), kBlock, 0, s>>>(d_key, d_val, d_keep, d_scan, m, d_key_out, d_val_out);
    return hipGetLastError();
}

hipError_t split_mark(uint64_t *d_src, const uint32_t *d_keep, uint32_t m, hipStream_t s) {
    if (m == 0) return hipSuccess;
    k_split_mark<<<grid(m), kBlock, 0, s>>>(d_src, d_keep, m);
    return hipGetLastError();
}

hipError_t split_keys(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, const uint16_t *d_file,
                      const uint64_t *d_tag_key, const uint32_t *d_tag_sel, const uint16_t *d_cell_cluster,
                      uint32_t n_cells, uint64_t *d_key, uint32_t *d_sel, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_split_keys<<<grid(n), kBlock, 0, s>>>(d_bytes, d_in_off, n, d_file, d_tag_key, d_tag_sel, d_cell_cluster,
                                            n_cells, d_key, d_sel);
    return hipGetLastError();
}

size_t split_sort_bytes(uint32_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                             (const uint32_t *)nullptr, (uint32_t *)nullptr, int(n));
    return b;
}

hipError_t split_sort(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in,
                      uint32_t *v_out, uint32_t n, int end_bit, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k_in, k_out, v_in, v_out, int(n), 0, end_bit, s);
}

hipError_t split_lengths(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                         uint64_t *d_src, uint64_t *d_len, hipStream_t s) {
    k_split_lengths<<<grid(uint64_t(m) + 1), kBlock, 0, s>>>(d_bytes, d_in_off, d_val, m, d_src, d_len);
    return hipGetLastError();
}

hipError_t split_extents(const uint64_t *d_key, const uint64_t *d_dst, uint32_t m, uint64_t *d_beg, hipStream_t s) {
    if (m == 0) return hipSuccess;
    k_split_extents<<<grid(m), kBlock, 0, s>>>(d_key, d_dst, m, d_beg);
    return hipGetLastError();
}

hipError_t split_gather(const uint8_t *d_bytes, const uint64_t *d_src, const uint64_t *d_dst, uint32_t m,
                        uint64_t total, uint8_t *d_out, hipStream_t s, bool marks) {
    if (m == 0 || total == 0) return hipSuccess;
    const uint64_t tiles = (total + kTileBytes - 1) / kTileBytes;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (marks) k_split_gather<true><<<uint32_t(tiles), kGatherLanes, 0, s>>>(d_bytes, d_src, d_dst, m, total, d_out);
    else k_split_gather<false><<<uint32_t(tiles), kGatherLanes, 0, s>>>(d_bytes, d_src, d_dst, m, total, d_out);
    return hipGetLastError();
}

hipError_t split_plan(const uint8_t *d_bytes, const uint64_t *d_in_off, const uint32_t *d_val, uint32_t m,
                      const uint16_t *d_file, const uint64_t *d_tag_key, const uint32_t *d_suf_off, uint64_t *d_src,
                      uint64_t *d_len, RecordPlan *d_plan, uint64_t *d_cnt, hipStream_t s) {
    k_split_plan<<<grid(uint64_t(m) + 1), kBlock, 0, s>>>(d_bytes, d_in_off, d_val, m, d_file, d_tag_key, d_suf_off,
                                                          d_src, d_len, d_plan,
                                                          reinterpret_cast<unsigned long long *>(d_cnt));
    return hipGetLastError();
}

hipError_t split_gather_rg(const uint8_t *d_bytes, const uint64_t *d_src, const uint64_t *d_dst,
                           const RecordPlan *d_plan, const uint32_t *d_suf_off, const uint8_t *d_suf, uint32_t m,
                           uint64_t total, uint8_t *d_out, hipStream_t s, bool marks) {
    if (m == 0 || total == 0) return hipSuccess;
    const uint64_t tiles = (total + kTileBytes - 1) / kTileBytes;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (marks)
        k_split_gather_rg<true><<<uint32_t(tiles), kGatherLanes, 0, s>>>(d_bytes, d_src, d_dst, d_plan, d_suf_off,
                                                                         d_suf, m, total, d_out);
    else
        k_split_gather_rg<false><<<uint32_t(tiles), kGatherLanes, 0, s>>>(d_bytes, d_src, d_dst, d_plan, d_suf_off,
                                                                          d_suf, m, total, d_out);
    return hipGetLastError();
}

}  // namespace bamsplit
}  // namespace secedo
