// pileup_device.hip -- device passes of the binary pileup loader (include/secedo_pileup.h) for gfx950.
//
// The host uploads a chunk of whole records (the bytes, 2-byte aligned, and the record starts it found by walking
// the 6-byte headers) and runs, in one stream:
//   heads       one thread per record: position (two aligned u16 loads), coverage, the coverage test
//               (coverage > max_coverage: skipped) and the value of the position max-scan (0 when skipped)
//   max-scan    inclusive max over the chunk (hipcub); with the carry of the earlier chunks it is M_r, the running
//               maximum of the coverage-passing positions up to record r
//   keep_flags  the host's monotone PositionFilter in parallel form: i_r = lower_bound(positions, M_r); record r
//               is kept iff i_r < n and positions[i_r] == pos_r; i_r == n on a coverage-passing record means the
//               list is exhausted (the host stops there; M is monotone, so nothing later is kept either). An empty
//               list keeps every coverage-passing record.
//   scans       inclusive sums of the keep flags (locus index) and of the kept coverages (entry offsets, u64)
//   gather      one wave per record: read ids from aligned u16 pairs at record + 6, packed ids at
//               record + 6 + 4 * coverage; cell = packed >> 2 checked against n_ids (the first offending entry in
//               file order wins: atomic min of record << 30 | entry << 14 | cell), id_base16 =
//               uint16(id_to_group[cell] << 2 | (packed & 3)); wave-reduced maxima of the cell and read ids
//   tail        the chunk's totals and the max-scan carry, read back once per chunk
// After a file, the read spans (position of the last appearance - position of the first, file order, u32) come
// from a dense first/last table (atomic min / max of the file's locus index per read id) when the largest read id
// is small, else from a radix sort of (read id, locus index) keys.
#include "pileup_device.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace secedo {
namespace pileup {

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr uint32_t kPass = 0x10000u;

struct MaxOp {
    __device__ __host__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};

__device__ inline uint32_t wave_max(uint32_t v) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, kWave);
        v = v > w ? v : w;
    }
    return v;
}

unsigned blocks_for(uint64_t threads) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((threads + kBlock - 1) / kBlock, 16384));
}

__global__ void heads(const uint16_t *__restrict__ b, const uint32_t *__restrict__ rec_off, uint32_t n,
                      uint32_t max_coverage, uint32_t *__restrict__ pos, uint32_t *__restrict__ cov,
                      uint32_t *__restrict__ mval) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint64_t o = rec_off[r] >> 1;
        const uint32_t p = uint32_t(b[o]) | uint32_t(b[o + 1]) << 16;
        const uint32_t c = b[o + 2];
        const bool pass = c <= max_coverage;
        pos[r] = p;
        cov[r] = c | (pass ? kPass : 0u);
        mval[r] = pass ? p : 0u;
    }
}

__device__ inline uint64_t lower_bound(const uint32_t *__restrict__ a, uint64_t n, uint32_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void keep_flags(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ cov,
                           const uint32_t *__restrict__ mscan, uint32_t n, uint32_t carry_max,
                           const uint32_t *__restrict__ positions, uint64_t n_positions, uint32_t *__restrict__ keep,
                           uint64_t *__restrict__ cnt, FileState *st) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t c = cov[r];
        uint32_t k = 0;
        if (c & kPass) {
            if (n_positions == 0) {
                k = 1;
            } else {
                const uint32_t m = max(carry_max, mscan[r]);
                const uint64_t i = lower_bound(positions, n_positions, m);
                if (i == n_positions) st->stopped = 1u;  // every writer stores the same value
                else k = positions[i] == pos[r];
            }
        }
        keep[r] = k;
        cnt[r] = k ? (c & 0xFFFFu) : 0u;
    }
}

__global__ void gather(Chunk c, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ cov,
                       const uint32_t *__restrict__ keep, const uint32_t *__restrict__ lidx,
                       const uint64_t *__restrict__ eoff, uint64_t l_base, uint64_t e_base,
                       const uint16_t *__restrict__ id_to_group, uint32_t n_ids, uint32_t *__restrict__ pos_out,
                       uint64_t *__restrict__ off_out, uint32_t *__restrict__ rid_out,
                       uint16_t *__restrict__ idb_out, FileState *st) {
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    const uint32_t n_waves = gridDim.x * blockDim.x / kWave;
    uint32_t mc = 0, mr = 0;
    for (uint32_t r = wave; r < c.n; r += n_waves) {  // wave-uniform
        if (!keep[r]) continue;
        const uint32_t cv = cov[r] & 0xFFFFu;
        const uint64_t e0 = e_base + eoff[r] - cv;
        if (lane == 0) {
            const uint64_t l = l_base + lidx[r] - 1;
            pos_out[l] = pos[r];
            off_out[l] = e0;
        }
        const uint64_t ids = (uint64_t(c.rec_off[r]) + 6) >> 1;  // u16 index of read_ids[0]
        const uint64_t packed = ids + 2ull * cv;                 // u16 index of the packed ids
        for (uint32_t j = lane; j < cv; j += kWave) {
            const uint32_t rid = uint32_t(c.bytes[ids + 2 * j]) | uint32_t(c.bytes[ids + 2 * j + 1]) << 16;
            const uint32_t pk = c.bytes[packed + j];
            const uint32_t cell = pk >> 2;
            uint16_t out = 0;
            if (cell >= n_ids) {
                atomicMin((unsigned long long *)&st->err_key,
                          (unsigned long long)((c.rec_base + r) << 30 | uint64_t(j) << 14 | cell));
            } else {
                out = uint16_t(uint32_t(id_to_group[cell]) << 2 | (pk & 3u));
                mc = max(mc, cell + 1);
            }
            rid_out[e0 + j] = rid;
            idb_out[e0 + j] = out;
            mr = max(mr, rid);
        }
    }
    mc = wave_max(mc);
    mr = wave_max(mr);
    if (lane == 0) {
        if (mc) atomicMax(&st->max_cell_plus1, mc);
        if (mr) atomicMax(&st->max_rid, mr);
    }
}

__global__ void tail_kernel(const uint32_t *lidx, const uint64_t *eoff, const uint32_t *mscan, uint32_t n,
                            uint32_t carry_max, ChunkTail *t) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t->loci = lidx[n - 1];
        t->entries = eoff[n - 1];
        t->max_pos = max(carry_max, mscan[n - 1]);
    }
}

__global__ void first_last(const uint64_t *__restrict__ off, const uint32_t *__restrict__ rid, uint64_t l0,
                           uint32_t n_loci, uint32_t *first, uint32_t *last) {
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    const uint32_t n_waves = gridDim.x * blockDim.x / kWave;
    for (uint32_t l = wave; l < n_loci; l += n_waves) {
        const uint64_t b = off[l0 + l], e = off[l0 + l + 1];
        for (uint64_t j = b + lane; j < e; j += kWave) {
            const uint32_t id = rid[j];
            atomicMin(&first[id], l);
            atomicMax(&last[id], l);
        }
    }
}

__global__ void span_table(const uint32_t *__restrict__ pos, uint64_t l0, const uint32_t *__restrict__ first,
                           const uint32_t *__restrict__ last, uint32_t table_n, FileState *st) {
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < table_n; i += gridDim.x * blockDim.x) {
        const uint32_t f = first[i];
        if (f != 0xFFFFFFFFu) m = max(m, pos[l0 + last[i]] - pos[l0 + f]);  // u32: wraps like the host
    }
    m = wave_max(m);
    if (threadIdx.x % kWave == 0 && m) atomicMax(&st->max_span, m);
}

__global__ void span_keys(const uint64_t *__restrict__ off, const uint32_t *__restrict__ rid, uint64_t l0,
                          uint32_t n_loci, uint64_t e0, uint64_t *__restrict__ keys) {
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    const uint32_t n_waves = gridDim.x * blockDim.x / kWave;
    for (uint32_t l = wave; l < n_loci; l += n_waves) {
        const uint64_t b = off[l0 + l], e = off[l0 + l + 1];
        for (uint64_t j = b + lane; j < e; j += kWave) keys[j - e0] = uint64_t(rid[j]) << 32 | l;
    }
}

// keys sorted by (read id, locus index): a read id's first appearance in file order is its segment's first key,
// its last appearance the segment's last key
__global__ void span_segments(const uint32_t *__restrict__ pos, uint64_t l0, const uint64_t *__restrict__ keys,
                              uint64_t n, FileState *st) {
    uint32_t m = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        if (i + 1 < n && (keys[i + 1] >> 32) == (k >> 32)) continue;
        const uint64_t lo_key = k & 0xFFFFFFFF00000000ull;
        uint64_t lo = 0, hi = i;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (keys[mid] < lo_key) lo = mid + 1;
            else hi = mid;
        }
        m = max(m, pos[l0 + uint32_t(k)] - pos[l0 + uint32_t(keys[lo])]);
    }
    m = wave_max(m);
    if (threadIdx.x % kWave == 0 && m) atomicMax(&st->max_span, m);
}

}  // namespace

size_t scan_bytes(uint64_t n) {
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, n);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, n);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, c, (const uint32_t *)nullptr, (uint32_t *)nullptr, MaxOp(), n);
    return std::max(a, std::max(b, c));
}

size_t sort_bytes(uint64_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, n, 0, 64);
    return b;
}

hipError_t decode_chunk(const Chunk &c, const ChunkScratch &w, uint32_t max_coverage, const uint32_t *d_positions,
                        uint64_t n_positions, uint32_t carry_max, uint64_t l_base, uint64_t e_base,
                        const uint16_t *d_id_to_group, uint32_t n_ids, uint32_t *pos_out, uint64_t *off_out,
                        uint32_t *rid_out, uint16_t *idb_out, FileState *st, ChunkTail *tail, hipStream_t s) {
    if (c.n == 0) return hipSuccess;
    const unsigned g = blocks_for(c.n);
    heads<<<g, kBlock, 0, s>>>(c.bytes, c.rec_off, c.n, max_coverage, w.pos, w.cov, w.mval);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = w.tmp_bytes;
    e = hipcub::DeviceScan::InclusiveScan(w.tmp, bytes, w.mval, w.mscan, MaxOp(), c.n, s);
    if (e != hipSuccess) return e;
    keep_flags<<<g, kBlock, 0, s>>>(w.pos, w.cov, w.mscan, c.n, carry_max, d_positions, n_positions, w.keep, w.cnt,
                                    st);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = w.tmp_bytes;
    if ((e = hipcub::DeviceScan::InclusiveSum(w.tmp, bytes, w.keep, w.lidx, c.n, s)) != hipSuccess) return e;
    bytes = w.tmp_bytes;
    if ((e = hipcub::DeviceScan::InclusiveSum(w.tmp, bytes, w.cnt, w.eoff, c.n, s)) != hipSuccess) return e;
    gather<<<blocks_for((uint64_t)c.n * kWave), kBlock, 0, s>>>(c, w.pos, w.cov, w.keep, w.lidx, w.eoff, l_base,
                                                                e_base, d_id_to_group, n_ids, pos_out, off_out,
                                                                rid_out, idb_out, st);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tail_kernel<<<1, kWave, 0, s>>>(w.lidx, w.eoff, w.mscan, c.n, carry_max, tail);
    return hipGetLastError();
}

hipError_t spans_dense(const uint32_t *pos, const uint64_t *off, const uint32_t *rid, uint64_t l0, uint32_t n_loci,
                       uint32_t *first, uint32_t *last, uint32_t table_n, FileState *st, hipStream_t s) {
    hipError_t e = hipMemsetAsync(first, 0xFF, (size_t)table_n * 4, s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(last, 0, (size_t)table_n * 4, s)) != hipSuccess) return e;
    if (n_loci) {
        first_last<<<blocks_for((uint64_t)n_loci * kWave), kBlock, 0, s>>>(off, rid, l0, n_loci, first, last);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    span_table<<<blocks_for(table_n), kBlock, 0, s>>>(pos, l0, first, last, table_n, st);
    return hipGetLastError();
}

hipError_t spans_sparse(const uint32_t *pos, const uint64_t *off, const uint32_t *rid, uint64_t l0, uint32_t n_loci,
                        uint64_t e0, uint64_t n_entries, uint64_t *keys, void *tmp, size_t tmp_bytes,
                        FileState *st, hipStream_t s) {
    if (n_entries == 0) return hipSuccess;
    span_keys<<<blocks_for((uint64_t)n_loci * kWave), kBlock, 0, s>>>(off, rid, l0, n_loci, e0, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = tmp_bytes;
    e = hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys, keys + n_entries, n_entries, 0, 64, s);
    if (e != hipSuccess) return e;
    span_segments<<<blocks_for(n_entries), kBlock, 0, s>>>(pos, l0, keys + n_entries, n_entries, st);
    return hipGetLastError();
}

}  // namespace pileup
}  // namespace secedo
