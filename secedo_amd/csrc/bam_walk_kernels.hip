// bam_walk_kernels.hip -- the BAM record walk on gfx950, over bytes bgzf_kernels.hip inflated in HBM: which offsets
// are records, their checks, the records of the requested chromosomes gathered for the host. The decisions are those
// of bam_walk.hpp (shared with the host test); what the host walk of bam_input.cpp reports, this reports.
//
// A batch is the bytes of many files, or one range of one file, in one buffer; a file's bytes are cut into segments,
// one per BGZF member, and start at a record.
//   1. k_place_carries, k_limits   the bytes a file carries in (its header members' tail, or the cut record of the
//                                  range before) go in front of its first member; a member that did not inflate ends
//                                  the file's bytes at its start and is noted for the message.
//   2. k_walk_segments             one wavefront per segment follows the chain from the segment's start through a
//                                  4 KiB window in LDS, staged with 16-byte loads by all lanes and restaged when the
//                                  chain leaves it; every lane follows the same chain, lane 0 lists the offsets.
//   3. k_join                      one thread per file: bam_walk.hpp's join over its segments, serial.
//   4. k_records                   one thread per record: offset, RefID, Position, l_read_name .. l_seq against
//                                  block_size, records per RefID (scan).
//   5. k_order, k_run_ends, k_select   sortedness against the record in front, the first run of each requested
//                                  chromosome (started / done), the negative-position and CIGAR checks on its records.
//   5b. k_span_check               indexed files: per span and requested chromosome, the RefID at the entry, the record
//                                  at the chromosome's start, the records between its start and end, the RefID at
//                                  the span's end (one thread each, binary searches over the file's record offsets).
//   6. k_runs, k_gather            after the scans: the runs' extents, and the taken records' bytes copied by 16
//                                  lanes a record in 16-byte vectors.
// Errors are the minimum of (record of the file << 8 | code) per file. LDS: 4 KiB per wave in pass 2 only, so the
// wave slots, not LDS, bound its occupancy (the inflate kernel's 39.5 KiB allow four waves per CU).
#include "bam_walk_kernels.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace secedo {
namespace bam {
namespace {

using namespace secedo::bamwalk;

constexpr uint32_t kLanes = 64, kBlock = 256;

inline unsigned grid(uint64_t n, uint32_t per = kBlock) { return unsigned((n + per - 1) / per); }

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// the u32 at an offset, through the wave's window in LDS; every lane asks for the same offset
struct WindowReader {
    const uint8_t *buf;
    uint64_t buf_bytes;
    uint8_t *win;
    uint32_t lane, w0 = 0;
    bool loaded = false;
    __device__ WindowReader(const uint8_t *b, uint64_t n, uint8_t *w, uint32_t l) : buf(b), buf_bytes(n), win(w), lane(l) {}
    __device__ uint32_t operator()(uint32_t o) {
        if (!loaded || o < w0 || o - w0 + 8 > kWalkWindow) {
            w0 = o & ~15u;
            loaded = true;
            __syncthreads();
            for (uint32_t v = lane; v < kWalkWindow / 16; v += kLanes) {
                const uint64_t off = uint64_t(w0) + 16 * v;
                uint4 x = make_uint4(0, 0, 0, 0);
                if (off + 16 <= buf_bytes) x = *reinterpret_cast<const uint4 *>(buf + off);
                reinterpret_cast<uint4 *>(win)[v] = x;
            }
            __syncthreads();
        }
        const uint32_t q = o - w0;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(win) + (q >> 2);
        return uint32_t((uint64_t(w[1]) << 32 | w[0]) >> ((q & 3) * 8));
    }
};

struct GlobalReader {
    const uint8_t *buf;
    __device__ uint32_t operator()(uint32_t o) const { return ld32(buf + o); }
};

__global__ void __launch_bounds__(kLanes) k_place_carries(WalkBatch b, const uint8_t *__restrict__ in) {
    const WalkFile &F = b.files[blockIdx.x];
    if (!F.carry_len || !F.n_seg) return;
    uint8_t *dst = b.buf + b.segs[F.first_seg].start;
    const uint8_t *src = in + F.carry_src;
    for (uint32_t i = threadIdx.x; i < F.carry_len; i += kLanes) dst[i] = src[i];
}

__global__ void __launch_bounds__(kBlock) k_limits(WalkBatch b, uint32_t n_members, const BgzfDesc *__restrict__ desc,
                                                   const uint32_t *__restrict__ status) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_members || status[k] == 0) return;
    WalkFile &F = b.files[b.segs[k].file];
    atomicMin(&F.limit, uint32_t(desc[k].out_off));
    atomicMin(&F.bad, (unsigned long long)k << 8 | (status[k] & 0xFF));
}

__global__ void __launch_bounds__(kLanes) k_walk_segments(WalkBatch b) {
    __shared__ __align__(16) uint8_t win[kWalkWindow];
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const Seg sg = b.segs[k];
    const uint32_t data_end = b.files[sg.file].limit;
    const uint32_t end = min(sg.end, data_end);
    SegWalk r{0, sg.start, kExit};
    if (sg.start < end) {
        WindowReader rd(b.buf, b.buf_bytes, win, lane);
        r = walk_segment(rd, sg.start, end, data_end, b.lists + sg.list, lane == 0);
    }
    if (lane == 0) b.walk[k] = r;
}

__global__ void __launch_bounds__(kLanes) k_join(WalkBatch b) {
    const uint32_t f = blockIdx.x * kLanes + threadIdx.x;
    if (f >= b.n_files) return;
    WalkFile &F = b.files[f];
    GlobalReader rd{b.buf};
    const Chain c = join_file(rd, b.segs + F.first_seg, b.walk + F.first_seg, b.lists, b.rewalk, F.n_seg, F.limit,
                              b.join + F.first_seg);
    for (uint32_t k = F.first_seg; k < F.first_seg + F.n_seg; ++k) b.seg_cnt[k] = b.join[k].n_rewalk + b.join[k].n_adopt;
    F.n_rec = c.n;
    F.stop_off = c.stop_off;
    F.rewalked = c.rewalked;
    const uint32_t code = stop_code(c.stop, F.final && F.limit == F.data_end);
    if (code) F.err = min(F.err, (unsigned long long)(F.rec_base + c.n) << 8 | code);
}

// the segment of record i: the last one whose base is <= i
__device__ __forceinline__ uint32_t segment_of(const uint32_t *base, uint32_t n_seg, uint32_t i) {
    uint32_t lo = 0, hi = n_seg;  // base[lo] <= i < base[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t aux_off(const uint8_t *c) {
    const uint32_t l_seq = ld32(c + 16);
    return 32 + uint64_t(c[8]) + 4ull * (uint32_t(c[12]) | uint32_t(c[13]) << 8) + (uint64_t(l_seq) + 1) / 2 + l_seq;
}

__device__ __forceinline__ void note(WalkFile &F, uint64_t local, uint32_t code) {
    atomicMin(&F.err, (unsigned long long)(F.rec_base + local) << 8 | code);
}

__global__ void __launch_bounds__(kBlock) k_records(WalkBatch b, WalkRecords r, unsigned long long *per_ref,
                                                    uint32_t n_ref) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t k = segment_of(b.seg_base, b.n_seg, i);
    const SegJoin j = b.join[k];
    const Seg sg = b.segs[k];
    const uint32_t at = i - b.seg_base[k];
    const uint32_t o = at < j.n_rewalk ? b.rewalk[sg.list + at] : b.lists[sg.list + j.from + (at - j.n_rewalk)];
    WalkFile &F = b.files[sg.file];
    const uint32_t first = b.seg_base[F.first_seg];
    if (i == first) F.first_rec = first;
    const uint8_t *c = b.buf + o + 4;
    const int32_t ref = int32_t(ld32(c)), pos = int32_t(ld32(c + 4));
    r.off[i] = o;
    r.file[i] = sg.file;
    r.ref[i] = ref;
    r.pos[i] = pos;
    if (aux_off(c) > ld32(b.buf + o)) note(F, i - first, kErrLonger);
    if (per_ref) {
        if (ref < 0) atomicAdd(per_ref + n_ref, 1ull);
        else if (uint32_t(ref) < n_ref) atomicAdd(per_ref + ref, 1ull);
    }
}

struct Prev {
    bool has;
    int32_t ref, pos;
};

__device__ __forceinline__ Prev prev_of(const WalkFile &F, const WalkRecords &r, uint32_t i, uint32_t local) {
    if (local) return Prev{true, r.ref[i - 1], r.pos[i - 1]};
    return Prev{F.has_prev != 0, F.prev_ref, F.prev_pos};
}

__global__ void __launch_bounds__(kBlock) k_order(WalkBatch b, WalkRecords r, const uint32_t *__restrict__ chr,
                                                  uint32_t n_chr, WalkRun *runs) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t f = r.file[i];
    WalkFile &F = b.files[f];
    const uint32_t local = i - b.seg_base[F.first_seg];
    const int32_t ref = r.ref[i], pos = r.pos[i];
    const Prev p = prev_of(F, r, i, local);
    if (p.has && sorts_before(ref, pos, p.ref, p.pos)) atomicMin(&F.unsorted, (unsigned long long)(F.rec_base + local));
    if (local + 1 == F.n_rec) F.last_ref = ref, F.last_pos = pos;
    for (uint32_t u = 0; u < n_chr; ++u) {
        const int32_t want = int32_t(chr[u]);
        if (want >= 0 && run_starts(ref == want, p.has, p.ref == want))
            atomicMin(&runs[uint64_t(f) * n_chr + u].first, local + 1);
    }
}

__global__ void __launch_bounds__(kBlock) k_run_ends(WalkBatch b, WalkRecords r, const uint32_t *__restrict__ chr,
                                                     uint32_t n_chr, WalkRun *runs) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t f = r.file[i];
    const WalkFile &F = b.files[f];
    const uint32_t local = i - b.seg_base[F.first_seg];
    const int32_t ref = r.ref[i];
    const Prev p = prev_of(F, r, i, local);
    for (uint32_t u = 0; u < n_chr; ++u) {
        const int32_t want = int32_t(chr[u]);
        WalkRun &run = runs[uint64_t(f) * n_chr + u];
        if (want >= 0 && run_ends(ref == want, p.has, p.ref == want) && local + 1 > run.first)
            atomicMin(&run.last, local + 1);
    }
}

__global__ void __launch_bounds__(kBlock) k_select(WalkBatch b, WalkRecords r, const uint32_t *__restrict__ chr,
                                                   uint32_t n_chr, const WalkRun *__restrict__ runs) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > r.n) return;
    if (i == r.n) {  // the scans' last element
        r.sel[i] = 0;
        r.size[i] = 0;
        return;
    }
    const uint32_t f = r.file[i];
    WalkFile &F = b.files[f];
    const uint32_t local = i - b.seg_base[F.first_seg];
    const int32_t ref = r.ref[i];
    bool take = false;
    for (uint32_t u = 0; u < n_chr; ++u) {
        const WalkRun &run = runs[uint64_t(f) * n_chr + u];
        if (ref >= 0 && uint32_t(ref) == chr[u] && run_takes(local + 1, run.first, run.last)) take = true;
    }
    const uint8_t *rec = b.buf + r.off[i];
    const uint32_t bs = ld32(rec);
    r.sel[i] = take;
    r.size[i] = take ? 4 + uint64_t(bs) : 0;
    if (!take) return;
    if (r.pos[i] < 0) {
        note(F, local, kErrNegative);
        return;
    }
    const uint8_t *c = rec + 4;
    if (aux_off(c) > bs) return;  // k_records reported it; the CIGAR may lie past the record
    const uint32_t l_name = c[8], n_cigar = uint32_t(c[12]) | uint32_t(c[13]) << 8, l_seq = ld32(c + 16);
    uint64_t query = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t v = ld32(c + 32 + l_name + 4 * k), t = v & 15;
        if (t > 8) {
            note(F, local, kErrCigarOp | t);
            return;
        }
        if (t == 0 || t == 1 || t == 4 || t == 7 || t == 8) query += v >> 4;
    }
    if (l_seq > 0 && n_cigar > 0 && query != l_seq) note(F, local, kErrCigarSeq);
}

// index of the first of the ascending offsets off[0, n) that is >= o
__device__ __forceinline__ uint32_t first_at_or_past(const uint32_t *off, uint32_t n, long long o) {
    if (o <= 0) return 0;
    if (o > (long long)UINT32_MAX) return n;
    return lower_bound(off, n, uint32_t(o));
}

// One thread per (file, requested chromosome) of a batch: the index's word on a span against what the walk found.
// Runs after k_records (r.off and r.ref of the file's records, ascending by offset) and k_join (F.n_rec, F.stop_off).
__global__ void __launch_bounds__(kBlock) k_span_check(WalkBatch b, WalkRecords r, uint32_t n_chr,
                                                       SpanCheck *__restrict__ checks) {
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= uint64_t(b.n_files) * n_chr) return;
    SpanCheck c = checks[t];
    if (!(c.flags & kSpanOn)) return;
    const WalkFile &F = b.files[t / n_chr];
    const uint32_t n = uint32_t(F.n_rec);
    const uint32_t first = b.seg_base[F.first_seg];
    const uint32_t *off = r.off + first;
    const long long enter = b.segs[F.first_seg].start;
    c.entry_bad = c.tail_bad = c.start = 0;
    if ((c.flags & kSpanEntry) && c.beg >= enter && c.beg + 8 <= (long long)F.limit)
        c.entry_bad = int32_t(ld32(b.buf + c.beg + 4)) != c.ref;
    const uint32_t i0 = n ? first_at_or_past(off, n, c.beg) : 0, i1 = n ? first_at_or_past(off, n, c.end) : 0;
    c.count = i1 - i0;
    if (c.beg >= enter && c.beg < (long long)F.stop_off)
        c.start = (i0 < n && off[i0] == c.beg && r.ref[first + i0] == c.ref) ? 1 : 2;
    if ((c.flags & kSpanTail) && F.limit == F.data_end && c.end >= enter && c.end + 8 <= (long long)b.buf_bytes)
        c.tail_bad = int32_t(ld32(b.buf + c.end + 4)) == c.ref;
    checks[t] = c;
}

__global__ void __launch_bounds__(kBlock) k_runs(WalkBatch b, WalkRecords r, uint32_t n_chr, WalkRun *runs,
                                                 uint64_t *totals) {
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t == 0) {
        totals[0] = r.sel_scan[r.n];
        totals[1] = r.size_scan[r.n];
    }
    if (t >= uint64_t(b.n_files) * n_chr) return;
    const WalkFile &F = b.files[t / n_chr];
    WalkRun &run = runs[t];
    run.j0 = run.j1 = 0;
    run.b0 = run.b1 = 0;
    if (run.first == kNoRun || !F.n_rec) return;
    const uint32_t first = b.seg_base[F.first_seg];
    const uint32_t i0 = first + (run.first ? run.first - 1 : 0);
    const uint32_t i1 = run.last == kNoRun ? first + uint32_t(F.n_rec) : first + (run.last ? run.last - 1 : 0);
    run.j0 = r.sel_scan[i0];
    run.j1 = r.sel_scan[i1];
    run.b0 = r.size_scan[i0];
    run.b1 = r.size_scan[i1];
}

struct __attribute__((packed, aligned(1))) Vec16 {
    uint32_t w[4];
};

// 16 lanes a record
__global__ void __launch_bounds__(kBlock) k_gather(WalkBatch b, WalkRecords r, uint8_t *__restrict__ out,
                                                   uint64_t *__restrict__ sel_off, int32_t *__restrict__ sel_pos,
                                                   uint64_t *__restrict__ sel_idx) {
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    const uint32_t i = uint32_t(t / 16), lane = uint32_t(t % 16);
    if (i >= r.n || !r.sel[i]) return;
    const uint32_t len = uint32_t(r.size[i]);
    const uint8_t *src = b.buf + r.off[i];
    uint8_t *dst = out + r.size_scan[i];
    for (uint32_t o = lane * 16; o + 16 <= len; o += 256)
        *reinterpret_cast<Vec16 *>(dst + o) = *reinterpret_cast<const Vec16 *>(src + o);
    const uint32_t tail = len & ~15u;
    if (tail + lane < len) dst[tail + lane] = src[tail + lane];
    if (lane == 0) {
        const WalkFile &F = b.files[r.file[i]];
        const uint32_t j = r.sel_scan[i];
        sel_off[j] = r.size_scan[i];
        sel_pos[j] = r.pos[i];
        sel_idx[j] = F.rec_base + (i - b.seg_base[F.first_seg]);
    }
}

}  // namespace

hipError_t walk_prepare(const WalkBatch &b, const uint8_t *d_in, const BgzfDesc *d_desc, const uint32_t *d_status,
                        uint32_t n_members, hipStream_t s) {
    if (b.n_files) hipLaunchKernelGGL(k_place_carries, dim3(b.n_files), dim3(kLanes), 0, s, b, d_in);
    if (n_members) hipLaunchKernelGGL(k_limits, dim3(grid(n_members)), dim3(kBlock), 0, s, b, n_members, d_desc, d_status);
    return hipGetLastError();
}

hipError_t walk_segments(const WalkBatch &b, hipStream_t s) {
    if (b.n_seg) hipLaunchKernelGGL(k_walk_segments, dim3(b.n_seg), dim3(kLanes), 0, s, b);
    if (b.n_files) hipLaunchKernelGGL(k_join, dim3(grid(b.n_files, kLanes)), dim3(kLanes), 0, s, b);
    return hipGetLastError();
}

hipError_t walk_records(const WalkBatch &b, const WalkRecords &r, const uint32_t *d_chr, uint32_t n_chr,
                        WalkRun *d_runs, unsigned long long *d_per_ref, uint32_t n_ref, hipStream_t s) {
    if (r.n) {
        hipLaunchKernelGGL(k_records, dim3(grid(r.n)), dim3(kBlock), 0, s, b, r, d_per_ref, n_ref);
        hipLaunchKernelGGL(k_order, dim3(grid(r.n)), dim3(kBlock), 0, s, b, r, d_chr, n_chr, d_runs);
        if (n_chr) hipLaunchKernelGGL(k_run_ends, dim3(grid(r.n)), dim3(kBlock), 0, s, b, r, d_chr, n_chr, d_runs);
    }
    hipLaunchKernelGGL(k_select, dim3(grid(uint64_t(r.n) + 1)), dim3(kBlock), 0, s, b, r, d_chr, n_chr, d_runs);
    return hipGetLastError();
}

hipError_t walk_span_check(const WalkBatch &b, const WalkRecords &r, uint32_t n_chr, SpanCheck *d_checks,
                           hipStream_t s) {
    const uint64_t n = uint64_t(b.n_files) * n_chr;
    if (n) hipLaunchKernelGGL(k_span_check, dim3(grid(n)), dim3(kBlock), 0, s, b, r, n_chr, d_checks);
    return hipGetLastError();
}

hipError_t walk_runs(const WalkBatch &b, const WalkRecords &r, uint32_t n_chr, WalkRun *d_runs, uint64_t *d_totals,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_runs, dim3(grid(std::max<uint64_t>(uint64_t(b.n_files) * n_chr, 1))), dim3(kBlock), 0, s, b, r,
                       n_chr, d_runs, d_totals);
    return hipGetLastError();
}

hipError_t walk_gather(const WalkBatch &b, const WalkRecords &r, uint8_t *d_out, uint64_t *d_sel_off,
                       int32_t *d_sel_pos, uint64_t *d_sel_idx, hipStream_t s) {
    if (!r.n) return hipSuccess;
    hipLaunchKernelGGL(k_gather, dim3(grid(uint64_t(r.n) * 16)), dim3(kBlock), 0, s, b, r, d_out, d_sel_off, d_sel_pos,
                       d_sel_idx);
    return hipGetLastError();
}

}  // namespace bam
}  // namespace secedo
