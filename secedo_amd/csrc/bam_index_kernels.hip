// bam_index_kernels.hip -- what a .bai index needs of the records of one batch of the device walk (gfx950), after
// walk_records has listed them (offset, file, RefID, Position per record; the batch passed the walk's checks and is
// coordinate-sorted, so RefIDs ascend within a file with -1 last and Positions ascend within a RefID).
//   1. k_index_records   one thread per record: flag and n_cigar_op from the inflated bytes, the CIGAR's reference
//                        length, end = pos + max(length, 1), the bin of [max(pos, 0), max(end, 1)), and a key
//                        (the (file, RefID)'s batch-wide number << 16 | the last 16 kb window the record overlaps).
//                        A thread per record, not a lane per CIGAR op: a record has one to a few ops, its 32 fixed
//                        bytes and its ops share one or two cache lines, and the walk's k_records has just pulled them
//                        through L2; spreading three ops over lanes would only add a reduction.
//   2. inclusive max scan of the keys (hipcub). The numbers ascend with the records, so the scan is a segmented one:
//                        behind record i it holds the last window any record of the same (file, RefID) up to i reaches.
//   3. k_index_flags     one thread per record: 1 where (file, RefID, bin, flag 0x4) differs from the record in front
//                        (the first record of a file's bytes in the batch always: the host joins runs across ranges),
//                        and the windows the record is the first to overlap: those past what the records in front of
//                        it reach. Positions ascend, so the first record in file order that overlaps a window is the
//                        one with the lowest offset, and every touched window is counted exactly once.
//   4. exclusive sums of both (the wrappers of bam_kernels.hpp), then k_index_emit: the heads and the windows, each in
//                        record order, with file-linear offsets (buffer offset + the file's delta).
// No atomics but the error minimum, which no valid file reaches: every output position comes from a scan. Nothing per
// record goes back to the host. Reads are bounded: a record the walk accepted lies inside the file's bytes, and the
// CIGAR is read only where it lies inside block_size.
#include "bam_index_kernels.hpp"

#include "bam_index_build.hpp"  // reg2bin, kMaxEnd

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

namespace secedo {
namespace bam {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kUnmappedBit = 1u << 31, kPlacedBit = 1u << 30;  // of meta; the bin is below 2^16

inline unsigned grid(uint64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

__global__ void __launch_bounds__(kBlock) k_index_records(WalkBatch b, WalkRecords r, IndexRecords x, IndexFile *files) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t f = r.file[i];
    const WalkFile &F = b.files[f];
    IndexFile &X = files[f];
    const uint64_t ord = F.rec_base + (i - b.seg_base[F.first_seg]);
    const int32_t ref = r.ref[i], pos = r.pos[i];
    if (ref < 0 || uint32_t(ref) >= X.n_ref) {  // no position: one run behind the file's last reference
        if (ref >= 0) atomicMin(&X.err, (unsigned long long)ord << 8 | kIndexErrRef);
        x.meta[i] = 0;
        x.key[i] = (X.seg_base + X.n_ref) << 16;
        return;
    }
    const uint32_t o = r.off[i];
    const uint32_t bs = ld32(b.buf + o);
    const uint8_t *c = b.buf + o + 4;
    const uint32_t l_name = c[8], flag = uint32_t(c[14]) | uint32_t(c[15]) << 8;
    uint32_t n_cigar = uint32_t(c[12]) | uint32_t(c[13]) << 8;
    if (32 + l_name + 4ull * n_cigar > bs || uint64_t(o) + 4 + bs > b.buf_bytes) {
        atomicMin(&X.err, (unsigned long long)ord << 8 | kIndexErrSize);
        n_cigar = 0;
    }
    uint64_t len = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t v = ld32(c + 32 + l_name + 4 * k), t = v & 15;
        if (t == 0 || t == 2 || t == 3 || t == 7 || t == 8) len += v >> 4;  // M D N = X
    }
    long long beg = pos < 0 ? 0 : pos;
    long long end = (long long)pos + (long long)(len ? len : 1);
    if (end < 1) end = 1;
    if (end > (long long)bamindexbuild::kMaxEnd) {
        atomicMin(&X.err, (unsigned long long)ord << 8 | kIndexErrEnd);
        end = (long long)bamindexbuild::kMaxEnd;
        if (beg >= end) beg = end - 1;
    }
    x.meta[i] = bamindexbuild::reg2bin(uint64_t(beg), uint64_t(end)) | kPlacedBit | (flag & 4 ? kUnmappedBit : 0);
    x.key[i] = (X.seg_base + uint32_t(ref)) << 16 | uint64_t((end - 1) >> 14);
}

// the windows record i (placed) is the first to overlap: [*lo, *hi], none if *lo > *hi
__device__ __forceinline__ void first_windows(const WalkRecords &r, const IndexRecords &x, uint32_t i, uint32_t local,
                                              uint32_t *lo, uint32_t *hi) {
    const uint64_t key = x.key[i];
    const int32_t pos = r.pos[i];
    *hi = uint32_t(key & 0xFFFF);
    uint32_t s = min(uint32_t(pos < 0 ? 0 : pos) >> 14, *hi);
    if (local) {  // record i - 1 is of the same file
        const uint64_t reach = x.key_max[i - 1];
        if (reach >> 16 == key >> 16) s = max(s, uint32_t(reach & 0xFFFF) + 1);
    }
    *lo = s;
}

__global__ void __launch_bounds__(kBlock) k_index_flags(WalkBatch b, WalkRecords r, IndexRecords x) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > r.n) return;
    if (i == r.n) {  // the scans' last element
        x.head[i] = 0;
        x.n_win[i] = 0;
        return;
    }
    const WalkFile &F = b.files[r.file[i]];
    const uint32_t local = i - b.seg_base[F.first_seg];
    const uint32_t meta = x.meta[i];
    const bool placed = meta & kPlacedBit;
    // records without a position form one run whatever their RefID field holds
    x.head[i] = !local || x.meta[i - 1] != meta || (placed && r.ref[i - 1] != r.ref[i]);
    uint32_t lo = 1, hi = 0;
    if (placed) first_windows(r, x, i, local, &lo, &hi);
    x.n_win[i] = lo <= hi ? hi - lo + 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_index_emit(WalkBatch b, WalkRecords r, IndexRecords x,
                                                       const IndexFile *__restrict__ files,
                                                       IndexHead *__restrict__ heads, IndexWin *__restrict__ wins) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t f = r.file[i];
    const WalkFile &F = b.files[f];
    const uint32_t local = i - b.seg_base[F.first_seg];
    const uint32_t meta = x.meta[i];
    const bool placed = meta & kPlacedBit;
    const uint64_t lin = uint64_t((long long)r.off[i] + files[f].delta);
    const int32_t ref = placed ? r.ref[i] : -1;
    if (x.head[i])
        heads[x.head_scan[i]] = IndexHead{lin, F.rec_base + local, ref, meta & 0xFFFF, f, meta & kUnmappedBit ? 1u : 0u};
    const uint64_t n = x.n_win[i];
    if (!n) return;
    uint32_t lo, hi;
    first_windows(r, x, i, local, &lo, &hi);
    IndexWin *dst = wins + x.n_win_scan[i];
    for (uint32_t w = lo; w <= hi; ++w) dst[w - lo] = IndexWin{lin, f, ref, w, 0};
}

}  // namespace

size_t index_scan_bytes(uint64_t n) {
    size_t b = 0;
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, hipcub::Max(), n);
    return b;
}

hipError_t index_records(const WalkBatch &b, const WalkRecords &r, const IndexRecords &x, IndexFile *d_files, void *tmp,
                         size_t tmp_bytes, hipStream_t s) {
    if (!r.n) return hipSuccess;
    hipLaunchKernelGGL(k_index_records, dim3(grid(r.n)), dim3(kBlock), 0, s, b, r, x, d_files);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, x.key, x.key_max, hipcub::Max(), uint64_t(r.n), s);
}

hipError_t index_flags(const WalkBatch &b, const WalkRecords &r, const IndexRecords &x, hipStream_t s) {
    hipLaunchKernelGGL(k_index_flags, dim3(grid(uint64_t(r.n) + 1)), dim3(kBlock), 0, s, b, r, x);
    return hipGetLastError();
}

hipError_t index_emit(const WalkBatch &b, const WalkRecords &r, const IndexRecords &x, const IndexFile *d_files,
                      IndexHead *d_heads, IndexWin *d_wins, hipStream_t s) {
    if (!r.n) return hipSuccess;
    hipLaunchKernelGGL(k_index_emit, dim3(grid(r.n)), dim3(kBlock), 0, s, b, r, x, d_files, d_heads, d_wins);
    return hipGetLastError();
}

}  // namespace bam
}  // namespace secedo
