// tabix_kernels.hip -- the line pass behind a .tbi index (gfx950): the lines of VCF texts in HBM found, their columns
// read where they lie, and the run heads, touched windows and name changes that tabix_build.hpp needs emitted in line
// order. The scheme is bam_index_kernels.hip's (a key, its inclusive max scan, flags, exclusive scans, an emit), with a
// line table in front since a text has no record lengths to hop along.
//   1. k_file_bits, k_mark   a thread per 16 text bytes (one aligned 16-byte load): the line starts (the range's first
//                        byte, a byte behind '\n', a file's first byte: a bit map the files of the range set) and, of
//                        those, the data lines (first byte neither '#' nor '\n'), counted per chunk as one 64-bit pair.
//   2. exclusive sum of the pairs (hipcub), k_list: the data lines' offsets and line numbers, compacted.
//      k_file_ranks: per file of the range, the lines and data lines in front of it.
//   3. k_parse           a lane per data line: the file (binary search in the bounds), then one walk over the line's
//                        bytes up to the end of column 8, read as aligned dwords and a shift: the name's length, POS,
//                        the length of REF, the first END= key of INFO; beg, end, the bin (reg2bin of
//                        bam_index_build.hpp).
//   4. k_changes         1 where the name differs from the data line in front (the carry line across a range start),
//                        and the order rule; their exclusive sum numbers the (file, name) segments.
//   5. k_keys, inclusive max scan: segment << 16 | last window, so that behind line i the scan holds the last window any
//                        line of the same segment up to i reaches.
//   6. k_flags, two exclusive sums, k_emit, k_tail: as the BAI pass.
// No atomics but the error minimum and the file bits. Nothing per line goes back to the host.
//
// Reads are bounded: every byte a kernel names lies in [a, a + n) of the range or is the carry line's name, inside the
// text; the aligned loads around them reach at most 15 bytes past either end of the text (kTextSlack). Every table index
// is below the count the scans gave: the window counts and their sum are 64 bits wide and the host refuses a range whose
// total passes its cap before k_emit runs, so the sum that sizes the window buffer cannot have wrapped. The kernels hold
// no arrays, so nothing goes to scratch.
//
// Bound (expected, not measured in isolation): the text is read three times (mark, list, parse) and 0.5 byte of counts
// per text byte is written and scanned; k_parse's lanes walk neighbouring lines, so a wave's loads fall into a few cache
// lines that L2 serves, and the walk is bound by the latency of dependent dword loads per lane, not by HBM.
#include "tabix_kernels.hpp"

#include "bam_index_build.hpp"  // reg2bin, kMaxEnd

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace secedo {
namespace tabix {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint64_t kSatPos = 1ull << 40;  // decimal numbers saturate here: far past every limit they are held against

inline unsigned grid(uint64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

// the range seen through 16-byte aligned loads: byte i of the range is t16[shift + i]
struct View {
    const uint8_t *t16;
    uint32_t shift, n, chunks;
    uint64_t a;
};

View view_of(const Text &t, const Range &r) {
    const uint32_t shift = uint32_t((reinterpret_cast<uintptr_t>(t.text) + r.a) & 15);
    return View{t.text + r.a - shift, shift, r.n, range_chunks(t, r), r.a};
}

// the text through aligned dwords: byte `at` (a text offset) is word[(gshift + at) >> 2]
struct Words {
    const uint32_t *w;
    uint32_t gshift;
};

Words words_of(const Text &t) {
    const uint32_t g = uint32_t(reinterpret_cast<uintptr_t>(t.text) & 3);
    return Words{reinterpret_cast<const uint32_t *>(t.text - g), g};
}

struct Reader {
    const uint32_t *w;
    uint64_t at = ~0ull;
    uint32_t cur = 0;
    __device__ explicit Reader(const uint32_t *words) : w(words) {}
    __device__ __forceinline__ uint32_t byte(uint64_t i) {
        if (i >> 2 != at) {
            at = i >> 2;
            cur = w[at];
        }
        return (cur >> (8 * (uint32_t(i) & 3))) & 0xFF;
    }
};

// bit k of *start: byte 16 c + k of the view starts a line; of *data: it starts a data line
__device__ __forceinline__ void chunk_masks(const View &v, const uint32_t *__restrict__ file_bits, uint32_t c,
                                            uint32_t *start, uint32_t *data) {
    const uint4 q = *reinterpret_cast<const uint4 *>(v.t16 + 16ull * c);
    const uint32_t word[4] = {q.x, q.y, q.z, q.w};
    uint32_t nl = 0, hash = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t b = (word[k >> 2] >> (8 * (k & 3))) & 0xFF;
        nl |= uint32_t(b == '\n') << k;
        hash |= uint32_t(b == '#') << k;
    }
    uint32_t st = (nl << 1) & 0xFFFF;
    if (c) st |= uint32_t(v.t16[16ull * c - 1] == '\n');
    else st |= 1u << v.shift;
    st |= (file_bits[c >> 1] >> (16 * (c & 1))) & 0xFFFF;
    // the bits of the range: view bytes [shift, shift + n)
    const uint64_t lo = v.shift, hi = uint64_t(v.shift) + v.n, b0 = 16ull * c;
    uint32_t valid = 0xFFFF;
    if (b0 < lo) valid &= 0xFFFFu << (lo - b0);
    if (b0 + 16 > hi) valid &= hi > b0 ? 0xFFFFu >> (b0 + 16 - hi) : 0u;
    st &= valid;
    *start = st;
    *data = st & ~hash & ~nl;
}

__global__ void __launch_bounds__(kBlock) k_file_bits(View v, const uint64_t *__restrict__ file_off, uint32_t f_lo,
                                                      uint32_t f_hi, uint32_t *file_bits) {
    const uint32_t f = f_lo + blockIdx.x * kBlock + threadIdx.x;
    if (f > f_hi) return;
    const uint64_t o = file_off[f];
    if (o >= file_off[f + 1] || o <= v.a || o - v.a >= v.n) return;  // empty, or its first byte is not inside
    const uint64_t bit = v.shift + (o - v.a);
    atomicOr(&file_bits[bit >> 5], 1u << (bit & 31));
}

__global__ void __launch_bounds__(kBlock) k_mark(View v, const uint32_t *__restrict__ file_bits, uint64_t *cnt) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c > v.chunks) return;
    if (c == v.chunks) {  // the scan's last element
        cnt[c] = 0;
        return;
    }
    uint32_t st, data;
    chunk_masks(v, file_bits, c, &st, &data);
    cnt[c] = uint64_t(__popc(st)) | uint64_t(__popc(data)) << 32;
}

__global__ void __launch_bounds__(kBlock) k_list(View v, const uint32_t *__restrict__ file_bits,
                                                 const uint64_t *__restrict__ scan, uint32_t *start, uint32_t *line) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= v.chunks) return;
    uint32_t st, data;
    chunk_masks(v, file_bits, c, &st, &data);
    const uint64_t before = scan[c];
    uint32_t d = uint32_t(before >> 32);
    while (data) {
        const uint32_t k = uint32_t(__ffs(int(data))) - 1;
        data &= data - 1;
        start[d] = 16 * c + k - v.shift;
        line[d] = uint32_t(before) + uint32_t(__popc(st & ((1u << k) - 1)));
        ++d;
    }
}

// lines | data lines << 32 in front of byte p of the range, p <= n
__device__ __forceinline__ uint64_t rank_at(const View &v, const uint32_t *file_bits, const uint64_t *scan, uint64_t p) {
    if (p >= v.n) return scan[v.chunks];
    const uint64_t at = v.shift + p;
    const uint32_t c = uint32_t(at >> 4), k = uint32_t(at & 15);
    uint32_t st, data;
    chunk_masks(v, file_bits, c, &st, &data);
    const uint32_t below = (1u << k) - 1;
    return scan[c] + (uint64_t(__popc(st & below)) | uint64_t(__popc(data & below)) << 32);
}

__global__ void __launch_bounds__(kBlock) k_file_ranks(View v, const uint32_t *__restrict__ file_bits,
                                                       const uint64_t *__restrict__ scan,
                                                       const uint64_t *__restrict__ file_off, uint32_t f_lo,
                                                       uint32_t f_hi, uint32_t *first_line, uint32_t *first_data) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k > f_hi - f_lo) return;
    const uint64_t o = file_off[f_lo + k];
    const uint64_t rank = rank_at(v, file_bits, scan, o > v.a ? o - v.a : 0);
    first_line[k] = uint32_t(rank);
    first_data[k] = uint32_t(rank >> 32);
}

__global__ void __launch_bounds__(kBlock) k_parse(View v, Words tw, const uint64_t *__restrict__ file_off,
                                                  uint32_t f_lo, uint32_t f_hi, uint32_t n_data, Work w) {
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= n_data) return;
    const uint64_t s = v.a + w.start[d];
    // the last file of the range that begins at or before the line
    uint32_t lo = f_lo, hi = f_hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (file_off[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t f = lo;
    const uint64_t limit = min(v.a + uint64_t(v.n), file_off[f + 1]);
    Reader in(tw.w);
    uint32_t col = 0, name_len = 0, pos_digits = 0, pos_bad = 0, ref_len = 0;
    uint32_t k = 0, end_digits = 0, end_bad = 0;  // INFO: k < 4 matches "END=", 4 its value, 5 another key, 6 done
    uint64_t pos = 0, endv = 0;
    for (uint64_t i = s; i < limit; ++i) {
        const uint32_t c = in.byte(tw.gshift + i);
        if (c == '\n') break;
        if (c == '\t') {
            if (col == 7) break;
            ++col;
            continue;
        }
        if (col == 0) {
            ++name_len;
        } else if (col == 1) {
            if (c >= '0' && c <= '9') {
                ++pos_digits;
                pos = min(pos * 10 + (c - '0'), kSatPos);
            } else {
                pos_bad = 1;
            }
        } else if (col == 3) {
            ++ref_len;
        } else if (col == 7) {
            if (k == 6) break;
            if (c == ';') {
                k = k == 4 ? 6 : 0;
            } else if (k < 4) {
                k = c == ((0x3D444E45u >> (8 * k)) & 0xFF) ? k + 1 : 5;  // "END="
            } else if (k == 4) {
                if (c >= '0' && c <= '9') {
                    ++end_digits;
                    endv = min(endv * 10 + (c - '0'), kSatPos);
                } else {
                    end_bad = 1;
                }
            }
        }
    }
    uint32_t err = 0;
    if (col == 0) err = kErrColumns;
    else if (!pos_digits || pos_bad) err = kErrPos;
    if (err) pos = 0;
    uint64_t beg = pos ? pos - 1 : 0;
    uint64_t end = beg + ref_len;
    if ((k == 4 || k == 6) && end_digits && !end_bad && endv > beg) end = endv;
    if (end <= beg) end = beg + 1;
    if (end > bamindexbuild::kMaxEnd) {
        if (!err) err = kErrEnd;
        end = bamindexbuild::kMaxEnd;
        if (beg >= end) beg = end - 1;
    }
    if (err) atomicMin(reinterpret_cast<unsigned long long *>(w.err), (unsigned long long)d << 8 | err);
    w.file[d] = f;
    w.name_len[d] = name_len;
    w.pos[d] = pos;
    w.beg[d] = uint32_t(beg);
    w.end[d] = uint32_t(end);
    w.bin[d] = bamindexbuild::reg2bin(beg, end);
}

__global__ void __launch_bounds__(kBlock) k_changes(View v, Words tw, Carry carry, uint32_t n_data, Work w) {
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d > n_data) return;
    if (d == n_data) {
        w.change[d] = 0;
        return;
    }
    const bool have = d ? true : carry.valid != 0;
    const uint32_t p_file = d ? w.file[d - 1] : carry.file, p_len = d ? w.name_len[d - 1] : carry.name_len;
    const uint64_t p_at = d ? v.a + w.start[d - 1] : carry.name_at, p_pos = d ? w.pos[d - 1] : carry.pos;
    const uint32_t len = w.name_len[d];
    bool same = have && p_file == w.file[d] && p_len == len;
    if (same) {
        Reader x(tw.w), y(tw.w);
        const uint64_t at = v.a + w.start[d];
        for (uint32_t k = 0; k < len && same; ++k) same = x.byte(tw.gshift + p_at + k) == y.byte(tw.gshift + at + k);
    }
    if (same && w.pos[d] < p_pos)
        atomicMin(reinterpret_cast<unsigned long long *>(w.err), (unsigned long long)d << 8 | kErrOrder);
    w.change[d] = !same;
}

__global__ void __launch_bounds__(kBlock) k_keys(uint32_t n_data, Work w) {
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= n_data) return;
    w.key[d] = uint64_t(w.seg_ex[d] + w.change[d]) << 16 | ((w.end[d] - 1) >> 14);
}

// the windows data line d is the first of its segment and range to overlap: [*lo, *hi], none if *lo > *hi
__device__ __forceinline__ void first_windows(const Work &w, uint32_t d, uint32_t *lo, uint32_t *hi) {
    const uint64_t key = w.key[d];
    *hi = uint32_t(key & 0xFFFF);
    uint32_t s = min(w.beg[d] >> 14, *hi);
    if (d) {
        const uint64_t reach = w.key_max[d - 1];
        if (reach >> 16 == key >> 16) s = max(s, uint32_t(reach & 0xFFFF) + 1);
    }
    *lo = s;
}

__global__ void __launch_bounds__(kBlock) k_flags(uint32_t n_data, Work w) {
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d > n_data) return;
    if (d == n_data) {
        w.head[d] = 0;
        w.n_win[d] = 0;
        return;
    }
    w.head[d] = !d || w.change[d] || w.bin[d] != w.bin[d - 1];
    uint32_t lo, hi;
    first_windows(w, d, &lo, &hi);
    w.n_win[d] = lo <= hi ? uint64_t(hi - lo + 1) : 0;
}

__global__ void __launch_bounds__(kBlock) k_emit(View v, const uint64_t *__restrict__ file_off, uint32_t f_lo,
                                                 uint32_t n_data, Work w, Head *__restrict__ heads,
                                                 Win *__restrict__ wins, Change *__restrict__ changes) {
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= n_data) return;
    const uint32_t f = w.file[d], seg = w.seg_ex[d] + w.change[d];
    const uint64_t at = v.a + w.start[d], off = at - file_off[f];
    if (w.change[d]) changes[w.seg_ex[d]] = Change{at, w.name_len[d], f, w.line[d] - w.first_line[f - f_lo], 0};
    if (w.head[d]) heads[w.head_scan[d]] = Head{off, f, seg, w.bin[d], d - w.first_data[f - f_lo]};
    if (!w.n_win[d]) return;
    uint32_t lo, hi;
    first_windows(w, d, &lo, &hi);
    Win *dst = wins + w.n_win_scan[d];
    for (uint32_t x = lo; x <= hi; ++x) dst[x - lo] = Win{off, f, seg, x, 0};
}

__global__ void k_tail(View v, Range r, Carry carry, uint32_t n_data, Work w) {
    if (blockIdx.x || threadIdx.x) return;
    Tail t{};
    t.err = *w.err;
    if (t.err != kNoErr) {
        const uint32_t d = uint32_t(t.err >> 8);
        t.err_file = w.file[d];
        t.err_line = w.line[d] - w.first_line[t.err_file - r.f_lo];
    }
    t.n_heads = w.head_scan[n_data];
    t.n_wins = w.n_win_scan[n_data];
    t.n_changes = w.seg_ex[n_data];
    t.carry = carry;
    if (n_data) {
        const uint32_t d = n_data - 1;
        t.carry = Carry{v.a + w.start[d], w.pos[d], w.name_len[d], w.file[d], 1, 0};
    }
    *w.tail = t;
}

__global__ void __launch_bounds__(kBlock) k_gather_names(Words tw, const uint64_t *__restrict__ name_at,
                                                         const uint32_t *__restrict__ len,
                                                         const uint64_t *__restrict__ out_at, uint32_t n, uint8_t *out) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    Reader in(tw.w);
    for (uint32_t j = 0; j < len[k]; ++j) out[out_at[k] + j] = uint8_t(in.byte(tw.gshift + name_at[k] + j));
}

#define TABIX_LAUNCHED()                    \
    do {                                    \
        const hipError_t e_ = hipGetLastError(); \
        if (e_ != hipSuccess) return e_;    \
    } while (0)

hipError_t sum32(const Work &w, const uint32_t *in, uint32_t *out, uint64_t n, hipStream_t s) {
    size_t bytes = w.scan_bytes;
    return hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, bytes, in, out, n, s);
}

}  // namespace

size_t scan_workspace(uint64_t chunks, uint64_t lines) {
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                           std::max(chunks, lines) + 1);  // the chunk pairs, and the window counts
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, lines + 1);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, c, (const uint64_t *)nullptr, (uint64_t *)nullptr, hipcub::Max(),
                                            lines + 1);
    return std::max(a, std::max(b, c));
}

hipError_t mark_lines(const Text &t, const Range &r, const Work &w, hipStream_t s) {
    const View v = view_of(t, r);
    hipError_t e = hipMemsetAsync(w.file_bits, 0, (size_t(v.chunks) / 2 + 1) * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_file_bits, dim3(grid(uint64_t(r.f_hi - r.f_lo) + 1)), dim3(kBlock), 0, s, v, t.file_off, r.f_lo,
                       r.f_hi, w.file_bits);
    TABIX_LAUNCHED();
    hipLaunchKernelGGL(k_mark, dim3(grid(uint64_t(v.chunks) + 1)), dim3(kBlock), 0, s, v, w.file_bits, w.chunk_cnt);
    TABIX_LAUNCHED();
    size_t bytes = w.scan_bytes;
    return hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, bytes, w.chunk_cnt, w.chunk_scan, uint64_t(v.chunks) + 1, s);
}

hipError_t index_lines(const Text &t, const Range &r, const Carry &carry, uint32_t n_data, const Work &w, hipStream_t s) {
    const View v = view_of(t, r);
    const Words tw = words_of(t);
    const uint32_t n_f = r.f_hi - r.f_lo + 1;
    hipError_t e = hipMemsetAsync(w.err, 0xFF, 8, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_file_ranks, dim3(grid(n_f)), dim3(kBlock), 0, s, v, w.file_bits, w.chunk_scan, t.file_off, r.f_lo,
                       r.f_hi, w.first_line, w.first_data);
    TABIX_LAUNCHED();
    if (n_data) {
        hipLaunchKernelGGL(k_list, dim3(grid(v.chunks)), dim3(kBlock), 0, s, v, w.file_bits, w.chunk_scan, w.start, w.line);
        TABIX_LAUNCHED();
        hipLaunchKernelGGL(k_parse, dim3(grid(n_data)), dim3(kBlock), 0, s, v, tw, t.file_off, r.f_lo, r.f_hi, n_data, w);
        TABIX_LAUNCHED();
    }
    const uint64_t n1 = uint64_t(n_data) + 1;
    hipLaunchKernelGGL(k_changes, dim3(grid(n1)), dim3(kBlock), 0, s, v, tw, carry, n_data, w);
    TABIX_LAUNCHED();
    if ((e = sum32(w, w.change, w.seg_ex, n1, s)) != hipSuccess) return e;
    if (n_data) {
        hipLaunchKernelGGL(k_keys, dim3(grid(n_data)), dim3(kBlock), 0, s, n_data, w);
        TABIX_LAUNCHED();
        size_t bytes = w.scan_bytes;
        e = hipcub::DeviceScan::InclusiveScan(w.scan_tmp, bytes, w.key, w.key_max, hipcub::Max(), uint64_t(n_data), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_flags, dim3(grid(n1)), dim3(kBlock), 0, s, n_data, w);
    TABIX_LAUNCHED();
    if ((e = sum32(w, w.head, w.head_scan, n1, s)) != hipSuccess) return e;
    {  // 64 bits: the total can pass 2^32 on a small text
        size_t bytes = w.scan_bytes;
        if ((e = hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, bytes, w.n_win, w.n_win_scan, n1, s)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_tail, dim3(1), dim3(64), 0, s, v, r, carry, n_data, w);
    return hipGetLastError();
}

hipError_t emit(const Text &t, const Range &r, uint32_t n_data, const Work &w, Head *d_heads, Win *d_wins,
                Change *d_changes, hipStream_t s) {
    if (!n_data) return hipSuccess;
    hipLaunchKernelGGL(k_emit, dim3(grid(n_data)), dim3(kBlock), 0, s, view_of(t, r), t.file_off, r.f_lo, n_data, w,
                       d_heads, d_wins, d_changes);
    return hipGetLastError();
}

hipError_t gather_names(const Text &t, const uint64_t *d_name_at, const uint32_t *d_len, const uint64_t *d_out_at,
                        uint32_t n, uint8_t *d_out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_gather_names, dim3(grid(n)), dim3(kBlock), 0, s, words_of(t), d_name_at, d_len, d_out_at, n, d_out);
    return hipGetLastError();
}

}  // namespace tabix
}  // namespace secedo
