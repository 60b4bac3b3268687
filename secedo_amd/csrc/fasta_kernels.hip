// fasta_kernels.hip -- a range of FASTA text in HBM -> one code byte per base and a table of its header lines, and
// the gather of the per-locus reference genotypes from those codes (gfx950). The text never visits the host.
//
// Whether a byte is a base depends on the role of its line, and a line's role on the line before (fasta_lines.hpp):
// a five-state machine over the bytes. Each lane takes one 16-byte vector of text. Three passes and two scans:
//   k_transfer   the chunk as a function entry state -> exit state (5 x 3 bits), for all five entry states at once
//   scan         the composition of the functions of all chunks before (hipCUB, an associative non-commutative op)
//   k_count      the chunk walked from its now known entry state: its bases and its header starts
//   scan         exclusive sums of both counts, packed in one u64
//   k_emit       the chunk walked again: codes[ordinal] = CharToInt(base); start, end, byte 1 and sequence ordinal of
//                each header line into its slot; the last chunk leaves the totals and the exit state
// Every index is bounded by the range's length, the slot capacity or the locus count before it is used. Stores are
// plain vector stores; no loop runs longer than 16 bytes or log2(n_chr) steps.
#include "fasta_kernels.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

namespace secedo {
namespace fasta {
namespace {

constexpr uint32_t kBlock = 256;

// Bytes [base, base + 16) of the range in two registers pairs, the rest (the one-byte look-ahead past a chunk) from HBM
struct ChunkText {
    const uint8_t *g;
    uint32_t base;
    uint64_t lo, hi;
    __device__ ChunkText(const uint8_t *text, uint32_t len, uint32_t chunk) : g(text), base(chunk * kChunk), lo(0), hi(0) {
        if (base + kChunk <= len) {
            const uint4 x = *reinterpret_cast<const uint4 *>(text + base);
            lo = uint64_t(x.y) << 32 | x.x;
            hi = uint64_t(x.w) << 32 | x.z;
        } else {
            for (uint32_t k = 0; base + k < len; ++k) {
                const uint64_t b = uint64_t(text[base + k]) << ((k & 7) * 8);
                if (k < 8) lo |= b;
                else hi |= b;
            }
        }
    }
    __device__ uint8_t operator[](uint32_t i) const {
        const uint32_t o = i - base;
        if (o >= kChunk) return g[i];
        return uint8_t((o < 8 ? lo : hi) >> ((o & 7) * 8));
    }
};

__device__ inline uint32_t chunk_bytes(uint32_t len, uint32_t chunk) { return min(kChunk, len - chunk * kChunk); }

__global__ __launch_bounds__(kBlock) void k_transfer(const uint8_t *__restrict__ text, uint32_t len, uint32_t chunks,
                                                     Transfer *__restrict__ tf) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= chunks) return;
    const ChunkText t(text, len, j);
    tf[j] = transfer_of(t, j * kChunk, chunk_bytes(len, j));
}

__global__ __launch_bounds__(kBlock) void k_count(const uint8_t *__restrict__ text, uint32_t len, uint32_t chunks,
                                                  uint32_t state, const Transfer *__restrict__ tf_in,
                                                  uint64_t *__restrict__ cnt) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= chunks) return;
    const ChunkText t(text, len, j);
    uint32_t seq = 0, headers = 0;
    walk(t, len, j * kChunk, chunk_bytes(len, j), apply(tf_in[j], state), &seq, &headers, nullptr, nullptr, 0);
    cnt[j] = uint64_t(headers) << 32 | seq;
}

__global__ __launch_bounds__(kBlock) void k_emit(const uint8_t *__restrict__ text, uint32_t len, uint32_t chunks,
                                                 uint32_t state, const Transfer *__restrict__ tf_in,
                                                 const uint64_t *__restrict__ cnt_before, uint8_t *__restrict__ codes,
                                                 RangeTotals *__restrict__ totals, uint32_t cap) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= chunks) return;
    const ChunkText t(text, len, j);
    const uint64_t before = cnt_before[j];
    uint32_t seq = uint32_t(before), headers = uint32_t(before >> 32);
    // seq never passes len: an ordinal counts bytes of the range in front of it
    const uint32_t exit = walk(t, len, j * kChunk, chunk_bytes(len, j), apply(tf_in[j], state), &seq, &headers, codes,
                               slots_of(totals), cap);
    if (j == chunks - 1) *totals = RangeTotals{headers, seq, exit, 0};
}

struct ComposeOp {
    __host__ __device__ Transfer operator()(Transfer a, Transfer b) const { return compose(a, b); }
};

__global__ __launch_bounds__(kBlock) void k_gather(const uint8_t *__restrict__ codes, uint32_t code_off, uint32_t count,
                                                   uint64_t q0, const uint32_t *__restrict__ pos, uint32_t l0,
                                                   uint32_t l1, uint8_t *__restrict__ dst) {
    const uint64_t l = uint64_t(l0) + uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (l >= l1) return;
    const uint64_t p = uint32_t(pos[l] - 1);  // uint32: position 0 wraps
    if (p < q0 || p - q0 >= count) return;
    dst[l] = codes[code_off + uint32_t(p - q0)];
}

// the chromosome of locus l: the last c with chr_off[c] <= l, below n_chr
__device__ inline uint32_t chromosome_of(const uint32_t *chr_off, uint32_t n_chr, uint32_t l) {
    uint32_t lo = 0, hi = n_chr;  // chr_off[lo] <= l < chr_off[hi] for offsets that run from 0 to n_loci
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (chr_off[mid] <= l) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void k_end_init(const uint32_t *__restrict__ chr_off, uint32_t n_chr,
                                                     uint32_t *__restrict__ end) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c < n_chr) end[c] = chr_off[c + 1];
}

__global__ __launch_bounds__(kBlock) void k_end_min(const uint32_t *__restrict__ chr_off, uint32_t n_chr,
                                                    const uint32_t *__restrict__ pos, uint32_t n_loci,
                                                    const uint64_t *__restrict__ len, uint32_t *__restrict__ end) {
    const uint64_t l = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (l >= n_loci) return;
    const uint32_t c = chromosome_of(chr_off, n_chr, uint32_t(l));
    if (uint64_t(uint32_t(pos[l] - 1)) >= len[c]) atomicMin(&end[c], uint32_t(l));
}

__global__ __launch_bounds__(kBlock) void k_locus_ref(const uint32_t *__restrict__ chr_off, uint32_t n_chr,
                                                      uint32_t n_loci, const uint8_t *__restrict__ hap,
                                                      const uint8_t *__restrict__ mat, const uint8_t *__restrict__ pat,
                                                      const uint32_t *__restrict__ end, uint8_t *__restrict__ locus_ref) {
    const uint64_t l = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (l >= n_loci) return;
    const uint32_t c = chromosome_of(chr_off, n_chr, uint32_t(l));
    uint8_t g = 0;
    if (l < end[c]) {
        const uint8_t m = mat[l];
        g = uint8_t(m << 3 | (hap[c] ? m : pat[l]));
    }
    locus_ref[l] = g;
}

inline unsigned blocks(uint64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

}  // namespace

size_t scan_workspace(uint32_t max_len) {
    const int n = int(num_chunks(max_len));
    size_t a = 0, b = 0;
    (void)hipcub::DeviceScan::ExclusiveScan(nullptr, a, (Transfer *)nullptr, (Transfer *)nullptr, ComposeOp(), kIdentity, n);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, n);
    return std::max(a, b);
}

hipError_t parse_range(const uint8_t *d_text, uint32_t len, uint32_t state, const RangeWork &w, hipStream_t s) {
    hipError_t e = hipMemsetAsync(w.totals, 0xFF, table_bytes(w.cap), s);
    if (e != hipSuccess) return e;
    if (len == 0) {
        const RangeTotals t{0, 0, state, 0};
        return hipMemcpyAsync(w.totals, &t, sizeof t, hipMemcpyHostToDevice, s);
    }
    const uint32_t chunks = num_chunks(len);
    hipLaunchKernelGGL(k_transfer, dim3(blocks(chunks)), dim3(kBlock), 0, s, d_text, len, chunks, w.tf);
    size_t bytes = w.scan_bytes;
    e = hipcub::DeviceScan::ExclusiveScan(w.scan_tmp, bytes, w.tf, w.tf_in, ComposeOp(), kIdentity, int(chunks), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_count, dim3(blocks(chunks)), dim3(kBlock), 0, s, d_text, len, chunks, state, w.tf_in, w.cnt);
    bytes = w.scan_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, bytes, w.cnt, w.cnt_before, int(chunks), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_emit, dim3(blocks(chunks)), dim3(kBlock), 0, s, d_text, len, chunks, state, w.tf_in,
                       w.cnt_before, w.codes, w.totals, w.cap);
    return hipGetLastError();
}

hipError_t emit_range(const uint8_t *d_text, uint32_t len, uint32_t state, const RangeWork &w, hipStream_t s) {
    if (len == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(w.totals, 0xFF, table_bytes(w.cap), s);
    if (e != hipSuccess) return e;
    const uint32_t chunks = num_chunks(len);
    hipLaunchKernelGGL(k_emit, dim3(blocks(chunks)), dim3(kBlock), 0, s, d_text, len, chunks, state, w.tf_in,
                       w.cnt_before, w.codes, w.totals, w.cap);
    return hipGetLastError();
}

hipError_t gather(const uint8_t *d_codes, uint32_t code_off, uint32_t count, uint64_t q0, const uint32_t *d_pos,
                  uint32_t l0, uint32_t l1, uint8_t *d_dst, hipStream_t s) {
    if (l1 <= l0 || !count || q0 > UINT32_MAX) return hipSuccess;
    hipLaunchKernelGGL(k_gather, dim3(blocks(l1 - l0)), dim3(kBlock), 0, s, d_codes, code_off, count, q0, d_pos, l0, l1,
                       d_dst);
    return hipGetLastError();
}

hipError_t finish(const uint32_t *d_chr_off, uint32_t n_chr, const uint32_t *d_pos, uint32_t n_loci,
                  const uint64_t *d_len, const uint8_t *d_hap, const uint8_t *d_mat, const uint8_t *d_pat,
                  uint8_t *d_locus_ref, uint32_t *d_end, hipStream_t s) {
    if (!n_chr) return hipSuccess;
    hipLaunchKernelGGL(k_end_init, dim3(blocks(n_chr)), dim3(kBlock), 0, s, d_chr_off, n_chr, d_end);
    if (n_loci) {
        hipLaunchKernelGGL(k_end_min, dim3(blocks(n_loci)), dim3(kBlock), 0, s, d_chr_off, n_chr, d_pos, n_loci, d_len,
                           d_end);
        hipLaunchKernelGGL(k_locus_ref, dim3(blocks(n_loci)), dim3(kBlock), 0, s, d_chr_off, n_chr, n_loci, d_hap, d_mat,
                           d_pat, d_end, d_locus_ref);
    }
    return hipGetLastError();
}

}  // namespace fasta
}  // namespace secedo
