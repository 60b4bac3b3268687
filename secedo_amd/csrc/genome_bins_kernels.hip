// genome_bins_kernels.hip -- the genome composition per bin (include/secedo_variant.h), counted from the
// FASTA text where it lies in HBM (gfx950).
//
// The contract, restated. Lines and their roles are those of fasta_lines.hpp (step): line 0 is a header, a '>' line
// directly after a header is sequence. Every header starts a contig, whose sequence is the sequence bytes up to the
// next header; its name is the header's bytes after its first, up to the first space, tab, '\r' or the line's end.
// Selected contig k of length L_k has ceil(L_k / S) bins [bS, min((b + 1)S, L_k)), numbered in selection order
// (bam_depth.hpp's layout). Per bin six u32 from the raw byte of every sequence byte in it: a (A a), c (C c), g (G g),
// t (T t U u), other (every other byte: N, IUPAC codes, a '\r' inside a sequence line, a '>' the line rule reads as
// sequence) and masked ('a'..'z', in addition to the byte's class). a + c + g + t + other == end - start, and only
// integer sums exist, so the table does not depend on the order of execution.
//
// k_compose reads a range's text a second time, after the scans of fasta_kernels.hip gave every 16-byte chunk its
// entry state (tf_in) and the sequence ordinal in front of it (cnt_before). A lane takes one chunk with one vector
// load, walks it from its entry state and maps each sequence byte's ordinal to (contig, position) through the piece
// table the host built from the range's header slots: one binary search and one division per lane, a step per byte
// after that. A wave's 1 KiB of text is at most 1024 consecutive positions, one or two bins at any realistic S, so the
// adds are reduced before they reach HBM: a lane's first run of bytes in one bin is summed over the wave's lanes that
// share the bin (found by ballot, packed 16-bit partial sums, a butterfly of shuffles), the sums of a wave's first
// bin then over the workgroup's 16 waves through LDS, and one lane per bin and class issues the atomic, zeros skipped.
// Many workgroups adding to one address is the slow shape of global atomics (MI355X_MICROARCH.md, 'Global float
// atomics', row 'contention'); a bin of S positions receives about 6 * S / 16384 adds this way. A lane's further runs
// (a bin or contig boundary inside its 16 bytes; every byte when S < 16) are added directly: correct, not fast.
// Every table index is checked against table_bins before the add; no loop runs longer than 16 bytes, the pieces of a
// range or the distinct bins of a wave.
#include "genome_bins_kernels.hpp"

#include "text_sink.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

namespace secedo {
namespace genomebins {
namespace {

using namespace secedo::fasta;

constexpr uint32_t kBlock = 256;
constexpr uint32_t kComposeBlock = 1024;  // 16 KiB of text per workgroup
constexpr uint32_t kWaves = kComposeBlock / 64;
constexpr uint64_t kNoBin = ~0ull;

// class counts of at most 16 * 64 * 16 bytes in 16-bit fields: a, c, g, t in `acgt`, other and masked in `om`
struct Packed {
    uint64_t acgt = 0;
    uint32_t om = 0;
    __device__ void add(uint8_t b) {
        const uint32_t k = byte_class(b);
        if (k < 4) acgt += 1ull << (16 * k);
        else om += 1;
        if (byte_masked(b)) om += 1u << 16;
    }
    __device__ uint32_t field(uint32_t k) const {
        return k < 4 ? uint32_t(acgt >> (16 * k)) & 0xFFFFu : (om >> (16 * (k - 4))) & 0xFFFFu;
    }
};

__device__ inline void add_field(uint32_t *table, uint64_t table_bins, uint64_t bin, uint32_t k, uint32_t v) {
    if (v && bin < table_bins) atomicAdd(&table[bin * kColumns + k], v);
}

__device__ inline void add_row(uint32_t *table, uint64_t table_bins, uint64_t bin, const Packed &p) {
    for (uint32_t k = 0; k < kColumns; ++k) add_field(table, table_bins, bin, k, p.field(k));
}

__device__ inline uint64_t shfl64(uint64_t v, int lane) {
    const uint32_t lo = __shfl(uint32_t(v), lane, 64), hi = __shfl(uint32_t(v >> 32), lane, 64);
    return uint64_t(hi) << 32 | lo;
}
__device__ inline uint64_t shfl_xor64(uint64_t v, int mask) {
    const uint32_t lo = __shfl_xor(uint32_t(v), mask, 64), hi = __shfl_xor(uint32_t(v >> 32), mask, 64);
    return uint64_t(hi) << 32 | lo;
}

// The (bin, p) of the wave's lanes with `valid`, summed per distinct bin; every lane of the wave calls it. With
// `keep`, the sums of the lowest valid lane's bin come back in every lane's (*kept_bin, *kept) instead of being added;
// all other sums are added to the table by lanes 0..5, one class each.
__device__ inline void wave_sums(uint64_t bin, const Packed &p, bool valid, bool keep, uint64_t *kept_bin, Packed *kept,
                                 uint32_t *table, uint64_t table_bins) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long active = __ballot(valid);  // uniform over the wave, so is the loop
    while (active) {
        const int leader = __ffsll(active) - 1;
        const uint64_t b = shfl64(bin, leader);
        const bool mine = valid && bin == b;
        Packed sum;
        sum.acgt = mine ? p.acgt : 0;
        sum.om = mine ? p.om : 0;
        for (int m = 32; m; m >>= 1) {
            sum.acgt += shfl_xor64(sum.acgt, m);
            sum.om += __shfl_xor(sum.om, m, 64);
        }
        if (keep) {
            *kept_bin = b;
            *kept = sum;
            keep = false;
        } else if (lane < kColumns) {
            add_field(table, table_bins, b, lane, sum.field(lane));
        }
        active &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(kComposeBlock) void k_compose(const uint8_t *__restrict__ text, uint32_t len,
                                                           uint32_t chunks, uint32_t state,
                                                           const Transfer *__restrict__ tf_in,
                                                           const uint64_t *__restrict__ cnt_before,
                                                           const Piece *__restrict__ pieces, uint32_t n_pieces,
                                                           uint32_t S, uint32_t *__restrict__ table,
                                                           uint64_t table_bins) {
    __shared__ uint64_t s_bin[kWaves];
    __shared__ uint64_t s_acgt[kWaves];
    __shared__ uint32_t s_om[kWaves];
    const uint32_t j = blockIdx.x * kComposeBlock + threadIdx.x;
    uint64_t first_bin = kNoBin;
    Packed first;
    if (j < chunks) {
        const uint32_t base = j * kChunk, n = min(kChunk, len - base);
        uint64_t lo = 0, hi = 0;  // the chunk's bytes, the next one lowest
        if (n == kChunk) {
            const uint4 x = *reinterpret_cast<const uint4 *>(text + base);
            lo = uint64_t(x.y) << 32 | x.x;
            hi = uint64_t(x.w) << 32 | x.z;
        } else {
            for (uint32_t k = 0; k < n; ++k) {
                const uint64_t b = uint64_t(text[base + k]) << ((k & 7) * 8);
                if (k < 8) lo |= b;
                else hi |= b;
            }
        }
        uint32_t st = apply(tf_in[j], state), o = uint32_t(cnt_before[j]);
        const bool have = n_pieces > 0 && pieces[0].code_off <= o;
        uint32_t p = have ? piece_of(pieces, n_pieces, o) : 0;
        Piece pc = have ? pieces[p] : Piece{0, kNotSelected, 0, 0};
        bool need_map = true;
        uint64_t at = 0, cur_bin = kNoBin;  // at: the bin of the last mapped byte
        uint32_t rem = 0;                   // its position's offset inside that bin
        Packed cur;
        for (uint32_t k = 0; k < n; ++k) {
            const uint8_t b = uint8_t(lo);
            lo = lo >> 8 | hi << 56;
            hi >>= 8;
            uint32_t kind;
            st = step(st, b, &kind);
            if (!(kind & kSeqByte)) continue;
            while (have && p + 1 < n_pieces && o - pc.code_off >= pc.count) {
                pc = pieces[++p];
                need_map = true;
            }
            if (have && o - pc.code_off < pc.count && pc.bin0 != kNotSelected) {
                if (need_map) {
                    at = bin_of_ordinal(pc, o, S, &rem);
                    need_map = false;
                } else if (++rem == S) {
                    rem = 0;
                    ++at;
                }
                if (at != cur_bin) {
                    if (cur_bin != kNoBin) {
                        if (first_bin == kNoBin) first_bin = cur_bin, first = cur;
                        else add_row(table, table_bins, cur_bin, cur);
                    }
                    cur_bin = at;
                    cur = Packed();
                }
                cur.add(b);
            }
            ++o;
        }
        if (cur_bin != kNoBin) {
            if (first_bin == kNoBin) first_bin = cur_bin, first = cur;
            else add_row(table, table_bins, cur_bin, cur);
        }
    }
    // the wave's lanes, then the workgroup's waves
    uint64_t wave_bin = kNoBin;
    Packed wave;
    wave_sums(first_bin, first, first_bin != kNoBin, true, &wave_bin, &wave, table, table_bins);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (lane == 0) s_bin[wv] = wave_bin, s_acgt[wv] = wave.acgt, s_om[wv] = wave.om;
    __syncthreads();
    if (wv == 0) {
        uint64_t b = kNoBin, unused_bin;
        Packed q, unused;
        if (lane < kWaves) b = s_bin[lane], q.acgt = s_acgt[lane], q.om = s_om[lane];
        wave_sums(b, q, b != kNoBin, false, &unused_bin, &unused, table, table_bins);
    }
}

template <class Sink>
__device__ __forceinline__ void row_line(Sink &s, const Rows &r, uint64_t g) {
    const uint32_t k = bd::chr_of_bin(r.base, r.n, g);
    const uint32_t b = uint32_t(g - r.base[k]);
    put_line(s, r.names.bytes + r.names.off[k], r.names.off[k + 1] - r.names.off[k], bd::bin_start(b, r.S),
             bd::bin_end(b, r.S, r.len[k]), r.counts + g * kColumns);
}

__global__ void __launch_bounds__(kBlock) k_lines_measure(Rows r, uint64_t i0, uint32_t n, uint64_t *__restrict__ len) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k > n) return;
    text::CountSink s;
    if (k < n) row_line(s, r, i0 + k);
    len[k] = s.n;
}

__global__ void __launch_bounds__(kBlock) k_lines_write(Rows r, uint64_t i0, uint32_t n,
                                                        const uint64_t *__restrict__ off, uint8_t *__restrict__ out) {
    const uint64_t k = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= n) return;
    text::ByteSink s{out + off[k]};
    row_line(s, r, i0 + k);
}

inline dim3 grid(uint64_t n, uint32_t block = kBlock) { return dim3(unsigned((n + block - 1) / block)); }

}  // namespace

hipError_t compose(const uint8_t *d_text, uint32_t len, uint32_t state, const fasta::RangeWork &w,
                   const Piece *d_pieces, uint32_t n_pieces, uint32_t S, uint32_t *d_table, uint64_t table_bins,
                   hipStream_t s) {
    if (len == 0 || n_pieces == 0 || S == 0) return hipSuccess;
    const uint32_t chunks = fasta::num_chunks(len);
    k_compose<<<grid(chunks, kComposeBlock), kComposeBlock, 0, s>>>(d_text, len, chunks, state, w.tf_in, w.cnt_before,
                                                                    d_pieces, n_pieces, S, d_table, table_bins);
    return hipGetLastError();
}

size_t scan_bytes(uint64_t n) {
    size_t b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, int(n));
    return b;
}

hipError_t exclusive_sum64(void *tmp, size_t bytes, const uint64_t *d_in, uint64_t *d_out, uint64_t n, hipStream_t s) {
    if (n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_in, d_out, int(n), s);
}

hipError_t lines_measure(const Rows &r, uint64_t i0, uint32_t n, uint64_t *d_len, hipStream_t s) {
    k_lines_measure<<<grid(uint64_t(n) + 1), kBlock, 0, s>>>(r, i0, n, d_len);
    return hipGetLastError();
}

hipError_t lines_write(const Rows &r, uint64_t i0, uint32_t n, const uint64_t *d_off, uint8_t *d_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_lines_write<<<grid(n), kBlock, 0, s>>>(r, i0, n, d_off, d_out);
    return hipGetLastError();
}

}  // namespace genomebins
}  // namespace secedo
