// variant_kernels.hip -- the per-locus work of the reference's variant_calling() (variant_calling.cpp:366-455)
// on the GPU: base counts per cluster, likely_homozygous / most_likely_genotype (:3-79), the all_same rule,
// which lines the reference writes, and the per-cell counters behind `scores`.
//
// Layout. One wave64 walks kLociPerWave consecutive loci in order, one locus at a time; its entries are read 64
// per chunk (id_base only; the first chunk stays in registers, later chunks of a long locus are re-read, from
// the caches). Per-cluster counts are built by electing clusters in ascending order: the wave's minimum cluster
// id above the last one (a xor-shuffle reduction) is the next present cluster, and its four base counts are
// popcounts of ballots. The work per locus is O(coverage x present clusters / 64), whatever the number of
// clusters: an absent cluster has cov = 0, which always yields NO_GENOTYPE (the cov < 9 branch compares
// against cov - 1 in uint32, which wraps), and never affects all_same (its `cov > 0` guard), so only present
// clusters are visited. Cluster ids are u16 and not capped.
//
// Two launches. k_count: the per-group counters (integer atomics, global or privatised per workgroup in LDS, see
// count_calls), the number of records of each
// wave's range and a flag per locus with records; an exclusive scan over the ranges gives each wave its first
// record. k_write revisits the flagged loci only and writes their records in the reference's write order:
// locus ascending, then the pooled line, then the common one, then clusters ascending. No floating-point
// accumulation: the outputs are deterministic.
//
// Exactness (bit-for-bit with the reference):
//   * the four logarithms come from the host's libm (Logs), and the likely_homozygous threshold
//     round(cov*theta + sqrt(cov*theta*(1-theta))) is a host table over every u16 coverage; the device only
//     multiplies and adds in fp64, in the reference's order, with -ffp-contract=off (no FMA).
//   * counts are u16 like the reference's std::array<uint16_t, 4>, and its sum() accumulates in the element
//     type, so coverages are taken mod 2^16 before they meet cov - 1, cov - max or cov > 9.
//   * the heterozygous +-1 sigma test (:70-78) is evaluated in integers. With s = n3 + n2 (n3 >= n2, the two
//     largest counts), mean = s / 2 is integer division, d1 = n3 - mean >= 0 and d2 = mean - n2 >= 0, and
//     std_dev = sqrt(0.25 * s) with 0.25 * s exact. For an integer d, d <= RN(sqrt(s/4)) <=> 4 d^2 <= s and
//     d < RN(sqrt(s/4)) <=> 4 d^2 < s: when 4 d^2 and s differ they differ by at least 1, so sqrt(s/4) is at
//     least 1/(8d + 2) away from d, far more than half an ulp of d for any u16 count, and rounding cannot cross d.
//   * ties: most_likely_genotype sorts with argsort (std::sort of 4 indices, which libstdc++ runs as an
//     insertion sort, stable ascending), so among tied maxima idx[3] is the HIGHEST base index;
//     likely_homozygous takes std::max_element, the LOWEST index. Both are restated as such.
//   * clusters are looked up by GROUP id (:381-386); the `abs(...) <= 0.05` test there is always true.
//   * first_genotype looks at clusters > 0 only, and a cluster with coverage but NO_GENOTYPE breaks all_same;
//     when all_same holds, common.vcf gets cluster 0's genotype with the pooled counts.
//   * mismatches need the cluster's coverage > 9 and are counted only at loci that are not all_same.
#include "variant_kernels.hpp"
#include "text_sink.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace secedo {
namespace variant {

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr uint32_t NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__device__ __forceinline__ uint32_t u16_sum(const uint32_t n[4]) {
    return (n[0] + n[1] + n[2] + n[3]) & 0xFFFFu;  // sum() of a std::array<uint16_t, 4>
}

// likely_homozygous (:3-16): std::max_element -> the first maximum.
__device__ __forceinline__ uint32_t likely_homozygous(const uint32_t n[4], const double *threshold) {
    const uint32_t cov = u16_sum(n);
    if (cov < 9) return kNoGenotype;
    uint32_t b = 0;
#pragma unroll
    for (uint32_t j = 1; j < 4; ++j)
        if (n[j] > n[b]) b = j;
    if ((double)(cov - n[b]) <= threshold[cov]) return b | (b << 3);  // cov - *max in uint32, then to double
    return kNoGenotype;
}

// most_likely_genotype (:18-79) for counts n (each < 2^16). *coverage: the u16 coverage.
__device__ __forceinline__ uint32_t most_likely_genotype(const uint32_t n[4], bool likely_homozygous_total,
                                                         const Logs &lg, uint32_t *coverage) {
    const uint32_t cov = u16_sum(n);
    *coverage = cov;
    // argsort, stable ascending: rank of j = #{k : n[k] < n[j]} + #{k < j : n[k] == n[j]}
    uint32_t idx[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        uint32_t r = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) r += (n[k] < n[j]) || (k < j && n[k] == n[j]);
        idx[r & 3] = j;
    }
    const uint32_t n0 = n[idx[0]], n1 = n[idx[1]], n2 = n[idx[2]], n3 = n[idx[3]];
    if (cov < 9) {
        if (n3 >= cov - 1u && likely_homozygous_total) return (idx[3] << 3) | idx[3];
        return kNoGenotype;
    }
    const double homo = (double)n3 * lg.log_one_minus + (double)(cov - n3) * lg.log_theta;
    const double hetero = (double)(n2 + n3) * lg.log_half_minus + (double)(n0 + n1) * lg.log_theta + lg.log_prior;
    if (homo == hetero) return kNoGenotype;
    if (homo > hetero) {
        if (n2 == n3) return kNoGenotype;
        return (idx[3] << 3) | idx[3];
    }
    if (n2 == n1) return kNoGenotype;
    const int64_t s = (int64_t)n3 + n2, mean = s / 2, d1 = (int64_t)n3 - mean, d2 = mean - (int64_t)n2;
    if (cov > 15 && 4 * d1 * d1 <= s && 4 * d2 * d2 < s) return (idx[3] << 3) | idx[2];
    return kNoGenotype;
}

// is_same_genotype (:243-245)
__device__ __forceinline__ bool same_genotype(uint32_t a, uint32_t b) {
    return a == b || (((a >> 3) | ((a & 7) << 3)) == b);
}

// write_vcf_line writes at least one line (:290-291)
__device__ __forceinline__ bool writes_line(uint32_t genotype, uint32_t ref) {
    return genotype != kNoGenotype && !same_genotype(genotype, ref);
}

struct Entry {
    uint32_t idb;
    uint32_t cluster;
    bool valid;
};

__device__ __forceinline__ Entry load_entry(const CallsIn &in, uint64_t i, uint64_t e, uint32_t *error) {
    Entry x{0, 0, false};
    if (i < e) {
        x.idb = in.id_base16 ? (uint32_t)in.id_base16[i] : in.id_base32[i];
        const uint32_t g = x.idb >> 2;
        if (g < in.n_groups) {
            x.cluster = in.clusters[g];
            x.valid = true;
        } else if (error) {
            atomicOr(error, 1u);
        }
    }
    return x;
}

__device__ __forceinline__ void count_bases(const Entry &x, uint32_t match, uint32_t c[4]) {
    const bool m = x.valid && x.cluster == match;
    const uint64_t all = __ballot(m), b0 = __ballot(m && (x.idb & 1)), b1 = __ballot(m && (x.idb & 2));
    c[0] += __popcll(all & ~b0 & ~b1);
    c[1] += __popcll(b0 & ~b1);
    c[2] += __popcll(~b0 & b1);
    c[3] += __popcll(b0 & b1);
}

// One locus, wave-uniform. COUNT: per-group counters and the record count; !COUNT: the records from `out`.
template <bool COUNT>
__device__ uint32_t locus_calls(const CallsIn &in, uint32_t l, uint32_t *mismatch, uint32_t *loci,
                                uint32_t *error, secedo_variant_record *records, uint32_t out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = in.locus_entry_off[l], e = in.locus_entry_off[l + 1];
    const Entry x0 = load_entry(in, b + lane, e, COUNT ? error : nullptr);
    auto entry = [&](uint64_t c) { return c == b ? x0 : load_entry(in, c + lane, e, nullptr); };

    // pooled counts (:379-388), the first cluster, the counted loci per group
    uint32_t tot[4] = {0, 0, 0, 0};
    uint32_t first = NONE;
    for (uint64_t c = b; c < e; c += 64) {
        const Entry x = c == b ? x0 : load_entry(in, c + lane, e, COUNT ? error : nullptr);
        if (COUNT && x.valid) atomicAdd(&loci[x.idb >> 2], 1u);
        const uint64_t all = __ballot(x.valid), b0 = __ballot(x.valid && (x.idb & 1)),
                       b1 = __ballot(x.valid && (x.idb & 2));
        tot[0] += __popcll(all & ~b0 & ~b1);
        tot[1] += __popcll(b0 & ~b1);
        tot[2] += __popcll(~b0 & b1);
        tot[3] += __popcll(b0 & b1);
        first = min(first, x.valid ? x.cluster : NONE);
    }
    first = wave_min(first);
#pragma unroll
    for (int j = 0; j < 4; ++j) tot[j] &= 0xFFFFu;  // std::array<uint16_t, 4> n_bases_total

    const uint32_t ref = in.locus_ref[l];
    const uint32_t pooled = likely_homozygous(tot, in.threshold);
    const bool lht = pooled != kNoGenotype;
    uint32_t n_rec = 0;
    auto emit = [&](uint32_t cluster, uint32_t genotype, uint32_t kind, const uint32_t c[4]) {
        if (!COUNT && lane == 0) {
            secedo_variant_record r;
            r.locus = l;
            r.cluster = (uint16_t)cluster;
            r.genotype = (uint8_t)genotype;
            r.kind = (uint8_t)kind;
#pragma unroll
            for (int j = 0; j < 4; ++j) r.counts[j] = (uint16_t)c[j];
            records[out + n_rec] = r;
        }
        ++n_rec;
    };
    if (pooled != kNoGenotype && pooled != ref) emit(0, pooled, SECEDO_VARIANT_POOLED, tot);

    // visit the present clusters in ascending order: f(cluster, counts) -> false stops
    auto for_each_cluster = [&](auto f) {
        uint32_t cur = first;
        while (cur != NONE) {
            uint32_t c[4] = {0, 0, 0, 0};
            uint32_t next = NONE;
            for (uint64_t k = b; k < e; k += 64) {
                const Entry x = entry(k);
                count_bases(x, cur, c);
                next = min(next, (x.valid && x.cluster > cur) ? x.cluster : NONE);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] &= 0xFFFFu;  // std::array<uint16_t, 4> per cluster
            if (!f(cur, c)) return;
            cur = wave_min(next);
        }
    };

    // sweep A (:411-426): all_same and cluster 0's genotype; stops once all_same is false
    bool all_same = true;
    uint32_t first_genotype = kNoGenotype, genotype0 = kNoGenotype;
    for_each_cluster([&](uint32_t cl, const uint32_t c[4]) {
        uint32_t cov;
        const uint32_t g = most_likely_genotype(c, lht, in.logs, &cov);
        if (cl == 0) genotype0 = g;
        if (g != kNoGenotype && first_genotype == kNoGenotype && cl > 0) first_genotype = g;
        if (first_genotype != kNoGenotype && cov > 0 && first_genotype != g) all_same = false;
        return all_same;
    });
    if (all_same) {
        if (writes_line(genotype0, ref)) emit(0, genotype0, SECEDO_VARIANT_COMMON, tot);
        return n_rec;
    }
    // sweep B (:433-455): the cluster lines, and the mismatches of the cells
    for_each_cluster([&](uint32_t cl, const uint32_t c[4]) {
        uint32_t cov;
        const uint32_t g = most_likely_genotype(c, lht, in.logs, &cov);
        if (!(pooled != kNoGenotype && g == pooled) && writes_line(g, ref)) emit(cl, g, SECEDO_VARIANT_CLUSTER, c);
        if (COUNT && g != kNoGenotype && cov > 9) {
            for (uint64_t k = b; k < e; k += 64) {
                const Entry x = entry(k);
                const uint32_t base = x.idb & 3;
                if (x.valid && x.cluster == cl && base != (g & 7) && base != (g >> 3))
                    atomicAdd(&mismatch[x.idb >> 2], 1u);
            }
        }
        return true;
    });
    return n_rec;
}

// the chromosome of locus l: chr_locus_off[c] <= l < chr_locus_off[c + 1]
__device__ __forceinline__ uint32_t chromosome_of(const CallsIn &in, uint32_t l) {
    uint32_t lo = 0, hi = in.n_chr;  // answer in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (in.chr_locus_off[mid] <= l) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool counted(const CallsIn &in, uint32_t l, uint32_t &chr) {
    while (l >= in.chr_locus_off[chr + 1]) ++chr;
    return l < in.chr_locus_end[chr];  // the reference's `break` (:374-376)
}

__device__ __forceinline__ void count_range(const CallsIn &in, uint32_t w, uint32_t *mismatch, uint32_t *loci,
                                            uint32_t *range_count, uint8_t *locus_flag, uint32_t *error) {
    const uint32_t l0 = w * kLociPerWave, l1 = min(in.n_loci, l0 + kLociPerWave);
    uint32_t chr = chromosome_of(in, l0), total = 0;
    for (uint32_t l = l0; l < l1; ++l) {
        uint32_t n = 0;
        if (counted(in, l, chr)) n = locus_calls<true>(in, l, mismatch, loci, error, nullptr, 0);
        if ((threadIdx.x & 63) == 0) locus_flag[l] = n > 0;
        total += n;
    }
    if ((threadIdx.x & 63) == 0) range_count[w] = total;
}

// counted entries per group with global atomics; a grid-stride loop over the wave ranges
__global__ __launch_bounds__(TPB) void k_count(CallsIn in, uint32_t n_ranges, uint32_t *mismatch, uint32_t *loci,
                                               uint32_t *range_count, uint8_t *locus_flag, uint32_t *error) {
    for (uint32_t w = blockIdx.x * WAVES + threadIdx.x / 64; w < n_ranges; w += gridDim.x * WAVES)
        count_range(in, w, mismatch, loci, range_count, locus_flag, error);
}

// the same with the counted entries privatised per workgroup in LDS (n_groups <= kLdsGroups), added to the global
// counters once at the end
__global__ __launch_bounds__(TPB) void k_count_lds(CallsIn in, uint32_t n_ranges, uint32_t *mismatch,
                                                   uint32_t *loci, uint32_t *range_count, uint8_t *locus_flag,
                                                   uint32_t *error) {
    __shared__ uint32_t hist[kLdsGroups];
    for (uint32_t i = threadIdx.x; i < in.n_groups; i += TPB) hist[i] = 0;
    __syncthreads();
    for (uint32_t w = blockIdx.x * WAVES + threadIdx.x / 64; w < n_ranges; w += gridDim.x * WAVES)
        count_range(in, w, mismatch, hist, range_count, locus_flag, error);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < in.n_groups; i += TPB)
        if (hist[i]) atomicAdd(&loci[i], hist[i]);
}

__global__ __launch_bounds__(TPB) void k_write(CallsIn in, uint32_t n_ranges, const uint32_t *range_off,
                                               const uint8_t *locus_flag, secedo_variant_record *records) {
    const uint32_t w = blockIdx.x * WAVES + threadIdx.x / 64;
    if (w >= n_ranges) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t l0 = w * kLociPerWave, l1 = min(in.n_loci, l0 + kLociPerWave);
    uint64_t flags = __ballot(l0 + lane < l1 && locus_flag[l0 + lane]);  // kLociPerWave <= 64
    uint32_t out = range_off[w];
    while (flags) {
        const uint32_t l = l0 + (uint32_t)__builtin_ctzll(flags);
        flags &= flags - 1;
        out += locus_calls<false>(in, l, nullptr, nullptr, nullptr, records, out);
    }
}

__global__ void k_genotypes(const uint16_t *counts, uint32_t n, int lht, const double *threshold, Logs logs,
                            uint8_t *homozygous, uint8_t *genotype) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = counts[4 * (size_t)i + j];
    uint32_t cov;
    homozygous[i] = (uint8_t)likely_homozygous(c, threshold);
    genotype[i] = (uint8_t)most_likely_genotype(c, lht != 0, logs, &cov);
}

uint32_t grid_for(uint32_t n_ranges) { return (n_ranges + WAVES - 1) / WAVES; }

// ---------------------------------------------------------------------------------------------------------------
// The VCF text (the bgzf output route): write_outputs, append_vcf_line, append_head and append_counts of
// vcf_output.cpp restated. A record's lines go through a sink, once to count their bytes and once to store them, so
// the length a line was given room for is the length it has.

using text::ByteSink;  // text_sink.hpp
using text::CountSink;
using text::put_str;
using text::put_uint;

__device__ __forceinline__ char base_char(uint32_t b) { return b < 6 ? "ACGTNN"[b] : 'N'; }

template <class S>
__device__ void put_head(S &s, uint32_t chr, uint32_t pos, char ref, char alt1, char alt2) {
    if (chr < 22) put_uint(s, chr + 1);  // id_to_chromosome
    else s.put(chr == 22 ? 'X' : 'Y');
    s.put('\t');
    put_uint(s, pos);
    put_str(s, "\t.\t");
    s.put(ref);
    s.put('\t');
    s.put(alt1);
    if (alt2) s.put(alt2);
    put_str(s, "\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t");
}

template <class S>
__device__ void put_tail(S &s, const char *gt, const uint16_t c[4]) {
    put_str(s, gt);
    s.put('\t');
    for (int j = 0; j < 4; ++j) {
        put_uint(s, c[j]);
        s.put(' ');
    }
    s.put('\n');
}

// the 0, 1 or 2 lines of one record
template <class S>
__device__ void put_record(S &s, const secedo_variant_record &r, uint32_t chr, uint32_t pos, uint32_t ref) {
    const uint32_t g = r.genotype;
    if (r.kind == SECEDO_VARIANT_POOLED) {
        const uint32_t new_base = g & 7;
        const uint32_t ref_base = (ref & 7) == new_base ? (ref >> 3) & 7 : ref & 7;
        put_head(s, chr, pos, base_char(ref_base), base_char(new_base), 0);
        put_tail(s, "1/1", r.counts);
        return;
    }
    if ((ref & 7) == (ref >> 3)) {  // homozygous reference
        const bool hom = (g & 7) == (g >> 3);
        put_head(s, chr, pos, base_char(ref & 7), base_char(g & 7), hom ? 0 : base_char(g >> 3));
        put_tail(s, hom ? "1/1" : "0/1", r.counts);
        return;
    }
    // heterozygous reference: get_differing_bases on the sorted pairs
    char r1 = base_char(ref & 7), r2 = base_char(ref >> 3), g1 = base_char(g & 7), g2 = base_char(g >> 3);
    if (r1 > r2) {
        const char t = r1;
        r1 = r2, r2 = t;
    }
    if (g1 > g2) {
        const char t = g1;
        g1 = g2, g2 = t;
    }
    const bool first = g1 != r1, second = g2 != r2;
    if (first && second) {
        put_head(s, chr, pos, r1, g1, 0);
        put_tail(s, "1/1", r.counts);
        put_head(s, chr, pos, r2, g2, 0);
        put_tail(s, "1/1", r.counts);
    } else if (second) {  // g1 == r1
        put_head(s, chr, pos, r2, g2, 0);
        put_tail(s, "1/1", r.counts);
    } else if (first) {  // g2 == r2
        put_head(s, chr, pos, r1, g1, 0);
        put_tail(s, "1/1", r.counts);
    }
}

// the chromosome write_outputs has reached at a record of this locus (records ascend in locus)
__device__ uint32_t chromosome_of(const uint32_t *__restrict__ chr_locus_off, uint32_t n_chr, uint32_t locus) {
    uint32_t chr = 0;
    while (chr + 1 < n_chr && locus >= chr_locus_off[chr + 1]) ++chr;
    return chr;
}

// the workspace of the two steps, carved from one allocation
struct FormatWork {
    uint32_t *key, *key_sorted, *idx, *idx_sorted, *len;
    uint64_t *len_sorted, *off;  // [n_records + 1]: the last length 0, the last offset the total
    void *cub;
    size_t cub_bytes, total;
};

size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

FormatWork carve(void *base, uint32_t n) {
    FormatWork w{};
    size_t sort_bytes = 0, scan_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 32);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (int)n + 1);
    uint8_t *p = static_cast<uint8_t *>(base);
    size_t at = 0;
    auto take = [&](size_t bytes) {  // base may be null: then only the total is wanted
        uint8_t *q = p ? p + at : nullptr;
        at += align_up(bytes);
        return q;
    };
    w.key = reinterpret_cast<uint32_t *>(take((size_t)n * 4));
    w.key_sorted = reinterpret_cast<uint32_t *>(take((size_t)n * 4));
    w.idx = reinterpret_cast<uint32_t *>(take((size_t)n * 4));
    w.idx_sorted = reinterpret_cast<uint32_t *>(take((size_t)n * 4));
    w.len = reinterpret_cast<uint32_t *>(take((size_t)n * 4));
    w.len_sorted = reinterpret_cast<uint64_t *>(take(((size_t)n + 1) * 8));
    w.off = reinterpret_cast<uint64_t *>(take(((size_t)n + 1) * 8));
    w.cub_bytes = std::max(sort_bytes, scan_bytes);
    w.cub = take(w.cub_bytes);
    w.total = at;
    return w;
}

__global__ __launch_bounds__(TPB) void k_vcf_measure(FormatIn in, uint32_t *__restrict__ key,
                                                     uint32_t *__restrict__ idx, uint32_t *__restrict__ len) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r >= in.n_records) return;
    const secedo_variant_record rec = in.records[r];
    CountSink s;
    put_record(s, rec, chromosome_of(in.chr_locus_off, in.n_chr, rec.locus), in.locus_pos[rec.locus],
               in.locus_ref[rec.locus]);
    key[r] = rec.kind == SECEDO_VARIANT_CLUSTER ? min((uint32_t)rec.cluster, in.num_clusters) : in.num_clusters;
    idx[r] = r;
    len[r] = s.n;
}

__global__ __launch_bounds__(TPB) void k_vcf_gather(const uint32_t *__restrict__ len,
                                                    const uint32_t *__restrict__ idx_sorted, uint32_t n,
                                                    uint64_t *__restrict__ len_sorted) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j <= n) len_sorted[j] = j < n ? len[idx_sorted[j]] : 0;
}

// file f begins where its preamble does: after the preambles of the files before and the lines sorted before its own
__global__ __launch_bounds__(TPB) void k_vcf_files(const uint32_t *__restrict__ key_sorted,
                                                   const uint64_t *__restrict__ off, uint32_t n,
                                                   const uint64_t *__restrict__ preamble_off, uint32_t n_files,
                                                   uint64_t *__restrict__ file_off) {
    const uint32_t f = blockIdx.x * TPB + threadIdx.x;
    if (f > n_files) return;
    uint32_t lo = 0, hi = n;  // the first sorted record with key >= f
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_sorted[mid] < f) lo = mid + 1;
        else hi = mid;
    }
    file_off[f] = preamble_off[f] + off[lo];
}

constexpr uint32_t kStageBytes = 2 * kMaxLineBytes * TPB + 64;  // a workgroup's lines when no preamble lies between

// A workgroup's 256 sorted records are consecutive in the buffer but for the preambles of the files that begin among
// them. Their lines are put together in LDS and leave as whole dwords; the preamble gaps carry whatever LDS held and
// are overwritten by k_vcf_preambles, which runs after. A group whose span exceeds the stage stores bytes directly.
__global__ __launch_bounds__(TPB) void k_vcf_write(FormatIn in, const uint32_t *__restrict__ key_sorted,
                                                   const uint32_t *__restrict__ idx_sorted,
                                                   const uint64_t *__restrict__ off, uint8_t *__restrict__ text) {
    __shared__ __align__(16) uint8_t stage[kStageBytes];
    const uint32_t n = in.n_records, j0 = blockIdx.x * TPB, j = j0 + threadIdx.x;
    const uint32_t j1 = min(n, j0 + TPB) - 1;  // the group's last record
    const uint64_t start = off[j0] + in.preamble_off[key_sorted[j0] + 1];
    const uint64_t end = off[j1 + 1] + in.preamble_off[key_sorted[j1] + 1];  // off[j1 + 1] - off[j1] is j1's length
    const bool staged = end - start <= kStageBytes;
    if (j < n) {
        const secedo_variant_record rec = in.records[idx_sorted[j]];
        const uint64_t at = off[j] + in.preamble_off[key_sorted[j] + 1];
        ByteSink s{staged ? stage + (at - start) : text + at};
        put_record(s, rec, chromosome_of(in.chr_locus_off, in.n_chr, rec.locus), in.locus_pos[rec.locus],
                   in.locus_ref[rec.locus]);
    }
    if (!staged) return;
    __syncthreads();
    const uint32_t span = uint32_t(end - start);
    uint8_t *dst = text + start;
    const uint32_t head = min(span, uint32_t(-reinterpret_cast<uintptr_t>(dst)) & 3u);
    const uint32_t words = (span - head) / 4, tail = head + 4 * words;
    if (threadIdx.x < head) dst[threadIdx.x] = stage[threadIdx.x];
    for (uint32_t k = threadIdx.x; k < words; k += TPB) {
        const uint8_t *b = stage + head + 4 * k;
        *reinterpret_cast<uint32_t *>(dst + head + 4 * k) =
            uint32_t(b[0]) | uint32_t(b[1]) << 8 | uint32_t(b[2]) << 16 | uint32_t(b[3]) << 24;
    }
    if (tail + threadIdx.x < span) dst[tail + threadIdx.x] = stage[tail + threadIdx.x];
}

__global__ __launch_bounds__(64) void k_vcf_preambles(const uint8_t *__restrict__ preamble,
                                                      const uint64_t *__restrict__ preamble_off,
                                                      const uint64_t *__restrict__ file_off, uint32_t n_files,
                                                      uint8_t *__restrict__ text) {
    const uint32_t f = blockIdx.x;
    if (f >= n_files) return;
    const uint64_t b = preamble_off[f], n = preamble_off[f + 1] - b;
    uint8_t *dst = text + file_off[f];
    for (uint64_t i = threadIdx.x; i < n; i += 64) dst[i] = preamble[b + i];
}

}  // namespace

static_assert(kLociPerWave <= 64, "k_write takes a wave's locus flags in one ballot");

uint32_t num_ranges(uint32_t n_loci) { return (n_loci + kLociPerWave - 1) / kLociPerWave; }

size_t scan_workspace(uint32_t n_loci) {
    size_t need = 0;
    const uint32_t r = num_ranges(n_loci);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, need, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)r + 1);
    return need;
}

hipError_t count_calls(const CallsIn &in, uint32_t *d_mismatch, uint32_t *d_loci, uint32_t *d_range_count,
                       uint32_t *d_range_off, uint8_t *d_locus_flag, uint32_t *d_error, void *scan_tmp,
                       size_t scan_bytes, bool lds_counters, uint32_t max_blocks, hipStream_t stream) {
    const uint32_t r = num_ranges(in.n_loci);
    hipError_t e;
    if ((e = hipMemsetAsync(d_mismatch, 0, (size_t)in.n_groups * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_loci, 0, (size_t)in.n_groups * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_error, 0, 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_range_count, 0, ((size_t)r + 1) * 4, stream)) != hipSuccess) return e;
    if (r > 0) {
        if (lds_counters && in.n_groups <= kLdsGroups)
            hipLaunchKernelGGL(k_count_lds, dim3(std::min(grid_for(r), max_blocks)), dim3(TPB), 0, stream, in, r,
                               d_mismatch, d_loci, d_range_count, d_locus_flag, d_error);
        else
            hipLaunchKernelGGL(k_count, dim3(std::min(grid_for(r), max_blocks)), dim3(TPB), 0, stream, in, r,
                               d_mismatch, d_loci, d_range_count, d_locus_flag, d_error);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, d_range_count, d_range_off, (int)r + 1, stream);
}

hipError_t write_calls(const CallsIn &in, const uint32_t *d_range_off, const uint8_t *d_locus_flag,
                       secedo_variant_record *d_records, hipStream_t stream) {
    const uint32_t r = num_ranges(in.n_loci);
    if (r > 0)
        hipLaunchKernelGGL(k_write, dim3(grid_for(r)), dim3(TPB), 0, stream, in, r, d_range_off, d_locus_flag,
                           d_records);
    return hipGetLastError();
}

hipError_t genotypes(const uint16_t *d_counts, uint32_t n, int likely_homozygous_total, const double *d_threshold,
                     Logs logs, uint8_t *d_homozygous, uint8_t *d_genotype, hipStream_t stream) {
    if (n > 0)
        hipLaunchKernelGGL(k_genotypes, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, stream, d_counts, n,
                           likely_homozygous_total, d_threshold, logs, d_homozygous, d_genotype);
    return hipGetLastError();
}

size_t format_workspace(uint32_t n_records) {
    return carve(nullptr, n_records).total;
}

hipError_t format_measure(const FormatIn &in, void *workspace, size_t workspace_bytes, uint64_t *d_file_off,
                          hipStream_t stream) {
    const uint32_t n = in.n_records, n_files = in.num_clusters + 1;
    const FormatWork w = carve(workspace, n);
    if (w.total > workspace_bytes) return hipErrorInvalidValue;
    hipError_t e;
    if (n > 0) {
        hipLaunchKernelGGL(k_vcf_measure, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, stream, in, w.key, w.idx, w.len);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        uint32_t bits = 1;  // keys are 0 .. num_clusters
        while (bits < 32 && (in.num_clusters >> bits)) ++bits;
        size_t cub_bytes = w.cub_bytes;
        if ((e = hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.key, w.key_sorted, w.idx, w.idx_sorted, (int)n,
                                                    0, (int)bits, stream)) != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(k_vcf_gather, dim3(n / TPB + 1), dim3(TPB), 0, stream, w.len, w.idx_sorted, n, w.len_sorted);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t cub_bytes = w.cub_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(w.cub, cub_bytes, w.len_sorted, w.off, (int)n + 1, stream)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_vcf_files, dim3(n_files / TPB + 1), dim3(TPB), 0, stream, w.key_sorted, w.off, n,
                       in.preamble_off, n_files, d_file_off);
    return hipGetLastError();
}

hipError_t format_write(const FormatIn &in, const void *workspace, size_t workspace_bytes, const uint64_t *d_file_off,
                        uint8_t *d_text, hipStream_t stream) {
    const uint32_t n = in.n_records, n_files = in.num_clusters + 1;
    const FormatWork w = carve(const_cast<void *>(workspace), n);
    if (w.total > workspace_bytes) return hipErrorInvalidValue;
    if (n > 0)
        hipLaunchKernelGGL(k_vcf_write, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, stream, in, w.key_sorted,
                           w.idx_sorted, w.off, d_text);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_vcf_preambles, dim3(n_files), dim3(64), 0, stream, in.preamble, in.preamble_off, d_file_off,
                       n_files, d_text);
    return hipGetLastError();
}

}  // namespace variant
}  // namespace secedo
