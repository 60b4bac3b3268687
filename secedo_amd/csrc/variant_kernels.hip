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

}  // namespace variant
}  // namespace secedo
