// allele_kernels.hip -- per-cell allele counts at the called variants (include/secedo_variant.h): which cells support
// which call, as (site, group, ad, rd, oth) pairs, and the Matrix Market / VCF text of the pairs.
//
// Site pass. The records stand in HBM in write order, so the records of a locus are consecutive: the thread of a
// locus' first record walks its run (at most 2 + clusters records), ORs the genotypes' bits and applies the mask rule
// (allele_kernels.hpp: site_masks). A scan of the flags numbers the sites; a second kernel compacts them.
//
// Count and write pass. One wave per site, like k_count / k_write of variant_kernels.hip. Every entry becomes the key
// group << 2 | class (class 0 = base in alt_mask, 1 = in ref_mask, 2 = the rest), the site's keys are SORTED, and the
// sorted keys are walked 64 at a time: a lane whose group differs from the lane before it is the head of a pair
// (__ballot / popcount give the pair's number), a lane whose key differs starts a (group, class) run. Nothing is
// assumed about the order of a locus' entries or about how often a group occurs.
//   * at most kWaveEntries = 128 entries (the common case: --max_coverage 100): two keys per lane, a bitonic network of
//     28 compare-exchange steps in registers (shuffles; the 64-apart step is in-lane), no LDS, no memory traffic.
//   * deeper loci: their keys, prefixed by the site number, are written to one buffer and sorted by ONE device radix
//     sort (hipcub) for all deep sites together; the site prefix keeps every site's keys in its own span. The cost is
//     linear in the entries whatever the number of distinct groups; the bound is 2^31 - 1 deep entries per call (the
//     sort's item count), whatever the depth of one locus.
// The count pass counts heads (pairs), run starts per class (the three nnz) and entries per class (the totals); a scan
// of the pairs per site gives each site its first pair. The write pass repeats the walk: the head lane stores (site,
// group), the last lane of a (group, class) run within a chunk adds the run's length to the pair's field (integer
// atomicAdd on zeroed pairs: a run may continue in the next chunk). Output order: site, then group, by construction.
//
// Format pass. A range of sites is turned into its four texts by measure (a length per line), scan, write, as k_vcf_*
// of variant_kernels.hip do: a thread per pair writes its up to three matrix lines, a thread per site its VCF line.
#include "allele_kernels.hpp"
#include "text_sink.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace secedo {
namespace allele {

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr uint32_t INVALID = 0xFFFFFFFFu;  // no key: a class is at most 2

__device__ __forceinline__ uint32_t entry_key(const Pileup &p, uint64_t i, uint32_t mask, unsigned long long *error) {
    const uint32_t idb = p.id_base16 ? (uint32_t)p.id_base16[i] : p.id_base32[i];
    const uint32_t g = idb >> 2, bit = 1u << (idb & 3);
    if (g >= p.n_cells) {
        if (error) atomicOr(error, 1ull);
        return INVALID;
    }
    return g << 2 | (((mask >> 4) & bit) ? 0u : (mask & bit) ? 1u : 2u);
}

// 128 keys ascending over the wave: afterwards a = sorted[lane], b = sorted[64 + lane]. Element e = lane + 64 * slot.
__device__ __forceinline__ void wave_sort128(uint32_t &a, uint32_t &b) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (uint32_t k = 2; k <= 128; k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (j == 64) {  // k == 128: the partner is this lane's other slot, ascending
                const uint32_t lo = min(a, b), hi = max(a, b);
                a = lo, b = hi;
                continue;
            }
            // ascending where bit k of e is clear: bit 64 of e is the slot, bit 128 is never set
            const bool asc_a = k >= 64 ? true : !(lane & k);
            const bool asc_b = k == 128 ? true : k == 64 ? false : !(lane & k);
            const bool upper = lane & j;
            const uint32_t pa = (uint32_t)__shfl_xor((int)a, (int)j), pb = (uint32_t)__shfl_xor((int)b, (int)j);
            a = (upper != asc_a) ? min(a, pa) : max(a, pa);
            b = (upper != asc_b) ? min(b, pb) : max(b, pb);
        }
    }
}

struct Walk {  // wave-uniform
    uint32_t prev = 0;  // the last key of the chunk before
    bool have_prev = false;
    uint32_t pairs = 0, nnz_ad = 0, nnz_dp = 0, nnz_oth = 0, ad = 0, rd = 0, oth = 0;
};

// 64 sorted keys, valid ones first. WRITE: the pairs from out[0] on (the site's first pair).
template <bool WRITE>
__device__ __forceinline__ void walk_chunk(uint32_t x, uint32_t site, Walk &w, secedo_allele_pair *out) {
    const uint32_t lane = threadIdx.x & 63;
    const bool valid = x != INVALID;
    const uint32_t up = (uint32_t)__shfl_up((int)x, 1);
    const bool has = lane ? true : w.have_prev;  // a valid lane above 0 follows a valid lane
    const uint32_t pv = lane ? up : w.prev;
    const bool start = valid && (!has || x != pv);
    const bool head = valid && (!has || (x >> 2) != (pv >> 2));
    const uint32_t cls = x & 3;
    const uint64_t hm = __ballot(head), vm = __ballot(valid);
    if (WRITE) {
        const uint64_t sm = __ballot(start) | 1ull;  // where a run begins within this chunk
        const uint64_t le = lane == 63 ? ~0ull : (2ull << lane) - 1;
        if (valid) {
            // a valid lane has a head at or before it, in this chunk or an earlier one: the index is never negative
            secedo_allele_pair *pair = out + ((uint64_t)w.pairs + __popcll(hm & le) - 1);
            if (head) {
                pair->site = site;
                pair->group = x >> 2;
            }
            const bool last = lane == 63 || !((vm >> (lane + 1)) & 1) || ((sm >> (lane + 1)) & 1);
            if (last) {
                const uint32_t first = 63u - (uint32_t)__builtin_clzll(sm & le);
                atomicAdd(&pair->ad + cls, lane - first + 1);  // ad, rd, oth are consecutive
            }
        }
    } else {
        w.nnz_ad += __popcll(__ballot(start && cls == 0));
        w.nnz_oth += __popcll(__ballot(start && cls == 2));
        w.nnz_dp += __popcll(__ballot(head && cls < 2));  // a head has its group's lowest class
        w.ad += __popcll(__ballot(valid && cls == 0));
        w.rd += __popcll(__ballot(valid && cls == 1));
        w.oth += __popcll(__ballot(valid && cls == 2));
    }
    w.pairs += __popcll(hm);
    const uint32_t n_valid = __popcll(vm);
    const uint32_t tail = (uint32_t)__shfl((int)x, (int)(n_valid ? n_valid - 1 : 0));
    if (n_valid) {
        w.prev = tail;
        w.have_prev = true;
    }
}

static_assert(offsetof(secedo_allele_pair, rd) == offsetof(secedo_allele_pair, ad) + 4 &&
                  offsetof(secedo_allele_pair, oth) == offsetof(secedo_allele_pair, ad) + 8,
              "walk_chunk addresses rd and oth from ad");

template <bool WRITE>
__device__ __forceinline__ Walk walk_site(const Pileup &p, const Sites &s, uint32_t site, uint64_t *depth_out,
                                          unsigned long long *error, secedo_allele_pair *out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t l = s.locus[site], mask = s.mask[site];
    const uint64_t b = p.locus_entry_off[l], e = p.locus_entry_off[l + 1], depth = e - b;
    *depth_out = depth;
    Walk w;
    if (depth <= kWaveEntries) {
        uint32_t k0 = b + lane < e ? entry_key(p, b + lane, mask, error) : INVALID;
        uint32_t k1 = b + 64 + lane < e ? entry_key(p, b + 64 + lane, mask, error) : INVALID;
        wave_sort128(k0, k1);
        walk_chunk<WRITE>(k0, site, w, out);
        if (depth > 64) walk_chunk<WRITE>(k1, site, w, out);
    } else {
        const uint64_t *keys = s.keys_sorted + s.deep_off[site];
        for (uint64_t c = 0; c < depth; c += 64) {
            const uint64_t i = c + lane;
            const uint32_t key = i < depth ? (uint32_t)keys[i] : INVALID;
            if (error && i < depth && key == INVALID) atomicOr(error, 1ull);  // a group id >= n_cells, sorted last
            walk_chunk<WRITE>(key, site, w, out);
        }
    }
    return w;
}

__global__ __launch_bounds__(TPB) void k_allele_count(Pileup p, Sites s, SiteCounts *__restrict__ counts,
                                                      Totals *__restrict__ totals, uint64_t *__restrict__ pair_len) {
    const uint32_t site = blockIdx.x * WAVES + threadIdx.x / 64;
    if (site > s.n) return;
    if (site == s.n) {
        if ((threadIdx.x & 63) == 0) pair_len[site] = 0;
        return;
    }
    uint64_t depth;
    const Walk w = walk_site<false>(p, s, site, &depth, &totals->error, nullptr);
    if ((threadIdx.x & 63) != 0) return;
    counts[site] = SiteCounts{w.pairs, w.nnz_ad, w.nnz_dp, w.nnz_oth, w.ad, w.rd, w.oth, 0};
    pair_len[site] = w.pairs;
    atomicAdd(&totals->entries, (unsigned long long)depth);
    atomicAdd(&totals->nnz_ad, (unsigned long long)w.nnz_ad);
    atomicAdd(&totals->nnz_dp, (unsigned long long)w.nnz_dp);
    atomicAdd(&totals->nnz_oth, (unsigned long long)w.nnz_oth);
    if (depth > kWaveEntries) atomicAdd(&totals->deep_sites, 1ull);
}

__global__ __launch_bounds__(TPB) void k_allele_write(Pileup p, Sites s, const uint64_t *__restrict__ pair_off,
                                                      secedo_allele_pair *__restrict__ pairs) {
    const uint32_t site = blockIdx.x * WAVES + threadIdx.x / 64;
    if (site >= s.n) return;
    uint64_t depth;
    (void)walk_site<true>(p, s, site, &depth, nullptr, pairs + pair_off[site]);
}

// the keys of the deep sites, a wave per site
__global__ __launch_bounds__(TPB) void k_allele_deep_keys(Pileup p, const uint32_t *__restrict__ site_locus,
                                                          const uint8_t *__restrict__ site_mask, uint32_t n_sites,
                                                          const uint64_t *__restrict__ deep_off,
                                                          uint64_t *__restrict__ keys) {
    const uint32_t site = blockIdx.x * WAVES + threadIdx.x / 64;
    if (site >= n_sites) return;
    const uint32_t l = site_locus[site], mask = site_mask[site];
    const uint64_t b = p.locus_entry_off[l], depth = p.locus_entry_off[l + 1] - b;
    if (depth <= kWaveEntries) return;
    uint64_t *out = keys + deep_off[site];  // deep_off[site + 1] - deep_off[site] == depth
    for (uint64_t i = threadIdx.x & 63; i < depth; i += 64)
        out[i] = (uint64_t)site << 32 | entry_key(p, b + i, mask, nullptr);  // a bad group id: the count pass reports it
}

__global__ __launch_bounds__(TPB) void k_allele_site_flags(const secedo_variant_record *__restrict__ records, uint32_t n,
                                                           const uint8_t *__restrict__ locus_ref, int selection,
                                                           uint32_t *__restrict__ flag, uint8_t *__restrict__ mask) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r > n) return;
    uint32_t f = 0, m = 0;
    if (r < n) {
        const uint32_t l = records[r].locus;
        if (r == 0 || records[r - 1].locus != l) {
            uint32_t g = 0;
            bool cluster = false;
            for (uint32_t k = r; k < n && records[k].locus == l; ++k) {
                g |= genotype_bits(records[k].genotype);
                cluster = cluster || records[k].kind == SECEDO_VARIANT_CLUSTER;
            }
            if (selection == SECEDO_ALLELE_ALL || cluster) {
                f = 1;
                m = site_masks(locus_ref[l], g);
            }
        }
    }
    flag[r] = f;  // flag[n] = 0 closes the scan
    mask[r] = (uint8_t)m;
}

__global__ __launch_bounds__(TPB) void k_allele_site_compact(const secedo_variant_record *__restrict__ records,
                                                             uint32_t n, const uint32_t *__restrict__ flag,
                                                             const uint8_t *__restrict__ mask,
                                                             const uint32_t *__restrict__ index, Pileup p,
                                                             uint32_t n_sites, uint32_t *__restrict__ site_locus,
                                                             uint8_t *__restrict__ site_mask,
                                                             uint64_t *__restrict__ deep_len) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r > n) return;
    if (r == n) {
        deep_len[n_sites] = 0;
        return;
    }
    if (!flag[r]) return;
    const uint32_t s = index[r], l = records[r].locus;  // s < n_sites = index[n]
    const uint64_t depth = p.locus_entry_off[l + 1] - p.locus_entry_off[l];
    site_locus[s] = l;
    site_mask[s] = mask[r];
    deep_len[s] = depth > kWaveEntries ? depth : 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The text, through the sinks of text_sink.hpp.

using text::ByteSink;
using text::CountSink;
using text::put_str;
using text::put_uint;

// "<site>\t<cell>\t<value>\n", 1-based; nothing for a value of 0
template <class S>
__device__ void put_mtx(S &s, uint32_t site, uint32_t group, uint32_t value) {
    if (value == 0) return;
    put_uint(s, site + 1);
    s.put('\t');
    put_uint(s, group + 1);
    s.put('\t');
    put_uint(s, value);
    s.put('\n');
}

template <class S>
__device__ void put_letters(S &s, uint32_t mask) {
    bool any = false;
    for (uint32_t b = 0; b < 4; ++b) {
        if (!((mask >> b) & 1)) continue;
        if (any) s.put(',');
        s.put("ACGT"[b]);
        any = true;
    }
    if (!any) s.put('N');
}

template <class S>
__device__ void put_vcf(S &s, const FormatIn &in, uint32_t site) {
    const uint32_t l = in.site_locus[site], mask = in.site_mask[site];
    uint32_t chr = 0;  // as the VCF writer names it: the chromosome the records' walk has reached
    while (chr + 1 < in.n_chr && l >= in.chr_locus_off[chr + 1]) ++chr;
    if (chr < 22) put_uint(s, chr + 1);
    else s.put(chr == 22 ? 'X' : 'Y');
    s.put('\t');
    put_uint(s, in.locus_pos[l]);
    put_str(s, "\t.\t");
    put_letters(s, mask & 15);
    s.put('\t');
    put_letters(s, mask >> 4);
    put_str(s, "\t.\tPASS\tAD=");
    const SiteCounts c = in.counts[site];
    put_uint(s, c.ad);
    put_str(s, ";DP=");
    put_uint(s, c.ad + c.rd);
    put_str(s, ";OTH=");
    put_uint(s, c.oth);
    s.put('\n');
}

__device__ __forceinline__ uint32_t pair_value(const secedo_allele_pair &q, uint32_t f) {
    return f == 0 ? q.ad : f == 1 ? q.ad + q.rd : q.oth;
}

// thread t: pair p0 + t for t < np, site s0 + (t - np) for the next ns, and one more for the headers and the closing item
__global__ __launch_bounds__(TPB) void k_allele_measure(FormatIn in, uint64_t *__restrict__ len) {
    const uint64_t np = in.p1 - in.p0, ns = in.s1 - in.s0, t = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (t < np) {
        const secedo_allele_pair q = in.pairs[in.p0 + t];
        for (uint32_t f = 0; f < 3; ++f) {
            CountSink s;
            put_mtx(s, q.site, q.group, pair_value(q, f));
            len[f * (np + 1) + 1 + t] = s.n;
        }
    } else if (t < np + ns) {
        CountSink s;
        put_vcf(s, in, in.s0 + (uint32_t)(t - np));
        len[3 * (np + 1) + 1 + (t - np)] = s.n;
    } else if (t == np + ns) {
        for (uint32_t f = 0; f < kFiles; ++f) len[f * (np + 1)] = in.hdr_len[f];
        len[3 * (np + 1) + 1 + ns] = 0;
    }
}

__global__ void k_allele_files(FormatIn in, const uint64_t *__restrict__ off, uint64_t *__restrict__ file_off) {
    const uint64_t np = in.p1 - in.p0, ns = in.s1 - in.s0;
    if (threadIdx.x < kFiles) file_off[threadIdx.x] = off[threadIdx.x * (np + 1)];
    if (threadIdx.x == kFiles) file_off[kFiles] = off[3 * (np + 1) + 1 + ns];
}

__global__ __launch_bounds__(TPB) void k_allele_text(FormatIn in, const uint64_t *__restrict__ off,
                                                     uint8_t *__restrict__ text) {
    const uint64_t np = in.p1 - in.p0, ns = in.s1 - in.s0, t = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (t < np) {
        const secedo_allele_pair q = in.pairs[in.p0 + t];
        for (uint32_t f = 0; f < 3; ++f) {
            ByteSink s{text + off[f * (np + 1) + 1 + t]};
            put_mtx(s, q.site, q.group, pair_value(q, f));
        }
    } else if (t < np + ns) {
        ByteSink s{text + off[3 * (np + 1) + 1 + (t - np)]};
        put_vcf(s, in, in.s0 + (uint32_t)(t - np));
    }
}

__global__ __launch_bounds__(64) void k_allele_headers(FormatIn in, const uint64_t *__restrict__ off,
                                                       const uint8_t *__restrict__ hdr, uint8_t *__restrict__ text) {
    const uint32_t f = blockIdx.x;
    uint32_t from = 0;
    for (uint32_t k = 0; k < f; ++k) from += in.hdr_len[k];
    uint8_t *dst = text + off[f * (in.p1 - in.p0 + 1)];
    for (uint32_t i = threadIdx.x; i < in.hdr_len[f]; i += 64) dst[i] = hdr[from + i];
}

uint32_t site_grid(uint32_t n_waves) { return (n_waves + WAVES - 1) / WAVES; }

template <class T>
size_t sum_workspace(uint64_t n) {
    size_t need = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, need, (T *)nullptr, (T *)nullptr, (int)n);
    return need;
}

uint32_t bits_of(uint32_t v) {
    uint32_t b = 1;
    while (b < 32 && (v >> b)) ++b;
    return b;
}

}  // namespace

size_t site_scan_workspace(uint32_t n_records) { return sum_workspace<uint32_t>((uint64_t)n_records + 1); }
size_t pair_scan_workspace(uint32_t n_sites) { return sum_workspace<uint64_t>((uint64_t)n_sites + 1); }
size_t format_scan_workspace(uint64_t items) { return sum_workspace<uint64_t>(items); }

hipError_t site_flags(const secedo_variant_record *d_records, uint32_t n_records, const uint8_t *d_locus_ref,
                      int selection, uint32_t *d_flag, uint8_t *d_mask, uint32_t *d_index, void *scan_tmp,
                      size_t scan_bytes, hipStream_t stream) {
    hipLaunchKernelGGL(k_allele_site_flags, dim3(n_records / TPB + 1), dim3(TPB), 0, stream, d_records, n_records,
                       d_locus_ref, selection, d_flag, d_mask);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, d_flag, d_index, (int)n_records + 1, stream);
}

hipError_t site_compact(const secedo_variant_record *d_records, uint32_t n_records, const uint32_t *d_flag,
                        const uint8_t *d_mask, const uint32_t *d_index, const Pileup &p, uint32_t n_sites,
                        uint32_t *d_site_locus, uint8_t *d_site_mask, uint64_t *d_deep_len, uint64_t *d_deep_off,
                        void *scan_tmp, size_t scan_bytes, hipStream_t stream) {
    hipLaunchKernelGGL(k_allele_site_compact, dim3(n_records / TPB + 1), dim3(TPB), 0, stream, d_records, n_records,
                       d_flag, d_mask, d_index, p, n_sites, d_site_locus, d_site_mask, d_deep_len);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, d_deep_len, d_deep_off, (int)n_sites + 1, stream);
}

size_t deep_sort_workspace(uint64_t n_deep) {
    size_t need = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, need, (uint64_t *)nullptr, (uint64_t *)nullptr, (int)n_deep, 0, 64);
    return need;
}

hipError_t deep_sort(const Pileup &p, const uint32_t *d_site_locus, const uint8_t *d_site_mask, uint32_t n_sites,
                     const uint64_t *d_deep_off, uint64_t n_deep, uint64_t *d_keys, uint64_t *d_keys_sorted,
                     void *sort_tmp, size_t sort_bytes, hipStream_t stream) {
    if (n_deep == 0 || n_sites == 0) return hipSuccess;
    if (n_deep > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_allele_deep_keys, dim3(site_grid(n_sites)), dim3(TPB), 0, stream, p, d_site_locus, d_site_mask,
                       n_sites, d_deep_off, d_keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortKeys(sort_tmp, sort_bytes, d_keys, d_keys_sorted, (int)n_deep, 0,
                                             (int)(32 + bits_of(n_sites)), stream);
}

hipError_t count_pairs(const Pileup &p, const Sites &s, SiteCounts *d_counts, Totals *d_totals, uint64_t *d_pair_len,
                       uint64_t *d_pair_off, void *scan_tmp, size_t scan_bytes, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_totals, 0, sizeof(Totals), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_allele_count, dim3(site_grid(s.n + 1)), dim3(TPB), 0, stream, p, s, d_counts, d_totals,
                       d_pair_len);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, d_pair_len, d_pair_off, (int)s.n + 1, stream);
}

hipError_t write_pairs(const Pileup &p, const Sites &s, const uint64_t *d_pair_off, uint64_t n_pairs,
                       secedo_allele_pair *d_pairs, hipStream_t stream) {
    if (s.n == 0 || n_pairs == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_pairs, 0, n_pairs * sizeof(secedo_allele_pair), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_allele_write, dim3(site_grid(s.n)), dim3(TPB), 0, stream, p, s, d_pair_off, d_pairs);
    return hipGetLastError();
}

hipError_t format_measure(const FormatIn &in, uint64_t *d_len, uint64_t *d_off, uint64_t *d_file_off, void *scan_tmp,
                          size_t scan_bytes, hipStream_t stream) {
    const uint64_t threads = (in.p1 - in.p0) + (in.s1 - in.s0) + 1, items = format_items(in);
    if (threads / TPB + 1 > 0x7FFFFFFFull || items > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_allele_measure, dim3((uint32_t)(threads / TPB + 1)), dim3(TPB), 0, stream, in, d_len);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, d_len, d_off, (int)items, stream)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_allele_files, dim3(1), dim3(64), 0, stream, in, d_off, d_file_off);
    return hipGetLastError();
}

hipError_t format_write(const FormatIn &in, const uint64_t *d_off, const uint8_t *d_hdr, uint8_t *d_text,
                        hipStream_t stream) {
    const uint64_t threads = (in.p1 - in.p0) + (in.s1 - in.s0) + 1;
    hipLaunchKernelGGL(k_allele_text, dim3((uint32_t)(threads / TPB + 1)), dim3(TPB), 0, stream, in, d_off, d_text);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_allele_headers, dim3(kFiles), dim3(64), 0, stream, in, d_off, d_hdr, d_text);
    return hipGetLastError();
}

}  // namespace allele
}  // namespace secedo
