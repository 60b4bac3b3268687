// pack_device.hip -- device-side packing of the raw flat pileup (see pack_device.hpp).
//
// Pipeline (every step a kernel or a hipCUB scan on `stream`; 3 scalar read-backs):
//   1  entry -> locus; entries grouped by (chromosome, read id) in pileup order. Sparse loci (most reads have one
//      entry): every entry stores its number in its id's slot and checks whether the slot still holds it -- the
//      entries of repeated ids ("M entries") are flagged, numbered, compacted and grouped by the entry that won
//      their slot; the others are their reads. Otherwise: histogram over the dense id space, scan, scatter with an
//      atomic cursor, rank inside the (short) group; the hipCUB radix sort when the ids are sparse or a group is
//      too long for that
//   2  duplicate-position rule per (read, locus) group (reference: similarity_matrix.cpp:387-395);
//      reads = runs of equal key, cut further where a flush erases a read that outlives
//      max_fragment_length (:368-371, :379-382; k_split_update, iterated with step 4)
//   3  kept entries -> per-read lists (CSR), multi-locus statistics
//   4  first-appearance rank of every read, completed-prefix count per locus, flush chain per
//      chromosome (reference :348-373) -> number of flushed reads F_c -> tail flags (:407-408)
//   5  kept entries grouped by (cell block, locus, cell) -- per-locus LDS histograms, scan, placement,
//      in-group ranking (or the radix sort) --, block offsets, pair bound, locus ranges, entry records
//      (window masks) written at their final position
//
// The host half (struct PackAttempt, at the end of the file) is a function per stage and per route of a stage, over
// the views of pack_workspace.hpp:
//   1    group_by_read -> group_by_read_single_entry | group_by_read_counting | group_by_read_radix
//   2-4  build_reads (reads, completed counts, the flush chain on the side stream), settle_flush_cuts (k_split_update
//        to its fixed point)
//   5    plan_tiles (cell blocks, staging limits, segments: host only), bin_counting | bin_radix,
//        records_counting | records_radix, close_attempt (read-back 3, the repair of wrongly assumed limits, the
//        fields of DevicePacked)
// scalar_verdict turns a read-back of the scalars into what the attempt does next; an attempt ends as one Attempt
// value (done, need the host, retry with the radix sorts, retry without assumptions, or an error with its text).
#include "pack_device.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace secedo {

DeviceArena::~DeviceArena() {
    if (p) (void)hipFree(p);
}

DevicePacked::~DevicePacked() {
    if (side) (void)hipStreamDestroy(side);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (ev_offsets) (void)hipEventDestroy(ev_offsets);
    if (ev_flush) (void)hipEventDestroy(ev_flush);
    if (mailbox) (void)hipHostFree(mailbox);
}

// SECEDO_POISON (a debugging aid): 1 fills every new allocation with 0xA5 bytes, 2 also refills the packing's
// scratch and outputs at the start of every prepare -- a kernel that reads a word nobody wrote then reads
// 0xA5A5A5A5 every time instead of whatever the allocation happened to hold (tools/poison_run.sh).
int poison_level() {
    static const int level = [] {
        const char *e = std::getenv("SECEDO_POISON");
        return e ? std::atoi(e) : 0;
    }();
    return level;
}

hipError_t DeviceArena::ensure(size_t n) {
    if (n <= bytes && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    const size_t want = n ? n + n / 8 + 256 : 256;  // head room: sizes vary a little from call to call
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) bytes = want;
    if (e == hipSuccess && poison_level() >= 1) e = hipMemset(p, 0xA5, want);
    return e;
}

namespace {

constexpr int TPB = 256;

inline uint32_t blocks_for(uint64_t n) {
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((n + TPB - 1) / TPB, 1u << 16)));
}

struct Scalars {
    uint32_t error;       // 1 group id outside group_id_to_pos, 2 row outside the matrix, 3 positions not increasing
    uint32_t need_host;
    uint32_t num_ranges;
    uint32_t max_read_id;
    uint32_t regroup;     // a group too long for the in-group ranking: redo with the radix sorts
    uint32_t long_reads;  // some id's entries span >= max_fragment_length: flushes may split it (k_split_update)
    uint32_t split_changed;
    uint32_t id_exceeded;  // the id space is larger than the caller assumed (the size of the previous call)
    uint32_t max_read_entries;  // kept entries of the longest read id run
    uint32_t caps_wrong;        // the locus ranges were cut for the count tile, and the pair bound forbids it
    uint32_t n_multi_id;        // entries whose read id occurs more than once in its chromosome (k_compact_m)
    uint32_t reads_total;       // reads of the whole pileup (k_ranks_runs)
    uint32_t n_wide;            // kept entries whose read reaches beyond their 8-locus windows (k_m_records / k_records)
    uint32_t max_range_span;    // loci of the longest locus range (k_ranges_compact; accumulate_counts' instance)
    // ticket words of the kernels whose last workgroup finishes the job (last_workgroup): zero between launches
    uint32_t ticket_ids, ticket_reads;
    unsigned long long id_space;  // sum over chromosomes of (largest - smallest read id + 1)
    unsigned long long multi_entries;
    unsigned long long pair_bound;
};

// Scalar read-backs. hipMemcpyAsync + hipStreamSynchronize leaves the GPU idle for 30-40 us per
// read-back (interrupt, wake-up, the first launches after it); instead a one-lane kernel publishes the
// scalars into pinned, coherent (fine-grained: visible to the host while the stream is still running,
// whatever HIP_HOST_COHERENT says) host memory and the host polls the sequence word next to them.
struct Mailbox {
    Scalars sc;
    unsigned long long totals;
    unsigned long long seq;
};

__global__ void k_publish(const Scalars *sc, const unsigned long long *totals, Mailbox *box, unsigned long long seq) {
    if (threadIdx.x == 0) {
        box->sc = *sc;
        box->totals = totals ? *totals : 0ull;
        __hip_atomic_store(&box->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// A word another workgroup of the same launch, or a kernel on the other stream, may have written: read at device scope
template <class T>
__device__ __forceinline__ T load_dev(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ void store_dev(T *p, T v) {  // write-through: at the device's coherence point when it has left
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ---- the last workgroup finishes the job -------------------------------------------------------------------------
// A serial step behind a grid (the id bases, the scan of the blocks' sums, the publishing of a read-back) without a
// one-workgroup launch of its own: every workgroup ends with one relaxed fetch_add on a ticket word, and the workgroup
// that draws the last ticket does the step and puts the ticket back to zero. Nobody waits for anybody. Two rules
// keep it cheap (round 32 measured the other way: an agent-scope release per workgroup, +301 us on C3):
//  * the few words that are handed over are written with atomics or store_dev (write-through), so no workgroup needs
//    a release -- every wave only waits until its own stores have left, then the barrier, then the ticket; the last
//    workgroup's first lane acquires once, and reads them with load_dev;
//  * the grid is a few hundred workgroups at the most: the tickets are same-address atomics, tens of ns each.
// All threads of every workgroup of the grid call it, once (it holds barriers).
__device__ __forceinline__ bool last_workgroup(uint32_t *ticket) {
    __shared__ uint32_t s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = drawn + 1u == gridDim.x;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            store_dev(ticket, 0u);
        }
        s_last = last ? 1u : 0u;
    }
    __syncthreads();
    return s_last != 0u;
}
// A read-back whose publishing is folded into the kernel in front of it: one lane of that kernel copies the scalars
// and releases the sequence word (k_publish's body). box == null: nothing is published here (the plain copies, or a
// call site that launches k_publish).
struct Publish {
    Mailbox *box;
    unsigned long long seq;
    const unsigned long long *totals;
};
__device__ __forceinline__ void publish_scalars(const Scalars *sc, const Publish &pub) {  // (one lane)
    static_assert(sizeof(Scalars) % 4 == 0, "copied word by word");
    const uint32_t *src = reinterpret_cast<const uint32_t *>(sc);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&pub.box->sc);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(Scalars) / 4; ++i) dst[i] = load_dev(src + i);
    pub.box->totals = pub.totals ? load_dev(pub.totals) : 0ull;
    __hip_atomic_store(&pub.box->seq, pub.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
bool plain_readback() {  // (asked per packing, not once per process: a test takes both ways on one handle)
    const char *e = std::getenv("SECEDO_PACK_READBACK");
    return e && std::strcmp(e, "memcpy") == 0;
}
Mailbox *mailbox_of(DevicePacked &pk) {  // null: no mailbox wanted or to be had
    if (plain_readback()) return nullptr;
    if (!pk.mailbox && !pk.mailbox_failed) {
        if (hipHostMalloc(&pk.mailbox, sizeof(Mailbox), hipHostMallocCoherent) == hipSuccess) {
            std::memset(pk.mailbox, 0, sizeof(Mailbox));
        } else {  // no pinned memory to be had: the plain copies
            (void)hipGetLastError();
            pk.mailbox = nullptr;
            pk.mailbox_failed = true;
        }
    }
    return static_cast<Mailbox *>(pk.mailbox);
}
// the sequence number of the next read-back, for the kernel that publishes it; read_scalars(.., &folded) waits for it
Publish fold_publish(DevicePacked &pk, const unsigned long long *totals) {
    Mailbox *box = mailbox_of(pk);
    return Publish{box, box ? ++pk.mailbox_seq : 0ull, totals};
}

// behind: launches that do not touch the scalars and whose results the caller wants whatever the scalars say. They
// are enqueued behind the publishing kernel and in front of the wait: the host has the scalars as early as without
// them, and the GPU has work while the host acts on them.
// folded: the kernel last launched on `stream` publishes (fold_publish): nothing is launched here, only `behind` is
// enqueued and the word polled. Without a mailbox (folded->box == null) the plain copies, as ever.
hipError_t read_scalars(DevicePacked &pk, hipStream_t stream, const Scalars *sc, const unsigned long long *totals,
                        Scalars *out, unsigned long long *out_totals, const std::function<void()> &behind = nullptr,
                        const Publish *folded = nullptr) {
    hipError_t e;
    Mailbox *const mailbox = folded ? folded->box : mailbox_of(pk);
    if (mailbox) {
        Mailbox *box = mailbox;
        unsigned long long seq;
        if (folded) {
            seq = folded->seq;
        } else {
            seq = ++pk.mailbox_seq;
            hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, stream, sc, totals, box, seq);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (behind) behind();
        // poll; every few thousand polls ask the runtime whether the stream died or drained without
        // the word arriving (then the plain copy below reports what happened)
        bool arrived = false;
        for (unsigned spins = 0;; ++spins) {
            if (__atomic_load_n(&box->seq, __ATOMIC_ACQUIRE) == seq) {
                arrived = true;
                break;
            }
            if ((spins & 0xFFFu) == 0xFFFu) {
                const hipError_t q = hipStreamQuery(stream);
                if (q != hipErrorNotReady) {
                    arrived = __atomic_load_n(&box->seq, __ATOMIC_ACQUIRE) == seq;
                    if (q != hipSuccess) return q;
                    break;
                }
            }
        }
        if (arrived) {
            *out = box->sc;
            if (out_totals) *out_totals = box->totals;
            return hipSuccess;
        }
    } else if (behind) {
        behind();
    }
    if (out_totals) {
        *out_totals = 0;
        if (totals && (e = hipMemcpyAsync(out_totals, totals, 8, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    }
    if ((e = hipMemcpyAsync(out, sc, sizeof(*out), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}

// SECEDO_PACK_TRACE=1: host-side time stamps of the packing's launch sequence on stderr
struct HostTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    HostTrace() : on(std::getenv("SECEDO_PACK_TRACE") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *what) const {
        if (on)
            std::fprintf(stderr, "[pack-trace] %8.1f us  %s\n",
                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), what);
    }
};

// Grouping without a sort (entries by read id, kept entries by (cell block, locus)): histogram of
// the group sizes, exclusive scan, scatter with an atomic cursor (arbitrary order inside a group),
// then every element finds its rank inside its group by scanning the group -- groups are short
// (a read covers a few loci; a cell block has a few entries at a locus), so this costs a few cached
// reads per element where a radix sort costs 4-7 passes over the data. The result is the order a
// stable sort gives. A group longer than kRankScanLimit raises Scalars::regroup and the caller
// falls back to the radix sorts.
constexpr uint32_t kRankScanLimit = 8192;
constexpr int kMaxSplitRounds = 32;  // rounds of k_split_update before the host emulation takes over
// the counting scheme for read ids needs a table over the id space: used while max id < factor * entries
constexpr uint32_t kIdSpaceFactor = 4;

struct Raw {  // by-value kernel argument: the raw pileup
    const uint32_t *chr_locus_off;
    uint32_t n_chr;
    const uint32_t *locus_pos;
    const uint64_t *locus_entry_off;
    const uint32_t *read_ids;
    const uint16_t *id_base16;
    const uint32_t *id_base32;
    const uint32_t *g2p;
    uint32_t n_groups;
    uint32_t n_loci;
    uint32_t n_entries;
    __device__ __forceinline__ uint32_t id_base(uint32_t e) const {
        return id_base16 ? (uint32_t)id_base16[e] : id_base32[e];
    }
};

// index of the last element <= x in a non-decreasing array a[0..n) with a[0] <= x  (u64 / u32)
template <class T>
__device__ __forceinline__ uint32_t last_le(const T *a, uint32_t n, T x) {
    uint32_t lo = 0, hi = n;  // invariant: a[lo] <= x, (hi == n or a[hi] > x)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// entry -> locus, one wave per locus (coalesced; empty loci cost nothing); lane 0 also checks that the
// positions increase strictly inside a chromosome (the reference asserts it, similarity_matrix.cpp:398)
__global__ __launch_bounds__(TPB) void k_entry_locus(Raw in, uint32_t *entry_locus, Scalars *sc) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TPB + threadIdx.x) >> 6, n_waves = (gridDim.x * TPB) >> 6;
    for (uint32_t l = wave; l < in.n_loci; l += n_waves) {
        const uint32_t b = (uint32_t)in.locus_entry_off[l], e = (uint32_t)in.locus_entry_off[l + 1];
        for (uint32_t i = b + lane; i < e; i += 64u) entry_locus[i] = l;
        if (lane == 0u && l + 1 < in.n_loci && in.locus_pos[l + 1] <= in.locus_pos[l]) {
            // allowed only across a chromosome boundary
            const uint32_t c = last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, l);
            if (l + 1 < in.chr_locus_off[c + 1]) sc->error = 3;
        }
    }
}

// first entry of chromosome c (c <= n_chr: the last one is the number of entries). Empty chromosomes share a start
// with their successor, trailing empty ones start at the end
__device__ __forceinline__ uint32_t chr_first_entry(const Raw &in, uint32_t c) {
    return (uint32_t)in.locus_entry_off[in.chr_locus_off[c]];
}

// per chromosome the largest and the smallest read id (the latter as max of ~id, so that zero-filled
// memory is the neutral element). A workgroup owns a contiguous chunk of entries and cuts it at the
// chromosome boundaries: one pair of atomics per (workgroup, chromosome) -- same-address atomics
// are slow.
// It also checks that the positions increase strictly inside a chromosome (the reference asserts it,
// similarity_matrix.cpp:398): a thread per locus, in front of the ids -- the single-entry path launches no
// k_entry_locus, which checks the same.
__device__ __forceinline__ void id_range_chunk(const Raw &in, uint32_t *id_max, uint32_t *id_negmin, int vec, Scalars *sc) {
    __shared__ uint32_t s_hi[TPB / 64], s_neg[TPB / 64];
    __shared__ uint32_t s_chr;
    for (uint32_t l = blockIdx.x * TPB + threadIdx.x; l + 1 < in.n_loci; l += gridDim.x * TPB) {
        if (in.locus_pos[l + 1] <= in.locus_pos[l]) {
            // allowed only across a chromosome boundary
            const uint32_t c = last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, l);
            if (l + 1 < in.chr_locus_off[c + 1]) sc->error = 3;
        }
    }
    const uint32_t E = in.n_entries;
    const uint32_t chunk = (E + gridDim.x - 1) / gridDim.x;
    uint32_t cur = min(E, blockIdx.x * chunk);
    const uint32_t e1 = min(E, cur + chunk);
    if (cur >= e1) return;
    // The chromosome of the chunk's first entry: the last one that starts at or before it. Every thread looks at the
    // chromosomes tid, tid + TPB, ...: two dependent reads per thread whatever their number. (A binary search over
    // the loci was 16 dependent reads in front of every workgroup's chunk and most of this kernel's time; until
    // round 17 the entry's locus came from k_entry_locus' table.)
    if (threadIdx.x == 0) s_chr = 0;
    __syncthreads();
    {
        uint32_t best = 0;
        for (uint32_t i = threadIdx.x; i < in.n_chr; i += TPB)
            if (chr_first_entry(in, i) <= cur) best = i;  // (ascending: the last hit is the largest)
        if (best) atomicMax(&s_chr, best);
    }
    __syncthreads();
    uint32_t c = s_chr;
    while (cur < e1) {
        // entries of chromosome c end where its last locus ends (skip chromosomes without entries)
        uint32_t c_end = (uint32_t)in.locus_entry_off[in.chr_locus_off[c + 1]];
        while (c_end <= cur && c + 1 < in.n_chr) {
            ++c;
            c_end = (uint32_t)in.locus_entry_off[in.chr_locus_off[c + 1]];
        }
        const uint32_t seg_end = (c + 1 < in.n_chr) ? min(e1, c_end) : e1;
        uint32_t hi = 0, neg = 0;
        uint32_t s_cur = cur, s_end = seg_end;  // what the scalar loop below is left with
        if (vec) {  // (the ids 16 bytes per lane, four loads in flight; the few before / behind the aligned part one by one)
            const uint32_t a = min(seg_end, (cur + 3u) & ~3u), b = max(a, seg_end & ~3u);
            if (threadIdx.x < a - cur) {
                const uint32_t id = in.read_ids[cur + threadIdx.x];
                hi = max(hi, id);
                neg = max(neg, ~id);
            }
            if (threadIdx.x < seg_end - b) {
                const uint32_t id = in.read_ids[b + threadIdx.x];
                hi = max(hi, id);
                neg = max(neg, ~id);
            }
            const uint4 *src = reinterpret_cast<const uint4 *>(in.read_ids);
            for (uint32_t q = a / 4u + threadIdx.x; q < b / 4u; q += TPB * 4) {
                uint4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = q + (uint32_t)u * TPB < b / 4u ? src[q + (uint32_t)u * TPB] : src[q];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    hi = max(max(hi, v[u].x), max(max(v[u].y, v[u].z), v[u].w));
                    neg = max(max(neg, ~v[u].x), max(max(~v[u].y, ~v[u].z), ~v[u].w));
                }
            }
            s_cur = s_end = seg_end;
        }
        // (eight loads of a thread in flight: one at a time, the kernel was 49 us of waiting on C3)
        for (uint32_t e = s_cur + threadIdx.x; e < s_end; e += TPB * 8) {
            uint32_t id[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t eu = e + (uint32_t)u * TPB;
                id[u] = eu < s_end ? in.read_ids[eu] : in.read_ids[e];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                hi = max(hi, id[u]);
                neg = max(neg, ~id[u]);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            hi = max(hi, (uint32_t)__shfl_down(hi, off));
            neg = max(neg, (uint32_t)__shfl_down(neg, off));
        }
        __syncthreads();  // the previous segment's partials have been read
        if ((threadIdx.x & 63u) == 0) {
            s_hi[threadIdx.x >> 6] = hi;
            s_neg[threadIdx.x >> 6] = neg;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < TPB / 64; ++w) {
                hi = max(hi, s_hi[w]);
                neg = max(neg, s_neg[w]);
            }
            atomicMax(&id_max[c], hi);
            atomicMax(&id_negmin[c], neg);
        }
        cur = seg_end;
    }
}

// ... and, by the last workgroup (the extremes are atomics: last_workgroup), the dense numbering of (chromosome, read
// id): id_base[c] + id - smallest id of c; the other lanes write the chromosomes' first entries, chr_entry[0 .. n_chr],
// for the kernels that find an entry's chromosome from its index. (A kernel of its own, k_id_bases, until round 32.)
__global__ __launch_bounds__(TPB) void k_id_range(Raw in, uint32_t *id_max, uint32_t *id_negmin, int vec,
                                                 uint32_t *id_base, uint32_t *chr_entry,
                                                 unsigned long long assumed_space, Scalars *sc) {
    id_range_chunk(in, id_max, id_negmin, vec, sc);
    if (!last_workgroup(&sc->ticket_ids)) return;
    const uint32_t n_chr = in.n_chr;
    for (uint32_t c = threadIdx.x; c <= n_chr; c += TPB) chr_entry[c] = chr_first_entry(in, c);
    if (threadIdx.x != 0) return;
    unsigned long long sum = 0;
    uint32_t top = 0;
    for (uint32_t c = 0; c < n_chr; ++c) {
        id_base[c] = (uint32_t)min(sum, 0xFFFFFFFFull);
        const uint32_t hi = load_dev(id_max + c), neg = load_dev(id_negmin + c);
        if ((hi | neg) != 0u) sum += (unsigned long long)(hi - ~neg) + 1ull;  // has entries
        top = max(top, hi);
    }
    id_base[n_chr] = (uint32_t)min(sum, 0xFFFFFFFFull);
    sc->id_space = sum;
    sc->max_read_id = top;
    // the caller may have sized the histogram from the previous call without waiting for this kernel
    if (assumed_space && sum > assumed_space) sc->id_exceeded = 1;
}

// radix path: sort key (chromosome, read id) with the read id in id_bits bits
__global__ void k_entry_keys(Raw in, const uint32_t *entry_locus, uint32_t id_bits, unsigned long long *key,
                             uint32_t *val) {
    for (uint32_t e = blockIdx.x * TPB + threadIdx.x; e < in.n_entries; e += gridDim.x * TPB) {
        const uint32_t c = last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, entry_locus[e]);
        key[e] = ((unsigned long long)c << id_bits) | in.read_ids[e];
        val[e] = e;
    }
}

// Per entry in sorted order: locus (30 bits) | base << 30. Written once with the one gather by entry
// index; the kernels of stages 2-4 then read it sequentially instead of gathering through sval.
constexpr uint32_t kSlocLocusMask = 0x3FFFFFFFu;
__device__ __forceinline__ uint32_t sloc_pack(uint32_t locus, uint32_t id_base) { return locus | (id_base << 30); }
__device__ __forceinline__ uint32_t sloc_locus(uint32_t v) { return v & kSlocLocusMask; }
__device__ __forceinline__ uint32_t sloc_base(uint32_t v) { return v >> 30; }

// radix path (the counting path writes sloc in k_id_rank)
__global__ void k_sorted_locus(Raw in, const uint32_t *sval, const uint32_t *entry_locus, uint32_t n, uint32_t *sloc) {
    for (uint32_t s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB)
        sloc[s] = sloc_pack(entry_locus[sval[s]], in.id_base(sval[s]));
}

// The dense id of an entry: its chromosome, then two per-chromosome words. The chromosome is a search over the
// chromosomes' first loci with the entry's locus as the key (`first` = chr_locus_off: the general path, which has the
// entry -> locus table), or over their first ENTRIES with the entry's index (`first` = chr_entry, k_id_range: the
// single-entry path, which has no such table -- the same search, no per-entry read in front of it). Empty chromosomes
// share a start with their successor and last_le picks the last of them, the one that holds the key.
// From LDS when the tables fit: from global memory the search is a chain of log2(C) dependent loads in front of
// whatever the kernel does with the id (k_id_store: 156 -> 117 us on C3).
constexpr uint32_t kChrLds = 1024;
struct ChrTables {
    uint32_t first[kChrLds + 1], base[kChrLds], min_id[kChrLds];
};
__device__ __forceinline__ bool chr_tables_load(const Raw &in, const uint32_t *first, const uint32_t *id_base,
                                                const uint32_t *id_negmin, ChrTables &t) {  // (all threads; ends with a barrier)
    const bool in_lds = in.n_chr <= kChrLds;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i <= in.n_chr; i += blockDim.x) t.first[i] = first[i];
        for (uint32_t i = threadIdx.x; i < in.n_chr; i += blockDim.x) {
            t.base[i] = id_base[i];
            t.min_id[i] = ~id_negmin[i];
        }
    }
    __syncthreads();
    return in_lds;
}
__device__ __forceinline__ uint32_t chr_of(const Raw &in, const uint32_t *first, const ChrTables &t, bool in_lds,
                                           uint32_t key) {
    return last_le<uint32_t>(in_lds ? t.first : first, in.n_chr + 1, key);
}
__device__ __forceinline__ uint32_t dense_of(const uint32_t *id_base, const uint32_t *id_negmin, const ChrTables &t,
                                             bool in_lds, uint32_t c, uint32_t id) {
    return in_lds ? t.base[c] + (id - t.min_id[c]) : id_base[c] + (id - ~id_negmin[c]);
}
__device__ __forceinline__ uint32_t dense_id(const Raw &in, const uint32_t *first, const uint32_t *id_base,
                                             const uint32_t *id_negmin, const ChrTables &t, bool in_lds, uint32_t key,
                                             uint32_t id) {
    return dense_of(id_base, id_negmin, t, in_lds, chr_of(in, first, t, in_lds, key), id);
}
// ... of four consecutive entries e0 .. e0 + 3 by their indices: one search where the first and the last are in the
// same chromosome (all but the quads that straddle a boundary)
__device__ __forceinline__ void dense_id_quad(const Raw &in, const uint32_t *chr_entry, const uint32_t *id_base,
                                              const uint32_t *id_negmin, const ChrTables &t, bool in_lds, uint32_t e0,
                                              const uint32_t (&id)[4], uint32_t (&d)[4]) {
    const uint32_t c0 = chr_of(in, chr_entry, t, in_lds, e0);
    const uint32_t next = in_lds ? t.first[c0 + 1] : chr_entry[c0 + 1];  // (c0 < n_chr: e0 is an entry)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t e = min(e0 + (uint32_t)u, in.n_entries - 1u);  // (the last quad may reach beyond the entries)
        const uint32_t c = e < next ? c0 : chr_of(in, chr_entry, t, in_lds, e);
        d[u] = dense_of(id_base, id_negmin, t, in_lds, c, id[u]);
    }
}

// counting path, entries by (chromosome, read id) through the dense numbering
__global__ void k_id_hist(Raw in, const uint32_t *entry_locus, const uint32_t *id_base, const uint32_t *id_negmin,
                          const Scalars *sc, uint32_t *dense, uint32_t *hist) {
    if (sc->id_exceeded) return;  // the table is too small: the caller starts over (k_id_rank)
    __shared__ ChrTables tables;
    const bool in_lds = chr_tables_load(in, in.chr_locus_off, id_base, id_negmin, tables);
    for (uint32_t e = blockIdx.x * TPB + threadIdx.x; e < in.n_entries; e += gridDim.x * TPB) {
        const uint32_t d = dense_id(in, in.chr_locus_off, id_base, id_negmin, tables, in_lds, entry_locus[e], in.read_ids[e]);
        dense[e] = d;
        atomicAdd(&hist[d], 1u);
    }
}

__global__ void k_id_scatter(const uint32_t *dense, uint32_t n, const uint32_t *id_off, const Scalars *sc,
                             uint32_t *hist, uint32_t *grouped) {
    if (sc->id_exceeded) return;
    for (uint32_t e = blockIdx.x * TPB + threadIdx.x; e < n; e += gridDim.x * TPB) {
        const uint32_t d = dense[e];
        grouped[id_off[d] + atomicSub(&hist[d], 1u) - 1u] = e;
    }
}

// rank inside the read's group = number of its entries with a smaller index: the entries of a read
// end up in pileup order (by locus), as a stable sort leaves them
__global__ void k_id_rank(Raw in, const uint32_t *dense, const uint32_t *id_off, const uint32_t *grouped,
                          const uint32_t *entry_locus, unsigned long long *skey, uint32_t *sval, uint32_t *sloc,
                          Scalars *sc) {
    const bool void_run = sc->id_exceeded != 0;
    for (uint32_t p = blockIdx.x * TPB + threadIdx.x; p < in.n_entries; p += gridDim.x * TPB) {
        if (void_run) {  // keep what follows inside its arrays until the host sees the flag and starts over
            skey[p] = p;
            sval[p] = p;
            sloc[p] = 0;
            continue;
        }
        const uint32_t e = grouped[p];
        const uint32_t d = dense[e];
        const uint32_t b = id_off[d], n = id_off[d + 1] - b;
        uint32_t rank = p - b;
        if (n > kRankScanLimit) {
            sc->regroup = 1;
        } else if (n > 1) {
            rank = 0;
            for (uint32_t q = b; q < b + n; ++q) rank += grouped[q] < e ? 1u : 0u;
        }
        skey[b + rank] = d;  // equal keys <=> same read; ascending in (chromosome, read id)
        sval[b + rank] = e;
        sloc[b + rank] = sloc_pack(entry_locus[e], in.id_base(e));  // the one gather by entry index
    }
}

// ---- stage 1 of the single-entry fast path: which ids repeat, and the reads of those that do ------------------
// Only WHICH ids occur more than once is wanted of all entries; how often and where only of the few that do. So the
// entries do not count their id and they need no atomic: every entry STORES its number in its id's slot (k_id_store:
// one of the entries of an id wins, whichever), then every entry looks whether the slot holds its own number
// (k_id_check): if not, its id occurs again -- it flags itself and the winner, so every entry of a repeated id ends up
// flagged, and the winner stands for the read. Two passes of plain coalesced stores and loads (the ids of
// neighbouring entries are neighbours) where one atomic per entry took 185-220 us on C3 (device-scope atomics are
// executed at the memory side), and the 48 MB table needs no zeroing: a slot is read only by entries that wrote it.
// The flags are a byte per entry IN PILEUP ORDER: numbering the M entries is a pass over 13 MB (k_flag_count,
// k_flag_scan, k_compact_m) where a scan that gathers hist[dense[e]] took 155 us; the reads of the M entries are
// the groups of equal winner (k_m_fields counts them per winner, a scan over the M entries, k_group_scatter,
// k_group_rank): no offsets over the id space (104 us), no histogram of the repeated ids.
// (kFlagBlock entries per workgroup of the numbering passes: pack_workspace.hpp)
// (a thread takes four consecutive entries, 16 bytes per lane and stream; `vec`: the caller's read-id array is 16-byte
// aligned -- the tables of this file are)
// (The dense id is made twice, here and in k_id_check, from the entry's id and index: until round 17 this kernel read
// an entry -> locus table for the chromosome and stored the dense id for k_id_check, 4 bytes per entry each way.)
__device__ __forceinline__ void load_id_quad(const Raw &in, uint32_t q, int vec, uint32_t (&id)[4]) {
    const uint32_t n = in.n_entries, e0 = q * 4u;
    if (vec && e0 + 4u <= n) {
        const uint4 iv = reinterpret_cast<const uint4 *>(in.read_ids)[q];
        id[0] = iv.x, id[1] = iv.y, id[2] = iv.z, id[3] = iv.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) id[u] = in.read_ids[min(e0 + (uint32_t)u, n - 1u)];
    }
}
__global__ void k_id_store(Raw in, const uint32_t *chr_entry, const uint32_t *id_base, const uint32_t *id_negmin,
                           const Scalars *sc, uint32_t *last, int vec) {
    if (sc->id_exceeded) return;  // the table is too small: no flags, no M entries; the caller starts over
    __shared__ ChrTables tables;
    const bool in_lds = chr_tables_load(in, chr_entry, id_base, id_negmin, tables);
    const uint32_t n = in.n_entries, stride = gridDim.x * TPB;
    for (uint32_t q = blockIdx.x * TPB + threadIdx.x; q < (n + 3u) / 4u; q += stride) {
        const uint32_t e0 = q * 4u;
        uint32_t id[4], d[4];
        load_id_quad(in, q, vec, id);
        dense_id_quad(in, chr_entry, id_base, id_negmin, tables, in_lds, e0, id, d);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + (uint32_t)u < n) last[d[u]] = e0 + (uint32_t)u + 1u;
    }
}
__global__ void k_id_check(Raw in, const uint32_t *chr_entry, const uint32_t *id_base, const uint32_t *id_negmin,
                           const Scalars *sc, const uint32_t *last, uint8_t *multi, int vec) {
    if (sc->id_exceeded) return;
    __shared__ ChrTables tables;
    const bool in_lds = chr_tables_load(in, chr_entry, id_base, id_negmin, tables);
    const uint32_t n = in.n_entries, stride = gridDim.x * TPB;
    for (uint32_t q = blockIdx.x * TPB + threadIdx.x; q < (n + 3u) / 4u; q += stride) {
        const uint32_t e0 = q * 4u;
        uint32_t id[4], d[4], w[4];
        load_id_quad(in, q, vec, id);
        dense_id_quad(in, chr_entry, id_base, id_negmin, tables, in_lds, e0, id, d);
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = e0 + (uint32_t)u < n ? last[d[u]] : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = e0 + (uint32_t)u;
            if (e < n && w[u] != e + 1u) {
                multi[e] = 1;
                multi[w[u] - 1u] = 1;
            }
        }
    }
}
// exclusive offsets of n_blocks block sums by the THREADS threads of ONE workgroup (3000 blocks on C3); returns the
// total in every thread. The sums are read at device scope: in a kernel's last workgroup other workgroups wrote them.
constexpr int TPB_SCAN = 1024;
template <int THREADS>
__device__ __forceinline__ uint32_t scan_block_sums(const uint32_t *block_sum, uint32_t n_blocks, uint32_t *block_off) {
    __shared__ uint32_t part[THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t carry = 0;  // (uniform)
    for (uint32_t base = 0; base < n_blocks; base += THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? load_dev(block_sum + i) : 0u;
        uint32_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= (uint32_t)off) incl += up;
        }
        __syncthreads();  // the previous round's partials have been read
        if (lane == 63u) part[wv] = incl;
        __syncthreads();
        uint32_t before = carry;
#pragma unroll
        for (int w2 = 0; w2 < THREADS / 64; ++w2) {
            const uint32_t pw = part[w2];
            if ((uint32_t)w2 < wv) before += pw;
            carry += pw;
        }
        if (i < n_blocks) block_off[i] = before + incl - v;
    }
    return carry;
}
// flags per block of kFlagBlock entries (the flag array is zero-padded to whole blocks)
// (Round 32 measured the scan as this kernel's tail -- 256 workgroups, a wave per block, sums written through, the last
// workgroup scans --: 22.8 us against 5.5 + 7.8 for the two kernels on C3. A kernel this short has nothing to hide
// 256 tickets behind.)
__global__ __launch_bounds__(TPB) void k_flag_count(const uint8_t *multi, uint32_t *block_sum) {
    __shared__ uint32_t part[TPB / 64];
    static_assert(kFlagBlock == TPB * 16, "a thread takes 16 consecutive flags");
    const uint4 w = reinterpret_cast<const uint4 *>(multi + (size_t)blockIdx.x * kFlagBlock)[threadIdx.x];
    uint32_t n = ((w.x * 0x01010101u) >> 24) + ((w.y * 0x01010101u) >> 24) + ((w.z * 0x01010101u) >> 24)
            + ((w.w * 0x01010101u) >> 24);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w2 = 1; w2 < TPB / 64; ++w2) n += part[w2];
        block_sum[blockIdx.x] = n;
    }
}
// the blocks' exclusive offsets as a kernel of its own, and the number of M entries
__global__ __launch_bounds__(TPB_SCAN) void k_flag_scan(const uint32_t *block_sum, uint32_t n_blocks, uint32_t *block_off,
                                                       uint32_t *total_out, Scalars *sc) {
    const uint32_t total = scan_block_sums<TPB_SCAN>(block_sum, n_blocks, block_off);
    if (threadIdx.x == 0u) {
        *total_out = total;  // the prefix of the closing chunk
        if (sc) sc->n_multi_id = total;  // (null: the flagged entries' lists, pack_flag_lists)
    }
}
// The numbering of the M entries, in the form the flagged entries' lists have below: per 64-entry chunk its flags
// (chunk_mask) and the M entries before it (chunk_pre) -- 12 bytes per 64 entries where the exclusive scan of the flags
// as an array (until round 17) was 4 bytes per entry, written here and read back by k_bin_hist for every entry to
// learn one bit. m_index(e) = M entries before entry e, for e <= E: both tables carry a closing chunk (no flags, all
// M entries before it) behind the last block, which is where E falls when it is a multiple of kFlagBlock.
struct MIndex {
    const uint32_t *chunk_pre;
    const unsigned long long *chunk_mask;
    __device__ __forceinline__ uint32_t operator()(uint32_t e) const {
        const uint32_t c = e >> 6, r = e & 63u;
        return chunk_pre[c] + (uint32_t)__popcll(chunk_mask[c] & ((1ull << r) - 1ull));
    }
};
// ... and the list of the M entries; k_m_fields, once their number is known, copies them out as a compacted pileup of
// their own and finds which of them holds its id's slot (the head its read is walked from). A thread takes 16
// consecutive flags, so four neighbouring lanes hold a chunk. (k_flag_scan writes the closing chunk's prefix.)
__global__ __launch_bounds__(TPB) void k_compact_m(Raw in, const uint8_t *multi, const uint32_t *block_off,
                                                  uint32_t *chunk_pre, unsigned long long *chunk_mask,
                                                  uint32_t *m_entry, uint32_t *count_m, Scalars *sc, Publish pub) {
    __shared__ uint32_t part[TPB / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t e0 = blockIdx.x * kFlagBlock + threadIdx.x * 16u;
    const uint4 w = reinterpret_cast<const uint4 *>(multi + (size_t)blockIdx.x * kFlagBlock)[threadIdx.x];
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    uint32_t bits = 0;  // this thread's 16 flags
#pragma unroll
    for (int i = 0; i < 16; ++i) bits |= ((words[i >> 2] >> ((i & 3) * 8)) & 1u) << i;
    const uint32_t mine = (uint32_t)__popc(bits);
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += up;
    }
    if (lane == 63u) part[wv] = incl;
    __syncthreads();
    uint32_t j = block_off[blockIdx.x] + incl - mine;
    for (uint32_t w2 = 0; w2 < wv; ++w2) j += part[w2];
    unsigned long long m = (unsigned long long)bits << ((lane & 3u) * 16u);
    m |= __shfl_xor(m, 1);
    m |= __shfl_xor(m, 2);
    if ((lane & 3u) == 0u) {  // (the padding behind the last entry holds no flags)
        const uint32_t chunk = blockIdx.x * (kFlagBlock / 64u) + (threadIdx.x >> 2);
        chunk_pre[chunk] = j;
        chunk_mask[chunk] = m;
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u) chunk_mask[gridDim.x * (kFlagBlock / 64u)] = 0ull;
    // (count_m: the M entries' counters of k_m_fields, n_m + 1 of them, zeroed where the M entries are numbered
    // instead of by a fill behind read-back 1b, which stood between the host's answer and k_m_fields)
    for (uint32_t b = bits; b; b &= b - 1u) {
        count_m[j] = 0u;
        m_entry[j++] = e0 + (uint32_t)__ffs((int)b) - 1u;
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == TPB - 1) count_m[j] = 0u;  // (j: all M entries)
    // Read-back 1b. What it carries (n_multi_id, the flags of the kernels in front) was complete before this kernel
    // began: the first workgroup publishes when it is through. The host therefore has the scalars while other
    // workgroups of this kernel still run -- a hand-over at read-back 1b (an error, a void attempt, the host packing)
    // no longer finds the stream drained. That is sound because whatever follows is enqueued on this stream or goes
    // through a synchronising hipFree, and this kernel writes scratch arenas only (M_ENTRY, M_CHUNKS, DENSE_M), which
    // the host packing's uploads do not replace (compare close_attempt's note on read-back 3).
    if (pub.box && blockIdx.x == 0u && threadIdx.x == 0u) publish_scalars(sc, pub);
}
// The same count -> scan -> compact chain numbers the FLAGGED entries of the packed pileup (C_TAIL | C_MULTI in
// entry32: the read was never flushed, or has further kept entries) for the correction of the sparse-loci pair
// kernel (pack_flag_lists). Here a workgroup's thread takes the words tid + k * TPB of its kFlagBlock entries (coalesced
// loads), so a wave's 64 entries of a round are consecutive: a 64-entry chunk, whose flags are one ballot.
__global__ __launch_bounds__(TPB) void k_pflag_count(const uint32_t *entry32, uint32_t n, uint32_t *block_sum) {
    __shared__ uint32_t part[TPB / 64];
    const uint32_t b0 = blockIdx.x * kFlagBlock + threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t e = b0 + (uint32_t)k * TPB;
        c += (e < n && (entry32[e] & (kC_Tail | kC_Multi)) != 0u) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w = 1; w < TPB / 64; ++w) c += part[w];
        block_sum[blockIdx.x] = c;
    }
}
// rec / idx: the flagged entries' records and indices, compact; per 64-entry chunk the flagged entries before it
// (chunk_pre) and its flags (chunk_mask) -- what k_pflag_groups needs of an exclusive scan over all entries, in 1/21
// of the bytes
__global__ __launch_bounds__(TPB) void k_pflag_compact(const uint32_t *entry32, const uint4 *entry, uint32_t n,
                                                      const uint32_t *block_off, uint4 *rec, uint32_t *idx,
                                                      uint32_t *chunk_pre, unsigned long long *chunk_mask) {
    constexpr int WAVES = TPB / 64;
    static_assert(16 * WAVES == 64, "one wave scans the (round, wave) counts");
    __shared__ uint32_t cnt[16 * WAVES];  // flagged entries per (round k, wave), in entry order
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t b0 = blockIdx.x * kFlagBlock + threadIdx.x;
    unsigned long long m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t e = b0 + (uint32_t)k * TPB;
        m[k] = __ballot(e < n && (entry32[e] & (kC_Tail | kC_Multi)) != 0u);
        if (lane == 0u) cnt[k * WAVES + wv] = (uint32_t)__popcll(m[k]);
    }
    __syncthreads();
    if (threadIdx.x < 64u) {
        const uint32_t v = cnt[threadIdx.x];
        uint32_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= (uint32_t)off) incl += up;
        }
        cnt[threadIdx.x] = incl - v;
    }
    __syncthreads();
    const uint32_t base = block_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t e = b0 + (uint32_t)k * TPB;
        const uint32_t before = base + cnt[k * WAVES + wv];
        if (lane == 0u) {
            const uint32_t chunk = (blockIdx.x * kFlagBlock + (uint32_t)k * TPB) / 64u + wv;
            chunk_pre[chunk] = before;
            chunk_mask[chunk] = m[k];
        }
        if ((m[k] >> lane) & 1ull) {
            const uint32_t j = before + (uint32_t)__popcll(m[k] & ((1ull << lane) - 1ull));
            rec[j] = entry[e];
            idx[j] = e;
        }
    }
}
// The same lists where k_entry_records has left the chunks' flags (chunk_mask, one ballot per 64 entries) and the
// blocks' sums behind it: this pass reads 8 bytes per 64 entries where k_pflag_compact reads entry32 a third time,
// and the count pass is gone. A wave takes the chunks wave + k * WAVES of its block, in k_pflag_compact's numbering.
__global__ __launch_bounds__(TPB) void k_pflag_compact_masks(const unsigned long long *chunk_mask, const uint4 *entry,
                                                            const uint32_t *block_off, uint4 *rec, uint32_t *idx,
                                                            uint32_t *chunk_pre) {
    constexpr int WAVES = TPB / 64;
    constexpr uint32_t CHUNKS = kFlagBlock / 64u;
    static_assert(CHUNKS == 64, "one wave scans the chunks' counts");
    __shared__ unsigned long long mask[CHUNKS];
    __shared__ uint32_t pre[CHUNKS];  // flagged entries of the block before the chunk
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t chunk0 = blockIdx.x * CHUNKS;
    if (threadIdx.x < 64u) {
        const unsigned long long m = chunk_mask[chunk0 + threadIdx.x];
        const uint32_t v = (uint32_t)__popcll(m);
        uint32_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= (uint32_t)off) incl += up;
        }
        mask[threadIdx.x] = m;
        pre[threadIdx.x] = incl - v;
        chunk_pre[chunk0 + threadIdx.x] = block_off[blockIdx.x] + incl - v;
    }
    __syncthreads();
    const uint32_t base = block_off[blockIdx.x];
#pragma unroll 4
    for (uint32_t c = wv; c < CHUNKS; c += WAVES) {
        const unsigned long long m = mask[c];
        if ((m >> lane) & 1ull) {  // (no flag lies behind the last entry: k_entry_records' ballots)
            const uint32_t e = (chunk0 + c) * 64u + lane;
            const uint32_t j = base + pre[c] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            rec[j] = entry[e];
            idx[j] = e;
        }
    }
}
// grp[i] = flagged entries before entry blk_off[i]: the flagged entries before each (block, locus) group. (An offset
// at the end of the last whole chunk reads the total behind the chunks, chunk_pre[n_chunks], and no mask.)
__global__ __launch_bounds__(TPB) void k_pflag_groups(const uint32_t *blk_off, size_t n_off, const uint32_t *chunk_pre,
                                                     const unsigned long long *chunk_mask, uint32_t *grp) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_off; i += (size_t)gridDim.x * TPB) {
        const uint32_t d = blk_off[i], c = d >> 6, r = d & 63u;
        grp[i] = chunk_pre[c] + (r ? (uint32_t)__popcll(chunk_mask[c] & ((1ull << r) - 1ull)) : 0u);
    }
}
// (the flag lists' scratch, struct FlagScratch: pack_workspace.hpp)
void flag_groups(const FlagScratch &fs, const uint32_t *blk_off, size_t n_off, uint32_t *grp, hipStream_t stream) {
    if (!n_off) return;
    const uint32_t blocks = (uint32_t)std::min<size_t>((n_off + TPB - 1) / TPB, 256 * 32);
    hipLaunchKernelGGL(k_pflag_groups, dim3(blocks), dim3(TPB), 0, stream, blk_off, n_off, fs.chunk_pre, fs.chunk_mask, grp);
}
// the lists behind a k_entry_records that has written fs.chunk_mask and fs.block_sum, and a k_records_tail that has
// scanned the sums
void flag_lists_from_masks(const FlagScratch &fs, const uint4 *entry, const uint32_t *blk_off, size_t n_off,
                           uint32_t *grp, uint4 *rec, uint32_t *idx, hipStream_t stream) {
    hipLaunchKernelGGL(k_pflag_compact_masks, dim3(fs.nb), dim3(TPB), 0, stream, fs.chunk_mask, entry, fs.block_off, rec,
                       idx, fs.chunk_pre);
    flag_groups(fs, blk_off, n_off, grp, stream);
}

// (the dense id once more, as in k_id_check; the locus of an M entry by a search over the loci's first entries -- the
// M entries are ascending, so neighbouring threads search neighbouring places --: the only entries whose locus the
// single-entry path ever looks up)
__global__ void k_m_fields(Raw in, const uint32_t *chr_entry, const uint32_t *id_base, const uint32_t *id_negmin,
                           const uint32_t *last, MIndex m_index, const uint32_t *m_entry, uint32_t n_m, uint32_t *rid_m,
                           uint32_t *idb_m, uint32_t *eloc_m, uint32_t *winner_m, uint32_t *count_m) {
    __shared__ ChrTables tables;
    const bool in_lds = chr_tables_load(in, chr_entry, id_base, id_negmin, tables);
    for (uint32_t j = blockIdx.x * TPB + threadIdx.x; j < n_m; j += gridDim.x * TPB) {
        const uint32_t e = m_entry[j];
        const uint32_t id = in.read_ids[e];
        rid_m[j] = id;
        idb_m[j] = in.id_base(e);
        eloc_m[j] = last_le<uint64_t>(in.locus_entry_off, in.n_loci + 1, (uint64_t)e);
        const uint32_t d = dense_id(in, chr_entry, id_base, id_negmin, tables, in_lds, e, id);
        const uint32_t w = m_index(last[d] - 1u);  // the M index of the entry that stands for this entry's id
        winner_m[j] = w;
        atomicAdd(&count_m[w], 1u);
    }
}
// the entries of a read next to each other (goff: exclusive sums of the counts; the counts are taken down again)
__global__ void k_group_scatter(const uint32_t *winner_m, uint32_t n_m, const uint32_t *goff, uint32_t *count_m,
                                uint32_t *members, uint32_t *g_begin, uint32_t *g_len) {
    for (uint32_t j = blockIdx.x * TPB + threadIdx.x; j < n_m; j += gridDim.x * TPB) {
        const uint32_t w = winner_m[j];
        const uint32_t b = goff[w], n = goff[w + 1] - b;
        members[b + atomicSub(&count_m[w], 1u) - 1u] = j;
        g_begin[j] = b;
        g_len[j] = n;
    }
}
// pileup order inside a read (the M indices grow with the pileup): a member's rank is the number of smaller members.
// skey: the read's first position stands for its id (equal keys <=> same read is all the stages behind need).
// (A read beyond kRankScanLimit keeps the order of the scatter and raises Scalars::regroup -- the attempt is void,
// the caller sorts --, but every position holds an entry.)
__global__ void k_group_rank(Raw sub, const uint32_t *members, const uint32_t *g_begin, const uint32_t *g_len,
                             const uint32_t *eloc_m, uint32_t n_m, unsigned long long *skey, uint32_t *sval,
                             uint32_t *sloc, Scalars *sc) {
    for (uint32_t p = blockIdx.x * TPB + threadIdx.x; p < n_m; p += gridDim.x * TPB) {
        const uint32_t m = members[p];
        const uint32_t b = g_begin[m], n = g_len[m];
        uint32_t rank = p - b;
        if (n > kRankScanLimit) {
            sc->regroup = 1;
        } else {
            rank = 0;
            for (uint32_t q = b; q < b + n; ++q) rank += members[q] < m ? 1u : 0u;
        }
        skey[b + rank] = b;
        sval[b + rank] = m;
        sloc[b + rank] = sloc_pack(eloc_m[m], sub.id_base(m));
    }
}

constexpr uint32_t kCibBits = 7;
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;  // low word of an entry_kc slot: the entry was dropped
// Single-entry fast path: an S entry (the only entry of its read) needs no k -- nothing of its read is looked
// up again -- so the low word of its entry_kc slot carries kSingle alone and its base sits above
// (block, cell in block) in the high word; k_bin_place turns the rank into the tail flag.
constexpr uint32_t kSingle = 0x80000000u;
constexpr uint32_t kSingleBaseShift = 29;  // in the high word of entry_kc (block << 7 | cell in block below)
constexpr uint32_t kSingleTail = 4u;       // in the low word of a grouped S entry: kSingle | tail | base

// ---- the single-entry fast path ---------------------------------------------------------------------
// With sparse loci nine reads in ten have ONE entry (k_id_check says which), and for those the whole
// read assembly -- scatter, rank, duplicate rule, per-read lists, per-read info -- is the identity. Only the
// entries of ids that occur more than once ("M entries") go through it, as a compacted pileup of their own
// (the kernels below see a Raw whose entry arrays are the compacted copies); the others ("S entries") meet
// them again at the appearance-rank scan (every S entry is the first and only entry of its read) and at
// the binning.
// Appearance rank of a pileup entry = marked entries before it. Single-entry fast path: every S entry is
// marked, so rank(e) = e - (unmarked M entries before e) = e - unm[m_index(e)], with unm the exclusive prefix of
// (1 - mark) over the M entries only -- a scan over 5 % of the pileup (C3) instead of one over all of it.
// Otherwise the ranks are an array (the scan over the marks).
struct Ranks {
    MIndex m_index;
    const uint32_t *unm;    // fast path (unm != null)
    const uint32_t *arank;  // or the array
    __device__ __forceinline__ uint32_t operator()(uint32_t e) const { return unm ? e - unm[m_index(e)] : arank[e]; }
};
struct UnmarkedM {  // input of the scan that gives unm
    const uint32_t *mark_m;
    uint32_t n_m;
    __device__ __forceinline__ uint32_t operator()(uint32_t j) const { return j < n_m ? 1u - mark_m[j] : 0u; }
};
// Input of the one scan over the sorted order: low word = first entry of a read (head of a run of
// equal keys), high word = the entry survives the duplicate rule. The inclusive sums give, per
// position, the 1-based read number and the number of kept entries up to and including it.
struct HeadKeepOp {
    const unsigned long long *skey;
    const uint32_t *keep;
    const uint32_t *split;  // 1 where a flush re-opens the id as a new read (k_split_update); null: nowhere
    __device__ __forceinline__ unsigned long long operator()(uint32_t s) const {
        const unsigned long long head = (s == 0 || skey[s] != skey[s - 1] || (split && split[s])) ? 1ull : 0ull;
        return head | ((unsigned long long)keep[s] << 32);
    }
};
__device__ __forceinline__ uint32_t incl_reads(unsigned long long v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t incl_kept(unsigned long long v) { return (uint32_t)(v >> 32); }

// duplicate-position rule (:387-395) per (read, locus) group of the sorted order, and the mark of
// every read's first entry (in pileup order) for the appearance rank
__global__ void k_dup_mark(Raw in, const unsigned long long *skey, const uint32_t *sval,
                           const uint32_t *sloc, const uint32_t *split, uint32_t n, uint32_t *keep,
                           uint32_t *mark) {
    for (uint32_t s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const uint32_t e = sval[s];
        const uint32_t l = sloc_locus(sloc[s]);
        const bool same_read = s > 0 && skey[s] == skey[s - 1];  // same id: a split starts at a new locus
        mark[e] = (same_read && !(split && split[s])) ? 0u : 1u;
        if (s == 0) mark[n] = 0u;
        if (same_read && sloc_locus(sloc[s - 1]) == l) continue;  // not a group head
        uint32_t stored = s;  // position of the stored entry of this (read, locus)
        bool have = true;
        keep[s] = 0u;
        for (uint32_t t = s + 1; t < n && skey[t] == skey[s] && sloc_locus(sloc[t]) == l; ++t) {
            keep[t] = 0u;
            if (have) {
                // second mate at the stored position: equal base -> ignored; different -> both go
                if (sloc_base(sloc[t]) != sloc_base(sloc[stored])) have = false;
            } else {
                stored = t;  // the position is free again: this entry is appended
                have = true;
            }
        }
        if (have) keep[stored] = 1u;
    }
}

// run starts (reads) and the per-read lists of kept entries (CSR payload)
__global__ void k_runs_csr(Raw in, const unsigned long long *incl, const uint32_t *sval,
                           const uint32_t *sloc, uint32_t n, uint32_t *run_start, uint32_t *read_locus,
                           uint8_t *read_base) {
    for (uint32_t s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const unsigned long long cur = incl[s], prev = s ? incl[s - 1] : 0ull;
        if (incl_reads(cur) != incl_reads(prev)) run_start[incl_reads(cur) - 1] = s;
        if (s == n - 1) run_start[incl_reads(cur)] = n;
        if (incl_kept(cur) != incl_kept(prev)) {
            const uint32_t k = incl_kept(prev), v = sloc[s];
            read_locus[k] = sloc_locus(v);
            read_base[k] = (uint8_t)sloc_base(v);
        }
    }
}
// Single-entry route, one launch for three independent things that all stand behind the two scans (k_arank_m, k_rbeg
// and k_runs_csr until round 32): the appearance ranks of the M entries (k_read_info reads the rank of a read's first
// entry) and the number of reads; the run starts and per-read lists as in k_runs_csr; per chromosome the first
// appearance rank. The grid is sized by the n_m M entries (`in` is the whole pileup) and walks the n_chr + 1
// chromosomes with its first threads.
__global__ void k_ranks_runs(Raw in, Ranks rank, const uint32_t *m_entry, uint32_t n_m, uint32_t *arank_m,
                             uint32_t *rbeg, const unsigned long long *incl, const uint32_t *sloc,
                             uint32_t *run_start, uint32_t *read_locus, uint8_t *read_base, Scalars *sc) {
    const uint32_t *unm = rank.unm;
    for (uint32_t s = blockIdx.x * TPB + threadIdx.x; s < n_m; s += gridDim.x * TPB) {
        arank_m[s] = m_entry[s] - unm[s];
        const unsigned long long cur = incl[s], prev = s ? incl[s - 1] : 0ull;
        if (incl_reads(cur) != incl_reads(prev)) run_start[incl_reads(cur) - 1] = s;
        if (s == n_m - 1) run_start[incl_reads(cur)] = n_m;
        if (incl_kept(cur) != incl_kept(prev)) {
            const uint32_t k = incl_kept(prev), v = sloc[s];
            read_locus[k] = sloc_locus(v);
            read_base[k] = (uint8_t)sloc_base(v);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->reads_total = in.n_entries - unm[n_m];
    for (uint32_t c = blockIdx.x * TPB + threadIdx.x; c <= in.n_chr; c += gridDim.x * TPB)
        rbeg[c] = rank((uint32_t)in.locus_entry_off[in.chr_locus_off[c]]);
}

// per read: span check, offsets into the per-read lists, appearance rank, start position in rank
// order, entries of multi-locus reads; per chromosome the first rank
__global__ __launch_bounds__(TPB) void k_read_info(Raw in, const unsigned long long *incl, const uint32_t *run_start,
                                                  const uint32_t *sval, const uint32_t *sloc,
                                                  const uint32_t *arank, uint32_t mfl, uint32_t *run_rank,
                                                  uint32_t *rbeg, uint32_t *read_off, Scalars *sc, Publish pub) {
    __shared__ unsigned long long part[TPB / 64];
    __shared__ uint32_t part_len[TPB / 64];
    const uint32_t n = in.n_entries;
    const uint32_t n_runs = n ? incl_reads(incl[n - 1]) : 0u;
    unsigned long long multi = 0;
    uint32_t longest = 0;
    for (uint32_t r = blockIdx.x * TPB + threadIdx.x; r < n_runs; r += gridDim.x * TPB) {
        const uint32_t s0 = run_start[r], s1 = run_start[r + 1];
        const uint32_t e0 = sval[s0];
        const uint32_t p0 = in.locus_pos[sloc_locus(sloc[s0])], p1 = in.locus_pos[sloc_locus(sloc[s1 - 1])];
        // a read whose entries reach start + mfl can be flushed before its last entry arrives and is
        // then re-opened as a new read (:368-371, :379-382): k_split_update finds where
        if (p1 - p0 >= mfl) store_dev(&sc->long_reads, 1u);  // (written through: the last workgroup publishes them)
        if ((unsigned long long)p1 + mfl > 0xFFFFFFFFull) store_dev(&sc->need_host, 1u);
        const uint32_t rk = arank[e0];
        run_rank[r] = rk;
        const uint32_t k0 = s0 ? incl_kept(incl[s0 - 1]) : 0u, k1 = incl_kept(incl[s1 - 1]);
        read_off[r] = k0;
        if (r == n_runs - 1) read_off[n_runs] = k1;
        if (k1 - k0 > 1) multi += k1 - k0;
        longest = max(longest, k1 - k0);
    }
    if (rbeg) {  // (the single-entry fast path has the ranks of all entries elsewhere: k_ranks_runs)
        for (uint32_t c = blockIdx.x * TPB + threadIdx.x; c <= in.n_chr; c += gridDim.x * TPB)
            rbeg[c] = arank[(uint32_t)in.locus_entry_off[in.chr_locus_off[c]]];
    }
    // one atomic per workgroup: same-address atomics are slow
    for (int off = 32; off > 0; off >>= 1) {
        multi += __shfl_down(multi, off);
        longest = max(longest, (uint32_t)__shfl_down(longest, off));
    }
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6] = multi;
        part_len[threadIdx.x >> 6] = longest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        uint32_t len = 0;
        for (int w = 0; w < TPB / 64; ++w) {
            sum += part[w];
            len = max(len, part_len[w]);
        }
        if (sum) atomicAdd(&sc->multi_entries, sum);
        if (len > 1) atomicMax(&sc->max_read_entries, len);  // reads of one entry are the rule: no atomic for them
    }
    // the read-back behind the build, published by the last workgroup: every workgroup's flags and sums are in
    if (pub.box && last_workgroup(&sc->ticket_reads) && threadIdx.x == 0) publish_scalars(sc, pub);
}

// completed-prefix count per locus (:348-352): reads of the chromosome with start + mfl <= position. A read
// starts at the position of its first entry, and `arank` counts the first entries in pileup order, so the
// reads that started at or before a locus are the ranks up to the end of that locus: a search over the
// chromosome's positions instead of a table of start positions per read.
__global__ void k_completed(Raw in, Ranks rank, const uint32_t *rbeg, uint32_t mfl, uint32_t *cnt, Scalars *sc) {
    for (uint32_t l = blockIdx.x * TPB + threadIdx.x; l < in.n_loci; l += gridDim.x * TPB) {
        const uint32_t c = last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, l);
        const uint32_t pos = in.locus_pos[l], l0 = in.chr_locus_off[c];
        if ((unsigned long long)pos + mfl > 0xFFFFFFFFull && in.locus_entry_off[l + 1] > in.locus_entry_off[l])
            sc->need_host = 1;  // start + mfl leaves 32 bits (the reference computes in uint32 there)
        uint32_t done = 0;
        if (pos >= mfl && in.locus_pos[l0] <= pos - mfl) {
            const uint32_t lp = l0 + last_le<uint32_t>(in.locus_pos + l0, l - l0 + 1, pos - mfl);
            done = rank((uint32_t)in.locus_entry_off[lp + 1]) - rbeg[c];
        }
        cnt[l] = done;
    }
}

// flush chain (:356-373): flushed = c(l) whenever c(l) - flushed >= 4 * num_threads. One workgroup
// per chromosome; the chain is sequential, so lane 0 walks LDS tiles of the counts.
// The loci at which a flush happens are listed per chromosome (flush_loci[l0 ..), flush_count[c]).
// (only when some id spans >= max_fragment_length -- Scalars::long_reads, set by k_read_info just
// before: nothing reads the list otherwise, and the bookkeeping triples the cost of the serial walk).
// Last, the first TAIL entry of the chromosome among the single-entry reads (tail_begin != null): such an entry
// is its read's first, the appearance ranks grow with the entry index, so "never flushed" -- rank - first rank of
// the chromosome >= flushed -- holds from one entry of the chromosome on. k_bin_place compares entry indices with
// it instead of looking every S entry's rank up. (A TPB-ary search: three rounds over 13 M entries.)
__global__ __launch_bounds__(TPB) void k_flush_chain(Raw in, const uint32_t *cnt, uint32_t threshold,
                                                    const Scalars *sc, uint32_t *flushed_out,
                                                    uint32_t *flush_loci, uint32_t *flush_count, Ranks rank,
                                                    const uint32_t *rbeg, uint32_t *tail_begin) {
    __shared__ uint32_t buf[2048];
    __shared__ uint32_t hits[2048];  // flush loci of the tile: the serial walk touches LDS only
    __shared__ uint32_t s_flushed, s_listed, s_hits;
    const uint32_t c = blockIdx.x;
    const uint32_t l0 = in.chr_locus_off[c], l1 = in.chr_locus_off[c + 1];
    if (threadIdx.x == 0) {
        s_flushed = 0;
        s_listed = 0;
    }
    for (uint32_t base = l0; base < l1; base += 2048) {
        const uint32_t n = min(2048u, l1 - base);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += TPB) buf[i] = cnt[base + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t f = s_flushed, h = 0;
            if (sc->long_reads) {
                for (uint32_t i = 0; i < n; ++i) {
                    const uint32_t v = buf[i];
                    if (v - f >= threshold) {  // v >= f: the counts never decrease
                        f = v;
                        hits[h++] = base + i;
                    }
                }
            } else {
                for (uint32_t i = 0; i < n; ++i) {
                    const uint32_t v = buf[i];
                    if (v - f >= threshold) f = v;
                }
            }
            s_flushed = f;
            s_hits = h;
        }
        __syncthreads();
        const uint32_t h = s_hits, listed = s_listed;
        for (uint32_t i = threadIdx.x; i < h; i += TPB) flush_loci[l0 + listed + i] = hits[i];
        __syncthreads();
        if (threadIdx.x == 0) s_listed = listed + h;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        flushed_out[c] = s_flushed;
        flush_count[c] = s_listed;
    }
    if (tail_begin) {
        __shared__ uint32_t s_first;
        const unsigned long long want = (unsigned long long)rbeg[c] + s_flushed;  // the first rank that is never flushed
        uint32_t lo = (uint32_t)in.locus_entry_off[l0], hi = (uint32_t)in.locus_entry_off[l1];
        // invariant: entries before lo have a smaller rank, the entry hi (or the chromosome's end) has not
        while (lo < hi) {  // (uniform)
            const uint32_t step = (hi - lo + TPB - 1) / TPB;
            const unsigned long long probe = (unsigned long long)lo + (unsigned long long)threadIdx.x * step;
            const bool reached = probe < hi && (unsigned long long)rank((uint32_t)probe) >= want;
            __syncthreads();
            if (threadIdx.x == 0) s_first = TPB;
            __syncthreads();
            if (reached) atomicMin(&s_first, threadIdx.x);
            __syncthreads();
            const uint32_t first = s_first;
            if (first == TPB) {  // none of the probes: behind the last one
                lo = lo + ((hi - lo - 1) / step) * step + 1;
            } else {
                hi = lo + first * step;
                if (first) lo = lo + (first - 1) * step + 1;
            }
        }
        if (threadIdx.x == 0) tail_begin[c] = lo;
    }
}

// Where do flushes cut the reads whose entries span >= max_fragment_length? A flush at locus f (before
// its entries are added, :356-373) erases every live read with start + mfl <= position(f); an entry
// of an erased id opens a new read that starts there (:379-382). One thread per id walks the id's
// entries (a handful) against the chromosome's flush loci. The cuts change the read starts, hence the
// completed counts, hence possibly later flushes: the caller iterates until nothing changes.
__global__ void k_split_update(Raw in, const unsigned long long *skey, const uint32_t *sloc, uint32_t mfl, const uint32_t *flush_loci,
                               const uint32_t *flush_count, uint32_t *split, Scalars *sc) {
    const uint32_t n = in.n_entries;
    for (uint32_t s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        if (s > 0 && skey[s] == skey[s - 1]) continue;  // not the first entry of an id
        uint32_t end = s + 1;
        while (end < n && skey[end] == skey[s]) ++end;
        if (end == s + 1) continue;
        const uint32_t l_first = sloc_locus(sloc[s]);
        const uint32_t p_first = in.locus_pos[l_first], p_last = in.locus_pos[sloc_locus(sloc[end - 1])];
        if (p_last - p_first < mfl) continue;  // never in a flushed prefix before its last entry
        const uint32_t c = last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, l_first);
        const uint32_t *fl = flush_loci + in.chr_locus_off[c];
        const uint32_t n_fl = flush_count[c];
        uint32_t seg_start = p_first, l_prev = l_first;
        for (uint32_t t = s + 1; t < end; ++t) {
            const uint32_t l_t = sloc_locus(sloc[t]);
            uint32_t cut = 0;
            if (l_t != l_prev) {
                // the first flush locus after l_prev whose position has reached seg_start + mfl
                uint32_t lo = 0, hi = n_fl;
                const unsigned long long reach = (unsigned long long)seg_start + mfl;
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (fl[mid] <= l_prev || in.locus_pos[fl[mid]] < reach) lo = mid + 1; else hi = mid;
                }
                if (lo < n_fl && fl[lo] <= l_t) {
                    cut = 1;
                    seg_start = in.locus_pos[l_t];
                }
            }
            if (split[t] != cut) {
                split[t] = cut;
                sc->split_changed = 1;
            }
            l_prev = l_t;
        }
    }
}

// The binning key: cell block | locus (lbits bits) | cell in block (7 bits) -- bit fields, so that
// taking it apart costs shifts instead of 64-bit divisions.
__device__ __forceinline__ unsigned long long bin_key(uint32_t blk, uint32_t l, uint32_t cib, uint32_t lbits) {
    return ((((unsigned long long)blk << lbits) | l) << kCibBits) | cib;
}

// binning key (cell block, locus, cell) of every kept entry, in per-read (CSR) order; validates the
// group -> row mapping
// ... and, per kept entry, what k_records needs of its read in 5 bytes (appearance rank; base | multi-locus
// flag): the reads are adjacent here, in k_records' binned order they are five scattered gathers
__global__ void k_keys2(Raw in, const uint32_t *sval, const unsigned long long *incl,
                        const uint32_t *read_locus, const uint32_t *run_rank, const uint32_t *read_off,
                        uint32_t num_cells, uint32_t B,
                        uint32_t lbits, unsigned long long *key2, uint32_t *val2, uint32_t *t_read,
                        uint32_t *krank, uint8_t *kflags, unsigned long long *entry_kc, const uint32_t *entry_map,
                        uint32_t *blk_cnt_add, uint32_t L, Scalars *sc) {
    // entry_map: the pileup entry of a (compacted) entry of `in` (single-entry fast path), or null: itself
    const uint32_t n = in.n_entries;
    for (uint32_t s = blockIdx.x * TPB + threadIdx.x; s < n; s += gridDim.x * TPB) {
        const unsigned long long cur = incl[s], prev = s ? incl[s - 1] : 0ull;
        const uint32_t e_out = entry_map ? entry_map[sval[s]] : sval[s];
        if (incl_kept(cur) == incl_kept(prev)) {
            if (entry_kc) entry_kc[e_out] = kNoEntry;
            continue;
        }
        const uint32_t k = incl_kept(prev);
        const uint32_t group = in.id_base(sval[s]) >> 2;
        uint32_t cell = 0;
        if (group >= in.n_groups) {
            sc->error = 1;
        } else {
            cell = in.g2p[group];
            if (cell >= num_cells) {
                sc->error = 2;
                cell = 0;
            }
        }
        const uint32_t blk = cell / B, cib = cell - blk * B;
        if (key2) {  // the radix path sorts these; the counting path bins through entry_kc
            key2[k] = bin_key(blk, read_locus[k], cib, lbits);
            val2[k] = k;
        }
        const uint32_t r = incl_reads(cur) - 1;
        t_read[k] = r;
        krank[k] = run_rank[r];
        kflags[k] = (uint8_t)((in.id_base(sval[s]) & 3u) | (read_off[r + 1] - read_off[r] > 1u ? 4u : 0u));
        // counting path: back in pileup order, where the entries of a locus are adjacent; one 8-byte
        // scatter per entry carries k and (block, cell in block)
        if (entry_kc) entry_kc[e_out] = ((unsigned long long)((blk << kCibBits) | cib) << 32) | k;
        // (single-entry fast path: k_bin_hist has counted the S entries, possibly long ago; the few kept M
        // entries join with one scattered atomic each)
        if (blk_cnt_add) atomicAdd(&blk_cnt_add[(size_t)blk * (L + 1) + read_locus[k]], 1u);
    }
}

// counting path, kept entries by (cell block, locus). The entries of a locus are adjacent in the
// pileup, so a wave counts a locus' entries per cell block in LDS -- global atomics would all hit the
// handful of addresses of the loci in flight.
// Single-entry fast path (m_mask != null: the M entries' flags, 64 entries a word): ONLY the S entries are counted, and their slots are made here -- (block,
// cell) from the group map, validated as k_keys2 does for the M entries -- with nothing of the read assembly:
// k_keys2 adds the kept M entries afterwards, and k_bin_place knows an S entry's tail flag from its index.
// (Measured and dropped, twice: this pass on a stream of its own beside the M entries' read assembly, which it does
// not depend on. Round 15, launched right behind read-back 1b for an assumed block size, C3 under the profiler: the
// pass took 196 us instead of 158, k_m_fields started 47 us later (the host's fork and launch), the assembly's
// fourteen kernels took 77 us longer and k_read_info ended 109 us later -- and with it the flush chain on the side
// stream, at 643 us instead of 524, which k_bin_place waits for: k_keys2 started 40 us earlier, k_bin_place and
// everything behind it not at all. The chain (118 us, serial, behind k_read_info) hides behind this pass in the
// serial order and is the critical path beside it. Round 3 had found the same with a 104 us id-space scan as the
// neighbour.)
// A workgroup takes TL consecutive loci at a time (TL a power of two, <= 64, nb * (TL + 1) words of LDS) and counts
// their entries -- one contiguous stretch of the pileup -- into hist[block][locus in tile], a thread per entry,
// four entries of a thread in flight; the locus of an entry comes from the tile's offsets in LDS (a search over 65
// words: a third of the pass' vector instructions, but reading k_entry_locus' table instead was SLOWER, 193 against
// 167 us -- the pass is bound by the memory streams it keeps open, see below). The tile leaves as rows of TL consecutive loci per block -- coalesced, where a column per locus touched nb
// different cache lines for 4 bytes each (6.3 M scattered stores on C3). Rows are TL + 1 words apart: the entries of
// one locus go to many blocks and a stride of TL would put them all on one bank.
// (Until round 3 a WAVE walked a locus at a time, sixteen loci one after the other with three dependent round trips
// each: 180 us on C3. What the pass costs is the sum of its memory streams, measured by switching them off one at a
// time in a twin launch into dead buffers: the 8-byte slot store 52 us, the group -> cell gather 37, the 2-byte
// id_base read 21, a 4-byte entry -> locus read 11, the LDS atomics and the count rows nothing, the empty loop 50.)
__device__ __forceinline__ uint32_t tile_locus(const uint32_t *s_off, uint32_t lo, uint32_t hi, uint32_t e) {
    // last j in [lo, hi) with s_off[j] <= e (s_off[lo] <= e; empty loci share an offset with their successor)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TPB) void k_bin_hist(Raw in, uint32_t nb, uint32_t TL, unsigned long long *__restrict__ entry_kc,
                                                 const unsigned long long *__restrict__ m_mask, uint32_t num_cells,
                                                 uint32_t B_log2, uint32_t *__restrict__ blk_cnt, Scalars *sc,
                                                 uint32_t g2p_lds) {
    extern __shared__ uint32_t lds_hist[];  // nb * (TL + 1); then (g2p_lds) the group -> cell map as 16-bit words
    __shared__ uint32_t s_off[65];          // first entry of each of the tile's loci, and the end
    static_assert(TPB >= 65, "one thread per offset");
    const uint32_t L = in.n_loci, TLP = TL + 1u, TL_log2 = 31u - (uint32_t)__clz((int)TL);
    const uint32_t n_tiles = (L + TL - 1u) / TL;
    constexpr int U = 4;
    // the group -> cell map from LDS (a workgroup then takes several tiles): the gather from global memory was 37
    // of this pass' 170 us on C3
    uint16_t *s_g2p = reinterpret_cast<uint16_t *>(lds_hist + nb * TLP);
    if (g2p_lds) {
        for (uint32_t i = threadIdx.x; i < in.n_groups; i += TPB) s_g2p[i] = (uint16_t)min(in.g2p[i], 0xFFFFu);
    }
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t l0 = tile * TL, n_l = min(TL, L - l0);
        for (uint32_t i = threadIdx.x; i < nb * TLP; i += TPB) lds_hist[i] = 0;
        if (threadIdx.x <= n_l) s_off[threadIdx.x] = (uint32_t)in.locus_entry_off[l0 + threadIdx.x];
        __syncthreads();
        const uint32_t eb = s_off[0], ee = s_off[n_l];
        for (uint32_t base = eb + threadIdx.x; base < ee; base += TPB * U) {
            uint32_t slot[U];  // block of the entry, or none
            constexpr uint32_t kNone = 0xFFFFFFFFu;
            if (m_mask) {
                unsigned long long mw[U];  // the flags of the entry's 64-entry chunk (a wave's entries touch two)
                uint32_t ib[U], cell[U];
                bool is_m[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t e = base + (uint32_t)u * TPB;
                    const bool in_tile = e < ee;
                    mw[u] = in_tile ? m_mask[e >> 6] : ~0ull;  // (outside the tile: as an M entry, skipped)
                    ib[u] = in_tile ? in.id_base(e) : 0u;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t group = ib[u] >> 2;
                    cell[u] = 0;
                    is_m[u] = (mw[u] >> ((base + (uint32_t)u * TPB) & 63u)) & 1ull;
                    if (!is_m[u]) {
                        if (group >= in.n_groups) sc->error = 1;
                        else cell[u] = g2p_lds ? (uint32_t)s_g2p[group] : in.g2p[group];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    slot[u] = kNone;
                    if (is_m[u]) continue;  // an M entry: k_keys2
                    const uint32_t e = base + (uint32_t)u * TPB;
                    uint32_t c = cell[u];
                    if (c >= num_cells) {
                        sc->error = 2;
                        c = 0;
                    }
                    const uint32_t blk = c >> B_log2, cib = c - (blk << B_log2);
                    entry_kc[e] = ((unsigned long long)(((ib[u] & 3u) << kSingleBaseShift) | (blk << kCibBits) | cib) << 32)
                            | kSingle;
                    slot[u] = blk;
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t e = base + (uint32_t)u * TPB;
                    const unsigned long long kc = e < ee ? entry_kc[e] : (unsigned long long)kNoEntry;
                    slot[u] = (uint32_t)kc != kNoEntry ? (uint32_t)(kc >> 32) >> kCibBits : kNone;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (slot[u] == kNone) continue;
                const uint32_t j = tile_locus(s_off, 0u, n_l, base + (uint32_t)u * TPB);
                atomicAdd(&lds_hist[slot[u] * TLP + j], 1u);
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb * TL; i += TPB) {
            const uint32_t b = i >> TL_log2, j = i & (TL - 1u);
            if (j < n_l) {
                blk_cnt[(size_t)b * (L + 1) + l0 + j] = lds_hist[b * TLP + j];
                if (l0 + j == L - 1) blk_cnt[(size_t)b * (L + 1) + L] = 0;  // the closing slot of the block's row
            }
        }
        __syncthreads();
    }
}

// ... and places them: position = group offset + LDS cursor (arbitrary order inside the group); the same
// tiles of loci, the offsets loaded as rows. grouped[pos] = (cell in block | locus << 7) << 32 | k
// It also finds the loci at which some cell has more than one kept entry (a bitmap over the cells per wave,
// bm_words words each; 0: no room, every locus is flagged): only there does k_entry_records have to count the
// entries of the same cell for the pair bound -- on sparse loci that scan of every group was 40 % of its time.
// The bitmap wants a locus at a time, so a wave takes a run of consecutive loci of the tile -- one contiguous stretch
// of entries -- in chunks of 64 with the chunks of the next round already asked for (D in flight), and inside a chunk
// goes through the loci it holds in order; a locus is closed (flag written, bitmap cleared) when the chunk that
// holds its last entry is done.
__global__ __launch_bounds__(TPB) void k_bin_place(Raw in, uint32_t nb, uint32_t TL,
                                                  const unsigned long long *__restrict__ entry_kc,
                                                  const uint32_t *__restrict__ blk_off, uint32_t B_log2, uint32_t bm_words,
                                                  const uint32_t *tail_begin,
                                                  unsigned long long *__restrict__ grouped, uint8_t *dupflag) {
    extern __shared__ uint32_t lds_hist[];  // cursors, nb * (TL + 1); then the waves' cell bitmaps
    __shared__ uint32_t s_off[65];          // first entry of each of the tile's loci, and the end
    __shared__ uint32_t s_tail[64];         // per locus of the tile: the first tail entry of its chromosome (S entries)
    constexpr uint32_t NW = TPB / 64;
    constexpr int D = 4;  // chunks of a wave in flight
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, L = in.n_loci, TLP = TL + 1u;
    const uint32_t TL_log2 = 31u - (uint32_t)__clz((int)TL);
    uint32_t *bm = lds_hist + nb * TLP + wv * bm_words;
    for (uint32_t i = lane; i < bm_words; i += 64u) bm[i] = 0;
    const uint32_t n_tiles = (L + TL - 1u) / TL;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t l0 = tile * TL, n_l = min(TL, L - l0);
        for (uint32_t i = threadIdx.x; i < nb * TL; i += TPB) {
            const uint32_t b = i >> TL_log2, j = i & (TL - 1u);
            if (j < n_l) lds_hist[b * TLP + j] = blk_off[(size_t)b * (L + 1) + l0 + j];
        }
        if (threadIdx.x <= n_l) s_off[threadIdx.x] = (uint32_t)in.locus_entry_off[l0 + threadIdx.x];
        if (threadIdx.x < n_l)
            s_tail[threadIdx.x] = tail_begin
                    ? tail_begin[last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, l0 + threadIdx.x)] : 0u;
        __syncthreads();
        const uint32_t per_wave = (n_l + NW - 1u) / NW;
        const uint32_t ja = min(n_l, wv * per_wave), jb = min(n_l, ja + per_wave);
        const uint32_t E0 = s_off[ja], E1 = s_off[jb];
        uint32_t cur = ja;                // the locus being filled (wave-uniform)
        bool twice = bm_words == 0u;      // ... has some cell twice (per lane until the locus is closed)
        auto close_locus = [&]() {  // every entry of locus `cur` has been placed
            const bool any_twice = __ballot(twice) != 0ull;
            if (lane == 0u) dupflag[l0 + cur] = any_twice ? 1 : 0;
            if (bm_words) {  // the next locus starts from an empty bitmap
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (uint32_t i = lane; i < bm_words; i += 64u) bm[i] = 0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            twice = bm_words == 0u;
            ++cur;
        };
        auto chunk = [&](unsigned long long kc, uint32_t base) {  // the 64 entries from `base`, loaded
            const uint32_t e = base + lane;
            const bool valid = e < E1;
            const uint32_t j = valid ? tile_locus(s_off, cur, jb, e) : 0xFFFFFFFFu;
            const uint32_t chunk_end = min(E1, base + 64u);
            while (true) {  // (wave-uniform)
                if (valid && j == cur) {
                    uint32_t k = (uint32_t)kc;
                    if (k != kNoEntry) {
                        uint32_t cc = (uint32_t)(kc >> 32);
                        if (k & kSingle) {  // entry index -> tail flag (k_flush_chain); base beside it
                            k = kSingle | (e >= s_tail[cur] ? kSingleTail : 0u) | (cc >> kSingleBaseShift);
                            cc &= (1u << kSingleBaseShift) - 1u;
                        }
                        if (bm_words) {
                            const uint32_t cell = ((cc >> kCibBits) << B_log2) + (cc & ((1u << kCibBits) - 1u));
                            const uint32_t bit = 1u << (cell & 31u);
                            twice |= (atomicOr(&bm[cell >> 5], bit) & bit) != 0u;
                        }
                        const uint32_t pos = atomicAdd(&lds_hist[(cc >> kCibBits) * TLP + cur], 1u);
                        // cell in block | locus << 7 above k (k_entry_records; the radix path never comes here)
                        grouped[pos] = ((unsigned long long)((cc & ((1u << kCibBits) - 1u)) | ((l0 + cur) << kCibBits)) << 32) | k;
                    }
                }
                if (s_off[cur + 1] > chunk_end) break;  // the locus goes on in the next chunk
                close_locus();
                if (cur >= jb) break;
            }
        };
        unsigned long long ring[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const uint32_t e = E0 + (uint32_t)d * 64u + lane;
            ring[d] = e < E1 ? entry_kc[e] : (unsigned long long)kNoEntry;
        }
        for (uint32_t base = E0; base < E1; base += 64u * D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const uint32_t b = base + (uint32_t)d * 64u;
                if (b >= E1) break;  // (wave-uniform)
                const unsigned long long kc = ring[d];
                const uint32_t nxt = b + 64u * D + lane;
                ring[d] = nxt < E1 ? entry_kc[nxt] : (unsigned long long)kNoEntry;
                chunk(kc, b);
            }
        }
        while (cur < jb) close_locus();  // (a run without entries)
        __syncthreads();
    }
}

// After the binning sort: entries per (block, locus) group -> blk_cnt (no atomics: the head of a
// group counts its run), and sum over loci of (entries of one cell at the locus)^2 per cell (the
// Cauchy-Schwarz pair bound), accumulated in LDS per workgroup: a workgroup's slice of the sorted
// order spans only a few cell blocks.
__global__ __launch_bounds__(TPB) void k_group_counts(const unsigned long long *skey2, uint32_t n, uint32_t B,
                                                     uint32_t L, uint32_t lbits, uint32_t *blk_cnt,
                                                     unsigned long long *per_cell_sq) {
    constexpr uint32_t SLOTS = 512;
    __shared__ unsigned long long sq[SLOTS];
    __shared__ uint32_t first_cell;
    const uint32_t per_block = (n + gridDim.x - 1) / gridDim.x;
    const uint32_t d0 = blockIdx.x * per_block, d1 = min(n, d0 + per_block);
    for (uint32_t i = threadIdx.x; i < SLOTS; i += TPB) sq[i] = 0;
    if (threadIdx.x == 0 && d0 < n) {
        const unsigned long long key = skey2[d0];
        first_cell = (uint32_t)(key >> (kCibBits + lbits)) * B;  // first cell of the slice's first block
    }
    __syncthreads();
    for (uint32_t d = d0 + threadIdx.x; d < d1; d += TPB) {
        const unsigned long long key = skey2[d];
        const unsigned long long grp = key >> kCibBits;  // (block, locus)
        const uint32_t blk = (uint32_t)(grp >> lbits), l = (uint32_t)grp & ((1u << lbits) - 1u);
        if (d == 0 || skey2[d - 1] >> kCibBits != grp) {
            uint32_t len = 1;
            for (uint32_t t = d + 1; t < n && skey2[t] >> kCibBits == grp; ++t) ++len;
            blk_cnt[(size_t)blk * (L + 1) + l] = len;
        }
        if (d == 0 || skey2[d - 1] != key) {
            unsigned long long cnt = 1;
            for (uint32_t t = d + 1; t < n && skey2[t] == key; ++t) ++cnt;
            const uint32_t cell = blk * B + ((uint32_t)key & ((1u << kCibBits) - 1u));
            const uint32_t rel = cell - first_cell;
            if (rel < SLOTS) atomicAdd(&sq[rel], cnt * cnt);
            else atomicAdd(&per_cell_sq[cell], cnt * cnt);
        }
    }
    __syncthreads();
    if (d0 < n) {
        for (uint32_t i = threadIdx.x; i < SLOTS; i += TPB) {
            if (sq[i]) atomicAdd(&per_cell_sq[first_cell + i], sq[i]);
        }
    }
}

// Locus ranges (one partition shared by all cell blocks). The loci are cut into segments of
// cap_loci loci, one workgroup per segment; inside its segment a workgroup cuts greedily: the
// longest range from `s` in which no block has more than cap_entries entries (feasibility is
// monotone in the range end; the search gallops from the previous range's length); a locus that
// exceeds the cap alone becomes a single-locus range. k_ranges_compact concatenates the segments.
//
// The staging limits depend on the tile variant, and the tile variant on the pair bound, which is
// still on the device: the kernels pick the limits themselves (CapChoice), the host learns the
// outcome with the final read-back.
struct CapChoice {
    uint32_t entries_plain, loci_plain;    // int64 tile (or the masks variant)
    uint32_t entries_counts, loci_counts;  // count tile
    unsigned long long count_limit;        // count tile iff allow_counts and pair bound < count_limit
    uint32_t allow_counts;
    __device__ __forceinline__ bool counts(const Scalars *sc) const {
        return allow_counts && sc->pair_bound < count_limit;
    }
};

// The pair bound that decides between the two sets of limits comes out of the grouping that is still
// running when the offsets are ready, so the ranges are cut for BOTH sets (blockIdx.y: 0 plain, 1 count
// tile) on the side stream meanwhile, and k_ranges_compact picks one.
__global__ __launch_bounds__(TPB) void k_ranges_segment(const uint32_t *blk_off, uint32_t nb, uint32_t L,
                                                       CapChoice caps, uint32_t *seg_ends_both,
                                                       uint32_t *seg_count_both, size_t variant_stride) {
    const bool use_counts = blockIdx.y == 1u;
    const uint32_t cap_entries = use_counts ? caps.entries_counts : caps.entries_plain;
    const uint32_t cap_loci = use_counts ? caps.loci_counts : caps.loci_plain;
    uint32_t *seg_ends = seg_ends_both + blockIdx.y * variant_stride;
    uint32_t *seg_count = seg_count_both + blockIdx.y * variant_stride;
    const size_t stride = (size_t)L + 1;
    const uint32_t seg = blockIdx.x;
    if ((unsigned long long)seg * cap_loci >= L) {  // the grid is sized for the smaller of the two limits
        if (threadIdx.x == 0) seg_count[seg] = 0;
        return;
    }
    const uint32_t seg_begin = seg * cap_loci, seg_end = min(L, seg_begin + cap_loci);
    uint32_t *ends = seg_ends + (size_t)seg * cap_loci;  // at most cap_loci ranges per segment
    uint32_t s = seg_begin, nr = 0, guess = 0;
    auto feasible = [&](uint32_t e) {
        int ok = 1;
        for (uint32_t b = threadIdx.x; b < nb; b += TPB)
            if (blk_off[b * stride + e] - blk_off[b * stride + s] > cap_entries) ok = 0;
        return __syncthreads_and(ok) != 0;
    };
    while (s < seg_end) {
        uint32_t e = s + 1;
        if (feasible(e)) {
            const uint32_t top = seg_end;
            uint32_t lo = e, hi = top;  // lo feasible, answer in [lo, hi]
            if (feasible(top)) {
                lo = top;
            } else if (guess > 1 && s + guess < top) {  // bracket around the previous length
                hi = top - 1;
                const uint32_t g = s + guess;
                if (feasible(g)) {
                    lo = g;
                    uint32_t step = max(guess / 8, 1u);
                    while (lo < hi) {  // gallop up
                        const uint32_t nx = min(hi, lo + step);
                        if (feasible(nx)) lo = nx; else { hi = nx - 1; break; }
                        step *= 2;
                    }
                } else {
                    hi = g - 1;
                    uint32_t step = max(guess / 8, 1u);
                    while (hi > lo) {  // gallop down
                        const uint32_t nx = (hi - lo > step) ? hi - step : lo;
                        if (feasible(nx)) { lo = nx; break; }
                        hi = nx - 1;
                        step *= 2;
                    }
                }
            } else {
                hi = top - 1;
            }
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                if (feasible(mid)) lo = mid; else hi = mid - 1;
            }
            e = lo;
        }
        guess = e - s;
        if (threadIdx.x == 0) ends[nr] = e;
        ++nr;
        s = e;
    }
    if (threadIdx.x == 0) seg_count[seg] = nr;
}

__global__ __launch_bounds__(TPB) void k_ranges_compact(const uint32_t *seg_ends_both, const uint32_t *seg_count_both,
                                                       size_t variant_stride, uint32_t n_seg, CapChoice caps,
                                                       uint32_t *range_off, const unsigned long long *per_cell_sq,
                                                       uint32_t n_cells_padded, int force_variant, Scalars *sc) {
    // force_variant < 0: the pair bound first (the largest per-cell sum of squares), then the limits it allows;
    // 0 / 1: the limits of the int64 tile / of the count tile, whatever the bound (the counting path cuts for
    // the count tile before the bound is known, k_records_tail checks afterwards)
    __shared__ unsigned long long s_best[TPB / 64];
    if (force_variant < 0) {
        unsigned long long best = 0;
        for (uint32_t i = threadIdx.x; i < n_cells_padded; i += TPB) best = max(best, per_cell_sq[i]);
        for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned long long)__shfl_down(best, off));
        if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < TPB / 64; ++w) best = max(best, s_best[w]);
            sc->pair_bound = max(sc->pair_bound, best);
        }
        __syncthreads();
    }
    const bool use_counts = force_variant < 0 ? caps.counts(sc) : force_variant == 1;
    const uint32_t cap_loci = use_counts ? caps.loci_counts : caps.loci_plain;
    const uint32_t *seg_ends = seg_ends_both + (use_counts ? variant_stride : 0);
    const uint32_t *seg_count = seg_count_both + (use_counts ? variant_stride : 0);
    // A sweep takes TPB segments: a thread per segment loads its count, one prefix over the workgroup gives every
    // segment its base, and all threads copy the sweep's ranges, a thread per range -- its segment by a search over
    // the bases in LDS. (Until round 32 a loop over the segments, two barriers each: 27 us for C3's segments.)
    __shared__ uint32_t s_first[TPB];  // ranges of the sweep before each of its segments
    __shared__ uint32_t s_part[TPB / 64];
    __shared__ uint32_t s_span;
    if (threadIdx.x == 0) {
        s_span = 0;
        range_off[0] = 0;
    }
    // (no barrier here: the sweep below has some in front of the atomicMax, and L >= 1 gives at least one sweep)
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t span = 0;  // the longest range this thread copies (a segment's first range begins with the segment)
    uint32_t done = 0;  // ranges of the sweeps before (uniform)
    for (uint32_t seg0 = 0; seg0 < n_seg; seg0 += TPB) {
        const uint32_t n_here = min((uint32_t)TPB, n_seg - seg0);
        const uint32_t cnt = threadIdx.x < n_here ? seg_count[seg0 + threadIdx.x] : 0u;
        uint32_t incl = cnt;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= (uint32_t)off) incl += up;
        }
        __syncthreads();  // the previous sweep's tables have been read
        if (lane == 63u) s_part[wv] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w2 = 0; w2 < TPB / 64; ++w2) {
            if ((uint32_t)w2 < wv) before += s_part[w2];
            total += s_part[w2];
        }
        s_first[threadIdx.x] = before + incl - cnt;
        __syncthreads();
        for (uint32_t r = threadIdx.x; r < total; r += TPB) {
            // the last segment that begins at or before r holds it (segments without ranges share a begin with their
            // successor; those behind the last range begin at `total`)
            const uint32_t sg = last_le<uint32_t>(s_first, n_here, r), i = r - s_first[sg];
            const uint32_t seg = seg0 + sg;
            const uint32_t *ends = seg_ends + (size_t)seg * cap_loci;
            // (the range's begin is the neighbouring lane's end where that lane holds the range before in the segment)
            const uint32_t e = ends[i];
            uint32_t begin = __shfl_up(e, 1);
            if (lane == 0u || i == 0u) begin = i ? ends[i - 1] : seg * cap_loci;
            range_off[1 + done + r] = e;
            span = max(span, e - begin);
        }
        done += total;
    }
    atomicMax(&s_span, span);
    __syncthreads();
    if (threadIdx.x == 0) {
        sc->num_ranges = done;
        sc->max_range_span = s_span;
    }
}

// per locus: its chromosome and its index inside its locus range (k_records looks both up per entry)
// (locus_rel: the range-relative locus in the low half; bit 31: some cell has two kept entries at the locus --
// k_bin_place's flag, so that k_entry_records reads ONE table per entry)
constexpr uint32_t kLocusDup = 0x80000000u;
__global__ void k_locus_info(Raw in, const uint32_t *range_off, const Scalars *sc, const uint8_t *dupflag,
                             uint32_t *locus_chr, uint32_t *locus_rel) {
    const uint32_t n_ranges = sc->num_ranges;
    for (uint32_t l = blockIdx.x * TPB + threadIdx.x; l < in.n_loci; l += gridDim.x * TPB) {
        locus_chr[l] = last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, l);
        locus_rel[l] = (l - range_off[last_le<uint32_t>(range_off, n_ranges + 1, l)])
                | ((dupflag && dupflag[l]) ? kLocusDup : 0u);
    }
}

// entry records at their final (binned) position d: window masks from the per-read lists
__global__ void k_records(Raw in, const unsigned long long *skey2, const uint32_t *sval2, uint32_t n,
                          const uint32_t *t_read, const uint32_t *read_off, const uint32_t *read_locus,
                          const uint8_t *read_base, const uint32_t *krank, const uint8_t *kflags, const uint32_t *rbeg,
                          const uint32_t *flushed, const uint32_t *locus_chr, const uint32_t *locus_rel, uint32_t B,
                          uint32_t lbits, uint4 *entry, uint32_t *entry32, uint32_t *mask32,
                          uint32_t *entry_read, Scalars *sc) {
    uint32_t n_wide = 0;
    for (uint32_t d = blockIdx.x * TPB + threadIdx.x; d < n; d += gridDim.x * TPB) {
        const unsigned long long key = skey2[d];
        const uint32_t k = sval2[d];
        const uint32_t cib = (uint32_t)key & ((1u << kCibBits) - 1u);
        const unsigned long long grp = key >> kCibBits;
        const uint32_t blk = (uint32_t)(grp >> lbits), l = (uint32_t)grp & ((1u << lbits) - 1u);
        const uint32_t cell = blk * B + cib;
        const uint32_t fl = kflags[k];
        const uint32_t base = fl & 3u;
        const bool multi = (fl & 4u) != 0u;
        const uint32_t chr = locus_chr[l];
        const bool tail = krank[k] - rbeg[chr] >= flushed[chr];
        // the read's list of kept entries: only a multi-locus read has neighbours to look for
        uint32_t r = 0, lo = k, hi = k + 1;
        if (multi) {
            r = t_read[k];
            lo = read_off[r];
            hi = read_off[r + 1];
        }
        uint32_t meta = cell | (base << kMetaBaseShift) | (tail ? kMetaTail : 0u);
        uint32_t masks = 0, bases = 0;
        bool wide = false;
        for (uint32_t j = k; j-- > lo;) {
            const uint32_t dist = l - read_locus[j];
            if (dist > kNarrowWindow) wide = true;
            if (dist > kWindow) {
                meta |= kMetaPrevOvf;
                break;
            }
            masks |= 1u << (dist - 1);
        }
        for (uint32_t j = k + 1; j < hi; ++j) {
            const uint32_t dist = read_locus[j] - l;
            if (dist > kNarrowWindow) wide = true;
            if (dist > kWindow) {
                meta |= kMetaNextOvf;
                break;
            }
            masks |= 1u << (16 + dist - 1);
            bases |= (uint32_t)(read_base[j] & 1u) << (dist - 1);
            bases |= (uint32_t)((read_base[j] >> 1) & 1u) << (16 + dist - 1);
        }
        // the 16-byte record and the read index serve the flagged entries only: pairs of two multi-locus
        // reads, and (correct_tiles) pairs of two reads that were never flushed
        if (multi || tail) {
            entry[d] = make_uint4(meta, masks, bases, l);
            entry_read[d] = r;  // (read only for pairs of two multi-locus reads)
        }
        entry32[d] = cib | (base << kC_BaseShift) | (tail ? kC_Tail : 0u) | (multi ? kC_Multi : 0u)
                | (wide ? kC_Wide : 0u) | ((locus_rel[l] & 0xFFFFu) << 16);
        if (mask32)  // staged by the clustered-loci tile variant only
            mask32[d] = (masks & 0xFFu) | (((masks >> 16) & 0xFFu) << 8) | ((bases & 0xFFu) << 16)
                    | (((bases >> 16) & 0xFFu) << 24);
        n_wide += wide ? 1u : 0u;
    }
    if (n_wide) atomicAdd(&sc->n_wide, n_wide);
}

// ---- counting path: k_bin_rank + k_records in one pass ------------------------------------------------
// Nothing depends on the order of the entries inside a (cell block, locus) group (the pair kernels enumerate
// every pair of a locus once, in whatever order the entries stand; diagonal tiles pair an entry with the
// entries after it), so the entries stay where k_bin_place put them: no ranking, no sorted copy of keys and
// values. k_bin_place packs the locus next to (cell in block, k) in its 8 bytes, the block follows from the
// position (a search over the nb block boundaries, held in LDS), and a thread per entry scans its group for
// the entries of the same cell: an entry of a cell with n entries at the locus adds n to the cell's sum, n of
// them n^2 -- the Cauchy-Schwarz pair bound. (A thread per GROUP instead read the tables once per group but
// walked its entries one after the other, a chain of gathers per thread: 7.4 ms on C3 against 2.7.)
// What the record of a kept M entry k needs of its read, made where the read's entries are adjacent (the per-read
// lists, k ascending) instead of in binned order, where it is a chain of five dependent gathers per entry -- a
// twentieth of the entries on sparse loci, but every wave of the record pass holds a few and waited for them
// (90 us of its 280 on C3). m_rec[k] = {base, tail, overflow flags as in an entry's meta word | kRecMulti | kRecWide,
// window masks, window bases, read index}; k_entry_records adds the cell and the locus.
constexpr uint32_t kRecMulti = 1u << 30, kRecWide = 1u << 31;
__global__ void k_m_records(Raw in, uint32_t n_kept_m, const uint32_t *t_read, const uint32_t *read_off,
                            const uint32_t *read_locus, const uint8_t *read_base, const uint32_t *krank,
                            const uint8_t *kflags, const uint32_t *rbeg, const uint32_t *flushed, uint4 *m_rec,
                            Scalars *sc) {
    // the chromosomes' first loci from LDS (up to 1024 of them): searched in global memory the chromosome of an entry
    // was a chain of dependent loads in front of everything else the thread does (C3 clustered: 68 M entries)
    __shared__ uint32_t s_chr[1025];
    const bool chr_lds = in.n_chr <= 1024u;
    if (chr_lds)
        for (uint32_t i = threadIdx.x; i <= in.n_chr; i += TPB) s_chr[i] = in.chr_locus_off[i];
    __syncthreads();
    uint32_t n_wide = 0;  // (rare: an atomic per thread that met one; the count rides on the packing's last read-back)
    for (uint32_t k = blockIdx.x * TPB + threadIdx.x; k < n_kept_m; k += gridDim.x * TPB) {
        const uint32_t fl = kflags[k], l = read_locus[k];
        const bool multi = (fl & 4u) != 0u;
        const uint32_t chr = chr_lds ? last_le<uint32_t>(s_chr, in.n_chr + 1, l)
                                     : last_le<uint32_t>(in.chr_locus_off, in.n_chr + 1, l);
        const bool tail = krank[k] - rbeg[chr] >= flushed[chr];
        // the read's list of kept entries: only a multi-locus read has neighbours to look for
        uint32_t r = 0, lo = k, hi = k + 1;
        if (multi) {
            r = t_read[k];
            lo = read_off[r];
            hi = read_off[r + 1];
        }
        uint32_t meta = ((fl & 3u) << kMetaBaseShift) | (tail ? kMetaTail : 0u) | (multi ? kRecMulti : 0u);
        uint32_t masks = 0, bases = 0;
        for (uint32_t j = k; j-- > lo;) {
            const uint32_t dist = l - read_locus[j];
            if (dist > kNarrowWindow) meta |= kRecWide;
            if (dist > kWindow) {
                meta |= kMetaPrevOvf;
                break;
            }
            masks |= 1u << (dist - 1);
        }
        for (uint32_t j = k + 1; j < hi; ++j) {
            const uint32_t dist = read_locus[j] - l;
            if (dist > kNarrowWindow) meta |= kRecWide;
            if (dist > kWindow) {
                meta |= kMetaNextOvf;
                break;
            }
            masks |= 1u << (16 + dist - 1);
            bases |= (uint32_t)(read_base[j] & 1u) << (dist - 1);
            bases |= (uint32_t)((read_base[j] >> 1) & 1u) << (16 + dist - 1);
        }
        m_rec[k] = make_uint4(meta, masks, bases, r);
        n_wide += (meta & kRecWide) ? 1u : 0u;
    }
    if (n_wide) atomicAdd(&sc->n_wide, n_wide);
}

struct RecordTables {  // by value: what a record needs beside the group's own entries
    const uint4 *m_rec;  // per kept M entry (k_m_records)
    const uint32_t *locus_rel;
    uint4 *entry;
    uint32_t *entry32, *mask32, *entry_read;
};

// rec: the M entry's m_rec word group, loaded by the caller (all zero for an S entry). Returns whether the entry is
// flagged (kC_Tail | kC_Multi): what the flagged entries' lists are made of
__device__ __forceinline__ bool emit_record(const RecordTables &t, uint32_t d, uint32_t k, uint4 rec, uint32_t cib,
                                            uint32_t cell, uint32_t l, uint32_t lrel) {
    uint32_t base, meta, masks = 0, bases = 0, r = 0;
    bool multi = false, wide = false, tail;
    if (k & kSingle) {  // single-entry fast path: all there is to know came along (k_bin_place)
        base = k & 3u;
        tail = (k & kSingleTail) != 0u;
        meta = cell | (base << kMetaBaseShift) | (tail ? kMetaTail : 0u);
    } else {
        base = (rec.x >> kMetaBaseShift) & 3u;
        tail = (rec.x & kMetaTail) != 0u;
        multi = (rec.x & kRecMulti) != 0u;
        wide = (rec.x & kRecWide) != 0u;
        meta = cell | (rec.x & ~(kRecMulti | kRecWide));
        masks = rec.y;
        bases = rec.z;
        r = rec.w;
    }
    // the 16-byte record and the read index serve the flagged entries only (see k_records)
    if (multi || tail) {
        t.entry[d] = make_uint4(meta, masks, bases, l);
        t.entry_read[d] = r;
    }
    t.entry32[d] = cib | (base << kC_BaseShift) | (tail ? kC_Tail : 0u) | (multi ? kC_Multi : 0u)
            | (wide ? kC_Wide : 0u) | (lrel << 16);
    if (t.mask32)
        t.mask32[d] = (masks & 0xFFu) | (((masks >> 16) & 0xFFu) << 8) | ((bases & 0xFFu) << 16)
                | (((bases >> 16) & 0xFFu) << 24);
    return multi || tail;
}

constexpr int TPB_REC = 512;
__global__ __launch_bounds__(TPB_REC) void k_entry_records(const unsigned long long *grouped, const uint32_t *blk_off,
                                                          uint32_t n, uint32_t nb, uint32_t L, uint32_t B,
                                                          uint32_t lbits, RecordTables t,
                                                          unsigned long long *per_cell_sq, Scalars *sc,
                                                          unsigned long long *chunk_mask, uint32_t *block_sum) {
    constexpr uint32_t SLOTS = 512;
    __shared__ unsigned long long sq[SLOTS];
    __shared__ uint32_t blk_start[1025];  // first entry of every cell block (nb <= 1024), and the end
    __shared__ uint32_t first_cell;
    __shared__ uint32_t n_flagged;  // of this workgroup's entries
    // A workgroup takes one block of kFlagBlock entries (the grid is their number), so that a wave's 64 entries of a
    // round are one 64-entry chunk of the flagged entries' lists: where chunk_mask is given, the chunks' flags (one
    // ballot each, zero behind the last entry) and the block's count leave from here, and the lists need no further
    // pass over entry32 (k_flag_scan, k_pflag_compact_masks, k_pflag_groups).
    constexpr int U = 4;
    static_assert(kFlagBlock % (TPB_REC * U) == 0, "whole rounds per block of the lists");
    const uint32_t d0 = blockIdx.x * kFlagBlock, d1 = min(n, d0 + kFlagBlock);  // (the last block starts below n < 2^31)
    if (threadIdx.x == 0) n_flagged = 0;
    for (uint32_t i = threadIdx.x; i < SLOTS; i += TPB_REC) sq[i] = 0;
    for (uint32_t i = threadIdx.x; i <= nb; i += TPB_REC) blk_start[i] = i < nb ? blk_off[(size_t)i * (L + 1)] : n;
    __syncthreads();
    auto block_of = [&](uint32_t p) {  // last block whose first entry is <= p (empty blocks share a start)
        uint32_t lo = 0, hi = nb;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (blk_start[mid] <= p) lo = mid; else hi = mid;
        }
        return lo;
    };
    if (threadIdx.x == 0 && d0 < n) first_cell = block_of(d0) * B;
    __syncthreads();
    const uint32_t lmask = (1u << lbits) - 1u;
    // A thread has U entries in flight, and an entry's chain of dependent reads is as short as it can be: its slot,
    // then ONE per-locus word (range-relative locus | duplicate flag) and, for an M entry (one in twenty on sparse
    // loci), the 16 bytes k_m_records made of its read; only at a locus with a duplicate cell are the group's bounds
    // read and its members counted. (Round 2 read group bounds, three per-locus tables and two per-chromosome words
    // for every entry and walked the read's lists here: 280 us on C3; switching the pieces off one at a time in a
    // twin launch showed 92 us for the per-locus level of the chain, 90 for the M entries' five levels, 126 for
    // the stores, 20 for the block search. Staging the slice's per-locus words in LDS -- the slots are in (block,
    // locus) order, a slice covers 2000 consecutive loci -- was measured SLOWER, 197 against 176 us: two more
    // dependent reads and two barriers in front of every slice.)
    uint32_t wave_flagged = 0;
    for (uint32_t base = d0; base < d0 + kFlagBlock; base += TPB_REC * U) {
        if (base >= d1 && !chunk_mask) break;
        unsigned long long mine[U];
        uint32_t blk[U], linfo[U], same[U];
        uint4 rec[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = base + (uint32_t)u * TPB_REC + threadIdx.x;
            mine[u] = p < d1 ? grouped[p] : (unsigned long long)kSingle;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = base + (uint32_t)u * TPB_REC + threadIdx.x;
            const uint32_t l = (uint32_t)(mine[u] >> (32 + kCibBits)) & lmask;
            blk[u] = p < d1 ? block_of(p) : 0u;
            linfo[u] = t.locus_rel[l];
            rec[u] = make_uint4(0u, 0u, 0u, 0u);
            if (((uint32_t)mine[u] & kSingle) == 0u) rec[u] = t.m_rec[(uint32_t)mine[u]];  // an M entry
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = base + (uint32_t)u * TPB_REC + threadIdx.x;
            same[u] = 1;
            if (p < d1 && (linfo[u] & kLocusDup)) {  // some cell has two kept entries at this locus: count mine
                const uint32_t l = (uint32_t)(mine[u] >> (32 + kCibBits)) & lmask;
                const uint32_t cib = (uint32_t)(mine[u] >> 32) & ((1u << kCibBits) - 1u);
                const size_t g = (size_t)blk[u] * (L + 1) + l;
                const uint32_t gb = blk_off[g], ge = blk_off[g + 1];
                if (ge - gb > kRankScanLimit) {
                    sc->regroup = 1;
                } else if (ge - gb > 1) {
                    same[u] = 0;
                    for (uint32_t q = gb; q < ge; ++q)
                        same[u] += ((uint32_t)(grouped[q] >> 32) & ((1u << kCibBits) - 1u)) == cib ? 1u : 0u;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = base + (uint32_t)u * TPB_REC + threadIdx.x;
            bool flagged = false;
            if (p < d1) {
                const uint32_t k = (uint32_t)mine[u], cib = (uint32_t)(mine[u] >> 32) & ((1u << kCibBits) - 1u);
                const uint32_t l = (uint32_t)(mine[u] >> (32 + kCibBits)) & lmask;
                const uint32_t cell = blk[u] * B + cib;
                flagged = emit_record(t, p, k, rec[u], cib, cell, l, linfo[u] & 0xFFFFu);
                const uint32_t rel = cell - first_cell;
                if (rel < SLOTS) atomicAdd(&sq[rel], (unsigned long long)same[u]);
                else atomicAdd(&per_cell_sq[cell], (unsigned long long)same[u]);
            }
            if (chunk_mask) {  // (uniform; p - lane is a multiple of 64: d0, TPB_REC and the wave's offset are)
                const unsigned long long m = __ballot(flagged);
                wave_flagged += (uint32_t)__popcll(m);
                if ((threadIdx.x & 63u) == 0u) chunk_mask[p >> 6] = m;
            }
        }
    }
    if (chunk_mask && (threadIdx.x & 63u) == 0u && wave_flagged) atomicAdd(&n_flagged, wave_flagged);
    __syncthreads();
    if (block_sum && threadIdx.x == 0) block_sum[blockIdx.x] = n_flagged;
    if (d0 < n)
        for (uint32_t i = threadIdx.x; i < SLOTS; i += TPB_REC)
            if (sq[i]) atomicAdd(&per_cell_sq[first_cell + i], sq[i]);
}

// The serial tail of the records pass in ONE one-workgroup kernel (k_pair_bound, k_publish and k_flag_scan until round
// 32): the pair bound (largest per-cell sum of squares) and whether the locus ranges, cut for the count tile before it
// was known, have to be cut again; the publishing of read-back 3 (pub.box; null: the host copies); then, behind it so
// that the host has the scalars first, the offsets of the list blocks (block_sum; null: no lists from this pass).
__global__ __launch_bounds__(TPB_SCAN) void k_records_tail(const unsigned long long *per_cell_sq, uint32_t n_cells_padded,
                                                          CapChoice caps, uint32_t assumed_counts, Scalars *sc,
                                                          Publish pub, const uint32_t *block_sum, uint32_t n_blocks,
                                                          uint32_t *block_off, uint32_t *total_out) {
    __shared__ unsigned long long s_best[TPB_SCAN / 64];
    unsigned long long best = 0;
    for (uint32_t i = threadIdx.x; i < n_cells_padded; i += TPB_SCAN) best = max(best, per_cell_sq[i]);
    for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned long long)__shfl_down(best, off));
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TPB_SCAN / 64; ++w) best = max(best, s_best[w]);
        sc->pair_bound = max(sc->pair_bound, best);
        sc->caps_wrong = (assumed_counts && !caps.counts(sc)) ? 1u : 0u;
        if (pub.box) {
            __threadfence();  // (this lane's two words, in front of the copy's device-scope loads)
            publish_scalars(sc, pub);
        }
    }
    if (block_sum) {  // (uniform)
        const uint32_t total = scan_block_sums<TPB_SCAN>(block_sum, n_blocks, block_off);
        if (threadIdx.x == 0) *total_out = total;
    }
}

// after the ranges were cut again: the range-relative locus of every entry (bits 16-31 of the compact form)
__global__ __launch_bounds__(TPB) void k_fix_locus_rel(const uint32_t *blk_off, uint32_t nb, uint32_t L,
                                                      const uint32_t *locus_rel, uint32_t *entry32) {
    const uint32_t n_groups = nb * (L + 1);
    for (uint32_t g = blockIdx.x * TPB + threadIdx.x; g < n_groups; g += gridDim.x * TPB) {
        const uint32_t l = g % (L + 1);
        // (the closing slot of a block's row is no group -- and behind the last one blk_off ends: its successor
        // is whatever the allocation held, which a fresh handle showed as a memory fault in
        // test_very_deep_loci_unstaged_ranges)
        if (l == L) continue;
        const uint32_t b = blk_off[g], e = blk_off[g + 1];
        if (b == e) continue;
        const uint32_t lrel = (locus_rel[l] & 0xFFFFu) << 16;
        for (uint32_t d = b; d < e; ++d) entry32[d] = (entry32[d] & 0xFFFFu) | lrel;
    }
}

int bits_for(unsigned long long max_value) {
    int b = 1;
    while (b < 64 && (max_value >> b) != 0) ++b;
    return b;
}

// ---- the host half: one attempt at the pipeline, a function per stage and per route of a stage ------------------

// What an attempt, or a step of one, comes to. Go: on with the next step (no attempt ends with it).
struct Attempt {
    enum Kind { Go, Done, NeedHost, RetryRadix, RetryPlain, Error } kind = Go;
    std::string text;  // of an Error
    bool go() const { return kind == Go; }
    static Attempt stop(Kind k) {
        Attempt a;
        a.kind = k;
        return a;
    }
    static Attempt error(std::string t) {
        Attempt a;
        a.kind = Error;
        a.text = std::move(t);
        return a;
    }
};

#define HIP_OK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) return Attempt::error(std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)
#define STEP(expr)                  \
    do {                            \
        Attempt a__ = (expr);       \
        if (!a__.go()) return a__;  \
    } while (0)

// What a read-back of the scalars says. Before the records are written: the input's order, a void attempt (the id
// space was assumed too small), a group too long for the counting scheme, a size this path does not cover. Behind
// them: the errors of the group mapping (k_keys2, k_bin_hist), a (block, locus) group too long (k_entry_records) --
// and the size limit once more: k_completed raises need_host on the side stream, beside read-back 2, which may or
// may not see it. The read-back behind the records does: `stream` has waited for the side stream's ev_join by then
// (PackAttempt::run, in front of the records), and every ev_join is recorded behind the build's k_completed.
Attempt scalar_verdict(const Scalars &h, bool records_written) {
    if (records_written) {
        if (h.error == 1) return Attempt::error("group id outside group_id_to_pos");
        if (h.error == 2) return Attempt::error("group_id_to_pos maps outside the matrix");
        if (h.regroup) return Attempt::stop(Attempt::RetryRadix);
        return h.need_host ? Attempt::stop(Attempt::NeedHost) : Attempt();
    }
    if (h.error == 3) return Attempt::error("positions must be strictly increasing within a chromosome");
    if (h.id_exceeded) return Attempt::stop(Attempt::RetryPlain);
    if (h.regroup) return Attempt::stop(Attempt::RetryRadix);
    return h.need_host ? Attempt::stop(Attempt::NeedHost) : Attempt();
}

// Stage 1's product: the entries in (chromosome, read id) order, pileup order inside a read. `sub` is the pileup the
// read assembly of stages 2-4 sees: the whole one, or (single-entry route) the compacted entries of the ids that
// occur more than once -- n_m of them; m_entry maps them back, m_index numbers them (the M entries before an entry).
struct Grouped : Attempt {
    Grouped() = default;
    Grouped(Attempt a) : Attempt(std::move(a)) {}
    unsigned long long *skey = nullptr;
    uint32_t *sval = nullptr, *sloc = nullptr;
    Raw sub{};
    uint32_t n_m = 0;
    MIndex m_index{nullptr, nullptr};
    const uint32_t *m_entry = nullptr;
    bool counting = false;      // not the radix sort
    bool single_entry = false;  // the single-entry route, held to the end
    bool abandoned = false;     // ... or given up (clustered loci): the caller takes the counting route
};

// What stages 2-4 write and stage 5 still reads. Marks and ranks are always those of the whole pileup; with the
// single-entry route the M entries have marks and ranks of their own beside them.
struct ReadViews {
    uint32_t *keep;
    unsigned long long *incl;
    MarksRanksCounts marks;
    Runs runs;
    uint32_t *mark_sub, *arank_m;  // null without the single-entry route
    Ranks ranks;
    uint32_t *read_off, *read_locus;
    uint8_t *read_base;
};

// Stage 5's decisions, all made on the host from what read-back 2 brought: cell blocks, the binning tiles, the two
// sets of staging limits the locus ranges are cut for, and the segments they are cut in.
struct TilePlan {
    uint32_t B, nb, B_log2, lbits;
    bool stage_masks;
    CapChoice caps;
    uint32_t n_seg;
    size_t variant_stride;
    uint32_t TL, locus_grid;  // tiles of TL consecutive loci per workgroup: nb * (TL + 1) words of LDS, 32 KiB at most
    size_t lds;
};
TilePlan plan_tiles(uint32_t num_cells, uint32_t L, uint32_t block_cells, StageGeometry (*geometry)(uint32_t),
                    bool allow_count_tile, uint32_t n_kept, uint64_t multi_entries) {
    TilePlan p;
    if (block_cells == 0) {
        const StageGeometry g64 = geometry(64);
        const bool clustered = n_kept && (double)multi_entries > g64.masks_threshold * (double)n_kept;
        block_cells = (clustered || num_cells <= 64) ? 64 : 128;
    }
    const StageGeometry geo = geometry(block_cells);
    p.B = block_cells;
    p.nb = (num_cells + p.B - 1) / p.B;
    p.B_log2 = p.B == 64 ? 6u : 7u;
    p.lbits = (uint32_t)bits_for(L - 1);
    p.stage_masks = n_kept && (double)multi_entries > geo.masks_threshold * (double)n_kept;
    // The pair bound decides the tile variant, and the tile variant the staging limits of the locus ranges;
    // the bound comes out of the grouping, the ranges need only the offsets: they are cut for both sets of
    // limits while the grouping runs (k_ranges_segment), and picked afterwards.
    CapChoice &caps = p.caps;
    caps.entries_plain = p.stage_masks ? geo.cap_entries_masks : geo.cap_entries_plain;
    caps.loci_plain = p.stage_masks ? geo.cap_loci_masks : geo.cap_loci_plain;
    caps.entries_counts = geo.cap_entries_counts;
    caps.loci_counts = geo.cap_loci_counts;
    caps.count_limit = kCountTileLimit;
    caps.allow_counts = (allow_count_tile && !p.stage_masks) ? 1u : 0u;
    // Segment length of the count tile's ranges. A segment is cut greedily -- full ranges, then a remainder --, and
    // every range costs a workgroup the same set-up and the same item slots whatever it holds: a segment that
    // needs 1.3 ranges (C5: 8190 loci x 1.3 entries per cell block and locus against 8192 staged entries) becomes
    // one full range and one at 29 %, 49 ranges where 34 would do. Where a full-length segment overflows the
    // entry limit, shorter segments that hold ONE range each at 93 % (the margin covers the densest block's
    // fluctuation; a segment that overflows all the same is cut in two) are taken if they give fewer ranges.
    if (caps.allow_counts && n_kept && L) {
        const double density = (double)n_kept / ((double)num_cells / p.B) / (double)L;  // entries per (full cell block, locus)
        const double per_segment = density * caps.loci_counts / caps.entries_counts;  // ranges a full-length segment needs
        if (per_segment > 1.0) {
            const double greedy = std::ceil((double)L / caps.loci_counts) * std::ceil(per_segment);
            const uint32_t one = std::max(64u, (uint32_t)(0.93 * caps.entries_counts / density));
            if (one < caps.loci_counts && std::ceil((double)L / one) * 1.05 < greedy) caps.loci_counts = one;
        }
    }
    const uint32_t lo_loci = caps.allow_counts ? std::min(caps.loci_plain, caps.loci_counts) : caps.loci_plain;
    const uint32_t hi_loci = caps.allow_counts ? std::max(caps.loci_plain, caps.loci_counts) : caps.loci_plain;
    p.n_seg = (L + lo_loci - 1) / lo_loci;
    p.variant_stride = (size_t)p.n_seg * hi_loci + p.n_seg + 2;
    p.TL = 64;
    while (p.TL > 1 && (size_t)p.nb * (p.TL + 1) * 4 > 32768) p.TL >>= 1;
    p.locus_grid = std::min<uint32_t>((L + p.TL - 1) / p.TL, 8192);
    p.lds = (size_t)p.nb * (p.TL + 1) * 4;
    return p;
}

// What stage 5 works on: the plan, the totals of read-back 2 and the views of its generations
struct Stage5 {
    TilePlan p;
    uint32_t n_kept, kept_m;  // kept entries, and those of them that went through the read assembly
    size_t n_off;
    uint32_t *t_read, *krank, *blk_off, *blk_cnt;
    uint8_t *kflags, *dupflag;
    unsigned long long *entry_kc;  // null on the radix route
    BinRadix bin;                  // (the radix route's; per_cell_sq is where both routes have it)
    uint4 *m_rec;                  // the counting route's
    unsigned long long *per_cell_sq;
    Segs segs;
};

// One attempt. With force_radix == false the two groupings (entries by read, kept entries by (cell block, locus))
// use the counting scheme when its preconditions hold; a group too long for it ends the attempt with RetryRadix.
struct PackAttempt {
    // fixed over the attempt
    const DeviceFlatPileup &in;
    const uint32_t num_cells, mfl, num_threads, block_cells;
    StageGeometry (*const geometry)(uint32_t);
    const bool allow_count_tile, force_radix, no_assumptions, overlap;
    const hipStream_t stream;
    DevicePacked &pk;
    DeviceArena *const S;
    const uint32_t E, L, C;
    const PackShape shape;
    const Raw raw;
    const int ids_aligned;
    HostTrace trace;
    // set by prepare_workspace
    MiscViews<Scalars> m{nullptr, PackShape{0, 0, 0, 0}};
    Scalars *sc = nullptr;
    void *cub_tmp = nullptr;

    PackAttempt(const DeviceFlatPileup &in_, uint32_t num_cells_, uint32_t mfl_, uint32_t num_threads_,
                uint32_t block_cells_, StageGeometry (*geometry_)(uint32_t), bool allow_count_tile_, bool force_radix_,
                bool no_assumptions_, bool overlap_, hipStream_t stream_, DevicePacked &pk_)
        : in(in_), num_cells(num_cells_), mfl(mfl_), num_threads(num_threads_), block_cells(block_cells_),
          geometry(geometry_), allow_count_tile(allow_count_tile_), force_radix(force_radix_),
          no_assumptions(no_assumptions_), overlap(overlap_), stream(stream_), pk(pk_), S(pk_.scratch),
          E(static_cast<uint32_t>(in_.n_entries)), L(in_.n_loci), C(in_.n_chr), shape{E, L, C, num_cells_},
          raw{in_.chr_locus_off, C, in_.locus_pos, in_.locus_entry_off, in_.read_ids, in_.id_base16, in_.id_base32,
              in_.group_id_to_pos, in_.n_groups, L, E},
          ids_aligned((reinterpret_cast<uintptr_t>(in_.read_ids) & 15u) == 0 ? 1 : 0) {}

    hipError_t ensure(Arena::Id a, size_t id_slots = 0) { return S[a].ensure(arena_bytes<Scalars>(a, shape, id_slots)); }
    template <class T>
    hipError_t exclusive_sum(const T &in_it, uint32_t *out, size_t n) {
        size_t cub_cap = S[Arena::CUB].bytes;
        return hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_cap, in_it, out, (int)n, stream);
    }

    // ---- buffers (sized up front: a re-allocation in mid-pipeline would synchronise) -----------
    Attempt prepare_workspace() {
        for (Arena::Id a : {Arena::MISC, Arena::KEY_A, Arena::KEY_B, Arena::VAL_A, Arena::VAL_B, Arena::WORK_A,
                            Arena::WORK_B, Arena::RUNS, Arena::ENTRY_KC, Arena::TMP, Arena::BIN})
            HIP_OK(ensure(a));
        m = MiscViews<Scalars>(S[Arena::MISC].p, shape);
        sc = m.sc;
        {
            // the counting scheme for read ids needs a table over the id space
            unsigned long long *key_a = UnsortedKeys(S[Arena::KEY_A].p, E), *key_b = SortedKeys(S[Arena::KEY_B].p, E);
            uint32_t *val_a = GroupedIds(S[Arena::VAL_A].p, E), *val_b = SortedValues(S[Arena::VAL_B].p, E);
            size_t need = 0, most = 0;
            HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, key_a, key_b, val_a, val_b, (int)E, 0, 64, stream));
            most = std::max(most, need);
            {
                hipcub::CountingInputIterator<uint32_t> positions(0u);
                hipcub::TransformInputIterator<unsigned long long, HeadKeepOp, hipcub::CountingInputIterator<uint32_t>>
                        flags(positions, HeadKeepOp{key_b, val_a, val_a});
                HIP_OK(hipcub::DeviceScan::InclusiveSum(nullptr, need, flags, key_a, (int)E, stream));
                most = std::max(most, need);
            }
            HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, val_a, val_b, (int)E + 1, stream));
            most = std::max(most, need);
            HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, val_a, val_b,
                                                    (int)std::max<size_t>(shape.n_off_max(), id_space_cap() + 2), stream));
            most = std::max(most, need);
            HIP_OK(S[Arena::CUB].ensure(most + 1024));
        }
        cub_tmp = S[Arena::CUB].p;
        HIP_OK(hipMemsetAsync(sc, 0, m.zeroed, stream));
        if (!pk.side) {
            HIP_OK(hipStreamCreateWithFlags(&pk.side, hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&pk.ev_fork, hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&pk.ev_join, hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&pk.ev_offsets, hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&pk.ev_flush, hipEventDisableTiming));
        }
        return Attempt();
    }
    size_t id_space_cap() const { return std::min<size_t>((size_t)kIdSpaceFactor * E + 1024, (size_t)1 << 30); }

    // ---- 1: entries grouped by (chromosome, read id), pileup order inside a read ---------------
    // The entry -> locus table serves the general counting route and the radix route. The single-entry route has none
    // (the chromosome of an entry follows from its index, the locus is wanted of the M entries only: k_m_fields), so
    // the table is made where that route is not tried, and behind read-back 1b where it is given up.
    Attempt make_entry_locus() {
        HIP_OK(ensure(Arena::ELOC));
        hipLaunchKernelGGL(k_entry_locus, dim3(blocks_for((uint64_t)L * 64)), dim3(TPB), 0, stream, raw,
                           EntryLocus(S[Arena::ELOC].p, E).p, sc);
        return Attempt();
    }
    Grouped whole_pileup(bool counting) const {
        Grouped g;
        g.skey = SortedKeys(S[Arena::KEY_B].p, E), g.sval = SortedValues(S[Arena::VAL_B].p, E);
        g.sloc = SortedLoci(S[Arena::ENTRY_KC].p, E);
        g.sub = raw;
        g.n_m = E;
        g.counting = counting;
        return g;
    }

    Grouped group_by_read() {
        // The size of the id space decides between the counting scheme and the radix sort and sizes the
        // histogram. A handle that has packed before assumes the size of the previous call and does not wait
        // (k_id_range raises Scalars::id_exceeded if that was too small: the attempt is then void and
        // repeated with the read-back).
        const bool assume = !force_radix && !no_assumptions && pk.id_space_hint && pk.id_space_hint <= id_space_cap();
        hipLaunchKernelGGL(k_id_range, dim3(std::min<uint32_t>(256, (E + 4095) / 4096)), dim3(TPB), 0, stream, raw,
                           m.id_max, m.id_negmin, ids_aligned, m.id_base, m.chr_entry,
                           (unsigned long long)(assume ? pk.id_space_hint : 0), sc);
        Scalars hsc;
        std::memset(&hsc, 0, sizeof(hsc));
        if (!assume) {
            HIP_OK(read_scalars(pk, stream, sc, nullptr, &hsc, nullptr));  // read-back 1: the size of the id space
            STEP(scalar_verdict(hsc, false));
        }
        const size_t id_space = assume ? (size_t)pk.id_space_hint
                                       : (size_t)std::min<unsigned long long>(hsc.id_space, 1ull << 40);
        const bool counting = !force_radix && id_space <= id_space_cap();
        HIP_OK(ensure(Arena::WORK_A, counting ? id_space + 1 : 0));
        HIP_OK(ensure(Arena::WORK_B, counting ? id_space + 1 : 0));
        // The single-entry route pays when most reads have one entry (counting scheme only): a call that finds more
        // than half of the entries in multi-entry reads gives it up, and the handle's next calls do not try.
        if (!pk.split_pays && ++pk.calls_without_split >= 16) {  // (pileups change: look again now and then)
            pk.split_pays = true;
            pk.calls_without_split = 0;
        }
        if (!(counting && pk.split_pays)) {
            STEP(make_entry_locus());
            return counting ? group_by_read_counting(id_space, false) : group_by_read_radix(hsc.max_read_id);
        }
        Grouped g = group_by_read_single_entry(id_space);
        if (!g.abandoned) return g;
        pk.split_pays = false;
        pk.calls_without_split = 0;
        return group_by_read_counting(id_space, true);
    }

    // which ids repeat (k_id_store, k_id_check), the entries of those as a compacted pileup of their own, and their
    // reads: the groups of equal winner
    Grouped group_by_read_single_entry(size_t id_space) {
        const uint32_t n_flag_blocks = (uint32_t)shape.flag_blocks();
        const size_t n_chunks = shape.chunks();
        uint32_t *last = IdSlots(S[Arena::WORK_A].p, id_space + 1);  // per id the number of one of its entries
        HIP_OK(ensure(Arena::M_CHUNKS));
        const MChunks chunks(S[Arena::M_CHUNKS].p, shape);
        HIP_OK(ensure(Arena::MARK_M));
        uint8_t *multi = MultiFlags(S[Arena::MARK_M].p, shape.flag_bytes());
        HIP_OK(hipMemsetAsync(multi, 0, shape.flag_bytes(), stream));
        hipLaunchKernelGGL(k_id_store, dim3(blocks_for((E + 3) / 4)), dim3(TPB), 0, stream, raw, m.chr_entry, m.id_base,
                           m.id_negmin, sc, last, ids_aligned);
        hipLaunchKernelGGL(k_id_check, dim3(blocks_for((E + 3) / 4)), dim3(TPB), 0, stream, raw, m.chr_entry, m.id_base,
                           m.id_negmin, sc, last, multi, ids_aligned);
        for (Arena::Id a : {Arena::M_ENTRY, Arena::RID_M, Arena::IDB_M, Arena::ELOC_M, Arena::ARANK_M, Arena::DENSE_M})
            HIP_OK(ensure(a));
        uint32_t *m_entry = PerM(S[Arena::M_ENTRY].p, E), *rid_m = PerM(S[Arena::RID_M].p, E);
        uint32_t *idb_m = PerM(S[Arena::IDB_M].p, E), *eloc_m = PerM(S[Arena::ELOC_M].p, E);
        const FlagBlockSums sums(S[Arena::VAL_A].p, shape);
        hipLaunchKernelGGL(k_flag_count, dim3(n_flag_blocks), dim3(TPB), 0, stream, multi, sums.block_sum);
        hipLaunchKernelGGL(k_flag_scan, dim3(1), dim3(TPB_SCAN), 0, stream, sums.block_sum, n_flag_blocks, sums.block_off,
                           chunks.chunk_pre + (n_chunks - 1), sc);
        // read-back 1b: how many entries take the general path (sizes every launch over them); k_compact_m's first
        // workgroup publishes it. (count_m sits at the base of DENSE_M whatever the number of M entries: MReads)
        const Publish pub = fold_publish(pk, nullptr);
        hipLaunchKernelGGL(k_compact_m, dim3(n_flag_blocks), dim3(TPB), 0, stream, raw, multi, sums.block_off,
                           chunks.chunk_pre, chunks.chunk_mask, m_entry, MReads(S[Arena::DENSE_M].p, 0).count_m, sc, pub);
        Scalars hsc;
        HIP_OK(read_scalars(pk, stream, sc, nullptr, &hsc, nullptr, nullptr, &pub));
        STEP(scalar_verdict(hsc, false));
        Grouped g = whole_pileup(true);
        g.n_m = hsc.n_multi_id;
        if ((uint64_t)g.n_m * 2 > E) {  // clustered loci: (nearly) every read has several entries, no short cut
            g.abandoned = true;
            return g;
        }
        g.single_entry = true;
        g.m_index = MIndex{chunks.chunk_pre, chunks.chunk_mask};
        g.m_entry = m_entry;
        g.sub.read_ids = rid_m;
        g.sub.id_base16 = nullptr;
        g.sub.id_base32 = idb_m;
        g.sub.n_entries = g.n_m;
        if (g.n_m) {
            const uint32_t n_m = g.n_m;
            const MReads r(S[Arena::DENSE_M].p, n_m);
            hipLaunchKernelGGL(k_m_fields, dim3(blocks_for(n_m)), dim3(TPB), 0, stream, raw, m.chr_entry, m.id_base,
                               m.id_negmin, last, g.m_index, m_entry, n_m, rid_m, idb_m, eloc_m, r.winner_m, r.count_m);
            HIP_OK(exclusive_sum(r.count_m, r.goff, (size_t)n_m + 1));
            hipLaunchKernelGGL(k_group_scatter, dim3(blocks_for(n_m)), dim3(TPB), 0, stream, r.winner_m, n_m, r.goff,
                               r.count_m, r.members, r.g_begin, r.g_len);
            hipLaunchKernelGGL(k_group_rank, dim3(blocks_for(n_m)), dim3(TPB), 0, stream, g.sub, r.members, r.g_begin,
                               r.g_len, eloc_m, n_m, g.skey,
                               g.sval, g.sloc, sc);
        }
        return g;
    }

    // histogram over the dense id space, scan, scatter with an atomic cursor, rank inside the (short) group
    Grouped group_by_read_counting(size_t id_space, bool single_entry_abandoned) {
        Grouped g = whole_pileup(true);
        uint32_t *hist = IdSlots(S[Arena::WORK_A].p, id_space + 1), *id_off = IdOffsets(S[Arena::WORK_B].p, id_space + 1);
        uint32_t *grouped = GroupedIds(S[Arena::VAL_A].p, E), *dense = DenseIds(S[Arena::KEY_A].p, E);
        // (given up: the id slots hold entry numbers, this route wants counts -- and the entry -> locus table)
        HIP_OK(hipMemsetAsync(hist, 0, (id_space + 1) * 4, stream));
        if (single_entry_abandoned) STEP(make_entry_locus());
        const uint32_t *eloc = EntryLocus(S[Arena::ELOC].p, E);
        hipLaunchKernelGGL(k_id_hist, dim3(blocks_for(E)), dim3(TPB), 0, stream, raw, eloc, m.id_base, m.id_negmin, sc,
                           dense, hist);
        HIP_OK(exclusive_sum(hist, id_off, id_space + 1));
        hipLaunchKernelGGL(k_id_scatter, dim3(blocks_for(E)), dim3(TPB), 0, stream, dense, E, id_off, sc, hist, grouped);
        hipLaunchKernelGGL(k_id_rank, dim3(blocks_for(E)), dim3(TPB), 0, stream, raw, dense, id_off, grouped, eloc,
                           g.skey, g.sval, g.sloc, sc);
        return g;
    }

    // the hipCUB radix sort: the ids are sparse, or a group was too long for the counting scheme
    Grouped group_by_read_radix(uint32_t max_read_id) {
        Grouped g = whole_pileup(false);
        unsigned long long *key_a = UnsortedKeys(S[Arena::KEY_A].p, E);
        uint32_t *val_a = GroupedIds(S[Arena::VAL_A].p, E);
        const uint32_t *eloc = EntryLocus(S[Arena::ELOC].p, E);
        const uint32_t id_bits = (uint32_t)bits_for(max_read_id);
        hipLaunchKernelGGL(k_entry_keys, dim3(blocks_for(E)), dim3(TPB), 0, stream, raw, eloc, id_bits, key_a, val_a);
        size_t cub_cap = S[Arena::CUB].bytes;
        HIP_OK(hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_cap, key_a, g.skey, val_a,
                                                   g.sval, (int)E, 0, (int)id_bits + bits_for(C),
                                                   stream));
        hipLaunchKernelGGL(k_sorted_locus, dim3(blocks_for(E)), dim3(TPB), 0, stream, raw, g.sval, eloc, E, g.sloc);
        return g;
    }

    // ---- 2-4: duplicate rule, reads = runs of equal key, per-read lists, appearance ranks ------
    // (the number of reads R stays on the device until read-back 2; buffers indexed by read are laid
    // out for the upper bound E)
    Attempt ensure_outputs() {
        const size_t n_off_max = shape.n_off_max();
        HIP_OK(pk.read_off.ensure(((size_t)E + 1) * 4));
        HIP_OK(pk.read_locus.ensure((size_t)E * 4));
        HIP_OK(pk.read_base.ensure(E));
        HIP_OK(pk.range_off.ensure(((size_t)L + 2) * 4));
        HIP_OK(pk.entry.ensure((size_t)E * 16));
        HIP_OK(pk.entry32.ensure((size_t)E * 4));
        HIP_OK(pk.mask32.ensure((size_t)E * 4));
        HIP_OK(pk.entry_read.ensure((size_t)E * 4));
        HIP_OK(pk.blk_off.ensure((n_off_max + 1) * 4));
        return Attempt();
    }
    ReadViews read_views(const Grouped &g) const {
        const MarksRanksCounts marks(S[Arena::KEY_A].p, shape);
        return ReadViews{KeepFlags(S[Arena::WORK_A].p, (size_t)E + 1),
                         InclSums(S[Arena::WORK_B].p, (size_t)E + 1),
                         marks,
                         Runs(S[Arena::RUNS].p, shape),
                         g.single_entry ? MarksOfM(S[Arena::MARK_M].p, (size_t)E + 2).p : nullptr,
                         g.single_entry ? PerM(S[Arena::ARANK_M].p, E).p : nullptr,
                         Ranks{g.m_index, g.single_entry ? marks.arank : nullptr, marks.arank},
                         pk.read_off.as<uint32_t>(),
                         pk.read_locus.as<uint32_t>(),
                         pk.read_base.as<uint8_t>()};
    }
    // Reads from the current `split` flags (cuts of reads that outlive max_fragment_length: none on the first build,
    // null), then completed counts and the flush chain. The chain is sequential (one lane per chromosome) and only
    // the final gather needs its result: it runs on a side stream, next to the grouping of the kept entries.
    // pub: where k_read_info publishes the read-back that follows the build (null, or no read: the caller's k_publish)
    Attempt build_reads(const Grouped &g, const ReadViews &v, const uint32_t *split, Publish *pub = nullptr) {
        const uint32_t n_m = g.n_m;
        uint32_t *mark_sub = g.single_entry ? v.mark_sub : v.marks.mark, *arank = v.marks.arank;
        if (n_m) {
            hipLaunchKernelGGL(k_dup_mark, dim3(blocks_for(n_m)), dim3(TPB), 0, stream, g.sub, g.skey, g.sval, g.sloc, split,
                               n_m, v.keep, mark_sub);
            hipcub::CountingInputIterator<uint32_t> positions(0u);
            hipcub::TransformInputIterator<unsigned long long, HeadKeepOp, hipcub::CountingInputIterator<uint32_t>>
                    flags(positions, HeadKeepOp{g.skey, v.keep, split});
            size_t cub_cap = S[Arena::CUB].bytes;
            HIP_OK(hipcub::DeviceScan::InclusiveSum(cub_tmp, cub_cap, flags, v.incl, (int)n_m, stream));
        }
        const uint32_t *arank_sub = arank;
        if (g.single_entry) {  // (the ranks' array holds the n_m + 1 prefix sums `unm` instead: struct Ranks)
            hipcub::CountingInputIterator<uint32_t> entries(0u);
            hipcub::TransformInputIterator<uint32_t, UnmarkedM, hipcub::CountingInputIterator<uint32_t>> unmarked(
                    entries, UnmarkedM{mark_sub, n_m});
            HIP_OK(exclusive_sum(unmarked, arank, (size_t)n_m + 1));
            hipLaunchKernelGGL(k_ranks_runs, dim3(blocks_for(std::max(n_m, 1u))), dim3(TPB), 0, stream, raw, v.ranks,
                               g.m_entry, n_m, v.arank_m, m.rbeg, v.incl, g.sloc, v.runs.run_start, v.read_locus,
                               v.read_base, sc);
            arank_sub = v.arank_m;
        } else {
            HIP_OK(exclusive_sum(v.marks.mark, arank, (size_t)E + 1));
            if (n_m)
                hipLaunchKernelGGL(k_runs_csr, dim3(blocks_for(n_m)), dim3(TPB), 0, stream, g.sub, v.incl, g.sval, g.sloc,
                                   n_m, v.runs.run_start, v.read_locus, v.read_base);
        }
        if (n_m) {
            // The single-entry route's few reads (the M entries) take a grid of 512 workgroups at the most, and its last
            // workgroup publishes (each draws a ticket; the scan's last sum rides along: reads | kept entries << 32).
            // The whole pileup's reads (clustered loci: tens of millions) keep the large grid and the k_publish behind.
            const bool fold = pub && g.single_entry;
            const Publish folded = fold ? (*pub = fold_publish(pk, v.incl + (n_m - 1))) : Publish{nullptr, 0ull, nullptr};
            hipLaunchKernelGGL(k_read_info, dim3(std::min<uint32_t>(blocks_for(n_m), fold ? 512 : 2048)), dim3(TPB), 0, stream, g.sub,
                               v.incl, v.runs.run_start, g.sval, g.sloc, arank_sub, mfl, v.runs.run_rank,
                               g.single_entry ? nullptr : m.rbeg, v.read_off, sc, folded);
        }
        HIP_OK(hipEventRecord(pk.ev_fork, stream));
        HIP_OK(hipStreamWaitEvent(pk.side, pk.ev_fork, 0));
        hipLaunchKernelGGL(k_completed, dim3(blocks_for(L)), dim3(TPB), 0, pk.side, raw, v.ranks, m.rbeg, mfl, m.cnt, sc);
        hipLaunchKernelGGL(k_flush_chain, dim3(C), dim3(TPB), 0, pk.side, raw, m.cnt, 4u * num_threads, sc, m.flushed,
                           m.flush_loci, m.flush_count, v.ranks, m.rbeg, g.single_entry ? m.tail_begin : nullptr);
        HIP_OK(hipEventRecord(pk.ev_flush, pk.side));
        HIP_OK(hipEventRecord(pk.ev_join, pk.side));
        return Attempt();
    }
    // Some id's entries span >= max_fragment_length: a flush may erase it before its last entry and the id re-opens
    // as a new read. Cut at the flush loci, rebuild, repeat until the cuts are stable (they move forward with the
    // flushes they cause: a few rounds). The cuts live in TMP, free until k_keys2.
    Attempt settle_flush_cuts(const Grouped &g, const ReadViews &v, Scalars *hsc, unsigned long long *totals) {
        const uint32_t n_m = g.n_m;
        uint32_t *split = SplitFlags(S[Arena::TMP].p, E);
        HIP_OK(hipMemsetAsync(split, 0, (size_t)std::max(n_m, 1u) * 4, stream));
        for (int round = 0; round < kMaxSplitRounds; ++round) {
            HIP_OK(hipStreamWaitEvent(stream, pk.ev_join, 0));  // the chain of the previous build
            HIP_OK(hipMemsetAsync(&sc->split_changed, 0, 4, stream));
            hipLaunchKernelGGL(k_split_update, dim3(blocks_for(n_m)), dim3(TPB), 0, stream, g.sub, g.skey, g.sloc, mfl,
                               m.flush_loci, m.flush_count, split, sc);
            HIP_OK(read_scalars(pk, stream, sc, nullptr, hsc, nullptr));
            if (!hsc->split_changed) return Attempt();
            HIP_OK(hipMemsetAsync(&sc->multi_entries, 0, 8, stream));  // k_read_info adds to it
            STEP(build_reads(g, v, split));
            HIP_OK(read_scalars(pk, stream, sc, n_m ? v.incl + (n_m - 1) : nullptr, hsc, totals));
        }
        return Attempt::stop(Attempt::NeedHost);  // did not settle: the exact sequential emulation decides
    }

    // ---- 5: kept entries grouped by (cell block, locus, cell), offsets, bound, ranges, records ----
    void launch_ranges_segment(const Stage5 &s, hipStream_t on) {
        hipLaunchKernelGGL(k_ranges_segment, dim3(s.p.n_seg, s.p.caps.allow_counts ? 2u : 1u), dim3(TPB), 0, on, s.blk_off,
                           s.p.nb, L, s.p.caps, s.segs.seg_ends, s.segs.seg_count, s.p.variant_stride);
    }
    // (call when blk_off is complete on `stream`; pick: the ranges are picked there as well, see bin_counting)
    Attempt cut_ranges_on_side(const Stage5 &s, bool pick) {
        HIP_OK(hipEventRecord(pk.ev_offsets, stream));
        HIP_OK(hipStreamWaitEvent(pk.side, pk.ev_offsets, 0));
        launch_ranges_segment(s, pk.side);
        if (pick) compact_ranges(s, 0u, assumed_variant(s.p), pk.side);
        HIP_OK(hipEventRecord(pk.ev_join, pk.side));
        return Attempt();
    }
    // the M entries' records, on the side stream beside the placing pass
    Attempt m_records_on_side(const Stage5 &s, const ReadViews &v) {
        hipLaunchKernelGGL(k_m_records, dim3(blocks_for(s.kept_m)), dim3(TPB), 0, pk.side, raw, s.kept_m, s.t_read,
                           v.read_off, v.read_locus, v.read_base, s.krank, s.kflags, m.rbeg, m.flushed,
                           s.m_rec, sc);
        HIP_OK(hipEventRecord(pk.ev_join, pk.side));
        return Attempt();
    }
    // the locus ranges picked from the segments (assumed: 1 the count tile's limits, 0 the plain ones, -1 by the pair
    // bound of sq_rows rows) and what a record needs of its locus
    void compact_ranges(const Stage5 &s, uint32_t sq_rows, int assumed, hipStream_t on) {
        hipLaunchKernelGGL(k_ranges_compact, dim3(1), dim3(TPB), 0, on, s.segs.seg_ends, s.segs.seg_count,
                           s.p.variant_stride, s.p.n_seg, s.p.caps, pk.range_off.as<uint32_t>(), s.per_cell_sq, sq_rows,
                           assumed, sc);
    }
    void locus_info(const Stage5 &s, const uint8_t *dupflag) {
        if (s.n_kept)
            hipLaunchKernelGGL(k_locus_info, dim3(blocks_for(L)), dim3(TPB), 0, stream, raw, pk.range_off.as<uint32_t>(),
                               sc, dupflag, m.locus_chr, m.locus_rel);
    }
    void pick_ranges(const Stage5 &s, uint32_t sq_rows, int assumed, const uint8_t *dupflag) {
        compact_ranges(s, sq_rows, assumed, stream);
        locus_info(s, dupflag);
    }
    // the limits the counting route cuts the ranges for before the pair bound is known
    static int assumed_variant(const TilePlan &p) { return p.caps.allow_counts ? 1 : 0; }

    // radix route: sort the kept entries by (block, locus, cell), count the groups
    Attempt bin_radix(const Stage5 &s) {
        const BinRadix &b = s.bin;
        if (s.n_kept) {
            size_t cub_cap = S[Arena::CUB].bytes;
            HIP_OK(hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_cap, b.key2_a, b.key2_b, b.val2_a, b.val2_b,
                                                       (int)s.n_kept, 0, (int)(kCibBits + s.p.lbits) + bits_for(s.p.nb - 1),
                                                       stream));
            hipLaunchKernelGGL(k_group_counts, dim3(std::min<uint32_t>(2048, (s.n_kept + 4095) / 4096)), dim3(TPB), 0,
                               stream, b.key2_b, s.n_kept, s.p.B, L, s.p.lbits, s.blk_cnt, s.per_cell_sq);
        }
        HIP_OK(exclusive_sum(s.blk_cnt, s.blk_off, s.n_off));
        return cut_ranges_on_side(s, false);
    }
    // counting route: per-locus LDS histograms (hist_first: launched already, in front of k_keys2), scan, placement
    Attempt bin_counting(const Grouped &g, const ReadViews &v, const Stage5 &s, bool hist_first) {
        const TilePlan &p = s.p;
        if (!hist_first)
            hipLaunchKernelGGL(k_bin_hist, dim3(p.locus_grid), dim3(TPB), p.lds, stream, raw, p.nb, p.TL, s.entry_kc, nullptr,
                               num_cells, p.B_log2, s.blk_cnt, sc, 0u);
        trace.mark("k_bin_hist launched");
        // Where most kept entries belong to multi-entry reads (clustered loci) the M entries' records are the longest
        // kernel of the packing (C3 clustered: 1.5 ms) and nothing but k_keys2 and the flush chain stands before
        // them: they start on the side stream as soon as k_keys2 is through -- beside the histogram, the offset scan
        // AND the placing pass, not behind the range cutting (round 4: 0.5 ms of a 7.6 ms packing) --, and the short
        // range cutting stays on the main stream in front of the placing pass. On sparse loci (few M entries) the
        // order of round 3: range cutting, then the records, both on the side stream.
        const bool records_first = s.kept_m && (uint64_t)s.kept_m * 4u > (uint64_t)s.n_kept;
        if (records_first) {
            HIP_OK(hipEventRecord(pk.ev_offsets, stream));  // k_keys2 is through
            HIP_OK(hipStreamWaitEvent(pk.side, pk.ev_offsets, 0));
            STEP(m_records_on_side(s, v));
        }
        HIP_OK(exclusive_sum(s.blk_cnt, s.blk_off, s.n_off));
        trace.mark("offset scan launched");
        // The picking of the ranges (k_ranges_compact) needs the segments only, nothing the placing pass writes: it
        // goes directly behind the cutting, beside the placing pass; k_locus_info, which wants the placing pass'
        // duplicate flags, stays behind it on the main stream (records_counting).
        if (records_first) {
            launch_ranges_segment(s, stream);
            compact_ranges(s, 0u, assumed_variant(p), stream);
        } else {
            STEP(cut_ranges_on_side(s, true));
            if (s.kept_m) STEP(m_records_on_side(s, v));  // behind the flush chain and the range cutting
        }
        if (s.n_kept) {
            HIP_OK(hipStreamWaitEvent(stream, pk.ev_flush, 0));  // the S entries' tail flags
            // (a bitmap over the cells per wave beside the cursors, if 48 KiB of LDS hold both)
            uint32_t bm_words = (p.nb * p.B + 31) / 32;
            if (p.lds + (size_t)(TPB / 64) * bm_words * 4 > 49152) bm_words = 0;
            hipLaunchKernelGGL(k_bin_place, dim3(p.locus_grid), dim3(TPB), p.lds + (size_t)(TPB / 64) * bm_words * 4, stream,
                               raw, p.nb, p.TL, s.entry_kc, s.blk_off, p.B_log2, bm_words,
                               g.single_entry ? m.tail_begin : nullptr, GroupedKept(S[Arena::KEY_B].p, E).p, s.dupflag);
        }
        return Attempt();
    }
    void records_radix(const ReadViews &v, const Stage5 &s) {
        const BinRadix &b = s.bin;
        pick_ranges(s, s.n_kept ? s.p.nb * s.p.B : 0u, -1, nullptr);
        if (s.n_kept)
            hipLaunchKernelGGL(k_records, dim3(blocks_for(s.n_kept)), dim3(TPB), 0, stream, raw, b.key2_b, b.val2_b, s.n_kept,
                               s.t_read, v.read_off, v.read_locus, v.read_base, s.krank, s.kflags, m.rbeg, m.flushed,
                               m.locus_chr, m.locus_rel, s.p.B, s.p.lbits, pk.entry.as<uint4>(), pk.entry32.as<uint32_t>(),
                               pk.stage_masks ? pk.mask32.as<uint32_t>() : nullptr, pk.entry_read.as<uint32_t>(), sc);
    }
    // Counting route: the entries stay in k_bin_place's order and one pass, a thread per (block, locus) group, writes
    // the records and sums the per-cell squares. The locus ranges (their range-relative locus is part of a record)
    // are cut for the count tile if it is allowed at all; the pair bound comes out of the same pass, and if it forbids
    // the count tile the ranges are cut again and the records patched (deep pileups only: close_attempt).
    // Returns whether the records pass left the flags the flagged entries' lists are made of.
    // pub: the read-back behind the records, published by the tail kernel (close_attempt launches nothing for it)
    bool records_counting(const Stage5 &s, Publish *pub) {
        const TilePlan &p = s.p;
        const int assumed = assumed_variant(p);
        bool lists_here = false;
        locus_info(s, s.dupflag);  // (the ranges were picked beside the placing pass: bin_counting)
        if (s.n_kept) {
            const RecordTables tables{s.m_rec, m.locus_rel, pk.entry.as<uint4>(), pk.entry32.as<uint32_t>(),
                                      pk.stage_masks ? pk.mask32.as<uint32_t>() : nullptr, pk.entry_read.as<uint32_t>()};
            // The flagged entries' lists are wanted wherever the count tile is taken, and they do not depend on what
            // read-back 3 decides (the records carry the absolute locus, k_fix_locus_rel touches the upper half of
            // entry32 only): the records pass leaves the chunks' flags, and the list chain goes behind the publishing
            // kernel of read-back 3. If the pair bound forbids the count tile the lists are not used.
            lists_here = overlap && p.caps.allow_counts && !pk.stage_masks && pk.flag_lists.scratch;
            const FlagScratch fs(pk.flag_lists.scratch, s.n_kept);
            hipLaunchKernelGGL(k_entry_records, dim3((s.n_kept + kFlagBlock - 1) / kFlagBlock), dim3(TPB_REC), 0, stream,
                               GroupedKept(S[Arena::KEY_B].p, E).p, s.blk_off, s.n_kept, p.nb, L, p.B, p.lbits, tables,
                               s.per_cell_sq, sc, lists_here ? fs.chunk_mask : nullptr, lists_here ? fs.block_sum : nullptr);
        }
        const FlagScratch fs(lists_here ? pk.flag_lists.scratch : nullptr, s.n_kept);
        *pub = fold_publish(pk, nullptr);
        hipLaunchKernelGGL(k_records_tail, dim3(1), dim3(TPB_SCAN), 0, stream, s.per_cell_sq, s.n_kept ? p.nb * p.B : 0u,
                           p.caps, (uint32_t)assumed, sc, *pub, lists_here ? fs.block_sum : nullptr, fs.nb,
                           lists_here ? fs.block_off : nullptr, lists_here ? fs.chunk_pre + 64 * (size_t)fs.nb : nullptr);
        return lists_here;
    }
    // read-back 3: errors of the group mapping, pair bound (-> tile variant), number of ranges. The list chain goes
    // behind its publishing kernel: the GPU works through the lists while the host reads the scalars, returns to its
    // caller and launches the pair kernel. (In front of the publishing kernel the host learned the scalars 50 us
    // later and the GPU then stood idle for as long as the host needs from there to the pair kernel's launch: 74 us
    // under the profiler on C3, and C2, whose lists take 15 us, lost 20 us against the lists behind the read-back.)
    Attempt close_attempt(const Stage5 &s, bool lists_launched, const Publish *folded) {
        const TilePlan &p = s.p;
        Scalars hsc;
        trace.mark("records launched");
        HIP_OK(read_scalars(pk, stream, sc, nullptr, &hsc, nullptr, [&] {
            if (lists_launched)
                flag_lists_from_masks(FlagScratch(pk.flag_lists.scratch, s.n_kept), pk.entry.as<uint4>(), s.blk_off, s.n_off,
                                      pk.flag_lists.grp, pk.flag_lists.rec, pk.flag_lists.idx, stream);
        }, folded));
        trace.mark("read-back 3 arrived");
        if (!force_radix && hsc.caps_wrong && !hsc.regroup && hsc.error == 0) {
            pick_ranges(s, 0u, 0, nullptr);
            if (s.n_kept)
                hipLaunchKernelGGL(k_fix_locus_rel, dim3(blocks_for(s.n_off)), dim3(TPB), 0, stream, s.blk_off, p.nb, L,
                                   m.locus_rel, pk.entry32.as<uint32_t>());
            HIP_OK(read_scalars(pk, stream, sc, nullptr, &hsc, nullptr));  // the number of ranges
        }
        const Attempt verdict = scalar_verdict(hsc, true);
        // (the host packing's uploads do not go through `stream`, and the list chain behind the read-back still
        // reads the records and offsets they replace: a hand-over this late waits for it)
        if (verdict.kind == Attempt::NeedHost) HIP_OK(hipStreamSynchronize(stream));
        STEP(verdict);
        pk.pair_bound = hsc.pair_bound;
        pk.cell_sq = s.per_cell_sq;
        pk.cell_sq_n = s.n_kept ? p.nb * p.B : 0u;
        pk.cell_sq_host.clear();
        pk.count_tile = p.caps.allow_counts && pk.pair_bound < kCountTileLimit;
        pk.cap_entries = pk.count_tile ? p.caps.entries_counts : p.caps.entries_plain;
        pk.cap_loci = pk.count_tile ? p.caps.loci_counts : p.caps.loci_plain;
        pk.num_ranges = hsc.num_ranges;
        pk.max_range_span = hsc.max_range_span;
        pk.n_wide = hsc.n_wide;
        pk.flag_lists_built = lists_launched;
        HIP_OK(hipGetLastError());
        return Attempt::stop(Attempt::Done);
    }

    Attempt run() {
        STEP(prepare_workspace());
        trace.t0 = std::chrono::steady_clock::now();
        trace.mark("begin");
        const Grouped g = group_by_read();
        if (!g.go()) return g;
        pk.used_single_entry = g.single_entry;

        STEP(ensure_outputs());
        const ReadViews v = read_views(g);
        Publish pub2{nullptr, 0ull, nullptr};  // read-back 2 rides on k_read_info on the single-entry route (n_m > 0)
        STEP(build_reads(g, v, nullptr, &pub2));
        struct SideJoin {  // every way out of this function leaves the side stream idle
            hipStream_t side;
            bool joined = false;
            ~SideJoin() { if (!joined) (void)hipStreamSynchronize(side); }
        } side_join{pk.side};

        // read-back 2: status flags, R, number of kept entries, multi-locus statistics
        Scalars hsc;
        unsigned long long totals = 0;  // reads | kept entries << 32
        trace.mark("reads built (launched)");
        HIP_OK(read_scalars(pk, stream, sc, g.n_m ? v.incl + (g.n_m - 1) : nullptr, &hsc, &totals, nullptr,
                            g.n_m && g.single_entry ? &pub2 : nullptr));
        trace.mark("read-back 2 arrived");
        const Attempt verdict = scalar_verdict(hsc, false);
        if (verdict.go() || verdict.kind == Attempt::RetryRadix || verdict.kind == Attempt::NeedHost)
            pk.id_space_hint = g.counting ? std::max<uint64_t>(hsc.id_space, 1) : 0;  // (a void attempt: the caller drops it)
        STEP(verdict);
        if (hsc.long_reads) STEP(settle_flush_cuts(g, v, &hsc, &totals));

        // (single-entry route: `totals` counts the reads and kept entries of the M entries; every S entry is a
        // read and a kept entry of its own)
        const uint32_t kept_m = (uint32_t)(totals >> 32);
        const uint32_t R = g.single_entry ? hsc.reads_total : (uint32_t)totals;
        const uint32_t n_kept = g.single_entry ? kept_m + (E - g.n_m) : kept_m;
        pk.multi_entries = hsc.multi_entries;
        pk.max_read_entries = std::max(hsc.max_read_entries, n_kept ? 1u : 0u);
        const TilePlan p = plan_tiles(num_cells, L, block_cells, geometry, allow_count_tile, n_kept, pk.multi_entries);
        if (p.B != 64 && p.B != 128) return Attempt::error("block_cells must be 64 or 128");
        // k_bin_place packs the locus into 25 bits at most, and bit 31 of a k marks an S entry
        if (!force_radix && (p.lbits + kCibBits > 32u || E >= kSingle)) return Attempt::stop(Attempt::RetryRadix);
        pk.num_cells = num_cells;
        pk.block_cells = p.B;
        pk.num_blocks = p.nb;
        pk.num_loci = L;
        pk.num_entries = n_kept;
        pk.num_reads = R;
        pk.stage_masks = p.stage_masks;

        HIP_OK(ensure(Arena::DUPF));
        HIP_OK(S[Arena::SEGS].ensure(carved<Segs>((size_t)p.n_seg, p.variant_stride)));
        const size_t nk = std::max<uint32_t>(n_kept, 1), rows = (size_t)p.nb * p.B;
        const BinRadix bin(S[Arena::BIN].p, nk, rows);
        const Stage5 s{p,
                       n_kept,
                       kept_m,
                       (size_t)p.nb * ((size_t)L + 1),
                       KeptRead(S[Arena::TMP].p, E),
                       KeptRank(S[Arena::WORK_A].p, E),
                       pk.blk_off.as<uint32_t>(),
                       v.marks.blk_cnt,
                       KeptFlags(S[Arena::VAL_A].p, E),
                       DupFlags(S[Arena::DUPF].p, L),
                       force_radix ? nullptr : EntryKC(S[Arena::ENTRY_KC].p, E).p,
                       bin,
                       reinterpret_cast<uint4 *>(BinCounting(S[Arena::BIN].p, nk, rows).m_rec),
                       bin.per_cell_sq,
                       Segs(S[Arena::SEGS].p, p.n_seg, p.variant_stride)};
        if (force_radix) HIP_OK(hipMemsetAsync(s.blk_cnt, 0, (s.n_off + 1) * 4, stream));
        HIP_OK(hipMemsetAsync(s.per_cell_sq, 0, (rows + 1) * 8, stream));
        const bool hist_first = g.single_entry && !force_radix;  // the S entries are counted before the M entries join
        if (hist_first) {
            // (the group -> cell map rides in LDS if it fits beside the tile: 2 bytes per group)
            const size_t g2p_bytes = ((size_t)in.n_groups * 2 + 15) / 16 * 16;
            const bool g2p_lds = num_cells <= 0xFFFFu && p.lds + g2p_bytes <= 49152;
            hipLaunchKernelGGL(k_bin_hist, dim3(g2p_lds ? std::min<uint32_t>(p.locus_grid, 1024) : p.locus_grid), dim3(TPB),
                               p.lds + (g2p_lds ? g2p_bytes : 0), stream, raw, p.nb, p.TL, s.entry_kc, g.m_index.chunk_mask,
                               num_cells, p.B_log2, s.blk_cnt, sc, g2p_lds ? 1u : 0u);
        }
        if (g.n_m) {
            hipLaunchKernelGGL(k_keys2, dim3(blocks_for(g.n_m)), dim3(TPB), 0, stream, g.sub, g.sval, v.incl, v.read_locus,
                               v.runs.run_rank, v.read_off, num_cells, p.B, p.lbits, force_radix ? bin.key2_a : nullptr,
                               force_radix ? bin.val2_a : nullptr, s.t_read, s.krank, s.kflags, s.entry_kc,
                               g.single_entry ? g.m_entry : nullptr, hist_first ? s.blk_cnt : nullptr, L, sc);
        }
        trace.mark("k_keys2 launched");
        STEP(force_radix ? bin_radix(s) : bin_counting(g, v, s, hist_first));
        // the locus ranges were cut for both sets of limits on the side stream (after the flush chain): pick
        HIP_OK(hipStreamWaitEvent(stream, pk.ev_join, 0));
        side_join.joined = true;
        bool lists_launched = false;
        Publish pub3{nullptr, 0ull, nullptr};
        if (force_radix)
            records_radix(v, s);
        else
            lists_launched = records_counting(s, &pub3);
        return close_attempt(s, lists_launched, force_radix ? nullptr : &pub3);
    }
};

}  // namespace

std::string pack_pileup_device(const DeviceFlatPileup &in, uint32_t num_cells, uint32_t mfl,
                               uint32_t num_threads, uint32_t block_cells,
                               StageGeometry (*geometry)(uint32_t), bool allow_count_tile,
                               hipStream_t stream, DevicePacked *out, bool *need_host) {
    *need_host = false;
    out->flag_lists_built = false;
    out->used_single_entry = false;
    out->route = DevicePacked::Route();
    if ((in.id_base16 != nullptr) == (in.id_base32 != nullptr))
        return "exactly one of id_base16 / id_base32 must be given";
    if (num_threads == 0) return "num_threads must be positive";
    if (num_cells == 0 || num_cells > 65535) return "num_cells must be in [1, 65535]";
    if (block_cells != 0 && block_cells != 64 && block_cells != 128) return "block_cells must be 0, 64 or 128";
    const uint64_t E64 = in.n_entries;
    const uint32_t L = in.n_loci;
    const size_t n_off_max = (size_t)((num_cells + 63) / 64) * ((size_t)L + 1);
    if (E64 >= (1ull << 31) || L == 0 || L >= (1u << 30) || E64 == 0 || (uint64_t)4 * num_threads > 0xFFFFFFFFull
        || n_off_max >= (1ull << 31)) {
        *need_host = out->route.asked_host = true;  // sizes this path does not cover (incl. the empty pileup)
        return std::string();
    }
    bool force_radix = false;
    if (const char *env = std::getenv("SECEDO_PACK_GROUPING")) force_radix = std::string(env) == "radix";
    // SECEDO_PACK_OVERLAP=0: the serial order -- the flagged entries' lists made by the caller from entry32
    // (pack_flag_lists) behind read-back 3, not from k_entry_records' ballots beside it
    bool overlap = true;
    if (const char *env = std::getenv("SECEDO_PACK_OVERLAP")) overlap = std::atoi(env) != 0;
    // an attempt can ask to be repeated: with the radix sorts (a group too long for the counting scheme),
    // or as it was but without assuming the previous call's sizes
    bool no_assumptions = false;
    for (int attempt = 0; attempt < 3; ++attempt) {
        if (poison_level() >= 2) {  // debugging aid: nothing may depend on what the buffers held
            if (hipStreamSynchronize(stream) != hipSuccess || (out->side && hipStreamSynchronize(out->side) != hipSuccess))
                return "poison: synchronise failed";
            DeviceArena *outputs[] = {&out->blk_off, &out->entry32, &out->mask32, &out->entry,
                                      &out->entry_read, &out->range_off, &out->read_off, &out->read_locus, &out->read_base};
            for (DeviceArena *a : outputs)
                if (a->p && hipMemset(a->p, 0xA5, a->bytes) != hipSuccess) return "poison: memset failed";
            for (DeviceArena &a : out->scratch)
                if (a.p && hipMemset(a.p, 0xA5, a.bytes) != hipSuccess) return "poison: memset failed";
        }
        ++out->route.attempts;
        out->route.radix = force_radix;
        Attempt result = PackAttempt(in, num_cells, mfl, num_threads, block_cells, geometry, allow_count_tile, force_radix,
                                     no_assumptions, overlap, stream, *out).run();
        switch (result.kind) {
            case Attempt::Error: return std::move(result.text);
            case Attempt::NeedHost: *need_host = out->route.asked_host = true; return std::string();
            case Attempt::RetryRadix: force_radix = true; break;
            case Attempt::RetryPlain:  // the sizes of the previous call did not hold: ask the device
                no_assumptions = out->route.retried_plain = true;
                out->id_space_hint = 0;
                break;
            default: return std::string();
        }
    }
    *need_host = out->route.asked_host = true;  // cannot happen: three attempts cover both requests
    return std::string();
}


size_t flag_list_scratch_bytes(uint32_t n_entries) { return FlagScratch::bytes(n_entries); }

hipError_t pack_flag_lists(const uint32_t *entry32, const uint4 *entry, uint32_t n_entries, const uint32_t *blk_off,
                           size_t n_off, void *scratch, uint32_t *grp, uint4 *rec, uint32_t *idx, hipStream_t stream) {
    const FlagScratch fs(scratch, n_entries);
    hipLaunchKernelGGL(k_pflag_count, dim3(fs.nb), dim3(TPB), 0, stream, entry32, n_entries, fs.block_sum);
    hipLaunchKernelGGL(k_flag_scan, dim3(1), dim3(TPB_SCAN), 0, stream, fs.block_sum, fs.nb, fs.block_off,
                       fs.chunk_pre + 64 * (size_t)fs.nb, static_cast<Scalars *>(nullptr));
    hipLaunchKernelGGL(k_pflag_compact, dim3(fs.nb), dim3(TPB), 0, stream, entry32, entry, n_entries, fs.block_off, rec, idx,
                       fs.chunk_pre, fs.chunk_mask);
    flag_groups(fs, blk_off, n_off, grp, stream);
    return hipGetLastError();
}

}  // namespace secedo

