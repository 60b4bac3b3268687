// simmat_handle.hpp -- what the host units of the product library share: the handle behind secedo_simmat_t, its
// buffer types, the environment switches, the common argument checks and the few functions one unit calls in
// another (simmat_api.cpp, simmat_accumulate.cpp, simmat_one_shot.cpp, filter_api.cpp). Internal: everything in
// here is in host_util.hpp's hidden namespace, nothing is exported.
#pragma once

#include "secedo_simmat.h"

#include "host_util.hpp"
#include "llr_table.hpp"
#include "pack_device.hpp"
#include "pack_host.hpp"
#include "simmat_kernels.hpp"

#include <cstdlib>
#include <cstring>

namespace secedo {
namespace host __attribute__((visibility("hidden"))) {

// ---- environment switches. WHEN a switch is read belongs to the caller: once per process where the call sits in
// the initialiser of a `static const`, on every call otherwise (tests and the sweep scripts rely on either).
inline int env_int(const char *name, int fallback) { const char *v = std::getenv(name); return v ? std::atoi(v) : fallback; }
inline bool env_enabled(const char *name) { return env_int(name, 1) != 0; }  // on unless set to 0
inline bool env_set(const char *name) { return std::getenv(name) != nullptr; }
inline bool env_is(const char *name, const char *value) { const char *v = std::getenv(name); return v && !std::strcmp(v, value); }

// Device bytes of exactly the size asked for (DeviceArena adds head room, host::Dev knows nothing of SECEDO_POISON)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, n ? n : 16);
        if (e == hipSuccess) bytes = n ? n : 16;
        if (e == hipSuccess && secedo::poison_level() >= 1) e = hipMemset(p, 0xA5, bytes);
        return e;
    }
    template <class T>
    hipError_t upload(const T *src, size_t n) {
        hipError_t e = ensure(n * sizeof(T));
        if (e != hipSuccess || n == 0) return e;
        return hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    template <class T>
    hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// Small host -> device uploads in the ORDER OF A STREAM (tables, workgroup plans, tile lists of accumulate): the
// bytes are copied into one of four host slots of the handle first, so that the caller's / the builder's memory
// is free at once and the copy may execute whenever the stream gets to it; a slot is taken again only after the
// copy that used it last has executed (its event), which blocks the host only when five uploads are in flight.
struct StagedUploads {
    static constexpr int kSlots = 4;
    std::vector<unsigned char> host[kSlots];
    hipEvent_t done[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool used[kSlots] = {false, false, false, false};
    int next = 0;
    hipError_t put(void *dst, const void *src, size_t bytes, hipStream_t s) {
        if (bytes == 0) return hipSuccess;
        const int k = next;
        next = (next + 1) % kSlots;
        hipError_t e = hipSuccess;
        if (done[k] && used[k] && hipEventSynchronize(done[k]) != hipSuccess) {
            // (the stream it was recorded on is gone -- destroyed streams finish their work first: a fresh event)
            (void)hipGetLastError();
            (void)hipEventDestroy(done[k]);
            done[k] = nullptr;
        }
        used[k] = false;
        if (!done[k]) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
        if (e != hipSuccess) return e;
        host[k].assign(static_cast<const unsigned char *>(src), static_cast<const unsigned char *>(src) + bytes);
        e = hipMemcpyAsync(dst, host[k].data(), bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(done[k], s);
        used[k] = (e == hipSuccess);
        return e;
    }
    // every upload so far has executed: called before the stream they were ordered on is destroyed
    void settle() {
        for (int k = 0; k < kSlots; ++k) {
            if (done[k] && used[k] && hipEventSynchronize(done[k]) != hipSuccess) (void)hipGetLastError();
            used[k] = false;
        }
    }
    void destroy() {
        for (int k = 0; k < kSlots; ++k) {
            if (done[k]) {
                if (used[k]) (void)hipEventSynchronize(done[k]);
                (void)hipEventDestroy(done[k]);
            }
            done[k] = nullptr;
            used[k] = false;
        }
    }
};

// Page-locked host memory kept between one-shot calls
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        const size_t want = n + n / 8 + 4096;  // some slack: the next sub-cluster is rarely the same size
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// ---- the raw flat pileup on the device
// (the one place a DeviceFlatPileup is filled)
inline DeviceFlatPileup make_device_view(const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                                         const uint64_t *locus_entry_off, const uint32_t *read_ids,
                                         const uint16_t *id_base16, const uint32_t *id_base32,
                                         const uint32_t *group_id_to_pos, uint32_t n_groups, uint32_t n_loci,
                                         uint64_t n_entries) {
    return DeviceFlatPileup{chr_locus_off, n_chr, locus_pos, locus_entry_off, read_ids, id_base16, id_base32,
                            group_id_to_pos, n_groups, n_loci, n_entries};
}

struct RawPileupBufs { DevBuf chr, pos, off, rid, idb, g2p; };

// host view -> HBM (synchronous copies); *out points into `b`
inline hipError_t upload_flat_pileup(const FlatPileupView &v, RawPileupBufs &b, DeviceFlatPileup *out) {
    const uint32_t L = v.n_loci();
    const uint64_t E = v.n_entries();
    hipError_t e = b.chr.upload(v.chr_locus_off, (size_t)v.n_chr + 1);
    if (e == hipSuccess) e = b.pos.upload(v.locus_pos, L);
    if (e == hipSuccess) e = b.off.upload(v.locus_entry_off, (size_t)L + 1);
    if (e == hipSuccess) e = b.rid.upload(v.read_ids, E);
    if (e == hipSuccess) e = v.id_base16 ? b.idb.upload(v.id_base16, E) : b.idb.upload(v.id_base32, E);
    if (e == hipSuccess) e = b.g2p.upload(v.group_id_to_pos, v.n_groups);
    if (e != hipSuccess) return e;
    *out = make_device_view(b.chr.as<uint32_t>(), v.n_chr, b.pos.as<uint32_t>(), b.off.as<uint64_t>(),
                            b.rid.as<uint32_t>(), v.id_base16 ? b.idb.as<uint16_t>() : nullptr,
                            v.id_base16 ? nullptr : b.idb.as<uint32_t>(), b.g2p.as<uint32_t>(), v.n_groups, L, E);
    return hipSuccess;
}

// FNV-1a over 64-bit words; id() is never 0, which the handle keeps for "none"
struct Fnv1a {
    uint64_t state = 0xcbf29ce484222325ull;
    void add(uint64_t v) { state = (state ^ v) * 0x100000001b3ull; }
    uint64_t id() const { return state | 1ull; }
};

}  // namespace host
}  // namespace secedo

struct secedo_simmat {
    int device = 0;
    // the pileup handed to set_pileup / set_pileup_device (borrowed until prepare returns)
    secedo::FlatPileupView view;         // host pointers
    secedo::DeviceFlatPileup dview;      // device pointers
    bool have_host = false, have_device = false;
    bool prepared = false;
    int packing_mode = 0;                // 0 auto (device, host when required), 1 host, 2 device only
    uint32_t num_threads = 1;            // of the last prepare (the reference's parameter; bounds helper threads)
    int used_device_packing = 0;

    using DevBuf = secedo::host::DevBuf;
    secedo::host::RawPileupBufs raw;     // raw pileup uploaded by prepare() when it came as host pointers

    // the packed pileup in HBM + geometry
    secedo::DevicePacked pk;
    uint32_t num_tiles = 0;
    DevBuf tile_row, tile_col, lut, counters, max_bits, slow_args, slab, plan_wg_tile, plan_wg_begin;
    uint32_t plan_tile_begin = 0xFFFFFFFFu, plan_tile_end = 0, plan_ranges = 0, plan_blocks = 0, plan_workgroups = 0;
    DevBuf flag_tmp, flag_grp, flag_rec, flag_idx;            // sparse-loci path: the flagged entries, compact
    bool flags_ready = false;                                 // ... of the current packed pileup
    bool wide_known = false;                                  // clustered loci: the reads that reach beyond their windows ...
    uint32_t n_wide = 0;                                      // ... their entries, listed per cell block
    DevBuf wide_tab, wide_list;
    DevBuf mk_words;                                          // ... the entries' words for accumulate_masks (y | xcol | xrow)
    DevBuf own_acc, own_out;  // used by the one-shot entry point only
    DevBuf tile_ids;          // tile list of accumulate_list / max_of_tiles
    std::vector<uint16_t> host_tile_row, host_tile_col;
    secedo::host::StagedUploads uploads;  // tables, plans and tile lists of accumulate, in the order of its stream
    // read pairs that share more than 128 loci: noted by the kernels, evaluated as the reference does on the host
    DevBuf beyond_list, beyond_count, beyond_index, beyond_value;
    uint64_t plan_list_hash = 0;  // 0: the cached workgroup plan belongs to a contiguous tile range

    // LLR table of the last accumulate()
    bool have_model = false, have_lut = false, have_slow = false;
    double lut_eps = 0, lut_h = 0, lut_theta = 0;
    int scale_log2 = 44;
    int scale_wanted = 44;               // llr_scale_for(table, scale_for_bound, scale_for_reach)
    uint64_t scale_for_bound = ~0ull;
    uint32_t scale_for_reach = ~0u;
    // secedo_simmat_set_pair_bound / set_scale_bounds: the bounds of everything that is summed into one
    // accumulator (shards on several ranks); they belong to the pileup that was set when they were given
    uint64_t pair_bound_override = 0;
    uint32_t max_shared_override = 0;
    uint64_t pileup_identity = 0, override_identity = 0;
    bool override_dropped = false;  // bounds were in force and another pileup took them away (scale_bounds_state 2)
    secedo::LlrModel model;
    secedo::LlrTable table;
    secedo::SlowPathArgs slow_host;

    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_mid = nullptr;
    bool timed_mid = false;
    bool timed = false;
    bool last_fused = false;  // the last accumulate corrected its tiles in accumulate_counts' epilogue
    bool last_locus_words = false;  // ... ran accumulate_counts' instance with a staged word per locus
};

namespace secedo {
namespace host __attribute__((visibility("hidden"))) {

// ---- the checks that open most entry points
inline int check_normalization(int normalization) {
    if (normalization < 0 || normalization > 2)
        return fail(SECEDO_E_INVALID_NORMALIZATION, "Invalid normalization: " + std::to_string(normalization));
    return SECEDO_OK;
}

// `args_ok`: the entry point's other pointers are there. need_table: an accumulate has set up the table and scale.
inline int check_ready(const secedo_simmat *h, bool need_table, bool args_ok = true) {
    if (!h || !args_ok) return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (!h->prepared) return fail(SECEDO_E_STATE, "prepare was not called");
    if (need_table && !h->have_lut) return fail(SECEDO_E_STATE, "accumulate was not called");
    return SECEDO_OK;
}

inline int check_row_range(const secedo_simmat *h, uint32_t row_begin, uint32_t row_end) {
    if (row_begin > row_end || row_end > h->pk.num_cells) return fail(SECEDO_E_INVALID_ARG, "row range outside the matrix");
    return SECEDO_OK;
}

inline int no_device(const char *what) {
    return fail(SECEDO_E_NO_DEVICE, std::string("no HIP device is visible: ") + what + " has no CPU fallback");
}

// the pileup this handle packs next (simmat_api.cpp; the one-shot call has it as a view already)
int set_pileup_view(secedo_simmat *h, const FlatPileupView &view);

// normalisation `mode` (3: the raw doubles) of rows [row_begin, row_end); keep_max: max_bits holds the maximum already
int finalize_mode(secedo_simmat *h, int mode, const int64_t *d_acc, uint32_t row_begin, uint32_t row_end,
                  double *d_out, void *stream, bool keep_max = false);  // simmat_api.cpp

// ---- simmat_one_shot.cpp
constexpr int kMaxLanes = 16;
// d_src (device) -> dst (pageable host memory) through page-locked ring `ring` with `threads` copying threads
hipError_t download_pipelined(const void *d_src, void *dst, size_t bytes, unsigned threads, int ring = 0);

}  // namespace host
}  // namespace secedo
