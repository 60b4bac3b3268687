// pack_device.hpp -- device-side read assembly, flush schedule and tile packing (gfx950).
//
// Same result as pack_host.cpp (see its header for the reference semantics) but computed on the
// GPU from the raw flat pileup resident in HBM. Reads that outlive max_fragment_length are cut where
// a flush erases them (the cuts and the flush chain are iterated to their fixed point). When a size
// limit of this path is exceeded (positions within max_fragment_length of 2^32, 2^31 entries, an
// empty pileup) or that iteration does not settle, `need_host` is set and the caller packs on the host.
#pragma once

#include "pack_host.hpp"
#include "pack_workspace.hpp"

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>
#include <string>
#include <vector>

namespace secedo {

// Raw flat pileup, device pointers (layout of include/secedo_simmat.h)
struct DeviceFlatPileup {
    const uint32_t *chr_locus_off = nullptr;
    uint32_t n_chr = 0;
    const uint32_t *locus_pos = nullptr;
    const uint64_t *locus_entry_off = nullptr;
    const uint32_t *read_ids = nullptr;
    const uint16_t *id_base16 = nullptr;
    const uint32_t *id_base32 = nullptr;
    const uint32_t *group_id_to_pos = nullptr;
    uint32_t n_groups = 0;
    uint32_t n_loci = 0;
    uint64_t n_entries = 0;
};

// Growable device allocation owned by the caller (the handle of simmat_handle.hpp)
int poison_level();  // SECEDO_POISON, a debugging aid (pack_device.hip)

struct DeviceArena {
    void *p = nullptr;
    size_t bytes = 0;
    ~DeviceArena();
    hipError_t ensure(size_t n);
    template <class T>
    __attribute__((visibility("hidden"))) hipError_t upload(const std::vector<T> &v) {  // synchronous
        hipError_t e = ensure(v.size() * sizeof(T));
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// The packed pileup in HBM: the arrays of PackedPileup, device resident
struct DevicePacked {
    DeviceArena blk_off, entry32, mask32, entry, entry_read, range_off, read_off, read_locus, read_base;
    DeviceArena scratch[Arena::kCount];  // temporaries (pack_workspace.hpp), kept between calls to avoid re-allocation
    uint32_t num_cells = 0, block_cells = 0, num_blocks = 0, num_loci = 0, num_ranges = 0;
    uint64_t num_entries = 0, num_reads = 0, pair_bound = 0, multi_entries = 0;
    uint32_t max_read_entries = 0;  // kept entries of the longest read (before flush splits: an upper bound)
    uint32_t n_wide = 0;            // kept entries whose read reaches beyond their 8-locus windows (C_WIDE in entry32)
    // per matrix row: sum over loci of (kept entries of the row at the locus)^2 -- pair_bound is its maximum.
    // Device packing: a pointer into the packing's scratch, valid until the next packing of this handle;
    // host packing: cell_sq_host. secedo_simmat_cell_squares() hands it out (shards that are added up
    // sum these vectors to get the exact bound of the union).
    const unsigned long long *cell_sq = nullptr;
    uint32_t cell_sq_n = 0;
    std::vector<uint64_t> cell_sq_host;
    bool stage_masks = false;
    bool count_tile = false;
    uint32_t cap_entries = 0, cap_loci = 0;
    // loci of the longest locus range (unknown: as long as cap_loci allows). An attempt that ends early leaves
    // the previous call's value: it only picks accumulate_counts' instance, which tests every range's span against
    // its own capacity before it stages it (a range too long for it is paired from HBM), so a stale value costs
    // speed, never results
    uint32_t max_range_span = 0xFFFFFFFFu;
    uint64_t id_space_hint = 0;  // size of the read-id space of the previous call (0: unknown): saves a read-back
    // the single-entry fast path pays when most reads have one entry: a call that finds more than half of the
    // entries in multi-entry reads finishes without it, and the handle's next calls do not try (every 16th does)
    bool split_pays = true;
    uint32_t calls_without_split = 0;
    // ... and whether the packing that has just returned took it to the end (secedo_simmat_used_single_entry_path)
    bool used_single_entry = false;
    // What the packing that has just returned decided (secedo_simmat_packing_route): the attempts it ran, whether
    // the last of them was made with the radix sorts (SECEDO_PACK_GROUPING=radix, or behind a RetryRadix), whether
    // one was repeated without the previous call's sizes (RetryPlain), and whether it asked for the host -- by a
    // size limit before any attempt, or by an attempt's verdict. pack_pileup_device alone writes it.
    struct Route {
        uint32_t attempts = 0;
        bool radix = false, retried_plain = false, asked_host = false;
    } route;
    // side stream for the branch of the pipeline nothing else waits for until the final gather
    // (completed counts + flush chain); created on first use
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_offsets = nullptr, ev_flush = nullptr;
    // The flagged entries' lists (see pack_flag_lists) in the caller's buffers. Where the packing's own records pass
    // has the flags in registers (counting route, count tile allowed, no staged masks) it builds the lists itself,
    // behind the publishing kernel of its last read-back and in front of the host's wait for it, and says so in
    // flag_lists_built; everywhere else the
    // caller builds them with pack_flag_lists. The caller sizes the buffers for the RAW pileup's entries and the
    // worst-case number of group offsets before the call (growing one in mid-pipeline would synchronise):
    // scratch flag_list_scratch_bytes(n_entries), rec 16 and idx 4 bytes per entry, grp 4 bytes per offset of
    // ceil(num_cells / 64) blocks. scratch == nullptr: the packing leaves the lists to the caller.
    struct FlagListBuffers {
        void *scratch = nullptr;
        uint32_t *grp = nullptr;
        uint4 *rec = nullptr;
        uint32_t *idx = nullptr;
    } flag_lists;
    bool flag_lists_built = false;  // ... of the packing that has just returned
    // pinned host words the packing's scalar read-backs arrive in (polled; see read_scalars)
    void *mailbox = nullptr;
    unsigned long long mailbox_seq = 0;
    bool mailbox_failed = false;
    DevicePacked() = default;
    DevicePacked(const DevicePacked &) = delete;
    DevicePacked &operator=(const DevicePacked &) = delete;
    ~DevicePacked();
};

// Returns "" on success. On success with *need_host == true nothing usable was produced and the
// caller must fall back to pack_pileup() on the host. Synchronises `stream` a few times (scalar
// read-backs).
std::string pack_pileup_device(const DeviceFlatPileup &in, uint32_t num_cells,
                               uint32_t max_fragment_length, uint32_t num_threads,
                               uint32_t block_cells, StageGeometry (*geometry)(uint32_t),
                               bool allow_count_tile, hipStream_t stream, DevicePacked *out,
                               bool *need_host);

// The flagged entries of a packed pileup (kC_Tail | kC_Multi in entry32), compacted in packed-entry order -- which
// is (cell block, locus) order -- for the correction of the sparse-loci pair kernel: grp[n_off] = flagged entries
// before each group offset blk_off[] (the last one is the end of the entries: grp[n_off - 1] is their number),
// rec[] / idx[] = the flagged entries' records and indices (room for n_entries each). scratch:
// flag_list_scratch_bytes(n_entries). Four kernels on `stream`, nothing read back. (For the packings that did not
// build the lists themselves, DevicePacked::flag_lists_built: host packing, the radix route, staged masks decided
// otherwise.)
size_t flag_list_scratch_bytes(uint32_t n_entries);
hipError_t pack_flag_lists(const uint32_t *entry32, const uint4 *entry, uint32_t n_entries, const uint32_t *blk_off,
                           size_t n_off, void *scratch, uint32_t *grp, uint4 *rec, uint32_t *idx, hipStream_t stream);

}  // namespace secedo
