// simmat_api.cpp -- the handle of the C-ABI declared in include/secedo_simmat.h: create / destroy, the pileup and
// its packing (prepare), the getters, the scale bounds, finalize and the timing and diagnostic getters.
//
// Host orchestration only: argument checks, host packing (pack_host.cpp), HBM buffers, kernel
// launches (simmat_kernels.hip). There is deliberately no CPU compute path in here: if no HIP
// device is usable the entry points fail with SECEDO_E_NO_DEVICE. The accumulation is in simmat_accumulate.cpp,
// the one-shot call and its lanes in simmat_one_shot.cpp, the locus filter in filter_api.cpp.
#include "simmat_handle.hpp"

#include <algorithm>
#include <cstdio>
#include <new>
#include <utility>

using namespace secedo::host;

namespace {

// Which pileup the handle holds, as far as the scale overrides care: sizes and the entry array. Bounds set for
// the shards of one pileup must not leak into the accumulation of another (they lower the fixed-point scale);
// packing the same arrays again (another tile edge, the next step of a loop) keeps them.
void note_pileup(secedo_simmat *h, uint32_t n_chr, uint64_t n_loci, uint64_t n_entries, const void *read_ids) {
    Fnv1a id;
    for (uint64_t v : {(uint64_t)n_chr, n_loci, n_entries, (uint64_t)reinterpret_cast<uintptr_t>(read_ids)}) id.add(v);
    h->pileup_identity = id.id();
    if (h->override_identity != h->pileup_identity) {
        if (h->pair_bound_override || h->max_shared_override) h->override_dropped = true;
        h->pair_bound_override = 0;
        h->max_shared_override = 0;
        h->override_identity = 0;
    }
}

int check_pileup_args(const secedo_simmat *h, const void *chr_locus_off, const void *locus_entry_off,
                      const void *id_base16, const void *id_base32, const void *group_id_to_pos, uint32_t n_groups) {
    if (!h) return fail(SECEDO_E_INVALID_ARG, "handle is null");
    if (!chr_locus_off || !locus_entry_off) return fail(SECEDO_E_INVALID_ARG, "null offset arrays");
    if ((id_base16 != nullptr) == (id_base32 != nullptr))
        return fail(SECEDO_E_INVALID_ARG, "exactly one of id_base16 / id_base32 must be given");
    if (!group_id_to_pos && n_groups) return fail(SECEDO_E_INVALID_ARG, "group_id_to_pos is null");
    return SECEDO_OK;
}

// ---- the steps of prepare, in the order they run

// the pileup lives in HBM only and the host packing needs it: bring it back into `store`, *v points there
struct HostPileupStore {
    std::vector<uint32_t> chr, pos, rid, g2p, idb32;
    std::vector<uint64_t> off;
    std::vector<uint16_t> idb16;
};
int fetch_pileup_to_host(const secedo::DeviceFlatPileup &d, hipStream_t s, HostPileupStore *store,
                         secedo::FlatPileupView *v) {
    SECEDO_TRY(hipStreamSynchronize(s));
    auto fetch = [](auto &to, const void *d_src, size_t n) {
        to.resize(n);
        return n ? hipMemcpy(to.data(), d_src, n * sizeof(to[0]), hipMemcpyDeviceToHost) : hipSuccess;
    };
    SECEDO_TRY(fetch(store->chr, d.chr_locus_off, (size_t)d.n_chr + 1));
    SECEDO_TRY(fetch(store->pos, d.locus_pos, d.n_loci));
    SECEDO_TRY(fetch(store->off, d.locus_entry_off, (size_t)d.n_loci + 1));
    SECEDO_TRY(fetch(store->rid, d.read_ids, d.n_entries));
    SECEDO_TRY(fetch(store->g2p, d.group_id_to_pos, d.n_groups));
    if (d.id_base16) SECEDO_TRY(fetch(store->idb16, d.id_base16, d.n_entries));
    else SECEDO_TRY(fetch(store->idb32, d.id_base32, d.n_entries));
    // (an empty vector's data() may be null, and "which of the two" is told by the pointers)
    static const uint16_t none16 = 0;
    static const uint32_t none32 = 0;
    *v = secedo::FlatPileupView{store->chr.data(), d.n_chr, store->pos.data(), store->off.data(), store->rid.data(),
                                d.id_base16 ? (store->idb16.empty() ? &none16 : store->idb16.data()) : nullptr,
                                d.id_base16 ? nullptr : (store->idb32.empty() ? &none32 : store->idb32.data()),
                                store->g2p.data(), d.n_groups};
    return SECEDO_OK;
}

// what the host packed, into the handle's arenas and geometry
int adopt_host_packing(secedo::PackedPileup &from, secedo::DevicePacked *pk) {
    SECEDO_TRY(pk->blk_off.upload(from.blk_off));
    SECEDO_TRY(pk->entry32.upload(from.entry32));
    SECEDO_TRY(pk->mask32.upload(from.mask32));
    SECEDO_TRY(pk->entry.upload(from.entry));
    SECEDO_TRY(pk->entry_read.upload(from.entry_read));
    SECEDO_TRY(pk->range_off.upload(from.range_off));
    SECEDO_TRY(pk->read_off.upload(from.read_off));
    SECEDO_TRY(pk->read_locus.upload(from.read_locus));
    SECEDO_TRY(pk->read_base.upload(from.read_base));
    pk->num_cells = from.num_cells;
    pk->block_cells = from.block_cells;
    pk->num_blocks = from.num_blocks;
    pk->num_loci = from.num_loci;
    pk->num_entries = from.num_entries;
    pk->num_reads = from.num_reads;
    pk->pair_bound = from.pair_bound;
    pk->cell_sq = nullptr;
    pk->cell_sq_n = 0;
    pk->cell_sq_host = std::move(from.cell_sq);
    pk->multi_entries = from.multi_entries;
    pk->max_read_entries = from.max_read_entries;
    pk->n_wide = from.n_wide;
    pk->flag_lists_built = false;
    pk->stage_masks = from.stage_masks;
    pk->count_tile = from.count_tile;
    pk->cap_entries = from.cap_entries;
    pk->cap_loci = from.cap_loci;
    pk->num_ranges = static_cast<uint32_t>(from.range_off.size()) - 1;
    pk->max_range_span = 0;
    for (size_t r = 0; r + 1 < from.range_off.size(); ++r)
        pk->max_range_span = std::max(pk->max_range_span, from.range_off[r + 1] - from.range_off[r]);
    return SECEDO_OK;
}

struct PrepareArgs {
    uint32_t num_cells, max_fragment_length, num_threads, block_cells;
    bool allow_count_tile;  // SECEDO_COUNT_TILE=0 forces the int64 tile (diagnostics)
    int mode;               // packing: 0 auto, 1 host, 2 device only
};

// Packs on the device (after the upload of a pileup that came as host pointers); *need_host: the host has to
int pack_on_device(secedo_simmat *h, const PrepareArgs &p, hipStream_t s, bool *need_host) {
    if (h->have_host) SECEDO_TRY(upload_flat_pileup(h->view, h->raw, &h->dview));  // raw pileup to HBM
    // the flagged entries' lists are built inside the packing where its records pass knows the flags: their buffers,
    // sized for what the packing can keep at most (an ensure in mid-pipeline would synchronise). Whether the lists
    // are wanted is known at read-back 2 only, so a pileup that ends on the masks kernel holds them for nothing: 20
    // bytes per raw entry and the scratch, 0.5 GB on C3 clustered beside its 8 GB of matrix -- released again in
    // build_flag_lists where the packed pileup stages masks, and not sized again while the handle's previous pileup
    // did (the first sparse pileup after a clustered one gets its lists from pack_flag_lists)
    h->pk.flag_lists = secedo::DevicePacked::FlagListBuffers();
    const bool was_clustered = h->pk.stage_masks && h->pk.num_entries;
    if (p.allow_count_tile && !was_clustered && h->dview.n_entries && h->dview.n_entries < (1ull << 31)) {
        const uint32_t ne = (uint32_t)h->dview.n_entries;
        const size_t n_off_max = (size_t)((p.num_cells + 63) / 64) * ((size_t)h->dview.n_loci + 1);
        SECEDO_TRY(h->flag_tmp.ensure(secedo::flag_list_scratch_bytes(ne)));
        SECEDO_TRY(h->flag_rec.ensure((size_t)ne * 16));
        SECEDO_TRY(h->flag_idx.ensure((size_t)ne * 4));
        SECEDO_TRY(h->flag_grp.ensure(std::max<size_t>(n_off_max, 1) * 4));
        h->pk.flag_lists.scratch = h->flag_tmp.p;
        h->pk.flag_lists.grp = h->flag_grp.as<uint32_t>();
        h->pk.flag_lists.rec = h->flag_rec.as<uint4>();
        h->pk.flag_lists.idx = h->flag_idx.as<uint32_t>();
    }
    const std::string err = secedo::pack_pileup_device(h->dview, p.num_cells, p.max_fragment_length, p.num_threads,
                                                       p.block_cells, &secedo::stage_geometry, p.allow_count_tile, s,
                                                       &h->pk, need_host);
    if (!err.empty()) {
        h->have_host = h->have_device = false;
        return fail(err.find("hip") == 0 ? SECEDO_E_HIP : SECEDO_E_INVALID_ARG, err);
    }
    if (*need_host && p.mode == 2) {
        h->have_host = h->have_device = false;
        return fail(SECEDO_E_LIMIT, "this pileup needs the host packing path (a read is longer than "
                                    "max_fragment_length, or a size limit of the device path)");
    }
    if (!*need_host) h->used_device_packing = 1;
    return SECEDO_OK;
}

// the exact sequential emulation on the host (reads split at flushes, any size)
int pack_on_host(secedo_simmat *h, const PrepareArgs &p, hipStream_t s) {
    HostPileupStore store;
    secedo::FlatPileupView v = h->view;
    if (!h->have_host) SECEDO_CALL(fetch_pileup_to_host(h->dview, s, &store, &v));
    secedo::PackedPileup packed;
    const std::string err = secedo::pack_pileup(v, p.num_cells, p.max_fragment_length, p.num_threads, p.block_cells,
                                                &secedo::stage_geometry, p.allow_count_tile, &packed);
    if (!err.empty()) {
        h->have_host = h->have_device = false;
        return fail(SECEDO_E_INVALID_ARG, err);
    }
    return adopt_host_packing(packed, &h->pk);
}

// upper-triangular tiles in row-major order, on the host and in HBM; kept while the number of blocks stays
int build_tile_table(secedo_simmat *h) {
    const uint32_t nb = h->pk.num_blocks;
    if (h->num_tiles == nb * (nb + 1) / 2 && h->tile_row.p) return SECEDO_OK;
    h->num_tiles = nb * (nb + 1) / 2;
    std::vector<uint16_t> trow, tcol;
    trow.reserve(h->num_tiles);
    tcol.reserve(h->num_tiles);
    for (uint32_t i = 0; i < nb; ++i) {
        for (uint32_t j = i; j < nb; ++j) {
            trow.push_back(static_cast<uint16_t>(i));
            tcol.push_back(static_cast<uint16_t>(j));
        }
    }
    SECEDO_TRY(h->tile_row.upload(trow));
    SECEDO_TRY(h->tile_col.upload(tcol));
    h->host_tile_row = trow;
    h->host_tile_col = tcol;
    return SECEDO_OK;
}

// The sparse-loci path's lists of the flagged entries, as the last step of the packing and on its stream: the
// pair kernel's epilogue and correct_tiles read them
int build_flag_lists(secedo_simmat *h, hipStream_t s) {
    const secedo::DevicePacked &pk = h->pk;
    if (!(pk.count_tile && !pk.stage_masks && pk.num_entries)) {
        if (pk.stage_masks) {  // clustered loci: no lists, and the next packing of this handle will hardly want them
            for (secedo_simmat::DevBuf *b : {&h->flag_tmp, &h->flag_rec, &h->flag_idx, &h->flag_grp}) b->release();
            h->pk.flag_lists = secedo::DevicePacked::FlagListBuffers();
        }
        return SECEDO_OK;
    }
    if (h->used_device_packing && pk.flag_lists_built) {  // the packing's records pass made them
        h->flags_ready = true;
        return SECEDO_OK;
    }
    const uint32_t ne = (uint32_t)pk.num_entries;
    const size_t n_off = (size_t)pk.num_blocks * (pk.num_loci + 1);
    SECEDO_TRY(h->flag_tmp.ensure(secedo::flag_list_scratch_bytes(ne)));
    SECEDO_TRY(h->flag_rec.ensure((size_t)ne * 16));
    SECEDO_TRY(h->flag_idx.ensure((size_t)ne * 4));
    SECEDO_TRY(h->flag_grp.ensure(std::max<size_t>(n_off, 1) * 4));
    SECEDO_TRY(secedo::pack_flag_lists(pk.entry32.as<uint32_t>(), pk.entry.as<uint4>(), ne, pk.blk_off.as<uint32_t>(),
                                       n_off, h->flag_tmp.p, h->flag_grp.as<uint32_t>(), h->flag_rec.as<uint4>(),
                                       h->flag_idx.as<uint32_t>(), s));
    h->flags_ready = true;
    return SECEDO_OK;
}

// what a diagnostic build (-DSECEDO_STAMPS) left in the counters, on stderr
int print_stamps(secedo_simmat *h) {
    const unsigned long long *counters = h->counters.as<unsigned long long>();
    const bool counts = env_set("SECEDO_STAMPS_COUNTS");
    unsigned long long st[16] = {0};
    SECEDO_TRY(hipMemcpy(st, counters, sizeof(st), hipMemcpyDeviceToHost));
    if (counts) {  // correct_tiles
        unsigned long long cf[11] = {0};
        SECEDO_TRY(hipMemcpy(cf, counters + 82, sizeof(cf), hipMemcpyDeviceToHost));
        if (cf[0])
            std::fprintf(stderr, "[stamps-correct] pair tests %llu, tail terms %llu, joint terms %llu, later-locus pairs %llu | "
                                 "per wave: pairs phase %.0f cycles (%.0f until the first q records are there), flush phase %.0f cycles, "
                                 "flagged row entries %.0f; busiest lane: %.1f q iterations, %.0f cycles until their records are there\n",
                         cf[0], cf[1], cf[2], cf[3], (double)cf[4] / (double)cf[6], (double)cf[8] / (double)cf[6],
                         (double)cf[5] / (double)cf[6], (double)cf[7] / (double)cf[6], (double)cf[10] / (double)cf[6],
                         (double)cf[9] / (double)cf[6]);
    }
    if (st[8] && counts) {  // accumulate_counts
        const double w = (double)st[8];
        std::fprintf(stderr, "[stamps-counts] sampled waves %llu | per wave cycles: total %.0f barrier-A %.0f stage+barrier-B %.0f "
                             "items(+col prefetch issue) %.0f primary groups %.0f drain %.0f | per primary batch %.0f, per drain batch %.0f "
                             "(%.2f drain batches per primary batch)\n",
                     st[8], st[7] / w, st[2] / w, st[3] / w, st[4] / w, st[5] / w, st[6] / w,
                     (double)st[5] / std::max<double>(1, (double)st[9]), (double)st[6] / std::max<double>(1, (double)st[10]),
                     (double)st[10] / std::max<double>(1, (double)st[9]));
        unsigned long long pw[64] = {0};
        SECEDO_TRY(hipMemcpy(pw, counters + 16, sizeof(pw), hipMemcpyDeviceToHost));
        const double wgs = w / 16.0;
        for (int k = 0; k < 16; ++k)
            std::fprintf(stderr, "[stamps-counts] wave %2d: barrier-A %8.0f  pairs %8.0f  items %8.0f  stage+B %8.0f\n", k,
                         pw[k * 4] / wgs, pw[k * 4 + 1] / wgs, pw[k * 4 + 2] / wgs, pw[k * 4 + 3] / wgs);
    } else if (st[8]) {
        std::fprintf(stderr, "[stamps] waves %llu batches %llu trips %llu | per wave: lifetime %.0f cyc, setup %.0f, "
                             "fill %.0f, trips %.0f | per batch: setup %.0f fill %.0f trips %.0f (%.2f trips)\n",
                     st[8], st[5], st[6], (double)st[7] / st[8], (double)st[2] / st[8], (double)st[3] / st[8],
                     (double)st[4] / st[8], (double)st[2] / st[5], (double)st[3] / st[5], (double)st[4] / st[5],
                     (double)st[6] / st[5]);
        std::fprintf(stderr, "[stamps] per wave: barrier-1 wait %.0f, staging+barrier-2 %.0f, prefetch issue %.0f\n",
                     (double)st[9] / st[8], (double)st[10] / st[8], (double)st[11] / st[8]);
        std::fprintf(stderr, "[stamps] per wave: post-trip %.0f, batch loop total %.0f\n",
                     (double)st[12] / st[8], (double)st[13] / st[8]);
        std::fprintf(stderr, "[stamps] longest wave lifetime %llu cyc; ranges %u workgroups %u\n", st[14],
                     h->pk.num_ranges, h->plan_workgroups);
        std::vector<unsigned long long> wg(std::min<uint32_t>(h->plan_workgroups, 2048u));
        SECEDO_TRY(hipMemcpy(wg.data(), counters + 16, wg.size() * 8, hipMemcpyDeviceToHost));
        std::vector<unsigned long long> det(wg.size() * 8);
        SECEDO_TRY(hipMemcpy(det.data(), counters + 16 + 2048, det.size() * 8, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < wg.size(); ++k)
            std::fprintf(stderr, "[stamps-wg] %zu %llu %llu %llu | hwid %llx ranges %llu listflush %llu endbarrier %llu slab %llu | realbegin %llu realend %llu batchloop %llu\n", k,
                         wg[k] & 0xFFFFFFFFull, (wg[k] >> 32) & 0xFFF, (wg[k] >> 44) & 0xFFF, det[k * 8], det[k * 8 + 1] / 1000,
                         det[k * 8 + 2] / 1000, det[k * 8 + 3] / 1000, det[k * 8 + 4] / 1000, det[k * 8 + 5], det[k * 8 + 6], det[k * 8 + 7] / 1000);
    }
    return SECEDO_OK;
}

}  // namespace

int secedo::host::set_pileup_view(secedo_simmat *h, const secedo::FlatPileupView &v) {
    SECEDO_CALL(check_pileup_args(h, v.chr_locus_off, v.locus_entry_off, v.id_base16, v.id_base32, v.group_id_to_pos,
                                  v.n_groups));
    h->view = v;
    h->have_host = true;
    h->have_device = false;
    h->prepared = false;
    note_pileup(h, v.n_chr, v.n_loci(), v.n_entries(), v.read_ids);
    return SECEDO_OK;
}

int secedo::host::finalize_mode(secedo_simmat *h, int mode, const int64_t *d_acc, uint32_t row_begin, uint32_t row_end,
                                double *d_out, void *stream, bool keep_max) {
    SECEDO_CALL(check_ready(h, true, d_acc && d_out));
    SECEDO_CALL(check_row_range(h, row_begin, row_end));
    SECEDO_TRY(hipSetDevice(h->device));
    SECEDO_TRY(secedo::launch_finalize(d_acc, h->tile_row.as<uint16_t>(), h->tile_col.as<uint16_t>(), h->num_tiles,
                                       h->pk.num_cells, h->pk.block_cells, h->scale_log2, mode,
                                       h->max_bits.as<unsigned long long>(), row_begin, row_end, d_out,
                                       static_cast<hipStream_t>(stream), keep_max));
    return SECEDO_OK;
}

extern "C" {

const char *secedo_simmat_last_error(void) { return g_error.c_str(); }

const char *secedo_simmat_version(void) { return "secedo-simmat-mi355x 0.1 (gfx950)"; }

int secedo_simmat_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int secedo_simmat_normalization_from_string(const char *name) {
    if (name) {
        if (!std::strcmp(name, "ADD_MIN")) return SECEDO_NORM_ADD_MIN;
        if (!std::strcmp(name, "EXPONENTIATE")) return SECEDO_NORM_EXPONENTIATE;
        if (!std::strcmp(name, "SCALE_MAX_1")) return SECEDO_NORM_SCALE_MAX_1;
    }
    return fail(SECEDO_E_INVALID_NORMALIZATION,
                std::string("Invalid normalization: ") + (name ? name : "(null)"));
}

double secedo_simmat_llr(uint32_t x_s, uint32_t x_d, double eps, double h, double theta) {
    if (x_s + x_d >= 1 && !secedo::llr_exact_mode()) return secedo::reference_llr_any(eps, h, theta, x_s, x_d, 8);
    return secedo::llr(secedo::make_llr_model(eps, h, theta), x_s, x_d);
}

double secedo_simmat_llr_closed_form(uint32_t x_s, uint32_t x_d, double eps, double h, double theta) {
    return secedo::llr(secedo::make_llr_model(eps, h, theta), x_s, x_d);
}

int secedo_simmat_create(secedo_simmat_t **handle, int device_id) {
    if (!handle) return fail(SECEDO_E_INVALID_ARG, "handle is null");
    *handle = nullptr;
    const int n = secedo_simmat_device_count();
    if (n <= 0) return no_device("the similarity-matrix path");
    if (device_id < 0 || device_id >= n) return fail(SECEDO_E_NO_DEVICE, "device id out of range");
    SECEDO_TRY(hipSetDevice(device_id));
    secedo_simmat *h = new (std::nothrow) secedo_simmat();
    if (!h) return fail(SECEDO_E_LIMIT, "out of host memory");
    h->device = device_id;
    hipError_t e = hipEventCreate(&h->ev_begin);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_end);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_mid);
    if (e != hipSuccess) {
        delete h;
        return fail(SECEDO_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
    }
    *handle = h;
    return SECEDO_OK;
}

void secedo_simmat_destroy(secedo_simmat_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ev_begin) (void)hipEventDestroy(h->ev_begin);
    if (h->ev_end) (void)hipEventDestroy(h->ev_end);
    if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
    h->uploads.destroy();
    delete h;
}

int secedo_simmat_set_pileup(secedo_simmat_t *h, const uint32_t *chr_locus_off, uint32_t n_chr,
                             const uint32_t *locus_pos, const uint64_t *locus_entry_off,
                             const uint32_t *read_ids, const uint16_t *id_base16,
                             const uint32_t *id_base32, const uint32_t *group_id_to_pos,
                             uint32_t n_groups) {
    return set_pileup_view(h, secedo::FlatPileupView{chr_locus_off, n_chr, locus_pos, locus_entry_off, read_ids,
                                                     id_base16, id_base32, group_id_to_pos, n_groups});
}

int secedo_simmat_set_pileup_device(secedo_simmat_t *h, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                                    const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                                    const uint32_t *d_read_ids, const uint16_t *d_id_base16,
                                    const uint32_t *d_id_base32, const uint32_t *d_group_id_to_pos,
                                    uint32_t n_groups, uint32_t n_loci, uint64_t n_entries) {
    SECEDO_CALL(check_pileup_args(h, d_chr_locus_off, d_locus_entry_off, d_id_base16, d_id_base32, d_group_id_to_pos,
                                  n_groups));
    h->dview = make_device_view(d_chr_locus_off, n_chr, d_locus_pos, d_locus_entry_off, d_read_ids, d_id_base16,
                                d_id_base32, d_group_id_to_pos, n_groups, n_loci, n_entries);
    h->have_device = true;
    h->have_host = false;
    h->prepared = false;
    note_pileup(h, n_chr, n_loci, n_entries, d_read_ids);
    return SECEDO_OK;
}

int secedo_simmat_set_packing(secedo_simmat_t *h, int mode) {
    if (!h) return fail(SECEDO_E_INVALID_ARG, "handle is null");
    if (mode < 0 || mode > 2) return fail(SECEDO_E_INVALID_ARG, "packing mode must be 0 (auto), 1 (host) or 2 (device)");
    h->packing_mode = mode;
    return SECEDO_OK;
}

int secedo_simmat_used_device_packing(const secedo_simmat_t *h) { return h ? h->used_device_packing : 0; }
int secedo_simmat_used_single_entry_path(const secedo_simmat_t *h) {
    return h && h->used_device_packing && h->pk.used_single_entry ? 1 : 0;
}
int secedo_simmat_packing_route(const secedo_simmat_t *h) {
    if (!h) return 0;
    const secedo::DevicePacked::Route &r = h->pk.route;
    return (int)(r.attempts & SECEDO_ROUTE_ATTEMPTS) | (r.radix ? SECEDO_ROUTE_RADIX : 0) |
           (r.retried_plain ? SECEDO_ROUTE_RETRIED_PLAIN : 0) | (r.asked_host ? SECEDO_ROUTE_ASKED_HOST : 0);
}

int secedo_simmat_prepare(secedo_simmat_t *h, uint32_t num_cells, uint32_t max_fragment_length,
                          uint32_t num_threads, uint32_t block_cells, void *stream) {
    if (!h) return fail(SECEDO_E_INVALID_ARG, "handle is null");
    if (!h->have_host && !h->have_device) return fail(SECEDO_E_STATE, "set_pileup was not called");
    if (block_cells == 0) {
        const int v = env_int("SECEDO_BLOCK_CELLS", 0);
        if (v == 64 || v == 128) block_cells = static_cast<uint32_t>(v);
    }
    PrepareArgs p{num_cells, max_fragment_length, num_threads, block_cells, env_enabled("SECEDO_COUNT_TILE"),
                  h->packing_mode};
    if (env_is("SECEDO_PACKING", "host")) p.mode = 1;
    if (env_is("SECEDO_PACKING", "device")) p.mode = 2;
    SECEDO_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    h->prepared = false;
    h->used_device_packing = 0;
    h->pk.route = secedo::DevicePacked::Route();  // (host mode: the device packing is not asked at all)
    h->num_threads = num_threads;

    bool need_host = (p.mode == 1);
    if (!need_host) SECEDO_CALL(pack_on_device(h, p, s, &need_host));
    if (need_host) SECEDO_CALL(pack_on_host(h, p, s));
    h->have_host = h->have_device = false;  // the borrow ends here

    SECEDO_CALL(build_tile_table(h));
    SECEDO_TRY(h->counters.ensure((16 + 2048 * 9) * sizeof(unsigned long long)));  // [16..): diagnostic builds
    SECEDO_TRY(h->max_bits.ensure(sizeof(unsigned long long)));
    SECEDO_TRY(hipMemsetAsync(h->counters.p, 0, 16 * sizeof(unsigned long long), s));
    h->prepared = true;
    h->timed = false;
    h->flags_ready = false;
    h->wide_known = false;
    return build_flag_lists(h, s);
}

uint32_t secedo_simmat_num_tiles(const secedo_simmat_t *h) { return h ? h->num_tiles : 0; }
uint32_t secedo_simmat_block_cells(const secedo_simmat_t *h) { return h ? h->pk.block_cells : 0; }
uint64_t secedo_simmat_acc_elems(const secedo_simmat_t *h) {
    return h ? static_cast<uint64_t>(h->num_tiles) * h->pk.block_cells * h->pk.block_cells : 0;
}
uint64_t secedo_simmat_num_entries(const secedo_simmat_t *h) { return h ? h->pk.num_entries : 0; }
uint64_t secedo_simmat_num_reads(const secedo_simmat_t *h) { return h ? h->pk.num_reads : 0; }
uint64_t secedo_simmat_num_loci(const secedo_simmat_t *h) { return h ? h->pk.num_loci : 0; }

uint64_t secedo_simmat_pair_bound(const secedo_simmat_t *h) { return h ? h->pk.pair_bound : 0; }
int secedo_simmat_scale_log2(const secedo_simmat_t *h) { return h ? h->scale_log2 : 0; }
uint32_t secedo_simmat_max_read_entries(const secedo_simmat_t *h) { return h ? h->pk.max_read_entries : 0; }
int secedo_simmat_set_scale_bounds(secedo_simmat_t *h, uint64_t pair_bound, uint32_t max_read_entries) {
    if (!h) return fail(SECEDO_E_INVALID_ARG, "handle is null");
    h->pair_bound_override = pair_bound;
    h->max_shared_override = max_read_entries;
    h->override_identity = (pair_bound || max_read_entries) ? h->pileup_identity : 0;
    h->override_dropped = false;
    return SECEDO_OK;
}
int secedo_simmat_scale_bounds_state(const secedo_simmat_t *h) {
    if (!h) return 0;
    if ((h->pair_bound_override || h->max_shared_override) && h->override_identity == h->pileup_identity) return 1;
    return h->override_dropped ? 2 : 0;
}
int secedo_simmat_set_pair_bound(secedo_simmat_t *h, uint64_t pair_bound) {
    return secedo_simmat_set_scale_bounds(h, pair_bound, h ? h->max_shared_override : 0);
}
int secedo_simmat_cell_squares(secedo_simmat_t *h, uint64_t *d_out, void *stream) {
    SECEDO_CALL(check_ready(h, false, d_out));
    SECEDO_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = h->pk.num_cells;
    SECEDO_TRY(hipMemsetAsync(d_out, 0, n * 8, s));
    if (h->pk.cell_sq && h->pk.cell_sq_n) {
        SECEDO_TRY(hipMemcpyAsync(d_out, h->pk.cell_sq, std::min<size_t>(n, h->pk.cell_sq_n) * 8, hipMemcpyDeviceToDevice, s));
    } else if (!h->pk.cell_sq_host.empty()) {
        SECEDO_TRY(hipMemcpyAsync(d_out, h->pk.cell_sq_host.data(), std::min(n, h->pk.cell_sq_host.size()) * 8,
                                  hipMemcpyHostToDevice, s));
        SECEDO_TRY(hipStreamSynchronize(s));  // the source is pageable host memory of the handle
    }
    return SECEDO_OK;
}

int secedo_simmat_zero_acc(secedo_simmat_t *h, int64_t *d_acc, void *stream) {
    SECEDO_CALL(check_ready(h, false, d_acc));
    SECEDO_TRY(hipSetDevice(h->device));
    SECEDO_TRY(hipMemsetAsync(d_acc, 0, secedo_simmat_acc_elems(h) * sizeof(int64_t),
                              static_cast<hipStream_t>(stream)));
    return SECEDO_OK;
}

int secedo_simmat_tiles_of_rows(const secedo_simmat_t *h, uint32_t row_begin, uint32_t row_end, uint32_t *tile_ids,
                                uint32_t *n_tile_ids) {
    SECEDO_CALL(check_ready(h, false, n_tile_ids));
    SECEDO_CALL(check_row_range(h, row_begin, row_end));
    uint32_t n = 0;
    if (row_begin < row_end) {
        const uint32_t B = h->pk.block_cells, b0 = row_begin / B, b1 = (row_end - 1) / B;
        for (uint32_t t = 0; t < h->num_tiles; ++t) {
            const uint32_t I = h->host_tile_row[t], J = h->host_tile_col[t];
            if ((I >= b0 && I <= b1) || (J >= b0 && J <= b1)) {
                if (tile_ids) tile_ids[n] = t;
                ++n;
            }
        }
    }
    *n_tile_ids = n;
    return SECEDO_OK;
}

int secedo_simmat_max_of_tiles(secedo_simmat_t *h, const int64_t *d_acc, const uint32_t *tile_ids, uint32_t n_tile_ids,
                               double *max_value, void *stream) {
    SECEDO_CALL(check_ready(h, true, d_acc && max_value && (tile_ids || !n_tile_ids)));
    for (uint32_t k = 0; k < n_tile_ids; ++k)
        if (tile_ids[k] >= h->num_tiles) return fail(SECEDO_E_INVALID_ARG, "tile id outside [0, num_tiles)");
    SECEDO_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf ids;
    SECEDO_TRY(ids.ensure((size_t)std::max(n_tile_ids, 1u) * 4));
    if (n_tile_ids) SECEDO_TRY(hipMemcpyAsync(ids.p, tile_ids, (size_t)n_tile_ids * 4, hipMemcpyHostToDevice, s));
    SECEDO_TRY(secedo::launch_tile_max(d_acc, h->tile_row.as<uint16_t>(), h->tile_col.as<uint16_t>(), ids.as<uint32_t>(),
                                       n_tile_ids, h->pk.block_cells, h->scale_log2, h->max_bits.as<unsigned long long>(),
                                       s));
    unsigned long long bits = 0;
    SECEDO_TRY(hipMemcpyAsync(&bits, h->max_bits.p, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    std::memcpy(max_value, &bits, 8);
    return SECEDO_OK;
}

int secedo_simmat_finalize_rows_max(secedo_simmat_t *h, int normalization, const int64_t *d_acc, uint32_t row_begin,
                                    uint32_t row_end, double max_value, double *d_out_rows, void *stream) {
    SECEDO_CALL(check_normalization(normalization));
    SECEDO_CALL(check_ready(h, true, d_acc && d_out_rows));
    SECEDO_CALL(check_row_range(h, row_begin, row_end));
    if (!(max_value >= 0.0)) return fail(SECEDO_E_INVALID_ARG, "max_value must be the (non-negative) maximum of D");
    SECEDO_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long bits;
    std::memcpy(&bits, &max_value, 8);
    SECEDO_TRY(hipMemcpyAsync(h->max_bits.p, &bits, 8, hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));  // `bits` lives on this stack frame
    SECEDO_TRY(secedo::launch_finalize(d_acc, h->tile_row.as<uint16_t>(), h->tile_col.as<uint16_t>(), h->num_tiles,
                                       h->pk.num_cells, h->pk.block_cells, h->scale_log2, normalization,
                                       h->max_bits.as<unsigned long long>(), row_begin, row_end, d_out_rows, s, true));
    return SECEDO_OK;
}

int secedo_simmat_finalize(secedo_simmat_t *h, int normalization, const int64_t *d_acc, double *d_out,
                           void *stream) {
    SECEDO_CALL(check_normalization(normalization));
    return finalize_mode(h, normalization, d_acc, 0, h ? h->pk.num_cells : 0, d_out, stream);
}

int secedo_simmat_finalize_rows(secedo_simmat_t *h, int normalization, const int64_t *d_acc, uint32_t row_begin,
                                uint32_t row_end, double *d_out_rows, void *stream) {
    SECEDO_CALL(check_normalization(normalization));
    return finalize_mode(h, normalization, d_acc, row_begin, row_end, d_out_rows, stream);
}

int secedo_simmat_finalize_raw(secedo_simmat_t *h, const int64_t *d_acc, double *d_out, void *stream) {
    return finalize_mode(h, 3, d_acc, 0, h ? h->pk.num_cells : 0, d_out, stream);
}

int secedo_simmat_last_counts(secedo_simmat_t *h, uint64_t *updates, uint64_t *read_pairs) {
    if (!h) return fail(SECEDO_E_INVALID_ARG, "handle is null");
    SECEDO_CALL(check_ready(h, false));
    SECEDO_TRY(hipSetDevice(h->device));
    SECEDO_TRY(hipDeviceSynchronize());
    unsigned long long c[2] = {0, 0};
    SECEDO_TRY(hipMemcpy(c, h->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    if (updates) *updates = c[0];
    if (read_pairs) *read_pairs = c[1];
    if (env_set("SECEDO_STAMPS_PRINT")) return print_stamps(h);  // diagnostic builds (-DSECEDO_STAMPS) only
    return SECEDO_OK;
}

int secedo_simmat_last_accumulate_ms(secedo_simmat_t *h, float *ms) {
    if (!h || !ms) return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (!h->timed) return fail(SECEDO_E_STATE, "accumulate was not called");
    SECEDO_TRY(hipSetDevice(h->device));
    SECEDO_TRY(hipEventSynchronize(h->ev_end));
    SECEDO_TRY(hipEventElapsedTime(ms, h->ev_begin, h->ev_end));
    return SECEDO_OK;
}

const char *secedo_simmat_pair_kernel(const secedo_simmat_t *h) {
    if (!h || !h->prepared) return "";
    if (h->pk.count_tile && !h->pk.stage_masks) return "accumulate_counts";
    return h->pk.stage_masks && h->pk.block_cells == 64 ? "accumulate_masks" : "accumulate_tiles";
}

int secedo_simmat_last_correction_fused(const secedo_simmat_t *h) { return h && h->last_fused ? 1 : 0; }

int secedo_simmat_last_locus_words(const secedo_simmat_t *h) { return h && h->last_locus_words ? 1 : 0; }

uint32_t secedo_simmat_last_workgroups(const secedo_simmat_t *h) { return h ? h->plan_workgroups : 0; }

int secedo_simmat_debug_flag_lists(secedo_simmat_t *h, uint64_t *n_flagged, uint32_t *grp, uint32_t *rec,
                                   uint32_t *idx) {
    if (!h || !n_flagged) return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (!h->prepared || !h->flags_ready) return fail(SECEDO_E_STATE, "the flagged entries' lists have not been built");
    SECEDO_TRY(hipSetDevice(h->device));
    SECEDO_TRY(hipDeviceSynchronize());
    const size_t n_off = (size_t)h->pk.num_blocks * (h->pk.num_loci + 1);
    uint32_t n = 0;  // (the last group offset is the end of the entries)
    if (n_off) SECEDO_TRY(hipMemcpy(&n, h->flag_grp.as<uint32_t>() + n_off - 1, 4, hipMemcpyDeviceToHost));
    *n_flagged = n;
    if (grp && n_off) SECEDO_TRY(hipMemcpy(grp, h->flag_grp.p, n_off * 4, hipMemcpyDeviceToHost));
    if (rec && n) SECEDO_TRY(hipMemcpy(rec, h->flag_rec.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (idx && n) SECEDO_TRY(hipMemcpy(idx, h->flag_idx.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SECEDO_OK;
}

int secedo_simmat_debug_ranges(secedo_simmat_t *h, uint32_t *num_ranges, uint32_t *max_range_span, uint32_t *cap_loci,
                               uint32_t *range_off) {
    if (!h || !num_ranges || !max_range_span || !cap_loci) return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (!h->prepared) return fail(SECEDO_E_STATE, "no pileup has been prepared");
    SECEDO_TRY(hipSetDevice(h->device));
    SECEDO_TRY(hipDeviceSynchronize());
    *num_ranges = h->pk.num_ranges;
    *max_range_span = h->pk.max_range_span;
    *cap_loci = h->pk.cap_loci;
    if (range_off)
        SECEDO_TRY(hipMemcpy(range_off, h->pk.range_off.p, ((size_t)h->pk.num_ranges + 1) * 4, hipMemcpyDeviceToHost));
    return SECEDO_OK;
}

int secedo_simmat_last_pair_kernel_ms(secedo_simmat_t *h, float *ms) {
    if (!h || !ms) return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (!h->timed || !h->timed_mid) return fail(SECEDO_E_STATE, "the last accumulate did not run the sparse-loci kernels");
    SECEDO_TRY(hipSetDevice(h->device));
    SECEDO_TRY(hipEventSynchronize(h->ev_mid));
    SECEDO_TRY(hipEventElapsedTime(ms, h->ev_begin, h->ev_mid));
    return SECEDO_OK;
}

}  // extern "C"
