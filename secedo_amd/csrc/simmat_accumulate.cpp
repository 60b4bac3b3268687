// simmat_accumulate.cpp -- the accumulation of the C-ABI in include/secedo_simmat.h: the workgroup plan, the LLR
// table and the slow-path arguments a launch needs, the launch itself and the four entry points on top of it
// (accumulate / assign, each over a tile range or a tile list), and assign_finalize.
//
// Everything here is ordered on the caller's stream: the steps of accumulate_impl run in the order they stand in,
// and so do the statements inside each.
#include "simmat_handle.hpp"

#include <algorithm>
#include <cmath>
#include <queue>
#include <utility>

using namespace secedo::host;

namespace {

// capacity of the list of read pairs beyond the table per launch (16 bytes each; allocated only for a pileup with a
// read of more than 128 kept entries)
constexpr uint32_t kBeyondCap = 1u << 20;

// The tiles of a launch: [begin, end) when list == nullptr, else the `end` tiles of `list` (global indices, begin 0)
struct TileSet {
    uint32_t begin, end;
    const uint32_t *list;
    uint64_t hash;  // of the list: key of the cached workgroup plan (0: a contiguous range)
    uint32_t size() const { return end - begin; }
};

int check_tiles(const secedo_simmat *h, TileSet *t) {
    if (!t->list) {
        if (t->begin > t->end || t->end > h->num_tiles) return fail(SECEDO_E_INVALID_ARG, "tile range outside [0, num_tiles]");
        return SECEDO_OK;
    }
    Fnv1a hash;
    for (uint32_t k = 0; k < t->end; ++k) {
        if (t->list[k] >= h->num_tiles) return fail(SECEDO_E_INVALID_ARG, "tile id outside [0, num_tiles)");
        hash.add(t->list[k]);
    }
    t->hash = hash.id();
    return SECEDO_OK;
}

// Workgroups: every tile is cut into chunks of locus ranges so that the launch fills the 256 CUs
// in whole rounds of about equally loaded workgroups (a diagonal tile holds half the pairs of an
// off-diagonal one and gets half the chunks). Cached per tile range.
int plan_workgroups(secedo_simmat *h, const TileSet &t, hipStream_t s) {
    const uint32_t n_tiles = t.size();
    if (h->plan_tile_begin == t.begin && h->plan_tile_end == t.end && h->plan_ranges == h->pk.num_ranges
        && h->plan_blocks == h->pk.num_blocks && h->plan_list_hash == t.hash)
        return SECEDO_OK;
    // workgroups resident per CU (LDS-limited): 1 (128-cell tiles), 2 (64-cell tiles with staged masks,
    // 512 threads), 4 (the other 64-cell variants)
    // (the 64-cell count tile runs accumulate_counts with 512 threads and 59 KiB of LDS: two per CU)
    const uint32_t wgs_per_round = h->pk.block_cells == 128 ? 256u : (h->pk.stage_masks || h->pk.count_tile) ? 512u : 1024u;
    const uint32_t rounds = std::max(1, env_int("SECEDO_ROUNDS", 1));
    // weight of a tile = the time it takes: per row-side entry a fixed part (the batch set-up) and a
    // part per column entry of the same locus (the pairs; half of them in a diagonal tile). Fitted to
    // the per-workgroup times on C2: the fixed part is worth 5.7 pairs.
    const uint32_t Bc = h->pk.block_cells;
    auto cells_of = [&](uint32_t blk) { return (double)std::min(Bc, h->pk.num_cells - blk * Bc); };
    const double per_cell_locus = h->pk.num_loci ? (double)h->pk.num_entries / h->pk.num_cells / h->pk.num_loci : 0.0;
    std::vector<double> weight(n_tiles);
    double total_weight = 0;
    for (uint32_t k = 0; k < n_tiles; ++k) {
        const uint32_t tile = t.list ? t.list[k] : t.begin + k;
        const uint32_t I = h->host_tile_row[tile], J = h->host_tile_col[tile];
        const double depth = per_cell_locus * cells_of(J) * (I == J ? 0.5 : 1.0);  // column entries per locus
        weight[k] = cells_of(I) * (5.7 + depth);
        total_weight += weight[k];
    }
    // whole rounds of workgroups, shared out so that the slowest chunk is as fast as possible: every
    // tile starts with one chunk and the next one always goes to the tile whose chunks are heaviest
    const uint64_t slots = static_cast<uint64_t>(wgs_per_round) * std::max<uint64_t>(rounds, (n_tiles + wgs_per_round - 1) / wgs_per_round);
    const uint32_t max_chunks = std::max(1u, h->pk.num_ranges);
    std::vector<uint32_t> chunks(n_tiles, 1u);
    if (total_weight > 0 && n_tiles < slots && n_tiles <= 2 * wgs_per_round) {  // more tiles: one workgroup each
        std::priority_queue<std::pair<double, uint32_t>> heaviest;  // (weight per chunk, tile)
        for (uint32_t k = 0; k < n_tiles; ++k) heaviest.push({weight[k], k});
        for (uint64_t given = n_tiles; given < slots && !heaviest.empty();) {
            const uint32_t k = heaviest.top().second;
            heaviest.pop();
            if (chunks[k] >= max_chunks) continue;  // one range per chunk at least
            ++chunks[k];
            ++given;
            heaviest.push({weight[k] / chunks[k], k});
        }
    }
    std::vector<uint32_t> wg_begin(n_tiles + 1, 0);
    std::vector<uint32_t> wg_tile;
    for (uint32_t k = 0; k < n_tiles; ++k) {
        wg_begin[k + 1] = wg_begin[k] + chunks[k];
        for (uint32_t c = 0; c < chunks[k]; ++c) wg_tile.push_back(k);
    }
    // (a larger plan than any before: the buffers grow, and hipFree waits for the device; otherwise the new plan
    // follows the launches that read the old one in stream order)
    SECEDO_TRY(h->plan_wg_tile.ensure(wg_tile.size() * 4));
    SECEDO_TRY(h->plan_wg_begin.ensure(wg_begin.size() * 4));
    SECEDO_TRY(h->uploads.put(h->plan_wg_tile.p, wg_tile.data(), wg_tile.size() * 4, s));
    SECEDO_TRY(h->uploads.put(h->plan_wg_begin.p, wg_begin.data(), wg_begin.size() * 4, s));
    h->plan_workgroups = wg_begin[n_tiles];
    h->plan_tile_begin = t.begin;
    h->plan_tile_end = t.end;
    h->plan_list_hash = t.hash;
    h->plan_ranges = h->pk.num_ranges;
    h->plan_blocks = h->pk.num_blocks;
    return SECEDO_OK;
}

// The read pairs of a launch that share more than 128 loci, as the kernels noted them: the call waits for the launch
// here (only a pileup with a read of more than 128 kept entries comes this way), evaluates the distinct (x_s, x_d) as
// the reference does and adds the terms
int add_beyond_terms(secedo_simmat *h, double eps, double hr, double theta, int64_t *d_acc, hipStream_t s) {
    uint32_t n_noted = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_noted, h->beyond_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (n_noted > kBeyondCap)
        return fail(SECEDO_E_LIMIT, std::to_string(n_noted) + " read pairs of this launch share more than 128 loci (at most "
                                    + std::to_string(kBeyondCap) + " per launch: accumulate fewer tiles at a time, or set "
                                    "SECEDO_LLR_EXACT=1 for the formula in exact arithmetic)");
    if (!n_noted) return SECEDO_OK;
    std::vector<uint32_t> noted((size_t)n_noted * 4);
    SECEDO_TRY(hipMemcpy(noted.data(), h->beyond_list.p, noted.size() * 4, hipMemcpyDeviceToHost));
    const uint32_t Bc = h->pk.block_cells, nb = h->pk.num_blocks;
    std::vector<unsigned long long> index(n_noted);
    std::vector<long long> value(n_noted);
    for (uint32_t k = 0; k < n_noted; ++k) {
        uint32_t ca = noted[(size_t)k * 4], cb = noted[(size_t)k * 4 + 1];
        const uint32_t xs = noted[(size_t)k * 4 + 2], xd = noted[(size_t)k * 4 + 3];
        if (ca / Bc > cb / Bc) std::swap(ca, cb);  // the tile's row block is the smaller one
        const uint32_t I = ca / Bc, J = cb / Bc;
        const uint64_t tile = (uint64_t)I * nb - (uint64_t)I * (I - 1) / 2 + (J - I);  // row-major upper triangle
        if (ca >= h->pk.num_cells || cb >= h->pk.num_cells || tile >= h->num_tiles || h->host_tile_row[tile] != I
            || h->host_tile_col[tile] != J)
            return fail(SECEDO_E_STATE, "a noted read pair lies outside the matrix");
        const double d = secedo::reference_llr_any(eps, hr, theta, xs, xd, std::max(1u, h->num_threads));
        if (!std::isfinite(d) || std::fabs(std::ldexp(d, h->scale_log2)) >= 0x1p62)
            return fail(SECEDO_E_INVALID_ARG, "a read pair sharing " + std::to_string(xs + xd) + " loci has a non-finite "
                                              "log-likelihood ratio in the reference's arithmetic (it would write "
                                              "inf / NaN into the matrix); SECEDO_LLR_EXACT=1 selects the exact formula");
        index[k] = tile * Bc * Bc + (uint64_t)(ca % Bc) * Bc + (cb % Bc);
        value[k] = std::llround(std::ldexp(d, h->scale_log2));
    }
    SECEDO_TRY(h->beyond_index.ensure((size_t)n_noted * 8));
    SECEDO_TRY(h->beyond_value.ensure((size_t)n_noted * 8));
    SECEDO_TRY(hipMemcpyAsync(h->beyond_index.p, index.data(), (size_t)n_noted * 8, hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(h->beyond_value.p, value.data(), (size_t)n_noted * 8, hipMemcpyHostToDevice, s));
    SECEDO_TRY(secedo::launch_add_terms(d_acc, h->beyond_index.as<unsigned long long>(), h->beyond_value.as<long long>(),
                                        n_noted, s));
    SECEDO_TRY(hipStreamSynchronize(s));  // (the sources are this frame's vectors)
    return SECEDO_OK;
}

// ---- the steps of accumulate_impl, in the order they run

// LLR table: the doubles depend on the rates only, the fixed-point scale on the pileup's pair
// bound; upload (synchronously, it is rare) only what changed since the last call
int refresh_llr_table(secedo_simmat *h, double eps, double hr, double theta, uint32_t reach, hipStream_t s) {
    if (!h->have_model || h->lut_eps != eps || h->lut_h != hr || h->lut_theta != theta) {
        h->table = secedo::make_llr_table(eps, hr, theta, h->pk.pair_bound);
        h->lut_eps = eps;
        h->lut_h = hr;
        h->lut_theta = theta;
        h->have_model = true;
        h->have_lut = false;
    }
    // the entries this pileup can reach (no read pair shares more loci than its shorter read has) as the
    // reference evaluates them, wrapping binomial products included (llr_table.hpp)
    if (h->table.ref_upto < std::min(reach, secedo::kLlrRefMax) && !secedo::llr_exact_mode())
        h->have_lut = false;
    if (!secedo::extend_reference(&h->table, reach, std::max(1u, h->num_threads)))
        return fail(SECEDO_E_INVALID_ARG, "these rates give a non-finite log-likelihood ratio (log of 0: the reference "
                                          "would write inf / NaN into the matrix)");
    // the fixed-point scale follows the pair bound of everything that is summed into one accumulator:
    // this pileup's own bound, or the one the caller set for all the shards that will be added up
    const uint64_t bound = std::max(h->pair_bound_override, h->pk.pair_bound);
    // (the bound is a pass over the whole table: kept per table, pair bound and reach)
    if (!h->have_lut || bound != h->scale_for_bound || reach != h->scale_for_reach) {
        h->scale_wanted = secedo::llr_scale_for(h->table, bound, reach);
        h->scale_for_bound = bound;
        h->scale_for_reach = reach;
    }
    const int want_scale = h->scale_wanted;
    if (!h->have_lut || want_scale != h->scale_log2) {
        secedo::requantize(&h->table, want_scale);
        SECEDO_TRY(h->lut.ensure(h->table.fixed.size() * sizeof(int64_t)));
        // (in the order of the caller's stream, as every upload of accumulate: a launch still running on a
        // non-blocking stream reads the tables and the workgroup plan of ITS call -- a plain hipMemcpy runs on the
        // null stream, which such streams do not wait for; the host sources stay alive in the handle)
        SECEDO_TRY(h->uploads.put(h->lut.p, h->table.fixed.data(), h->table.fixed.size() * sizeof(int64_t), s));
        h->scale_log2 = want_scale;
        h->model = h->table.model;
        h->have_lut = true;
    }
    return SECEDO_OK;
}

// What the kernels' slow path reads, uploaded when it changed. *beyond: this launch notes the read pairs that
// share more than 128 loci.
int refresh_slow_path_args(secedo_simmat *h, uint32_t reach, hipStream_t s, bool *beyond) {
    secedo::SlowPathArgs sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.entry = h->pk.entry.as<uint4>();
    sp.entry_read = h->pk.entry_read.as<uint32_t>();
    sp.read_off = h->pk.read_off.as<uint32_t>();
    sp.read_locus = h->pk.read_locus.as<uint32_t>();
    sp.read_base = h->pk.read_base.as<uint8_t>();
    sp.lut = h->lut.as<long long>();
    const secedo::LlrModel &m = h->table.model;
    sp.model = secedo::LlrModelDev{m.ln_u1, m.ln_v1, m.ln_u2, m.ln_v2, m.ln_w1, m.ln_z1, m.ln_w2, m.ln_z2};
    sp.scale_log2 = h->scale_log2;
    // Read pairs that share more than 128 loci (possible when a read has more kept entries than that): what the
    // reference returns there is the value of its wrapped integer sums -- O(x_s^2 x_d^2) terms per entry, nothing
    // for a table. The kernels note such pairs instead of adding their joint term, and after the launch the
    // host evaluates the few distinct (x_s, x_d) as the reference does and adds them (add_beyond_terms).
    // SECEDO_LLR_EXACT=1: the closed form on the device, nothing noted.
    *beyond = reach > secedo::kLlrRefMax && !secedo::llr_exact_mode();
    if (*beyond) {
        SECEDO_TRY(h->beyond_list.ensure((size_t)kBeyondCap * sizeof(uint4)));
        SECEDO_TRY(h->beyond_count.ensure(sizeof(uint32_t)));
        sp.beyond_list = h->beyond_list.as<uint4>();
        sp.beyond_count = h->beyond_count.as<uint32_t>();
        sp.beyond_cap = kBeyondCap;
    }
    if (!h->have_slow || std::memcmp(&sp, &h->slow_host, sizeof(sp)) != 0) {
        SECEDO_TRY(h->slow_args.ensure(sizeof(sp)));
        h->slow_host = sp;
        SECEDO_TRY(h->uploads.put(h->slow_args.p, &sp, sizeof(sp), s));
        h->have_slow = true;
    }
    return SECEDO_OK;
}

// nothing to add (a rank whose shard is empty): the table and the scale are all finalize needs
int accumulate_nothing(secedo_simmat *h, const TileSet &t, int64_t *d_acc, bool overwrite, hipStream_t s) {
    if (overwrite) {  // ... and the tiles of the launch are zero
        const size_t b2 = (size_t)h->pk.block_cells * h->pk.block_cells;
        if (t.list) {
            for (uint32_t k = 0; k < t.end; ++k)
                SECEDO_TRY(hipMemsetAsync(d_acc + (size_t)t.list[k] * b2, 0, b2 * sizeof(int64_t), s));
        } else {
            SECEDO_TRY(hipMemsetAsync(d_acc + (size_t)t.begin * b2, 0, (size_t)t.size() * b2 * sizeof(int64_t), s));
        }
    }
    SECEDO_TRY(hipMemsetAsync(h->counters.p, 0, 96 * sizeof(unsigned long long), s));
    SECEDO_TRY(hipEventRecord(h->ev_begin, s));
    SECEDO_TRY(hipEventRecord(h->ev_end, s));
    h->timed = true;
    h->timed_mid = false;  // no pair kernel ran: last_pair_kernel_ms has nothing to report
    return SECEDO_OK;
}

// the kernel arguments that are pointers and sizes of the handle (the plan's follow plan_workgroups)
secedo::AccumulateArgs base_args(const secedo_simmat *h, const TileSet &t, int64_t *d_acc, bool overwrite) {
    secedo::AccumulateArgs a;
    a.blk_off = h->pk.blk_off.as<uint32_t>();
    a.stride = h->pk.num_loci + 1;
    a.entry32 = h->pk.entry32.as<uint32_t>();
    a.mask32 = h->pk.mask32.as<uint32_t>();
    a.entry = h->pk.entry.as<uint4>();
    a.range_off = h->pk.range_off.as<uint32_t>();
    a.num_ranges = h->pk.num_ranges;
    a.tile_row = h->tile_row.as<uint16_t>();
    a.tile_col = h->tile_col.as<uint16_t>();
    a.tile_begin = t.begin;
    a.tile_ids = nullptr;
    a.n_tiles = t.size();
    a.debug = static_cast<uint32_t>(env_int("SECEDO_DEBUG_ABLATE", 0));
    a.lut = h->lut.as<long long>();
    a.slow = h->slow_args.as<secedo::SlowPathArgs>();
    a.acc = d_acc;
    a.overwrite = overwrite;
    a.counters = h->counters.as<unsigned long long>();
    return a;
}

// accumulate_masks pairs from the 8-locus windows alone; the entries of reads that reach beyond them are
// listed per cell block once per prepare for its second kernel
int prepare_masks_lists(secedo_simmat *h, hipStream_t s, secedo::AccumulateArgs *a) {
    const size_t ne = (size_t)h->pk.num_entries;
    if (!h->wide_known) {
        // how many there are came with the packing's last read-back (DevicePacked::n_wide): count per block, scan
        // and fill are enqueued behind each other, nothing waits for the device here
        const uint32_t nb = h->pk.num_blocks;
        h->n_wide = h->pk.n_wide;
        if (h->n_wide) {
            SECEDO_TRY(h->wide_tab.ensure(((size_t)3 * nb + 2) * 4));
            uint32_t *cnt = h->wide_tab.as<uint32_t>(), *off = cnt + nb, *cur = off + nb + 1;
            SECEDO_TRY(secedo::wide_count(a->entry32, a->blk_off, a->stride, nb, cnt, off, cur, s));
            SECEDO_TRY(h->wide_list.ensure((size_t)h->n_wide * 4));
            SECEDO_TRY(secedo::wide_fill(a->entry32, a->blk_off, a->stride, nb, cur, h->wide_list.as<uint32_t>(), s));
        }
        // ... and the words the kernel pairs from, once per prepare
        SECEDO_TRY(h->mk_words.ensure(std::max<size_t>(ne, 1) * 12));
        SECEDO_TRY(secedo::masks_words(a->entry32, a->mask32, (uint32_t)ne, h->mk_words.as<uint32_t>(),
                                       h->mk_words.as<uint32_t>() + ne, h->mk_words.as<uint32_t>() + 2 * ne, s));
        h->wide_known = true;
    }
    a->mk_y = h->mk_words.as<uint32_t>();
    a->mk_xcol = a->mk_y + ne;
    a->mk_xrow = a->mk_y + 2 * ne;
    if (h->n_wide) {
        a->wide_off = h->wide_tab.as<uint32_t>() + h->pk.num_blocks;
        a->wide_list = h->wide_list.as<uint32_t>();
    }
    return SECEDO_OK;
}

// accumulate_counts, and correct_tiles or the pair kernel's own epilogue; both read the flagged entries' lists,
// which prepare builds with the packing
int choose_correction(secedo_simmat *h, const TileSet &t, bool overwrite, secedo::AccumulateArgs *a) {
    if (!h->flags_ready) return fail(SECEDO_E_STATE, "the flagged entries' lists were not built");
    // the epilogue when every tile of the launch has one workgroup and correct_tiles would have one per tile too
    // (SECEDO_CORRECT_FUSED=0: never)
    static const bool fused_env = env_enabled("SECEDO_CORRECT_FUSED");
    a->fused = fused_env && h->plan_workgroups == t.size()
               && (secedo::counts_split(t.size()) == 1u || (overwrite && t.list != nullptr));
    h->last_fused = a->fused;
    a->flag_grp = h->flag_grp.as<uint32_t>();
    a->flag_rec = h->flag_rec.as<uint4>();
    a->flag_idx = h->flag_idx.as<uint32_t>();
    const double per_block_locus = h->pk.num_loci && h->pk.num_blocks
            ? (double)h->pk.num_entries / h->pk.num_loci / h->pk.num_blocks : 0.0;
    a->group_hint = per_block_locus < 2.5 ? 2 : per_block_locus < 3.2 ? 3 : 4;
    // the instance with a staged word per locus holds half the loci of a range: by the longest range the packing cut
    a->short_ranges = h->pk.block_cells == 128 && h->pk.max_range_span <= secedo::kCapL128W;
    return SECEDO_OK;
}

// overwrite: acc[tiles of the launch] = result instead of +=
// max_done (assign_finalize): set when the launch left the maximum finalize needs in max_bits
int accumulate_impl(secedo_simmat *h, double eps, double hr, double theta, TileSet t, int64_t *d_acc, void *stream,
                    bool overwrite = false, bool *max_done = nullptr) {
    if (max_done) *max_done = false;
    SECEDO_CALL(check_ready(h, false, d_acc));
    SECEDO_CALL(check_tiles(h, &t));
    SECEDO_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (with shards on several ranks: what ANY of them can reach, so that all quantise the same table)
    const uint32_t reach = std::max(h->max_shared_override, h->pk.max_read_entries);
    bool beyond = false;
    SECEDO_CALL(refresh_llr_table(h, eps, hr, theta, reach, s));
    SECEDO_CALL(refresh_slow_path_args(h, reach, s, &beyond));
    if (h->pk.num_entries == 0) return accumulate_nothing(h, t, d_acc, overwrite, s);

    const uint32_t n_tiles = t.size();
    secedo::AccumulateArgs a = base_args(h, t, d_acc, overwrite);
    if (t.list) {
        if (h->plan_list_hash != t.hash) {
            SECEDO_TRY(h->tile_ids.ensure((size_t)std::max(t.end, 1u) * 4));
            SECEDO_TRY(h->uploads.put(h->tile_ids.p, t.list, (size_t)t.end * 4, s));
        }
        a.tile_ids = h->tile_ids.as<uint32_t>();
    }
    SECEDO_CALL(plan_workgroups(h, t, s));
    a.n_workgroups = h->plan_workgroups;
    a.wg_tile = h->plan_wg_tile.as<uint32_t>();
    a.tile_wg_begin = h->plan_wg_begin.as<uint32_t>();
    // the maximum finalize needs, on the way (assign_finalize: all tiles, stored, one workgroup per tile)
    if (max_done && !beyond && overwrite && !t.list && t.begin == 0 && t.end == h->num_tiles && h->pk.count_tile
        && !h->pk.stage_masks && secedo::counts_split(n_tiles) == 1) {
        SECEDO_TRY(hipMemsetAsync(h->max_bits.p, 0, sizeof(unsigned long long), s));
        a.max_bits = h->max_bits.as<unsigned long long>();
        a.max_scale = std::ldexp(1.0, -h->scale_log2);
        *max_done = true;
    }
    if (h->pk.stage_masks && h->pk.block_cells == 64) SECEDO_CALL(prepare_masks_lists(h, s, &a));

    SECEDO_TRY(hipMemsetAsync(h->counters.p, 0, 96 * sizeof(unsigned long long), s));
    if (beyond) SECEDO_TRY(hipMemsetAsync(h->beyond_count.p, 0, sizeof(uint32_t), s));
    h->last_fused = false;
    h->last_locus_words = false;
    if (h->pk.count_tile && !h->pk.stage_masks) SECEDO_CALL(choose_correction(h, t, overwrite, &a));
    SECEDO_TRY(hipEventRecord(h->ev_begin, s));
    // 16-bit pair counters per cell pair are safe when no cell pair can collect 65536 pairs
    const bool count_tile = h->pk.count_tile;
    SECEDO_TRY(h->slab.ensure(secedo::accumulate_slab_bytes(h->pk.block_cells, count_tile, a.n_workgroups)));
    a.slab = h->slab.p;
    h->timed_mid = count_tile && !h->pk.stage_masks;
    SECEDO_TRY(secedo::launch_accumulate(a, h->pk.block_cells, h->pk.stage_masks, count_tile, n_tiles, s,
                                         h->timed_mid ? h->ev_mid : nullptr, &h->last_locus_words));
    if (beyond) SECEDO_CALL(add_beyond_terms(h, eps, hr, theta, d_acc, s));
    h->timed_mid = h->timed_mid && n_tiles > 0;
    SECEDO_TRY(hipEventRecord(h->ev_end, s));
    h->timed = true;
    return SECEDO_OK;
}

// a tile list of the C-ABI (null when empty) as a TileSet
int list_tiles(const uint32_t *tile_ids, uint32_t n_tile_ids, TileSet *t) {
    if (!tile_ids && n_tile_ids) return fail(SECEDO_E_INVALID_ARG, "tile_ids is null");
    static const uint32_t none = 0;
    *t = TileSet{0, n_tile_ids, tile_ids ? tile_ids : &none, 0};
    return SECEDO_OK;
}

}  // namespace

extern "C" {

int secedo_simmat_accumulate(secedo_simmat_t *h, double eps, double hr, double theta, uint32_t tile_begin,
                             uint32_t tile_end, int64_t *d_acc, void *stream) {
    return accumulate_impl(h, eps, hr, theta, TileSet{tile_begin, tile_end, nullptr, 0}, d_acc, stream);
}

int secedo_simmat_assign(secedo_simmat_t *h, double eps, double hr, double theta, uint32_t tile_begin,
                         uint32_t tile_end, int64_t *d_acc, void *stream) {
    return accumulate_impl(h, eps, hr, theta, TileSet{tile_begin, tile_end, nullptr, 0}, d_acc, stream, true);
}

int secedo_simmat_assign_list(secedo_simmat_t *h, double eps, double hr, double theta, const uint32_t *tile_ids,
                              uint32_t n_tile_ids, int64_t *d_acc, void *stream) {
    TileSet t;
    SECEDO_CALL(list_tiles(tile_ids, n_tile_ids, &t));
    return accumulate_impl(h, eps, hr, theta, t, d_acc, stream, true);
}

int secedo_simmat_accumulate_list(secedo_simmat_t *h, double eps, double hr, double theta, const uint32_t *tile_ids,
                                  uint32_t n_tile_ids, int64_t *d_acc, void *stream) {
    TileSet t;
    SECEDO_CALL(list_tiles(tile_ids, n_tile_ids, &t));
    return accumulate_impl(h, eps, hr, theta, t, d_acc, stream);
}

int secedo_simmat_assign_finalize(secedo_simmat_t *h, double eps, double hr, double theta, int normalization,
                                  int64_t *d_acc, double *d_out, void *stream) {
    SECEDO_CALL(check_normalization(normalization));
    if (!h || !d_acc || !d_out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    bool max_done = false;
    SECEDO_CALL(accumulate_impl(h, eps, hr, theta, TileSet{0, h->prepared ? h->num_tiles : 0, nullptr, 0}, d_acc, stream,
                                true, (normalization == 0 || normalization == 2) ? &max_done : nullptr));
    return finalize_mode(h, normalization, d_acc, 0, h->pk.num_cells, d_out, stream, max_done);
}

}  // extern "C"
