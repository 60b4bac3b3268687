// pack_workspace.hpp -- the scratch memory of the device packing (pack_device.hip): its arenas, what each holds at
// which time, and the one carver that gives both an arena's size and the pointers into it. Plain C++ (no HIP), so a
// host program can lay every arena over a malloc block (tests/cpp/pack_workspace_test.cpp).
//
// An arena (DevicePacked::scratch[Arena::X]) is reused for unrelated data at different times. A GENERATION is a set of
// views that are alive together: its views are carved one behind the other and are disjoint by construction; the
// generations of one arena alias each other, and the comment at each says which kernel writes it first and which
// reads it last. An arena's size (arena_bytes) is the largest of its generations plus the slack named there.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace secedo {

constexpr uint32_t kFlagBlock = 4096;  // entries per workgroup of the numbering passes (k_flag_count, k_compact_m, ...)

struct alignas(16) Rec16 {  // 16 bytes per kept M entry (a uint4 on the device: k_m_records)
    uint32_t w[4];
};

struct CarveLog {  // what a carver handed out (the host test reads it)
    struct View {
        size_t off, count, elem, align;
    } view[16];
    int n = 0;
};

// Bump carver over one arena. The same sequence of take() calls runs with a null base for the byte count and with the
// arena's base for the pointers, so the two cannot disagree. No padding: a view starts where the previous one ends.
struct Carver {
    char *base;
    CarveLog *log;
    size_t off = 0;
    Carver(void *b, CarveLog *l = nullptr) : base(static_cast<char *>(b)), log(l) {}
    template <class T>
    T *take(size_t count) {
        if (log) log->view[log->n++] = {off, count, sizeof(T), alignof(T)};
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};
template <class G, class... D>
size_t carved(D... dims) {
    return G(Carver(nullptr), dims...).end;
}

struct Arena {
    enum Id { KEY_A, KEY_B, VAL_A, VAL_B, ELOC, WORK_A, WORK_B, RUNS, CUB, TMP, MISC, BIN, ENTRY_KC,
              M_CHUNKS, M_ENTRY, RID_M, IDB_M, ELOC_M, DENSE_M, MARK_M, ARANK_M, DUPF, SEGS, kCount };
};

// What sizes the workspace: raw entries, loci, chromosomes, cells
struct PackShape {
    size_t E, L, C, cells;
    // group offsets of the worst case (64-cell blocks): sized before the tile size is chosen
    size_t n_off_max() const { return (cells + 63) / 64 * (L + 1); }
    // the single-entry route's flag bytes (whole blocks and a closing 16) and 64-entry chunks (and the closing one)
    size_t flag_blocks() const { return (E + kFlagBlock - 1) / kFlagBlock; }
    size_t flag_bytes() const { return flag_blocks() * kFlagBlock + 16; }
    size_t chunks() const { return flag_blocks() * (kFlagBlock / 64) + 1; }
};

// a generation of one view
template <class T>
struct One {
    T *p;
    size_t end;
    One(Carver c, size_t count) : p(c.take<T>(count)), end(c.off) {}
    operator T *() const { return p; }
};

// ---- MISC: the scalars and the per-chromosome / per-locus tables; one generation, alive over the whole attempt -----
// (k_id_range writes, the closing read-back reads.) The attempt begins by clearing the prefix [0, zeroed): the
// scalars (among them the ticket words of the kernels whose last workgroup finishes the job), the id extremes
// k_id_range raises with atomics and the bases its last workgroup sums up.
template <class Scalars>
struct MiscViews {
    Scalars *sc;
    uint32_t *id_max, *id_negmin, *id_base;  // [C] [C] [C + 1]
    size_t zeroed;
    uint32_t *rbeg, *flushed;                // [C + 1] [C]
    uint32_t *cnt, *locus_chr, *locus_rel, *flush_loci;  // [L] each
    uint32_t *flush_count, *tail_begin;      // [C] [C]
    uint32_t *chr_entry;  // [C + 1] first entry of every chromosome, and the number of entries (k_id_range)
    size_t end;
    MiscViews(Carver c, const PackShape &s) {
        sc = c.take<Scalars>(1);
        id_max = c.take<uint32_t>(s.C), id_negmin = c.take<uint32_t>(s.C), id_base = c.take<uint32_t>(s.C + 1);
        zeroed = c.off;
        rbeg = c.take<uint32_t>(s.C + 1), flushed = c.take<uint32_t>(s.C);
        cnt = c.take<uint32_t>(s.L), locus_chr = c.take<uint32_t>(s.L), locus_rel = c.take<uint32_t>(s.L);
        flush_loci = c.take<uint32_t>(s.L);
        flush_count = c.take<uint32_t>(s.C), tail_begin = c.take<uint32_t>(s.C), chr_entry = c.take<uint32_t>(s.C + 1);
        end = c.off;
    }
};

// ---- KEY_A ---------------------------------------------------------------------------------------------------------
using UnsortedKeys = One<unsigned long long>;  // [E] radix route: k_entry_keys -> the radix sort
using DenseIds = One<uint32_t>;                // [E] counting route: k_id_hist -> k_id_rank
// k_dup_mark (mark), the rank scan (arank) -> k_keys2 / k_bin_hist, which read the ranks while they write the counts
// (blk_cnt: memset or k_bin_hist -> the offset scan); on the single-entry route arank first holds the prefix sums
// `unm` (struct Ranks)
struct MarksRanksCounts {
    uint32_t *mark, *arank, *blk_cnt;  // [E + 1] [E + 1] [n_off_max + 1]
    size_t end;
    MarksRanksCounts(Carver c, const PackShape &s) {
        mark = c.take<uint32_t>(s.E + 1), arank = c.take<uint32_t>(s.E + 1), blk_cnt = c.take<uint32_t>(s.n_off_max() + 1);
        end = c.off;
    }
};
// ---- KEY_B ---------------------------------------------------------------------------------------------------------
using SortedKeys = One<unsigned long long>;   // [E] k_id_rank / k_group_rank / the radix sort -> k_split_update
using GroupedKept = One<unsigned long long>;  // [E] counting route of stage 5: k_bin_place -> k_entry_records
// ---- VAL_A ---------------------------------------------------------------------------------------------------------
using GroupedIds = One<uint32_t>;  // [E] k_id_scatter -> k_id_rank; radix route: the unsorted values, k_entry_keys -> sort
struct FlagBlockSums {             // single-entry route: k_flag_count -> k_compact_m
    uint32_t *block_sum, *block_off;  // [flag_blocks + 1] each
    size_t end;
    FlagBlockSums(Carver c, const PackShape &s) {
        block_sum = c.take<uint32_t>(s.flag_blocks() + 1), block_off = c.take<uint32_t>(s.flag_blocks() + 1);
        end = c.off;
    }
};
using KeptFlags = One<uint8_t>;  // [kept] base | multi flag per kept entry: k_keys2 -> k_records / k_m_records
// ---- VAL_B, ELOC, ENTRY_KC, TMP ------------------------------------------------------------------------------------
using SortedValues = One<uint32_t>;  // VAL_B [E] stage 1 -> k_keys2
using EntryLocus = One<uint32_t>;    // ELOC [E] k_entry_locus -> k_id_rank / k_sorted_locus (no single-entry route)
using SortedLoci = One<uint32_t>;    // ENTRY_KC [E] locus | base in sorted order: stage 1 -> k_split_update / k_runs_csr / k_ranks_runs
using EntryKC = One<unsigned long long>;  // ENTRY_KC [E] counting route, (k, cell) per entry: k_bin_hist / k_keys2 -> k_bin_place
using SplitFlags = One<uint32_t>;    // TMP [E] cuts of long reads: memset / k_split_update -> k_dup_mark of the last build
using KeptRead = One<uint32_t>;      // TMP [E] read index per kept entry: k_keys2 -> k_records / k_m_records
// ---- WORK_A, WORK_B (grown behind read-back 1 for the id space: id_slots = id space + 1, counting route) ------------
using IdSlots = One<uint32_t>;   // WORK_A [id_slots] counts (k_id_hist) or entry numbers (k_id_store) -> k_id_scatter / k_m_fields
using KeepFlags = One<uint32_t>; // WORK_A [E + 1] duplicate rule: k_dup_mark -> the read scan (HeadKeepOp)
using KeptRank = One<uint32_t>;  // WORK_A [E] appearance rank per kept entry: k_keys2 -> k_records / k_m_records
using IdOffsets = One<uint32_t>; // WORK_B [id_slots] the scan of the counts -> k_id_rank
using InclSums = One<unsigned long long>;  // WORK_B [E + 1] reads | kept entries << 32 so far: the read scan -> k_keys2
// ---- RUNS: k_runs_csr / k_ranks_runs, k_read_info -> k_keys2 ----------------------------------------------------------------------
struct Runs {
    uint32_t *run_start, *run_rank;  // [E + 1] [E] (reads R <= E)
    size_t end;
    Runs(Carver c, const PackShape &s) {
        run_start = c.take<uint32_t>(s.E + 1), run_rank = c.take<uint32_t>(s.E);
        end = c.off;
    }
};
// ---- BIN (nk: kept entries, at least 1; rows: cells padded to whole blocks) -----------------------------------------
struct BinRadix {  // radix route of stage 5: k_keys2 -> the sort -> k_records; per_cell_sq outlives the attempt
    unsigned long long *key2_a, *key2_b, *per_cell_sq;  // [nk] [nk] [rows + 1]
    uint32_t *val2_a, *val2_b;                          // [nk] each
    size_t end;
    BinRadix(Carver c, size_t nk, size_t rows) {
        key2_a = c.take<unsigned long long>(nk), key2_b = c.take<unsigned long long>(nk);
        per_cell_sq = c.take<unsigned long long>(rows + 1);
        val2_a = c.take<uint32_t>(nk), val2_b = c.take<uint32_t>(nk);
        end = c.off;
    }
};
struct BinCounting {  // counting route: k_m_records -> k_entry_records; per_cell_sq where the radix route has it
    Rec16 *m_rec;                     // [nk]
    unsigned long long *per_cell_sq;  // [rows + 1]
    size_t end;
    BinCounting(Carver c, size_t nk, size_t rows) {
        m_rec = c.take<Rec16>(nk), per_cell_sq = c.take<unsigned long long>(rows + 1);
        end = c.off;
    }
};
// ---- the single-entry route's own arenas (ensured on that route only) ----------------------------------------------
struct MChunks {  // M_CHUNKS: k_compact_m / k_flag_scan -> k_bin_hist (struct MIndex)
    unsigned long long *chunk_mask;  // [chunks]
    uint32_t *chunk_pre;             // [chunks]
    size_t end;
    MChunks(Carver c, const PackShape &s) {
        chunk_mask = c.take<unsigned long long>(s.chunks()), chunk_pre = c.take<uint32_t>(s.chunks());
        end = c.off;
    }
};
using MultiFlags = One<uint8_t>;  // MARK_M [flag_bytes] a byte per entry: memset / k_id_check -> k_compact_m
using MarksOfM = One<uint32_t>;   // MARK_M [E + 2] the marks of the M entries: k_dup_mark -> the scan of UnmarkedM
using PerM = One<uint32_t>;       // M_ENTRY, RID_M, IDB_M, ELOC_M (k_compact_m / k_m_fields -> k_keys2), ARANK_M (k_ranks_runs -> k_read_info): [E]
struct MReads {  // DENSE_M, the reads of the n_m <= E / 2 M entries: k_m_fields -> k_group_rank. count_m is zeroed by
                 // k_compact_m, which does not know n_m yet: it is the FIRST view, at the arena's base whatever n_m is
                 // (E + 1 words at the most, within the arena: a route given up at n_m > E / 2 has zeroed them too)
    uint32_t *count_m, *goff, *winner_m, *g_begin, *g_len, *members;  // [n_m + 1] [n_m + 1] [n_m] ...
    size_t end;
    MReads(Carver c, size_t n_m) {
        count_m = c.take<uint32_t>(n_m + 1), goff = c.take<uint32_t>(n_m + 1), winner_m = c.take<uint32_t>(n_m);
        g_begin = c.take<uint32_t>(n_m), g_len = c.take<uint32_t>(n_m), members = c.take<uint32_t>(n_m);
        end = c.off;
    }
};
// ---- DUPF, SEGS (stage 5) ------------------------------------------------------------------------------------------
using DupFlags = One<uint8_t>;  // DUPF [L] some cell has two kept entries at the locus: k_bin_place -> k_locus_info
struct Segs {  // k_ranges_segment -> k_ranges_compact (on the side stream beside the placing pass; the repair behind
               // read-back 3 included); both variants of limits
    uint32_t *seg_count, *seg_ends;  // [n_seg] [2 variant_stride - n_seg]
    size_t end;
    Segs(Carver c, size_t n_seg, size_t variant_stride) {
        seg_count = c.take<uint32_t>(n_seg), seg_ends = c.take<uint32_t>(2 * variant_stride - n_seg);
        end = c.off;
    }
};

// Bytes an arena is ensured for (CUB and SEGS apart: hipCUB's own queries, and Segs at its run-time sizes). The
// constants are slack behind the last view: vector loads of a kernel's last lanes and rounding of the sizes.
template <class Scalars>
size_t arena_bytes(Arena::Id a, const PackShape &s, size_t id_slots = 0) {
    using std::max;
    switch (a) {
        case Arena::MISC: return carved<MiscViews<Scalars>>(s) + 84;
        case Arena::KEY_A: return max({carved<UnsortedKeys>(s.E), carved<DenseIds>(s.E), carved<MarksRanksCounts>(s) + 8});
        case Arena::KEY_B: return max(carved<SortedKeys>(s.E), carved<GroupedKept>(s.E));
        case Arena::VAL_A: return max({carved<GroupedIds>(s.E), carved<FlagBlockSums>(s), carved<KeptFlags>(s.E), (size_t)256});
        case Arena::VAL_B: return carved<SortedValues>(s.E);
        case Arena::ELOC: return carved<EntryLocus>(s.E) + 16;
        case Arena::WORK_A: return max({carved<IdSlots>(id_slots), carved<KeepFlags>(s.E + 1), carved<KeptRank>(s.E)});
        case Arena::WORK_B: return max(carved<IdOffsets>(id_slots), carved<InclSums>(s.E + 1));
        case Arena::RUNS: return carved<Runs>(s);
        case Arena::TMP: return max(carved<SplitFlags>(s.E), carved<KeptRead>(s.E)) + 64;
        case Arena::BIN: return max(carved<BinRadix>(s.E, s.cells + 127), carved<BinCounting>(s.E, s.cells + 127)) + 80;
        case Arena::ENTRY_KC: return max(carved<SortedLoci>(s.E), carved<EntryKC>(s.E));
        case Arena::M_CHUNKS: return carved<MChunks>(s) + 16;
        case Arena::MARK_M: return max(carved<MultiFlags>(s.flag_bytes()), carved<MarksOfM>(s.E + 2));
        case Arena::DENSE_M: return carved<MReads>(s.E / 2) + 48;
        case Arena::DUPF: return carved<DupFlags>(s.L) + 16;
        case Arena::M_ENTRY: case Arena::RID_M: case Arena::IDB_M: case Arena::ELOC_M: case Arena::ARANK_M:
            return carved<PerM>(s.E) + 16;
        default: return 0;
    }
}

// The caller's scratch of the flagged entries' lists (pack_flag_lists, k_entry_records): block sums and offsets, the
// prefix per 64-entry chunk with its closing word (and one more: the masks are 8-byte aligned), the chunks' masks
inline uint32_t flag_blocks(uint32_t n_entries) { return std::max<uint32_t>(1u, (n_entries + kFlagBlock - 1) / kFlagBlock); }
struct FlagScratch {
    uint32_t nb;
    uint32_t *block_sum, *block_off, *chunk_pre;  // [nb] [nb] [64 nb + 2]
    unsigned long long *chunk_mask;               // [64 nb]
    size_t end;
    FlagScratch(Carver c, uint32_t n_entries) : nb(flag_blocks(n_entries)) {
        block_sum = c.take<uint32_t>(nb), block_off = c.take<uint32_t>(nb), chunk_pre = c.take<uint32_t>(64 * (size_t)nb + 2);
        chunk_mask = c.take<unsigned long long>(64 * (size_t)nb);
        end = c.off;
    }
    static size_t bytes(uint32_t n_entries) { return carved<FlagScratch>(n_entries); }
};

}  // namespace secedo
