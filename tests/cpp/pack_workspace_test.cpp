// pack_workspace_test.cpp -- the device packing's workspace (secedo_amd/csrc/pack_workspace.hpp) laid over host
// memory, built with plain g++ under AddressSanitizer and UBSan. Every generation of every arena is carved over a
// malloc block of exactly the bytes arena_bytes() asks for, over a grid of shapes: every view lies inside its arena
// behind the view before it, is aligned for its element type, and its first and last element are written through a
// pointer of that type (an overrun is the sanitizer's to report). The cleared prefix of MISC covers the scalars and
// the three id tables, no more; FlagScratch's bytes() and constructor agree.
//
//   pack_workspace_test        prints the number of shapes and views checked; exit code 0, or 1 with the first failure
#include "pack_workspace.hpp"

#include <cstdio>
#include <cstdlib>

using namespace secedo;

namespace {

struct Scalars {  // size and alignment of pack_device.hip's: 14 words and three 64-bit sums
    uint32_t words[14];
    unsigned long long sums[3];
};

size_t n_views = 0;
char *held = nullptr;

[[noreturn]] void fail(const char *what, const char *gen, const PackShape &s) {
    std::fprintf(stderr, "%s: %s (E %zu L %zu C %zu cells %zu)\n", gen, what, s.E, s.L, s.C, s.cells);
    std::exit(1);
}

template <class T>
void touch(char *p, size_t count) {
    T *v = reinterpret_cast<T *>(p);
    v[0] = T{};
    v[count - 1] = T{};
}

// carve generation G over a block of exactly `bytes`
template <class G, class... D>
G check(const char *gen, const PackShape &s, size_t bytes, D... dims) {
    std::free(held);  // (the block outlives the call: the caller compares the pointers it gets back)
    char *buf = held = static_cast<char *>(std::malloc(bytes ? bytes : 1));
    CarveLog log;
    const G g(Carver(buf, &log), dims...);
    if (g.end != carved<G>(dims...)) fail("size and pointers disagree", gen, s);
    if (g.end > bytes) fail("generation larger than its arena", gen, s);
    size_t prev_end = 0;
    for (int i = 0; i < log.n; ++i) {
        const CarveLog::View &v = log.view[i];
        if (v.off != prev_end) fail("views not one behind the other", gen, s);
        prev_end = v.off + v.count * v.elem;
        if (prev_end > bytes) fail("view outside its arena", gen, s);
        if (!v.count) continue;
        if (reinterpret_cast<uintptr_t>(buf + v.off) % v.align || v.off % v.align) fail("view misaligned", gen, s);
        switch (v.elem) {
            case 1: touch<uint8_t>(buf + v.off, v.count); break;
            case 4: touch<uint32_t>(buf + v.off, v.count); break;
            case 8: touch<unsigned long long>(buf + v.off, v.count); break;
            case 16: touch<Rec16>(buf + v.off, v.count); break;
            default: touch<Scalars>(buf + v.off, v.count); break;
        }
        ++n_views;
    }
    return g;
}

void check_shape(const PackShape &s, size_t id_space) {
    const auto bytes = [&](Arena::Id a, size_t id_slots = 0) { return arena_bytes<Scalars>(a, s, id_slots); };
    const size_t E = s.E, id_slots = id_space + 1;

    const MiscViews<Scalars> m = check<MiscViews<Scalars>>("MISC", s, bytes(Arena::MISC), s);
    const char *base = reinterpret_cast<const char *>(m.sc);
    if (reinterpret_cast<const char *>(m.id_max) - base != (ptrdiff_t)sizeof(Scalars)
        || m.id_negmin != m.id_max + s.C || m.id_base != m.id_negmin + s.C
        || reinterpret_cast<const char *>(m.id_base + s.C + 1) - base != (ptrdiff_t)m.zeroed
        || reinterpret_cast<const char *>(m.rbeg) - base != (ptrdiff_t)m.zeroed)
        fail("the cleared prefix is not Scalars | id_max | id_negmin | id_base", "MISC", s);

    check<UnsortedKeys>("KEY_A keys", s, bytes(Arena::KEY_A), E);
    check<DenseIds>("KEY_A dense ids", s, bytes(Arena::KEY_A), E);
    check<MarksRanksCounts>("KEY_A marks | ranks | counts", s, bytes(Arena::KEY_A), s);
    check<SortedKeys>("KEY_B sorted keys", s, bytes(Arena::KEY_B), E);
    check<GroupedKept>("KEY_B grouped", s, bytes(Arena::KEY_B), E);
    check<GroupedIds>("VAL_A grouped ids", s, bytes(Arena::VAL_A), E);
    check<FlagBlockSums>("VAL_A block sums", s, bytes(Arena::VAL_A), s);
    check<KeptFlags>("VAL_A kept flags", s, bytes(Arena::VAL_A), E);
    check<SortedValues>("VAL_B", s, bytes(Arena::VAL_B), E);
    check<EntryLocus>("ELOC", s, bytes(Arena::ELOC), E);
    check<SortedLoci>("ENTRY_KC sorted loci", s, bytes(Arena::ENTRY_KC), E);
    check<EntryKC>("ENTRY_KC (k, cell)", s, bytes(Arena::ENTRY_KC), E);
    check<SplitFlags>("TMP cuts", s, bytes(Arena::TMP), E);
    check<KeptRead>("TMP read per kept entry", s, bytes(Arena::TMP), E);
    // WORK_A and WORK_B: before the id space is known, and grown for it
    for (size_t slots : {(size_t)0, id_slots}) {
        check<IdSlots>("WORK_A id slots", s, bytes(Arena::WORK_A, slots), slots);
        check<KeepFlags>("WORK_A keep", s, bytes(Arena::WORK_A, slots), E + 1);
        check<KeptRank>("WORK_A kept rank", s, bytes(Arena::WORK_A, slots), E);
        check<IdOffsets>("WORK_B id offsets", s, bytes(Arena::WORK_B, slots), slots);
        check<InclSums>("WORK_B inclusive sums", s, bytes(Arena::WORK_B, slots), E + 1);
    }
    check<Runs>("RUNS", s, bytes(Arena::RUNS), s);
    if (bytes(Arena::RUNS) != (2 * E + 1) * 4) fail("RUNS is not run_start[E + 1] | run_rank[E]", "RUNS", s);
    // BIN at the fewest and the most kept entries, 64- and 128-cell blocks
    for (size_t nk : {(size_t)1, E})
        for (size_t B : {(size_t)64, (size_t)128}) {
            const size_t rows = (s.cells + B - 1) / B * B;
            const BinRadix r = check<BinRadix>("BIN radix", s, bytes(Arena::BIN), nk, rows);
            const BinCounting c = check<BinCounting>("BIN counting", s, bytes(Arena::BIN), nk, rows);
            if (reinterpret_cast<const char *>(r.per_cell_sq) - reinterpret_cast<const char *>(r.key2_a)
                != reinterpret_cast<const char *>(c.per_cell_sq) - reinterpret_cast<const char *>(c.m_rec))
                fail("per_cell_sq differs between the routes", "BIN", s);
        }
    check<MChunks>("M_CHUNKS", s, bytes(Arena::M_CHUNKS), s);
    check<MultiFlags>("MARK_M flags", s, bytes(Arena::MARK_M), s.flag_bytes());
    check<MarksOfM>("MARK_M marks", s, bytes(Arena::MARK_M), E + 2);
    for (Arena::Id a : {Arena::M_ENTRY, Arena::RID_M, Arena::IDB_M, Arena::ELOC_M, Arena::ARANK_M})
        check<PerM>("per M entry", s, bytes(a), E);
    for (size_t n_m : {(size_t)0, E / 2}) check<MReads>("DENSE_M", s, bytes(Arena::DENSE_M), n_m);
    check<DupFlags>("DUPF", s, bytes(Arena::DUPF), s.L);
    // SEGS: one set of limits (lo == hi) and two
    for (size_t lo : {(size_t)64, (size_t)512})
        for (size_t hi : {lo, (size_t)4096}) {
            const size_t n_seg = (s.L + lo - 1) / lo, stride = n_seg * hi + n_seg + 2;
            check<Segs>("SEGS", s, carved<Segs>(n_seg, stride), n_seg, stride);
            if (carved<Segs>(n_seg, stride) != 2 * stride * 4) fail("not two variants of variant_stride words", "SEGS", s);
        }
}

void check_flag_scratch(uint32_t n) {
    const PackShape none{n, 0, 0, 0};
    const size_t bytes = FlagScratch::bytes(n);
    const FlagScratch fs = check<FlagScratch>("FlagScratch", none, bytes, n);
    const size_t nb = fs.nb;
    if (nb != (n + kFlagBlock - 1) / kFlagBlock + (n == 0)) fail("blocks", "FlagScratch", none);
    if (fs.end != bytes || bytes != (2 * nb + 64 * nb + 2) * 4 + 64 * nb * 8) fail("bytes()", "FlagScratch", none);
    // what pack_flag_lists and k_entry_records expect: sums, offsets, prefixes with the closing word, aligned masks
    if (fs.block_off != fs.block_sum + nb || fs.chunk_pre != fs.block_off + nb
        || reinterpret_cast<uint32_t *>(fs.chunk_mask) != fs.chunk_pre + 64 * nb + 2)
        fail("layout", "FlagScratch", none);
    const FlagScratch null_fs(nullptr, n);
    if (null_fs.block_sum || null_fs.block_off || null_fs.chunk_pre || null_fs.chunk_mask || null_fs.nb != nb)
        fail("no scratch, no pointers", "FlagScratch", none);
}

}  // namespace

int main() {
    size_t n_shapes = 0;
    for (size_t E : {1, 63, 64, 4095, 4096, 4097})
        for (size_t L : {1, 2, 65})
            for (size_t C : {1, 3, 70})
                for (size_t cells : {1, 64, 65, 129, 65535})
                    for (size_t id_space : {(size_t)1, 4 * E + 1024}) {
                        check_shape(PackShape{E, L, C, cells}, id_space);
                        ++n_shapes;
                    }
    for (uint32_t n : {0u, 1u, 4096u, 4097u}) check_flag_scratch(n);
    std::free(held);
    std::printf("%zu shapes, %zu views\n", n_shapes, n_views);
    return 0;
}
