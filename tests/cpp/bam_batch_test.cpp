// bam_batch_test -- secedo_amd/csrc/bam_batch.hpp on the host, under AddressSanitizer and UBSan: the layout of a batch
// of the BAM device route, the range cut of bgzf_members.hpp and the words of a record defect.
//   bam_batch_test files | spans | index | limits | ranges | words
//       the checks of that group; prints "ok ..." and exits 0, or names the line of the first check that failed and
//       exits 1.
// The files are synthetic: a member table with real coff / poff / clen / isize / out over bytes that are a function of
// their offset, so a descriptor that points elsewhere than at its member's payload is seen. Staging is a heap block
// of exactly in_bytes, filled from the copy list, so a copy past it is a sanitizer report.
#include "bam_batch.hpp"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

using namespace secedo::bam;
using namespace secedo::bam_host;
namespace bw = secedo::bamwalk;

namespace {

using Bytes = std::vector<uint8_t>;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

// a file of members with the given ISIZEs; member k has a payload of 20 + 7 * (k % 5) bytes behind an 18-byte header
struct File {
    std::vector<Block> m;
    Bytes bytes, carry;
    uint64_t total = 0;
    FileWalk walk;
    File(std::initializer_list<uint32_t> isizes, size_t carry_len, unsigned seed, size_t n_chr = 0) {
        walk.run_first.assign(n_chr, bw::kNoRun);
        walk.run_last.assign(n_chr, bw::kNoRun);
        uint64_t coff = 0;
        for (const uint32_t isize : isizes) {
            const uint32_t clen = 20 + 7 * uint32_t(m.size() % 5);
            m.push_back(Block{coff, total, isize, 18, clen, uint32_t(0xC0000000u + m.size())});
            coff += 18 + clen + 8;
            total += isize;
        }
        bytes.resize(coff);
        for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = uint8_t((i * 131 + seed * 17) ^ (i >> 8));
        carry.resize(carry_len);
        for (size_t i = 0; i < carry_len; ++i) carry[i] = uint8_t(0x40 + seed + i);
    }
    // members [b0, b1) as a piece; carry: the host carry's length on the first range, else the device carry's
    BatchPiece piece(size_t b0, size_t b1, bool first, bool final, uint64_t carry_bytes) const {
        BatchPiece p;
        p.blocks = &m;
        p.b0 = b0, p.b1 = b1;
        p.file = bytes.data(), p.file_bytes = bytes.size();
        p.carry_bytes = carry.data(), p.carry = carry_bytes;
        p.first_range = first, p.final = final;
        p.walk = &walk;
        p.lin0 = b0 < m.size() ? m[b0].out : total;
        return p;
    }
    BatchPiece whole(size_t hb) const { return piece(hb, m.size(), true, true, carry.size()); }
};

// Everything a layout owes, whatever the pieces: files[k] holds the bytes of piece k.
int check_layout(const std::vector<BatchPiece> &in, const std::vector<const File *> &files,
                 const std::vector<uint32_t> &chr_ids, bool index, const BatchLayout &L) {
    const size_t n = in.size(), n_chr = chr_ids.size();
    CHECK(L.overflow == UINT32_MAX && L.files.size() == n && L.first_member.size() == n);
    CHECK(L.runs.size() == n * n_chr && L.checks.size() == n * n_chr);
    CHECK(L.buf_bytes == L.out_bytes + kWalkWindow && L.out_bytes % 16 == 0 && L.out_bytes <= kMaxBatchBytes);
    CHECK(L.n_list <= L.out_bytes);  // a list entry per started record, a record per byte at most
    // the copies: inside staging, no two over the same byte, their sources inside the file or the carry
    std::unique_ptr<uint8_t[]> staged(new uint8_t[L.in_bytes]);
    std::vector<char> used(L.in_bytes, 0);
    std::memset(staged.get(), 0xEE, L.in_bytes);
    const auto inside = [](const Bytes &b, const BatchCopy &c) {
        return !b.empty() && c.src >= b.data() && c.n <= b.size() && c.src <= b.data() + (b.size() - c.n);
    };
    for (const BatchCopy &c : L.copies) {
        CHECK(c.n >= 1 && c.n <= kCopyChunk && c.dst + c.n <= L.in_bytes);
        bool found = false;
        for (const File *f : files) found = found || inside(f->bytes, c) || inside(f->carry, c);
        CHECK(found);
        for (uint64_t i = 0; i < c.n; ++i) {
            CHECK(!used[c.dst + i]);
            used[c.dst + i] = 1;
        }
        std::memcpy(staged.get() + c.dst, c.src, c.n);
    }
    uint64_t out = 0, list = 0, n_desc = 0, ix_seg = 0;
    std::vector<uint64_t> data_start(n), seg_end(n);
    for (size_t k = 0; k < n; ++k) {
        const BatchPiece &p = in[k];
        const File &f = *files[k];
        const WalkFile &F = L.files[k];
        const uint64_t ds = data_start[k] = (out + 15) / 16 * 16;  // a file's bytes start 16-aligned, behind the last
        const size_t nm = p.b1 - p.b0;
        CHECK(L.first_member[k] == n_desc);
        // the carry: uploaded only on a first range, and then with the decoder's slack around it
        if (p.first_range && p.carry) {
            CHECK(F.carry_len == p.carry && F.carry_src >= kBgzfInSlack);
            CHECK(F.carry_src + F.carry_len + kBgzfInSlack <= L.in_bytes);
            CHECK(std::memcmp(staged.get() + F.carry_src, f.carry.data(), p.carry) == 0);
        } else {
            CHECK(F.carry_src == 0 && F.carry_len == 0);
        }
        // the descriptors: 16-byte loads inside the upload, the payload where they point, outputs one behind the other
        uint64_t o = ds + p.carry;
        for (size_t j = 0; j < nm; ++j) {
            const BgzfDesc &d = L.desc[n_desc + j];
            const Block &x = (*p.blocks)[p.b0 + j];
            CHECK(d.in_off >= kBgzfInSlack && d.in_off + d.clen + kBgzfInSlack <= L.in_bytes);
            CHECK(d.clen == x.clen && d.isize == x.isize && d.crc == x.crc && d.reserved == 0);
            CHECK(std::memcmp(staged.get() + d.in_off, f.bytes.data() + x.payload(), x.clen) == 0);
            CHECK(d.out_off == o && d.out_off + d.isize <= L.out_bytes);
            o += d.isize;
        }
        seg_end[k] = o;
        // the segments of its members tile [data_start (+ entry), the end of its bytes)
        if (nm) {
            CHECK(F.first_seg == n_desc && F.n_seg == nm);
            uint64_t at = ds + (p.span && p.first_range ? p.span->entry : 0), end = ds + p.carry;
            for (size_t j = 0; j < nm; ++j) {
                const bw::Seg &s = L.segs[n_desc + j];
                end += (*p.blocks)[p.b0 + j].isize;
                CHECK(s.start == at && s.end == end && s.file == k && s.list == list);
                list += bw::list_cap(uint32_t(end - at));
                at = end;
            }
            CHECK(at == o);
        }
        n_desc += nm;
        const uint64_t data_end = p.span && p.final ? ds + p.carry - p.span->blocks[p.b0].out + p.span->limit : o;
        CHECK(F.data_end == data_end && F.limit == data_end && F.stop_off == data_end && data_end <= o);
        CHECK(F.bad == ~0ull && F.err == ~0ull && F.unsorted == ~0ull);
        CHECK(F.final == (p.final ? 1u : 0u) && F.has_prev == (p.walk->has_prev ? 1u : 0u));
        CHECK(F.rec_base == p.walk->rec_base && F.prev_ref == p.walk->prev_ref && F.prev_pos == p.walk->prev_pos);
        CHECK(F.n_rec == 0 && F.first_rec == 0 && F.rewalked == 0 && F.last_ref == 0 && F.last_pos == 0);
        for (size_t u = 0; u < n_chr; ++u) {
            const WalkRun &r = L.runs[k * n_chr + u];
            CHECK(r.first == p.walk->run_first[u] && r.last == p.walk->run_last[u] && !r.j0 && !r.j1 && !r.b0 && !r.b1);
            const SpanCheck &ck = L.checks[k * n_chr + u];
            const SpanChr *sc = nullptr;
            size_t c = 0;
            for (; p.span && c < p.span->chrs.size(); ++c)
                if (p.span->chrs[c].chromosome == chr_ids[u]) {
                    sc = &p.span->chrs[c];
                    break;
                }
            CHECK(!ck.start && !ck.entry_bad && !ck.tail_bad && !ck.reserved && !ck.count);
            if (!sc) {
                CHECK(ck.flags == 0 && ck.beg == 0 && ck.end == 0 && ck.ref == 0);
                continue;
            }
            const long long base = (long long)(ds + p.carry) - (long long)p.span->blocks[p.b0].out;
            CHECK(ck.beg == base + (long long)sc->beg && ck.end == base + (long long)sc->end);
            CHECK(ck.ref == int32_t(sc->chromosome) && (ck.flags & kSpanOn));
            CHECK(bool(ck.flags & kSpanEntry) == (c == 0 && p.first_range));
            CHECK(bool(ck.flags & kSpanTail) ==
                  (c + 1 == p.span->chrs.size() && p.final && p.span->limit + 8 <= p.span->bytes));
            CHECK((ck.flags & ~(kSpanOn | kSpanEntry | kSpanTail)) == 0);
        }
        CHECK(L.any_span || !p.span);
        if (index) {
            const IndexFile &x = L.ix_files[k];
            CHECK((long long)(ds + p.carry) + x.delta == (long long)p.lin0);
            CHECK(x.seg_base == ix_seg && x.n_ref == p.n_ref && x.pad == 0 && x.err == ~0ull);
            ix_seg += uint64_t(p.n_ref) + 1;
        }
        out = o;
    }
    CHECK(n_desc == L.desc.size() && L.out_bytes == (out + 15) / 16 * 16);
    // the pieces without a member walk their carry as one segment each, behind the members' segments
    size_t s_at = n_desc;
    for (size_t k = 0; k < n; ++k) {
        if (in[k].b0 < in[k].b1) continue;
        const bw::Seg &s = L.segs[s_at];
        CHECK(L.files[k].first_seg == s_at && L.files[k].n_seg == 1);
        CHECK(s.start == data_start[k] && s.end == seg_end[k] && s.end - s.start == in[k].carry);
        CHECK(s.file == k && s.list == list);
        list += bw::list_cap(uint32_t(in[k].carry));
        ++s_at;
    }
    CHECK(s_at == L.segs.size() && list == L.n_list);
    return 0;
}

int lay(const std::vector<BatchPiece> &in, const std::vector<const File *> &files,
        const std::vector<uint32_t> &chr_ids, bool index, BatchLayout *L) {
    CHECK(lay_out_batch(in, chr_ids, index, L));
    return check_layout(in, files, chr_ids, index, *L);
}

int files_group() {
    BatchLayout L;  // one layout for every batch, as the route keeps it
    const std::vector<uint32_t> chrs{3, 0};
    // one file, one member, no carry
    const File one({5000}, 0, 1, 2);
    if (lay({one.whole(0)}, {&one}, chrs, false, &L)) return 1;
    CHECK(L.in_bytes == 3 * kBgzfInSlack + one.m[0].clen && L.out_bytes == 5008 && L.segs.size() == 1);
    CHECK(L.n_list == bw::list_cap(5000) && L.copies.size() == 1 && !L.any_span);
    // its header's members held all of it: no member in the batch, a carry of 37 bytes, one segment
    const File held({3000}, 37, 2, 2);
    if (lay({held.whole(1)}, {&held}, chrs, false, &L)) return 1;
    CHECK(L.desc.empty() && L.segs.size() == 1 && L.segs[0].start == 0 && L.segs[0].end == 37 && L.n_list == 2);
    CHECK(L.in_bytes == 37 + 2 * kBgzfInSlack && L.out_bytes == 48 && L.files[0].carry_src == kBgzfInSlack);
    // three files with carries of 0, 1 and 17 bytes, the middle one with nothing but its carry
    const File a({700, 4000, 65536, 0}, 0, 3, 2), b({900}, 1, 4, 2), c({1200, 333, 0}, 17, 5, 2);
    if (lay({a.whole(1), b.whole(1), c.whole(1)}, {&a, &b, &c}, chrs, false, &L)) return 1;
    CHECK(L.segs.size() == 6 && L.files[1].first_seg == 5 && L.segs[5].file == 1);
    CHECK(L.files[2].first_seg == 3 && L.first_member[2] == 3 && L.segs[5].end - L.segs[5].start == 1);
    CHECK(L.segs[3].start % 16 == 0 && L.segs[3].end - L.segs[3].start == 17 + 333);
    // an empty member in the middle and a tail of empty members: segments of no bytes, no list entries
    const File e({2000, 0, 3000, 0, 0, 0}, 5, 6, 2);
    if (lay({e.whole(0)}, {&e}, chrs, false, &L)) return 1;
    CHECK(L.segs.size() == 6 && L.segs[1].start == L.segs[1].end && L.segs[5].start == L.segs[5].end);
    CHECK(L.n_list == bw::list_cap(2005) + bw::list_cap(3000) && L.files[0].data_end == 5005);
    // a later range of a file that goes alone: the device carry of 35 bytes lies in the buffer, nothing of it goes up
    File late({60000, 60000, 60000, 60000, 0}, 9, 7, 2);
    late.walk.run_first[1] = 0;
    late.walk.rec_base = 777, late.walk.has_prev = true, late.walk.prev_ref = 3, late.walk.prev_pos = 123456;
    BatchPiece p = late.piece(2, 4, false, false, 35);
    if (lay({p}, {&late}, chrs, false, &L)) return 1;
    CHECK(L.segs[0].start == 0 && L.segs[0].end == 60035 && L.segs[1].start == 60035 && L.desc[0].out_off == 35);
    CHECK(L.copies.size() == 1 && L.copies[0].src == late.bytes.data() + late.m[2].payload() - kBgzfInSlack);
    CHECK(L.runs[1].first == 0 && L.runs[0].first == bw::kNoRun);
    p = late.piece(4, 5, false, true, 35);  // its last range: the EOF member
    if (lay({p}, {&late}, chrs, false, &L)) return 1;
    CHECK(L.files[0].data_end == 35 && L.files[0].final == 1 && L.n_list == 1);
    std::printf("ok files\n");
    return 0;
}

// a span over the members of f from member m0 on: `out` from 0, entered mid-member, two chromosomes
Span span_of(const File &f, size_t m0, uint64_t entry, uint64_t mid, uint64_t limit) {
    Span sp;
    for (size_t b = m0; b < f.m.size(); ++b) {
        sp.blocks.push_back(f.m[b]);
        sp.blocks.back().out -= f.m[m0].out;
    }
    sp.entry = entry, sp.limit = limit;
    sp.bytes = f.total - f.m[m0].out;
    sp.chrs = {SpanChr{7, entry, mid, 11}, SpanChr{2, mid, limit, 5}};
    return sp;
}

int span_piece(const File &f, const Span &sp, size_t b0, size_t b1, uint64_t carry, BatchLayout *L, uint32_t flags7,
               uint32_t flags2) {
    const std::vector<uint32_t> chrs{2, 9, 7};  // 9 is requested and not in the span
    BatchPiece p = f.piece(b0, b1, b0 == 0, b1 == sp.blocks.size(), carry);
    p.blocks = &sp.blocks;
    p.span = &sp;
    if (lay({p}, {&f}, chrs, false, L)) return 1;
    CHECK(L->any_span && L->checks[2].flags == flags7 && L->checks[0].flags == flags2 && L->checks[1].flags == 0);
    return 0;
}

int spans_group() {
    BatchLayout L;
    const File f({1000, 30000, 30000, 30000, 30000, 500}, 0, 8, 3);
    // entered 123 bytes into its first member, the limit 100 bytes into its last: first and final range in one
    const Span sp = span_of(f, 1, 123, 70000, 120100);
    if (span_piece(f, sp, 0, 5, 0, &L, kSpanOn | kSpanEntry, kSpanOn | kSpanTail)) return 1;
    CHECK(L.segs[0].start == 123 && L.files[0].data_end == 120100 && L.checks[2].beg == 123);
    CHECK(L.checks[0].beg == 70000 && L.checks[0].end == 120100);
    // the same span in three ranges: the middle one is neither first nor final, and starts behind a device carry
    if (span_piece(f, sp, 0, 2, 0, &L, kSpanOn | kSpanEntry, kSpanOn)) return 1;
    CHECK(L.segs[0].start == 123 && L.files[0].data_end == 60000 && L.checks[0].beg == 70000);
    if (span_piece(f, sp, 2, 4, 35, &L, kSpanOn, kSpanOn)) return 1;
    CHECK(L.segs[0].start == 0 && L.segs[0].end == 30035 && L.files[0].data_end == 60035);
    CHECK(L.checks[2].beg == 123 + 35 - 60000 && L.checks[2].beg < 0 && L.checks[0].beg == 70000 + 35 - 60000);
    if (span_piece(f, sp, 4, 5, 20, &L, kSpanOn, kSpanOn | kSpanTail)) return 1;
    CHECK(L.files[0].data_end == 20 + 100 && L.checks[0].end == 120 && L.checks[2].end < 0);
    // no 8 bytes behind the limit: no tail check
    const Span shut = span_of(f, 1, 123, 70000, 120493);
    CHECK(shut.limit + 8 > shut.bytes);
    if (span_piece(f, shut, 0, 5, 0, &L, kSpanOn | kSpanEntry, kSpanOn)) return 1;
    // a span beside a file read in full, the span behind the file's bytes
    const std::vector<uint32_t> chrs{7, 2};
    const File g({4000, 0}, 3, 9, 2);
    BatchPiece p = f.piece(0, 5, true, true, 0);
    p.blocks = &sp.blocks;
    p.span = &sp;
    p.walk = &g.walk;
    if (lay({g.whole(0), p}, {&g, &f}, chrs, false, &L)) return 1;
    CHECK(L.checks[0].flags == 0 && L.checks[1].flags == 0 && L.checks[2].flags == (kSpanOn | kSpanEntry));
    CHECK(L.checks[2].beg == 4016 + 123 && L.segs[2].start == 4016 + 123);
    std::printf("ok spans\n");
    return 0;
}

int index_group() {
    BatchLayout L;
    const File a({700, 4000, 65536, 0}, 0, 3), b({900}, 1, 4), c({1200, 333, 0}, 17, 5);
    BatchPiece pa = a.whole(1), pb = b.whole(1), pc = c.whole(1);
    pa.n_ref = 3, pb.n_ref = 0, pc.n_ref = 25;
    if (lay({pa, pb, pc}, {&a, &b, &c}, {}, true, &L)) return 1;
    CHECK(L.ix_files[0].seg_base == 0 && L.ix_files[1].seg_base == 4 && L.ix_files[2].seg_base == 5);
    CHECK(L.ix_files[0].delta == 700 && pb.lin0 == 900 && pc.lin0 == 1200);
    // a later range of a file that goes alone
    const File late({60000, 60000, 60000, 0}, 9, 7);
    BatchPiece p = late.piece(1, 3, false, false, 35);
    p.n_ref = 2;
    if (lay({p}, {&late}, {}, true, &L)) return 1;
    CHECK(L.ix_files[0].delta == 60000 - 35);
    std::printf("ok index\n");
    return 0;
}

int limits_group() {
    BatchLayout L;
    // a member table alone: kMaxBatchBytes is 65520 members of 64 KiB
    File big({}, 0, 1);
    const auto grow = [&](uint32_t n_members) {
        while (big.m.size() < n_members) {
            big.m.push_back(Block{big.m.size() * 50, big.total, 65536, 18, 24, 0});
            big.total += 65536;
        }
        big.bytes.resize(big.m.size() * 50);
        return big.whole(0);
    };
    const File small({100}, 0, 2);
    BatchPiece p = grow(65519);
    CHECK(lay_out_batch<BatchPiece>({small.whole(0), p}, {}, false, &L) && L.overflow == UINT32_MAX);
    CHECK(L.out_bytes == 112 + big.total && L.out_bytes <= kMaxBatchBytes && L.n_list <= UINT32_MAX);
    p = grow(65520);
    CHECK(big.total == kMaxBatchBytes && lay_out_batch<BatchPiece>({p}, {}, false, &L));
    CHECK(L.out_bytes == kMaxBatchBytes);
    CHECK(!lay_out_batch<BatchPiece>({small.whole(0), p}, {}, false, &L) && L.overflow == 1);
    CHECK(!lay_out_batch<BatchPiece>({small.whole(0), p, small.whole(0)}, {}, false, &L) && L.overflow == 1);
    CHECK(!lay_out_batch<BatchPiece>({p, small.whole(0)}, {}, false, &L) && L.overflow == 1);
    p = grow(65521);
    CHECK(!lay_out_batch<BatchPiece>({p, small.whole(0)}, {}, false, &L) && L.overflow == 0);
    // the lists: an entry per kMinRecord bytes of a segment, rounded up, so their number stays below the bytes' and
    // the u32 limit on it cannot be passed before the limit on the bytes is; a later batch is laid out as ever
    CHECK(lay_out_batch<BatchPiece>({small.whole(0)}, {}, false, &L) && L.overflow == UINT32_MAX && L.n_list == 3);
    std::printf("ok limits\n");
    return 0;
}

// the ranges next_range cuts a list into
std::vector<size_t> cut(const std::vector<Block> &m, uint64_t batch, bool fold, uint64_t total) {
    std::vector<size_t> ends;
    for (size_t b0 = 0; b0 < m.size();) {
        const size_t b1 = fold ? bm::next_range(m, b0, batch, total) : bm::next_range(m, b0, batch);
        if (b1 <= b0 || b1 > m.size()) return {};  // the ranges tile the list: each starts where the last ended
        ends.push_back(b1);
        b0 = b1;
    }
    return ends;
}

int ranges_group() {
    using V = std::vector<size_t>;
    const File f({100, 200, 300, 1000, 50, 50}, 0, 1);
    for (const bool fold : {false, true}) {
        CHECK(cut(f.m, 0, fold, f.total) == (V{1, 2, 3, 4, 5, 6}));   // batch 0: one member per range
        CHECK(cut(f.m, 600, fold, f.total) == (V{3, 4, 6}));          // an exact fit; a member above the batch alone
        CHECK(cut(f.m, 599, fold, f.total) == (V{2, 3, 4, 6}));
        CHECK(cut(f.m, 1u << 20, fold, f.total) == (V{6}));
        CHECK(cut({}, 100, fold, 0).empty());
    }
    CHECK(bm::range_bytes(f.m, 0, 3) == 600 && bm::range_bytes(f.m, 3, 4) == 1000 && bm::range_bytes(f.m, 2, 2) == 0);
    CHECK(bm::range_bytes(f.m, 0, 6) == f.total);
    // a tail of one and of three empty members behind a member above the batch: with the fold it joins that range
    const File t1({100, 200, 400, 0}, 0, 1), t3({100, 200, 400, 0, 0, 0}, 0, 1);
    CHECK(cut(t1.m, 300, true, t1.total) == (V{2, 4}) && cut(t1.m, 300, false, 0) == (V{2, 3, 4}));
    CHECK(cut(t3.m, 300, true, t3.total) == (V{2, 6}) && cut(t3.m, 300, false, 0) == (V{2, 3, 6}));
    CHECK(cut(t3.m, 0, true, t3.total) == (V{1, 2, 6}) && cut(t3.m, 0, false, 0) == (V{1, 2, 3, 6}));
    // an empty member in the middle is no tail
    const File mid({100, 0, 300, 0}, 0, 1);
    CHECK(cut(mid.m, 100, true, mid.total) == (V{2, 4}) && cut(mid.m, 100, false, 0) == (V{2, 3, 4}));
    // only empty members: one range either way, from a later start too
    const File none({0, 0, 0}, 0, 1);
    CHECK(cut(none.m, 0, true, 0) == (V{3}) && bm::next_range(none.m, 1, 0, 0) == 3);
    CHECK(cut(none.m, 0, false, 0) == (V{3}) && cut(none.m, 10, false, 0) == (V{3}));
    std::printf("ok ranges\n");
    return 0;
}

int words_group() {
    // as bam_host.hpp's defect_tail puts them together
    const auto tail = [](uint32_t code) {
        return bw::defect_words(code) + (bw::is_cigar_op(code) ? std::to_string(code & 15) : std::string());
    };
    CHECK(tail(bw::kErrTruncated) == " is truncated");
    CHECK(tail(bw::kErrBlockSize) == " has a bad block_size");
    CHECK(tail(bw::kErrLonger) == " is longer than its block_size");
    CHECK(tail(bw::kErrUnsorted) == ": input is not coordinate-sorted");
    CHECK(tail(bw::kErrNegative) == " has a negative position");
    CHECK(tail(bw::kErrCigarSeq) == ": CIGAR and SEQ lengths differ");
    CHECK(tail(bw::kErrCigarOp | 9) == ": invalid CIGAR op code 9");
    CHECK(tail(bw::kErrCigarOp | 11) == ": invalid CIGAR op code 11");
    CHECK(tail(bw::kErrCigarOp | 15) == ": invalid CIGAR op code 15");
    for (const uint32_t c : {1u, 2u, 3u, 4u, 5u, 0x20u}) CHECK(!bw::is_cigar_op(c));
    const std::vector<uint32_t> ids{5, 0, 9};
    CHECK(slot_of(ids, 5) == 0 && slot_of(ids, 0) == 1 && slot_of(ids, 9) == 2 && slot_of(ids, 1) == 3);
    CHECK(slot_of({}, 0) == 0);
    std::printf("ok words\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc == 2 ? argv[1] : "";
    if (mode == "files") return files_group();
    if (mode == "spans") return spans_group();
    if (mode == "index") return index_group();
    if (mode == "limits") return limits_group();
    if (mode == "ranges") return ranges_group();
    if (mode == "words") return words_group();
    std::fprintf(stderr, "usage: bam_batch_test files | spans | index | limits | ranges | words\n");
    return 2;
}
