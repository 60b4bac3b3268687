// bam_split_select_test -- the selection rules of secedo_amd/csrc/bam_split.hpp on the host, under AddressSanitizer
// and UBSan: marked_byte against a record edited the plain way at every offset of a few hundred random records, alone
// and on top of the read-group edit; the gather's lanes replayed over streams of such records at every residue of the
// record start mod 16 (mark_vector in the lanes wholly inside a record or inside the copied segment in front of the
// hole, plain bytes in all others) against the stream edited the plain way; the mark bit through pack_src for offsets
// up to 2^62; the mask validation. Records live in heap blocks of their exact size. Prints "ok <n> checks" and exits
// 0, or names the first check that failed.
#include "bam_split.hpp"

#include <cstdio>
#include <memory>
#include <random>

using namespace secedo::bamsplit;

namespace {

int g_checks = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

using Bytes = std::vector<uint8_t>;

void put32(Bytes *b, uint32_t v) {
    for (int k = 0; k < 4; ++k) b->push_back(uint8_t(v >> (8 * k)));
}

// a record with random fixed bytes, a name of l_name bytes (NUL included), l_seq bases, an XP:Z field of `pad` bytes
// and, with rg_len >= 0, an RG:Z field with a value of rg_len bytes in front of or behind it
Bytes record(std::mt19937 &rng, uint32_t l_name, uint32_t l_seq, int pad, int rg_len, bool rg_first) {
    Bytes body(32);
    for (uint8_t &b : body) b = uint8_t(rng());
    body[8] = uint8_t(l_name);
    body[12] = 0, body[13] = 0;
    for (int k = 0; k < 4; ++k) body[16 + k] = uint8_t(l_seq >> (8 * k));
    for (uint32_t k = 0; k + 1 < l_name; ++k) body.push_back(uint8_t('a' + rng() % 26));
    body.push_back(0);
    for (uint32_t k = 0; k < (l_seq + 1) / 2 + l_seq; ++k) body.push_back(uint8_t(rng()));
    Bytes xp, rg;
    if (pad >= 0) {
        xp = {'X', 'P', 'Z'};
        xp.insert(xp.end(), size_t(pad), uint8_t('p'));
        xp.push_back(0);
    }
    if (rg_len >= 0) {
        rg = {'R', 'G', 'Z'};
        rg.insert(rg.end(), size_t(rg_len), uint8_t('g'));
        rg.push_back(0);
    }
    const Bytes &a = rg_first ? rg : xp, &b = rg_first ? xp : rg;
    body.insert(body.end(), a.begin(), a.end());
    body.insert(body.end(), b.begin(), b.end());
    Bytes rec;
    put32(&rec, uint32_t(body.size()));
    rec.insert(rec.end(), body.begin(), body.end());
    return rec;
}

Bytes random_record(std::mt19937 &rng) {
    const int pad = int(rng() % 4) == 0 ? -1 : int(rng() % 40);
    const int rg = int(rng() % 3) == 0 ? -1 : int(rng() % 12);
    return record(rng, 1 + rng() % 30, rng() % 60, pad, rg, rng() % 2 == 0);
}

// the plain way: the record with 0x400 set in its FLAG, the u16 at byte 18
Bytes marked_plain(Bytes rec) {
    uint32_t flag = uint32_t(rec[18]) | uint32_t(rec[19]) << 8;
    flag |= 0x400;
    rec[18] = uint8_t(flag), rec[19] = uint8_t(flag >> 8);
    return rec;
}

// the plain way: the record without its hole, the suffix appended, block_size patched
Bytes edited_plain(const Bytes &rec, const AuxHole &h, const Bytes &suffix) {
    Bytes out(rec.begin(), rec.begin() + h.hole_off);
    out.insert(out.end(), rec.begin() + h.hole_off + h.hole_len, rec.end());
    out.insert(out.end(), suffix.begin(), suffix.end());
    const uint32_t bs = uint32_t(out.size()) - 4;
    for (int k = 0; k < 4; ++k) out[k] = uint8_t(bs >> (8 * k));
    return out;
}

int test_bytes() {
    std::mt19937 rng(12);
    const std::string sfx = rg_suffix("cell-7");
    const Bytes suffix(sfx.begin(), sfx.end());
    for (int it = 0; it < 400; ++it) {
        const Bytes rec = random_record(rng);
        std::unique_ptr<uint8_t[]> exact(new uint8_t[rec.size()]);
        std::memcpy(exact.get(), rec.data(), rec.size());
        const Bytes want = marked_plain(rec);
        for (uint32_t o = 0; o < rec.size(); ++o) {
            CHECK(marked_byte(exact[o], o, true) == want[o]);
            CHECK(marked_byte(exact[o], o, false) == rec[o]);
        }
        // on top of the read-group edit: the FLAG lies in front of any hole
        const AuxHole h = aux_walk(exact.get(), uint32_t(rec.size()));
        CHECK(h.parsed && h.hole_off >= kMinRecord);
        const Edit e{uint32_t(rec.size()), h.hole_off, h.hole_len, uint32_t(suffix.size())};
        const Bytes both = marked_plain(edited_plain(rec, h, suffix));
        CHECK(both == edited_plain(marked_plain(rec), h, suffix));  // the two edits commute
        CHECK(both.size() == edited_len(e));
        for (uint32_t o = 0; o < both.size(); ++o)
            CHECK(marked_byte(edited_byte(exact.get(), e, suffix.data(), o), o, true) == both[o]);
        // an incoming mark stays, marked or not
        Bytes had = marked_plain(rec);
        CHECK(marked_byte(had[kDupByte], kDupByte, false) == had[kDupByte]);
        CHECK(marked_byte(had[kDupByte], kDupByte, true) == had[kDupByte]);
    }
    return 0;
}

// The gather's lanes over a stream of records (edited when `suffix` is given), the first record at stream offset
// `lead` behind a filler record: a lane wholly inside a record (and, edited, inside one copied segment) takes its 16
// bytes and mark_vector, every other lane takes bytes without any mark, as the kernels do.
int replay(const std::vector<Bytes> &recs, const std::vector<bool> &marked, const Bytes *suffix) {
    std::vector<Bytes> plain, want;
    std::vector<AuxHole> holes;
    for (size_t k = 0; k < recs.size(); ++k) {
        AuxHole h{uint32_t(recs[k].size()), 0, true};
        if (suffix) h = aux_walk(recs[k].data(), uint32_t(recs[k].size()));
        holes.push_back(h);
        const Bytes p = suffix ? edited_plain(recs[k], h, *suffix) : recs[k];
        plain.push_back(p);
        want.push_back(marked[k] ? marked_plain(p) : p);
    }
    Bytes stream, expect;
    std::vector<uint64_t> dst{0};
    for (size_t k = 0; k < recs.size(); ++k) {
        stream.insert(stream.end(), plain[k].begin(), plain[k].end());
        expect.insert(expect.end(), want[k].begin(), want[k].end());
        dst.push_back(stream.size());
    }
    Bytes got(stream.size(), 0);
    size_t patched = 0;
    for (uint64_t b = 0; b < stream.size(); b += kGatherVec) {
        const uint32_t j = record_of(dst.data(), 0, uint32_t(recs.size()), b);
        const uint64_t r = b - dst[j];
        bool fast = b + kGatherVec <= dst[j + 1];
        if (suffix) {
            const uint32_t kept = uint32_t(recs[j].size()) - holes[j].hole_len;
            const bool before = r >= 4 && r + kGatherVec <= holes[j].hole_off;
            const bool after = r >= holes[j].hole_off && r + kGatherVec <= kept;
            fast = fast && (before || after);
        }
        if (fast) {
            uint32_t v[4];
            for (int i = 0; i < 4; ++i) {
                v[i] = 0;
                for (int q = 0; q < 4; ++q) v[i] |= uint32_t(stream[b + 4 * i + q]) << (8 * q);
            }
            const uint32_t before[4] = {v[0], v[1], v[2], v[3]};
            if (src_marked(pack_src(b, marked[j]))) mark_vector(v, r);
            patched += std::memcmp(before, v, sizeof v) != 0;
            for (int i = 0; i < 4; ++i)
                for (int q = 0; q < 4; ++q) got[b + 4 * i + q] = uint8_t(v[i] >> (8 * q));
        } else {
            for (uint64_t q = b; q < b + kGatherVec && q < stream.size(); ++q) got[q] = stream[q];
        }
    }
    CHECK(got == expect);
    size_t changes = 0;  // marked records whose bit was not set on arrival
    for (size_t k = 0; k < recs.size(); ++k) changes += marked[k] && !(plain[k][kDupByte] & kDupBits);
    CHECK(patched == changes);
    return 0;
}

int test_lanes() {
    std::mt19937 rng(13);
    const std::string sfx = rg_suffix("c");
    const Bytes suffix(sfx.begin(), sfx.end());
    bool residue[2][16] = {};
    for (int it = 0; it < 300; ++it) {
        std::vector<Bytes> recs;
        std::vector<bool> marked;
        // the first record's length moves every later record start over the residues mod 16
        recs.push_back(record(rng, 1 + it % 16, 0, -1, -1, false));
        marked.push_back(it % 2 == 0);
        for (int k = 0; k < 12; ++k) {
            Bytes r = random_record(rng);
            r[kDupByte] &= uint8_t(~kDupBits);  // the bit is off on arrival: every mark is a change
            if (k == 5) r = record(rng, 1, 0, -1, -1, false);  // the shortest record: kMinRecord bytes
            recs.push_back(r);
            marked.push_back(rng() % 2 == 0);
        }
        recs[0][kDupByte] &= uint8_t(~kDupBits);
        CHECK(recs[6].size() == kMinRecord);
        if (replay(recs, marked, nullptr)) return 1;
        if (replay(recs, marked, &suffix)) return 1;
        for (int mode = 0; mode < 2; ++mode) {
            uint64_t at = 0;
            for (size_t k = 0; k < recs.size(); ++k) {
                if (marked[k]) residue[mode][(at + kDupByte) % 16] = true;
                uint64_t len = recs[k].size();
                if (mode) {
                    const AuxHole h = aux_walk(recs[k].data(), uint32_t(len));
                    len = len - h.hole_len + suffix.size();
                }
                at += len;
            }
        }
    }
    for (int mode = 0; mode < 2; ++mode)
        for (int r = 0; r < 16; ++r) CHECK(residue[mode][r]);  // the marked byte stood on every residue
    return 0;
}

int test_packing() {
    for (const uint64_t off : {0ull, 1ull, 19ull, 0xFFFFFFFFull, 1ull << 32, 1ull << 40, (1ull << 40) + 12345, 1ull << 62,
                               (1ull << 63) - 1}) {
        CHECK(src_off(pack_src(off, true)) == off && src_marked(pack_src(off, true)));
        CHECK(src_off(pack_src(off, false)) == off && !src_marked(pack_src(off, false)));
        CHECK(pack_src(off, false) == off);  // without a mark the source offset is as the plain call has it
    }
    return 0;
}

int test_masks() {
    CHECK(masks_fault(0, 0).empty());
    CHECK(masks_fault(0xFFFF, 0).empty() && masks_fault(0, 0xFFFF).empty());
    CHECK(masks_fault(3, 0xF04).empty() && masks_fault(0x1, 0xFFFE).empty());
    CHECK(!masks_fault(0x10000, 0).empty() && !masks_fault(0, 0x10000).empty());
    CHECK(!masks_fault(0xFFFFFFFFull, 0).empty() && !masks_fault(1ull << 40, 0).empty());
    CHECK(!masks_fault(0x400, 0x400).empty() && !masks_fault(0x3, 0x2).empty());
    CHECK(masks_fault(0x400, 0x400).find("share a bit") != std::string::npos);
    CHECK(masks_fault(0x10000, 0x10000).find("0xFFFF") != std::string::npos);  // the range is told first
    return 0;
}

}  // namespace

int main() {
    if (test_bytes() || test_lanes() || test_packing() || test_masks()) return 1;
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
