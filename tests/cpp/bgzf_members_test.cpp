// bgzf_members_test -- secedo_amd/csrc/bgzf_members.hpp on the host, under AddressSanitizer and UBSan.
//   bgzf_members_test list <file>
//       prints "total <inflated bytes>" and "member coff poff clen crc isize out" per member, or "rejected: <why>".
//   bgzf_members_test small | hostile | span | cuts | words | inflate
//       the checks of that group on files the program writes itself (zlib deflates their members); prints "ok ..." and
//       exits 0, or names the line of the first check that failed and exits 1.
// Every listing reads a heap block of the file's exact size, so a read past the bytes is a sanitizer report.
#include "bgzf_members.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace secedo::bgzf_members;
namespace bz = secedo::bgzf;

namespace {

using Bytes = std::vector<uint8_t>;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

void put16(Bytes *b, uint32_t v) { b->push_back(uint8_t(v)), b->push_back(uint8_t(v >> 8)); }
void put32(Bytes *b, uint32_t v) { put16(b, v & 0xFFFF), put16(b, v >> 16); }

Bytes deflate_raw(const Bytes &data) {
    Bytes out(data.size() + data.size() / 8 + 64);
    z_stream z{};
    if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) std::abort();
    uint8_t none = 0;
    z.next_in = data.empty() ? &none : const_cast<Bytef *>(data.data());
    z.avail_in = uInt(data.size());
    z.next_out = out.data();
    z.avail_out = uInt(out.size());
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) std::abort();
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

// one member around the raw DEFLATE of data; lead: another 6-byte subfield in front of BC (XLEN 12, not 6)
Bytes member(const Bytes &data, bool lead = false) {
    const Bytes pay = deflate_raw(data);
    const uint32_t xlen = lead ? 12 : 6;
    Bytes b{31, 139, 8, 4, 0, 0, 0, 0, 0, 255};
    put16(&b, xlen);
    if (lead) b.insert(b.end(), {'X', 'Y', 2, 0, 0xAA, 0xBB});
    b.insert(b.end(), {'B', 'C', 2, 0});
    put16(&b, uint32_t(12 + xlen + pay.size() + 8 - 1));
    b.insert(b.end(), pay.begin(), pay.end());
    put32(&b, uint32_t(crc32(crc32(0, nullptr, 0), data.data(), uInt(data.size()))));
    put32(&b, uint32_t(data.size()));
    return b;
}

const Bytes kEof{0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0,
                 0x03, 0,    0,    0,    0, 0, 0, 0, 0, 0};

Bytes text(size_t n, unsigned seed) {
    Bytes d(n);
    uint64_t state = seed;
    for (size_t k = 0; k < n; ++k) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        d[k] = uint8_t("ACGTN\n"[(state >> 33) % 6]);
    }
    return d;
}

Bytes join(std::initializer_list<Bytes> parts) {
    Bytes out;
    for (const Bytes &p : parts) out.insert(out.end(), p.begin(), p.end());
    return out;
}

// list_members on a copy of exactly n bytes
std::string list_exact(const uint8_t *d, size_t n, std::vector<Member> *members, uint64_t *total) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(exact.get(), d, n);
    members->clear();
    *total = 0;
    return list_members(exact.get(), n, members, total);
}

bool one_of_the_three(const std::string &why) {
    return why.rfind("not a BGZF block at byte ", 0) == 0 || why.rfind("bad BGZF block size at byte ", 0) == 0 ||
           why == "BGZF ISIZE above 64 KiB";
}

bool read_file(const char *path, Bytes *out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + got);
    std::fclose(f);
    return true;
}

int small() {
    std::vector<Member> m;
    uint64_t total = 7;
    CHECK(list_exact(nullptr, 0, &m, &total).empty() && m.empty() && total == 0);
    CHECK(kEof.size() == 28 && member(Bytes()) == kEof);
    CHECK(list_exact(kEof.data(), kEof.size(), &m, &total).empty() && m.size() == 1 && total == 0);
    CHECK(m[0].coff == 0 && m[0].poff == 18 && m[0].clen == 2 && m[0].crc == 0 && m[0].isize == 0 && m[0].out == 0);
    // another subfield in front of BC: the payload starts 6 bytes later
    const Bytes data = text(3000, 1), lead = member(data, true), file = join({lead, member(data), kEof});
    CHECK(list_exact(file.data(), file.size(), &m, &total).empty() && m.size() == 3 && total == 6000);
    CHECK(m[0].poff == 24 && m[0].clen == lead.size() - 24 - 8 && m[0].isize == 3000);
    CHECK(m[1].coff == lead.size() && m[1].poff == 18 && m[1].out == 3000 && m[2].out == 6000 && m[2].isize == 0);
    CHECK(m[0].crc == m[1].crc && m[0].payload() == 24 && m[1].payload() == lead.size() + 18);
    Bytes back(3000);
    CHECK(inflate_member_zlib(file.data() + m[0].payload(), m[0], back.data()).empty() && back == data);
    // an extra field that runs past the file has no BSIZE that can be read
    Bytes past = member(data);
    past[10] = past[11] = 0xFF;
    CHECK(list_exact(past.data(), past.size(), &m, &total) == "bad BGZF block size at byte 0");
    // read_member leaves `out` to the caller and gives the member's length
    Member one;
    uint32_t len = 0;
    CHECK(read_member(file.data(), file.size(), lead.size(), &one, &len).empty());
    CHECK(len == file.size() - lead.size() - 28);
    CHECK(one.coff == lead.size() && one.out == 0 && one.isize == 3000);
    CHECK(read_member(file.data(), file.size(), file.size(), &one, &len) ==
          "not a BGZF block at byte " + std::to_string(file.size()));
    std::printf("ok small\n");
    return 0;
}

int hostile() {
    const Bytes m0 = member(text(2000, 2)), m1 = member(text(1500, 3), true);
    const Bytes file = join({m0, m1, kEof});
    std::vector<Member> m;
    uint64_t total = 0;
    unsigned long listed = 0, refused = 0;
    const auto run = [&](const Bytes &b, size_t n) -> int {
        const std::string why = list_exact(b.data(), n, &m, &total);
        if (why.empty()) {
            uint64_t sum = 0;
            for (const Member &x : m) {
                CHECK(x.payload() + x.clen + 8 <= n && x.poff >= 18 && x.isize <= kBgzfMaxIsize && x.out == sum);
                sum += x.isize;
            }
            CHECK(sum == total);
            ++listed;
        } else {
            CHECK(one_of_the_three(why));
            ++refused;
        }
        return 0;
    };
    for (size_t n = 0; n <= file.size(); ++n) {
        const unsigned long before = listed;
        if (run(file, n)) return 1;
        // a cut is a list exactly where it falls between members
        const bool between = n == 0 || n == m0.size() || n == m0.size() + m1.size() || n == file.size();
        CHECK(between == (listed > before));
    }
    CHECK(listed == 4 && refused == file.size() - 3);
    CHECK(list_exact(file.data(), m0.size() + 1, &m, &total) ==
          "not a BGZF block at byte " + std::to_string(m0.size()));
    for (size_t at = 0; at < 18; ++at)
        for (const uint8_t v : {uint8_t(0x00), uint8_t(0xFF)}) {
            Bytes b = file;
            b[m0.size() + at] = v;
            if (run(b, b.size())) return 1;
        }
    std::printf("ok hostile listed %lu refused %lu\n", listed, refused);
    return 0;
}

// payload_span and fill_desc of members [b0, b1) of a file, under both pairs of bases
int span_case(const Bytes &file, size_t b0, size_t b1, uint64_t want_lo, bool clamped) {
    std::vector<Member> m;
    uint64_t total = 0;
    CHECK(list_exact(file.data(), file.size(), &m, &total).empty() && b0 < b1 && b1 <= m.size());
    const PayloadSpan sp = payload_span(m, b0, b1, file.size());
    const uint64_t pay_end = m[b1 - 1].payload() + m[b1 - 1].clen;
    CHECK(sp.lo >= 2 && sp.lo == want_lo && sp.lo == m[b0].payload() - 16 && sp.needed == pay_end + 16 - sp.lo);
    CHECK(sp.hi <= file.size() && sp.hi == (clamped ? file.size() : pay_end + 16) && sp.hi - sp.lo <= sp.needed);
    for (const uint64_t base : {uint64_t(0), uint64_t(4099)}) {
        const uint64_t in_base = base, out_base = base ? base * 3 + 1 : 0;
        Bytes dev(in_base + sp.needed, 0xEE);  // the device input as the routes fill it
        std::memcpy(dev.data() + in_base, file.data() + sp.lo, sp.hi - sp.lo);
        std::vector<BgzfDesc> desc(b1 - b0);
        fill_desc(m, b0, b1, sp.lo, in_base, out_base, desc.data());
        uint64_t out = out_base;
        for (size_t k = 0; k < desc.size(); ++k) {
            const BgzfDesc &d = desc[k];
            const Member &x = m[b0 + k];
            CHECK(d.in_off >= in_base + 16 && d.in_off + d.clen + 16 <= in_base + sp.needed);
            CHECK(d.clen == x.clen && d.isize == x.isize && d.crc == x.crc && d.reserved == 0);
            CHECK(std::memcmp(dev.data() + d.in_off, file.data() + x.payload(), x.clen) == 0);
            CHECK(d.out_off == out);  // one behind the other: no gap, no overlap
            out += d.isize;
        }
        CHECK(out == out_base + (b1 < m.size() ? m[b1].out : total) - m[b0].out);
    }
    return 0;
}

int span() {
    const Bytes a = member(text(5000, 4)), b = member(text(4000, 5)), c = member(text(10, 6));
    // no EOF member: the last payload ends 8 bytes (CRC32, ISIZE) before the file does, and hi stops at the file's end
    const Bytes open_end = join({a, b, c});
    if (span_case(open_end, 0, 3, 2, true)) return 1;
    const Bytes closed = join({a, b, c, kEof});
    if (span_case(closed, 0, 2, 2, false)) return 1;                    // from member 0: lo is 18 - 16
    if (span_case(closed, 1, 3, a.size() + 2, false)) return 1;         // a middle range
    if (span_case(closed, 2, 3, a.size() + b.size() + 2, false)) return 1;
    if (span_case(closed, 0, 4, 2, true)) return 1;                     // to the EOF member: 8 + 16 > what is left
    if (span_case(kEof, 0, 1, 2, true)) return 1;                       // one empty member
    if (span_case(join({member(text(700, 7), true), kEof}), 0, 1, 8, false)) return 1;  // XLEN 12
    std::printf("ok span\n");
    return 0;
}

// the writers' cut rule: the members of an extent, one every kCut bytes from its start
int cuts() {
    using bz::kCut;
    const uint64_t base = 12345;  // an extent need not start at 0: cuts count from its start
    const uint64_t sizes[] = {0, 1, kCut - 1, kCut, kCut + 1, 3ull * kCut};
    const size_t want[] = {0, 1, 1, 1, 2, 3};
    for (size_t i = 0; i < 6; ++i) {
        std::vector<bz::DeflateDesc> desc;
        bz::member_cuts(base, base + sizes[i], &desc);
        CHECK(desc.size() == want[i]);
        uint64_t at = base;
        for (size_t k = 0; k < desc.size(); ++k) {
            CHECK(desc[k].in_off == at && desc[k].n >= 1 && desc[k].n <= kCut && desc[k].reserved == 0);
            CHECK(k + 1 == desc.size() || desc[k].n == kCut);  // every member but the last is full
            at += desc[k].n;
        }
        CHECK(at == base + sizes[i]);
    }
    std::vector<bz::DeflateDesc> desc;
    bz::member_cuts(0, kCut + 1, &desc);
    CHECK(desc[1].in_off == kCut && desc[1].n == 1);
    bz::member_cuts(7, 7, &desc);  // appends nothing
    CHECK(desc.size() == 2);
    bz::member_cuts(7, 8, &desc);  // appends behind what is there
    CHECK(desc.size() == 3 && desc[2].in_off == 7 && desc[2].n == 1);
    std::printf("ok cuts\n");
    return 0;
}

int words() {
    for (uint32_t s = 0; s < bz::kStatusCodes; ++s)
        CHECK(std::string(status_text(s)) ==
              (s == bz::kCrcMismatch ? "CRC32 mismatch" : "inflate failed or ISIZE mismatch"));
    CHECK(block_where(0) == "BGZF block 0" && block_where(4294967296ull) == "BGZF block 4294967296");
    CHECK(block_where_byte(65536) == "BGZF block at byte 65536");
    const uint32_t ok[5] = {0, 0, 0, 0, 0}, head[5] = {bz::kInputEnd, 0, 0, 0, bz::kCrcMismatch};
    const uint32_t tail[5] = {0, 0, 0, 0, bz::kCrcMismatch};
    const uint32_t two[5] = {0, 0, bz::kBadDist, bz::kCrcMismatch, 0};
    CHECK(first_bad(nullptr, 0) == 0 && first_bad(ok, 0) == 0 && first_bad(ok, 5) == 5 && first_bad(ok, 1) == 1);
    CHECK(first_bad(head, 5) == 0 && first_bad(tail, 5) == 4 && first_bad(tail, 4) == 4 && first_bad(two, 5) == 2);
    std::printf("ok words\n");
    return 0;
}

int inflate_cases() {
    const Bytes data = text(20000, 8), file = member(data);
    std::vector<Member> m;
    uint64_t total = 0;
    CHECK(list_exact(file.data(), file.size(), &m, &total).empty() && m.size() == 1);
    const std::string size_words = "inflate failed or ISIZE mismatch", crc_words = "CRC32 mismatch";
    // the payload from a heap block of its exact size, the output into one of ISIZE bytes
    const auto run = [&](const Bytes &f, const Member &x, Bytes *out) {
        std::unique_ptr<uint8_t[]> pay(new uint8_t[x.clen ? x.clen : 1]);
        std::memcpy(pay.get(), f.data() + x.payload(), x.clen);
        out->assign(x.isize, 0);
        return inflate_member_zlib(pay.get(), x, x.isize ? out->data() : nullptr);
    };
    Bytes out;
    CHECK(run(file, m[0], &out).empty() && out == data);
    unsigned long by_size = 0, by_crc = 0;
    for (size_t bit = 0; bit < 8 * size_t(m[0].clen); bit += 37) {  // a flipped payload bit: one sentence or the other
        Bytes f = file;
        f[m[0].payload() + bit / 8] ^= uint8_t(1u << (bit % 8));
        const std::string why = run(f, m[0], &out);
        CHECK(why == size_words || why == crc_words);
        (why == size_words ? by_size : by_crc)++;
    }
    CHECK(by_size > 0 && by_crc > 0);
    Member x = m[0];
    x.crc ^= 1;
    CHECK(run(file, x, &out) == crc_words);
    for (const uint32_t isize : {m[0].isize - 1, m[0].isize + 1, 0u}) {
        x = m[0];
        x.isize = isize;
        CHECK(run(file, x, &out) == size_words);
    }
    x = m[0];
    x.clen -= 1;  // the stream ends before its end-of-block
    CHECK(run(file, x, &out) == size_words);
    CHECK(list_exact(kEof.data(), kEof.size(), &m, &total).empty() && run(kEof, m[0], &out).empty());
    std::printf("ok inflate flips %lu %lu\n", by_size, by_crc);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "list" && argc == 3) {
        Bytes file;
        if (!read_file(argv[2], &file)) return 2;
        std::vector<Member> m;
        uint64_t total = 0;
        const std::string why = list_exact(file.data(), file.size(), &m, &total);
        if (!why.empty()) {
            std::printf("rejected: %s\n", why.c_str());
            return 0;
        }
        std::printf("total %llu\n", (unsigned long long)total);
        for (const Member &x : m)
            std::printf("member %llu %u %u %u %u %llu\n", (unsigned long long)x.coff, x.poff, x.clen, x.crc, x.isize,
                        (unsigned long long)x.out);
        return 0;
    }
    if (argc == 2 && mode == "small") return small();
    if (argc == 2 && mode == "hostile") return hostile();
    if (argc == 2 && mode == "span") return span();
    if (argc == 2 && mode == "cuts") return cuts();
    if (argc == 2 && mode == "words") return words();
    if (argc == 2 && mode == "inflate") return inflate_cases();
    std::fprintf(stderr, "usage: bgzf_members_test list <file> | small | hostile | span | cuts | words | inflate\n");
    return 2;
}
