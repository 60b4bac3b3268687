// bam_split_rg_test -- the read-group rules of secedo_amd/csrc/bam_split.hpp on the host, under AddressSanitizer and
// UBSan: the strict aux walk on every type and every failure, edited_byte against an edited record built the plain
// way for every offset of a few hundred random records, the name rules, the default names and the @RG header lines.
// Records and suffixes live in heap blocks of their exact size, so a read past them is a sanitizer report. Prints
// "ok <n> checks" and exits 0, or names the first check that failed.
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

Bytes field(const char *tag, char type, const Bytes &value) {
    Bytes f{uint8_t(tag[0]), uint8_t(tag[1]), uint8_t(type)};
    f.insert(f.end(), value.begin(), value.end());
    return f;
}

Bytes text(const std::string &s) {  // a Z or H value with its NUL
    Bytes b(s.begin(), s.end());
    b.push_back(0);
    return b;
}

Bytes array(char sub, uint32_t count, uint32_t elem) {
    Bytes b{uint8_t(sub)};
    put32(&b, count);
    for (uint32_t k = 0; k < count * elem; ++k) b.push_back(uint8_t("RGZ"[k % 3]));  // the bytes R G Z mean nothing
    return b;
}

// a record with a name of l_name bytes (NUL included), n_cigar operations, l_seq bases and the aux bytes
Bytes record(uint32_t l_name, uint32_t n_cigar, uint32_t l_seq, const Bytes &aux) {
    Bytes body(32, 0);
    body[8] = uint8_t(l_name);
    body[12] = uint8_t(n_cigar), body[13] = uint8_t(n_cigar >> 8);
    for (int k = 0; k < 4; ++k) body[16 + k] = uint8_t(l_seq >> (8 * k));
    for (uint32_t k = 0; k + 1 < l_name; ++k) body.push_back('n');
    body.push_back(0);
    body.resize(body.size() + 4 * n_cigar + (l_seq + 1) / 2 + l_seq, 'R');  // RG bytes in front of the aux area too
    body.insert(body.end(), aux.begin(), aux.end());
    Bytes rec;
    put32(&rec, uint32_t(body.size()));
    rec.insert(rec.end(), body.begin(), body.end());
    return rec;
}

// the walk over a heap block of the record's exact size
AuxHole walk(const Bytes &rec) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[rec.size()]);
    std::memcpy(exact.get(), rec.data(), rec.size());
    return aux_walk(exact.get(), uint32_t(rec.size()));
}

Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes out;
    for (const Bytes &p : parts) out.insert(out.end(), p.begin(), p.end());
    return out;
}

int test_walk() {
    const uint32_t aux0 = 36 + 5 + 8 + 4 + 7;  // record(5, 2, 7, ...)
    // no aux area
    AuxHole h = walk(record(5, 2, 7, {}));
    CHECK(h.parsed && h.hole_len == 0 && h.hole_off == aux0);
    // every type, no RG
    const Bytes all = cat({field("XA", 'A', {'x'}), field("Xc", 'c', {1}), field("XC", 'C', {2}),
                           field("Xs", 's', {1, 2}), field("XS", 'S', {1, 2}), field("Xi", 'i', {1, 2, 3, 4}),
                           field("XI", 'I', {1, 2, 3, 4}), field("Xf", 'f', {1, 2, 3, 4}), field("XZ", 'Z', text("RGZx")),
                           field("XH", 'H', text("1AE3")), field("Bc", 'B', array('c', 3, 1)),
                           field("BC", 'B', array('C', 6, 1)), field("Bs", 'B', array('s', 3, 2)),
                           field("BS", 'B', array('S', 0, 2)), field("Bi", 'B', array('i', 2, 4)),
                           field("BI", 'B', array('I', 1, 4)), field("Bf", 'B', array('f', 3, 4))});
    Bytes rec = record(5, 2, 7, all);
    h = walk(rec);
    CHECK(h.parsed && h.hole_len == 0 && h.hole_off == rec.size());
    // RG first, in the middle and last; whatever its type; the first of two
    const Bytes rgz = field("RG", 'Z', text("group")), rgi = field("RG", 'i', {7, 0, 0, 0});
    const Bytes rgb = field("RG", 'B', array('S', 5, 2));
    h = walk(record(5, 2, 7, cat({rgz, all})));
    CHECK(h.parsed && h.hole_off == aux0 && h.hole_len == rgz.size());
    h = walk(record(1, 0, 0, cat({all, rgi, all})));
    CHECK(h.parsed && h.hole_off == 37 + all.size() && h.hole_len == 7);
    h = walk(record(5, 2, 7, cat({all, rgb})));
    CHECK(h.parsed && h.hole_off == aux0 + all.size() && h.hole_len == rgb.size() && rgb.size() == 3 + 5 + 10);
    h = walk(record(5, 2, 7, cat({all, rgz, rgi})));
    CHECK(h.parsed && h.hole_off == aux0 + all.size() && h.hole_len == rgz.size());
    // a long B array is skipped by its count
    h = walk(record(9, 1, 100, cat({field("ML", 'B', array('C', 70000, 1)), rgz})));
    CHECK(h.parsed && h.hole_len == rgz.size());

    // the failures: nothing is removed, hole_off is the record's length
    const auto fails = [](const Bytes &r) {
        const AuxHole f = walk(r);
        return !f.parsed && f.hole_len == 0 && f.hole_off == r.size();
    };
    CHECK(fails(record(5, 2, 7, cat({rgz, field("XQ", '?', {1, 2, 3})}))));  // an unknown type
    CHECK(fails(record(5, 2, 7, cat({rgz, field("XB", 'B', array('Z', 1, 1))}))));  // an unknown subtype
    CHECK(fails(record(5, 2, 7, cat({rgz, field("XB", 'B', array('A', 1, 1))}))));
    CHECK(fails(record(5, 2, 7, cat({rgz, {'X', 'Y'}}))));       // two bytes left
    CHECK(fails(record(5, 2, 7, cat({rgz, {'X'}}))));            // one byte left
    CHECK(fails(record(5, 2, 7, cat({rgz, field("Xi", 'i', {1, 2, 3})}))));  // a value past the end
    CHECK(fails(record(5, 2, 7, cat({rgz, field("XS", 'S', {1})}))));
    CHECK(fails(record(5, 2, 7, cat({rgz, field("XA", 'A', {})}))));
    Bytes open_z = field("XZ", 'Z', text("no-nul"));
    open_z.pop_back();
    CHECK(fails(record(5, 2, 7, cat({rgz, open_z}))));           // a Z value without its NUL
    Bytes short_b = field("XB", 'B', array('i', 3, 4));
    short_b.pop_back();
    CHECK(fails(record(5, 2, 7, cat({rgz, short_b}))));          // an array past the end
    CHECK(fails(record(5, 2, 7, cat({rgz, {'X', 'B', 'B', 'C', 1, 0}}))));  // no room for the count
    Bytes huge = field("XB", 'B', {'i', 0xFF, 0xFF, 0xFF, 0xFF});
    CHECK(fails(record(5, 2, 7, cat({rgz, huge}))));             // count * size does not wrap
    // the fixed part alone runs past the record
    Bytes cut = record(5, 2, 7, {});
    cut[20] = 200;  // l_seq
    CHECK(fails(cut));
    CHECK(!walk(Bytes(20, 0)).parsed);
    return 0;
}

int test_edited_byte() {
    std::mt19937 rng(12);
    const auto pick = [&](uint32_t n) { return uint32_t(rng() % n); };
    uint32_t holes = 0, unparsed = 0, shrunk = 0;
    for (int t = 0; t < 300; ++t) {
        Bytes aux;
        const uint32_t n_fields = pick(5);
        const uint32_t rg_at = pick(7);  // past n_fields: none
        for (uint32_t f = 0; f < n_fields; ++f) {
            const char *tag = f == rg_at ? "RG" : "XY";
            Bytes one;
            switch (pick(5)) {
                case 0: one = field(tag, 'Z', text(std::string(pick(40), 'z'))); break;
                case 1: one = field(tag, 'i', {1, 2, 3, 4}); break;
                case 2: one = field(tag, 'B', array('S', pick(9), 2)); break;
                case 3: one = field(tag, 'A', {'a'}); break;
                default: one = field(tag, 'H', text("00FF")); break;
            }
            aux.insert(aux.end(), one.begin(), one.end());
        }
        if (t % 10 == 9) aux.insert(aux.end(), {'X', 'Q', '!', 1});  // does not parse
        const Bytes rec = record(1 + pick(30), pick(4), pick(60), aux);
        const std::string suffix = rg_suffix(std::string(1 + pick(t % 3 ? 20 : 254), 'N'));
        const AuxHole h = walk(rec);
        holes += h.hole_len != 0, unparsed += !h.parsed;
        // the edited record, built the plain way
        Bytes want(rec.begin() + 4, rec.begin() + h.hole_off);
        want.insert(want.end(), rec.begin() + h.hole_off + h.hole_len, rec.end());
        want.insert(want.end(), suffix.begin(), suffix.end());
        Bytes whole;
        put32(&whole, uint32_t(want.size()));
        whole.insert(whole.end(), want.begin(), want.end());
        shrunk += whole.size() < rec.size();

        std::unique_ptr<uint8_t[]> r(new uint8_t[rec.size()]), s(new uint8_t[suffix.size()]);
        std::memcpy(r.get(), rec.data(), rec.size());
        std::memcpy(s.get(), suffix.data(), suffix.size());
        const Edit e{uint32_t(rec.size()), h.hole_off, h.hole_len, uint32_t(suffix.size())};
        CHECK(edited_len(e) == whole.size());
        bool same = true;
        for (uint32_t o = 0; o < whole.size(); ++o) same = same && edited_byte(r.get(), e, s.get(), o) == whole[o];
        CHECK(same);
    }
    CHECK(holes > 50 && unparsed == 30 && shrunk > 5);
    return 0;
}

int test_names() {
    CHECK(rg_suffix("ab") == std::string("RGZab\0", 6));
    CHECK(name_fault("a").empty() && name_fault(std::string(254, '~')).empty() && name_fault("!x~").empty());
    CHECK(!name_fault("").empty() && !name_fault(std::string(255, 'a')).empty());
    CHECK(!name_fault("a\tb").empty() && !name_fault("a b").empty() && !name_fault("a\x7f").empty());
    CHECK(!name_fault("\xc3\xa9").empty() && !name_fault(std::string("a\0b", 3)).empty());
    CHECK(names_fault({"a", "b", "ab"}).empty());
    CHECK(names_fault({"a", "b", ""}) == "the name of cell 2 is empty");
    CHECK(names_fault({"a", "b\tc", ""}).find("the name of cell 1 has byte 9 at offset 1") == 0);
    CHECK(names_fault({std::string(255, 'a')}).find("the name of cell 0 is 255 bytes long") == 0);
    CHECK(names_fault({"x", "a", "b", "a", "x"}) == "cells 1 and 3 share the name a");

    CHECK(default_name("/data/run/cell1.bam") == "cell1" && default_name("cell1.sam") == "cell1");
    CHECK(default_name("dir.bam/cell1.sam.gz") == "cell1" && default_name("cell1.bam.sam") == "cell1.bam");
    CHECK(default_name("cell1.gz") == "cell1.gz" && default_name("a/b/.bam") == "" && default_name("x.sam.gz.bam") == "x.sam.gz");
    CHECK(names_fault({default_name("a/cell1.bam"), default_name("b/cell1.bam")}) == "cells 0 and 1 share the name cell1");
    return 0;
}

int test_header() {
    const std::vector<std::string> names{"n0", "n1", "n2", "n3"};
    const std::vector<uint16_t> cluster{2, 0, 2, 0};
    CHECK((rg_header_lines(names, cluster, 2) ==
           std::vector<std::string>{"@RG\tID:n0\tSM:cluster_2", "@RG\tID:n2\tSM:cluster_2"}));
    CHECK(rg_header_lines(names, cluster, 1).empty());
    const std::vector<Ref> refs{{"chr1", 1000}};
    CHECK(header_text(refs, rg_header_lines(names, cluster, 0), 0, 2, 4) ==
          "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:1000\n@RG\tID:n1\tSM:cluster_0\n@RG\tID:n3\tSM:cluster_0\n"
          "@PG\tID:secedo_amd.split\tPN:secedo_amd\n@CO\tsecedo_amd cluster 0: 2 of 4 cells\n");
    return 0;
}

}  // namespace

int main() {
    if (test_walk() || test_edited_byte() || test_names() || test_header()) return 1;
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
