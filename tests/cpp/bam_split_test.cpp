// bam_split_test -- secedo_amd/csrc/bam_split.hpp on the host, under AddressSanitizer and UBSan: the header text
// (@RG merge, the ID clash, a reference-list mismatch), the key and the lookup from an output byte to its record (the
// member cuts of an extent are checked with their home, in bgzf_members_test.cpp). Arrays the lookup and the parsers read live in heap blocks of their exact size, so a read
// past them is a sanitizer report. Prints "ok <n> checks" and exits 0, or names the first check that failed.
#include "bam_split.hpp"

#include <cstdio>
#include <memory>

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

int test_header() {
    const std::vector<Ref> refs{{"chr1", 1000}, {"chr2", 2000}};
    // the binary list and back, from a heap block of its exact size
    const std::vector<uint8_t> list = ref_list_bytes(refs);
    CHECK(list.size() == 2 * (4 + 5 + 4));
    std::unique_ptr<uint8_t[]> exact(new uint8_t[list.size()]);
    std::memcpy(exact.get(), list.data(), list.size());
    std::vector<Ref> back;
    CHECK(parse_ref_list(exact.get(), list.size(), 2, &back));
    CHECK(back == refs);
    back.clear();
    CHECK(!parse_ref_list(exact.get(), list.size() - 1, 2, &back));  // cut short
    back.clear();
    CHECK(!parse_ref_list(exact.get(), list.size(), 3, &back));

    // a SAM header's @SQ lines give the same list; other lines, field order and a trailing NUL do not matter
    const std::string text = std::string("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:1000\n@SQ\tLN:2000\tSN:chr2\tM5:x\n") +
                             "@RG\tID:a\tSM:s1\n@PG\tID:bwa\n@CO\tSQ\tSN:no\n" + std::string(1, '\0');
    CHECK(refs_from_text(text) == refs);
    CHECK(refs_differ(refs, refs).empty());

    // a reference-list mismatch: the count, a name, a length
    std::vector<Ref> other = refs;
    other.pop_back();
    CHECK(refs_differ(refs, other) == "1 references, the first file has 2");
    other = refs;
    other[1].name = "chrX";
    CHECK(refs_differ(refs, other) == "reference 1 is chrX of length 2000, in the first file chr2 of length 2000");
    other = refs;
    other[0].len = 999;
    CHECK(refs_differ(refs, other) == "reference 0 is chr1 of length 999, in the first file chr1 of length 1000");

    // the @RG merge: whole lines, first appearance, files in list order
    const std::vector<std::string> texts{
        "@HD\tVN:1.6\n@RG\tID:b\tSM:x\n@RG\tID:a\tSM:x\n@PG\tID:p\n",
        "@RG\tID:a\tSM:x\n@RG\tID:c\tSM:y\r\n@CO\t@RG\tID:zz\n",
        "",
        "@RG\tID:b\tSM:x\n",
    };
    RgMerge rg;
    size_t a = 9, b = 9;
    std::string id;
    CHECK(merge_rg(texts, &rg, &a, &b, &id));
    CHECK(rg.lines == (std::vector<std::string>{"@RG\tID:b\tSM:x", "@RG\tID:a\tSM:x", "@RG\tID:c\tSM:y"}));
    CHECK(rg.file == (std::vector<size_t>{0, 0, 1}));
    // the ID clash: the same ID on a different line
    std::vector<std::string> clash = texts;
    clash.push_back("@RG\tID:c\tSM:other\n");
    RgMerge rg2;
    CHECK(!merge_rg(clash, &rg2, &a, &b, &id));
    CHECK(a == 1 && b == 4 && id == "c");

    // the text and the bytes
    const std::string t = header_text(refs, rg.lines, 3, 2, 12);
    CHECK(t == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:2000\n@RG\tID:b\tSM:x\n"
               "@RG\tID:a\tSM:x\n@RG\tID:c\tSM:y\n@PG\tID:secedo_amd.split\tPN:secedo_amd\n"
               "@CO\tsecedo_amd cluster 3: 2 of 12 cells\n");
    const std::vector<uint8_t> h = header_bytes(t, 2, list);
    CHECK(h.size() == 4 + 4 + t.size() + 4 + list.size());
    CHECK(std::memcmp(h.data(), "BAM\1", 4) == 0 && rd32(h.data() + 4) == t.size());
    CHECK(std::memcmp(h.data() + 8, t.data(), t.size()) == 0 && rd32(h.data() + 8 + t.size()) == 2);
    CHECK(std::memcmp(h.data() + 12 + t.size(), list.data(), list.size()) == 0);
    CHECK(header_text({}, {}, 0, 0, 1) == "@HD\tVN:1.6\tSO:coordinate\n@PG\tID:secedo_amd.split\tPN:secedo_amd\n"
                                          "@CO\tsecedo_amd cluster 0: 0 of 1 cells\n");
    return 0;
}

int test_key() {
    const uint32_t clusters[] = {0, 1, 2, 255, 256, 65535};
    const uint32_t positions[] = {0, 1, 999999, 0x7FFFFFFF, 0xFFFFFFFFu};
    for (uint32_t c : clusters)
        for (uint32_t p : positions) {
            const uint64_t k = pack_key(c, p);
            CHECK(key_cluster(k) == c && key_pos(k) == p);
        }
    // the order of keys is (cluster, Position)
    CHECK(pack_key(0, 0xFFFFFFFFu) < pack_key(1, 0));
    CHECK(pack_key(2, 5) < pack_key(2, 6));
    // the sort's end bit covers every key in use and no more
    CHECK(key_bits(0) == 32 && key_bits(1) == 33 && key_bits(2) == 34 && key_bits(3) == 34 && key_bits(4) == 35);
    CHECK(key_bits(65535) == 48);
    for (uint32_t c : clusters) CHECK(pack_key(c, 0xFFFFFFFFu) >> key_bits(c) == 0);
    return 0;
}

int test_lookup() {
    // records of 40, 37, 70000 and 41 bytes; dst has n + 1 entries, in a heap block of its exact size
    const uint64_t len[] = {40, 37, 70000, 41};
    const uint32_t n = 4;
    std::unique_ptr<uint64_t[]> dst(new uint64_t[n + 1]);
    dst[0] = 0;
    for (uint32_t j = 0; j < n; ++j) dst[j + 1] = dst[j] + len[j];
    for (uint32_t j = 0; j < n; ++j) {
        CHECK(record_of(dst.get(), 0, n, dst[j]) == j);          // its first byte
        CHECK(record_of(dst.get(), 0, n, dst[j + 1] - 1) == j);  // its last byte
        CHECK(record_of(dst.get(), j, n, dst[j]) == j);          // a range that starts at it
        CHECK(record_of(dst.get(), j, j + 1, dst[j + 1] - 1) == j);
    }
    // the bounded range of a tile: from the record of the tile's first byte, kTileRecords on
    for (uint64_t tile = 0; tile < dst[n]; tile += kTileBytes) {
        const uint32_t lo = record_of(dst.get(), 0, n, tile);
        const uint32_t hi = lo + kTileRecords < n ? lo + kTileRecords : n;
        for (uint64_t b = tile; b < tile + kTileBytes && b < dst[n]; b += kGatherVec)
            CHECK(record_of(dst.get(), lo, hi, b) == record_of(dst.get(), 0, n, b));
    }
    // a tile full of the shortest records stays inside the bound
    {
        const uint32_t m = 2 * kTileRecords;
        std::unique_ptr<uint64_t[]> d(new uint64_t[m + 1]);
        for (uint32_t j = 0; j <= m; ++j) d[j] = uint64_t(j) * kMinRecord;
        for (uint64_t tile = 0; tile < d[m]; tile += kTileBytes) {
            const uint32_t lo = record_of(d.get(), 0, m, tile);
            const uint32_t hi = lo + kTileRecords < m ? lo + kTileRecords : m;
            for (uint64_t b = tile; b < tile + kTileBytes && b < d[m]; ++b)
                CHECK(record_of(d.get(), lo, hi, b) == uint32_t(b / kMinRecord));
        }
    }
    // zero-length gaps: equal entries are skipped over, the last of them holds the byte
    {
        std::unique_ptr<uint64_t[]> d(new uint64_t[7]{0, 0, 50, 50, 50, 90, 90});
        CHECK(record_of(d.get(), 0, 6, 0) == 1);
        CHECK(record_of(d.get(), 0, 6, 49) == 1);
        CHECK(record_of(d.get(), 0, 6, 50) == 4);
        CHECK(record_of(d.get(), 0, 6, 89) == 4);
        CHECK(record_of(d.get(), 2, 6, 50) == 4);
    }
    // one record
    {
        std::unique_ptr<uint64_t[]> d(new uint64_t[2]{0, 37});
        CHECK(record_of(d.get(), 0, 1, 0) == 0 && record_of(d.get(), 0, 1, 36) == 0);
    }
    return 0;
}

}  // namespace

int main() {
    if (test_header() || test_key() || test_lookup()) return 1;
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
