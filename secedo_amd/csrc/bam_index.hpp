// bam_index.hpp -- the BAI index reader (SAM spec 5.2), header-only, in plain host C++ that g++ compiles alone
// (tests/cpp/bam_index_test.cpp runs it under the sanitizers; bam_input.cpp plans the spans of a file from it).
//
// Of an index only three numbers per reference are used: where its records start (the minimum chunk_beg over its bins
// other than the pseudo-bin 37450), where they end (the maximum chunk_end over the same bins) and, where the pseudo-bin
// is present (samtools writes it, BamTools does not), its n_mapped + n_unmapped. The linear index is skipped. Every
// length is checked against the bytes left before it is used, and nothing is allocated from a count that was not.
// A virtual offset is coffset << 16 | uoffset: the byte of a BGZF member in the file and a byte of its inflated data.
#pragma once

#include "bgzf_members.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace secedo {
namespace bamindex {

constexpr uint32_t kPseudoBin = 37450;
constexpr uint64_t kNoCount = UINT64_MAX;

struct RefRange {
    uint64_t beg = 0, end = 0;  // virtual offsets; a reference without bins is empty: beg == end == 0
    uint64_t count = kNoCount;  // records of the reference (the pseudo-bin), or kNoCount
    bool empty() const { return beg == 0 && end == 0; }
};

inline uint64_t coffset(uint64_t v) { return v >> 16; }
inline uint32_t uoffset(uint64_t v) { return uint32_t(v & 0xFFFF); }

inline std::string voffset_str(uint64_t v) { return std::to_string(coffset(v)) + ":" + std::to_string(uoffset(v)); }

namespace detail {
inline uint32_t rd32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint64_t rd64(const uint8_t *p) { uint64_t v; std::memcpy(&v, p, 8); return v; }
}  // namespace detail

// The index in d[0, n): one RefRange per reference. Empty on success, else why the bytes are no index.
inline std::string parse(const uint8_t *d, uint64_t n, std::vector<RefRange> *out) {
    using namespace detail;
    out->clear();
    if (n < 8 || std::memcmp(d, "BAI\1", 4) != 0) return "not a BAI index (magic)";
    const uint32_t n_ref = rd32(d + 4);
    uint64_t o = 8;
    // a reference takes 8 bytes or more (n_bin, n_intv)
    if (n_ref > (n - o) / 8) return "truncated index (n_ref)";
    for (uint32_t r = 0; r < n_ref; ++r) {
        if (n - o < 4) return "truncated index (n_bin)";
        const uint32_t n_bin = rd32(d + o);
        o += 4;
        RefRange rr;
        bool any = false;
        for (uint32_t b = 0; b < n_bin; ++b) {
            if (n - o < 8) return "truncated index (bin)";
            const uint32_t bin = rd32(d + o), n_chunk = rd32(d + o + 4);
            o += 8;
            if (n_chunk > (n - o) / 16) return "truncated index (chunks)";
            if (bin == kPseudoBin) {
                if (n_chunk >= 2) {
                    const uint64_t mapped = rd64(d + o + 16), unmapped = rd64(d + o + 24);
                    if (unmapped > kNoCount - 1 || mapped > kNoCount - 1 - unmapped) return "pseudo-bin counts overflow";
                    rr.count = mapped + unmapped;
                }
            } else {
                for (uint32_t c = 0; c < n_chunk; ++c) {
                    const uint64_t beg = rd64(d + o + 16ull * c), end = rd64(d + o + 16ull * c + 8);
                    if (!any || beg < rr.beg) rr.beg = beg;
                    if (!any || end > rr.end) rr.end = end;
                    any = true;
                }
            }
            o += 16ull * n_chunk;
        }
        if (n - o < 4) return "truncated index (n_intv)";
        const uint32_t n_intv = rd32(d + o);
        o += 4;
        if (n_intv > (n - o) / 8) return "truncated index (linear index)";
        o += 8ull * n_intv;
        if (any && rr.beg > rr.end) return "a reference starts behind its end";
        if (any && rr.beg == 0 && rr.end == 0) any = false;
        if (!any) rr.beg = rr.end = 0;
        out->push_back(rr);
    }
    return std::string();  // n_no_coor may follow
}

// a BGZF member stands at byte off of p[0, n) (bgzf_members.hpp holds the one parse of a member's header)
inline bool member_at(const uint8_t *p, uint64_t n, uint64_t off, uint32_t *len, uint32_t *isize) {
    uint32_t xlen = 0;
    return bgzf_members::member_header(p, n, off, len, isize, &xlen) == bgzf_members::kMember;
}

// The file-level checks of parsed ranges against the BAM they are said to index: n_ref, and for the start and the end
// of every reference (the two virtual offsets that are used; a bin's other chunks are never followed) a BGZF member at
// its coffset whose ISIZE covers its uoffset. Empty when they hold.
inline std::string check(const std::vector<RefRange> &refs, uint32_t bam_n_ref, const uint8_t *bam, uint64_t bam_bytes) {
    if (refs.size() != bam_n_ref)
        return "n_ref " + std::to_string(refs.size()) + " differs from the BAM header's " + std::to_string(bam_n_ref);
    for (const RefRange &r : refs) {
        if (r.empty()) continue;
        for (const uint64_t v : {r.beg, r.end}) {
            if (coffset(v) >= bam_bytes) return "virtual offset " + voffset_str(v) + " lies past the file";
            uint32_t len = 0, isize = 0;
            if (!member_at(bam, bam_bytes, coffset(v), &len, &isize))
                return "no BGZF member at virtual offset " + voffset_str(v);
            if (uoffset(v) > isize) return "virtual offset " + voffset_str(v) + " lies past its member's ISIZE";
        }
    }
    return std::string();
}

// <path>.bai, else <path without .bam>.bai; empty when neither can be opened
inline std::string find(const std::string &bam_path) {
    std::vector<std::string> names{bam_path + ".bai"};
    if (bam_path.size() > 4 && bam_path.compare(bam_path.size() - 4, 4, ".bam") == 0)
        names.push_back(bam_path.substr(0, bam_path.size() - 4) + ".bai");
    for (const std::string &name : names)
        if (FILE *f = std::fopen(name.c_str(), "rb")) {
            std::fclose(f);
            return name;
        }
    return std::string();
}

// the bytes of a file; false when it cannot be read
inline bool read_file(const std::string &path, std::vector<uint8_t> *out) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    out->clear();
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + got);
    const bool ok = !std::ferror(f);
    std::fclose(f);
    return ok;
}

}  // namespace bamindex
}  // namespace secedo
