// bam_split.hpp -- everything that decides the bytes of secedo_bam_split_clusters (include/secedo_bam.h),
// header-only, in plain C++ that g++ compiles alone (tests/cpp/bam_split_test.cpp runs it under the sanitizers): the
// header every cluster_<k>.bam starts with (reference list, @RG merge, the fixed lines), the sort key of a record, and
// the lookup from an output byte to the record that holds it, which the gather kernel (bam_split_kernels.hip) compiles
// as device code (the member cuts of a cluster's extent are every writer's: bgzf_members.hpp). Failures come back as
// the reason's text. At the end, the rules of secedo_bam_split_clusters_rg: the strict aux walk, the
// edited bytes of a record, the cells' names and the @RG header lines; and those of secedo_bam_split_clusters_select
// (DESIGN 12t): the mask rule, the marked byte and how the mark rides to the gather
// (tests/cpp/bam_split_select_test.cpp).
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define SPLIT_HD __host__ __device__ inline
#else
#define SPLIT_HD inline
#endif

namespace secedo {
namespace bamsplit {

// ---- the sort key of a record: cluster << 32 | Position. A stable sort of it over records in (file, record) order
// gives (cluster, Position, file, record).

SPLIT_HD uint64_t pack_key(uint32_t cluster, uint32_t pos) { return uint64_t(cluster) << 32 | pos; }
SPLIT_HD uint32_t key_cluster(uint64_t key) { return uint32_t(key >> 32); }
SPLIT_HD uint32_t key_pos(uint64_t key) { return uint32_t(key); }

// the key bits in use with clusters 0..max_cluster: the radix sort's end bit
inline int key_bits(uint32_t max_cluster) {
    int b = 32;
    while (b < 64 && (uint64_t(max_cluster) >> (b - 32)) != 0) ++b;
    return b;
}

// ---- the gather's lookup. dst[0..n] are the ascending output offsets of the n records of the sorted order, dst[n] the
// total. The record of output byte `b` is the last j in [lo, hi) with dst[j] <= b; the caller gives a range that holds
// it (dst[lo] <= b, and hi == n or dst[hi] > b). Equal entries (records of no bytes, which BAM does not have, or the
// entries of an empty tail) are skipped over: the last of them is taken.
SPLIT_HD uint32_t record_of(const uint64_t *dst, uint32_t lo, uint32_t hi, uint64_t b) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (dst[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One workgroup of the gather writes kTileBytes of output. A record is at least kMinRecord bytes (block_size, the 32
// fixed bytes and a name of one NUL), so the records that start inside a tile, and the one that reaches into it, are
// at most kTileRecords; the lookup of every lane runs over that range only.
constexpr uint32_t kGatherLanes = 256, kGatherVec = 16;
constexpr uint32_t kTileBytes = kGatherLanes * kGatherVec;
constexpr uint32_t kMinRecord = 4 + 32 + 1;
constexpr uint32_t kTileRecords = kTileBytes / kMinRecord + 2;

// ---- the header

struct Ref {
    std::string name;
    uint32_t len = 0;
    bool operator==(const Ref &o) const { return name == o.name && len == o.len; }
};

inline uint32_t rd32(const uint8_t *p) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
}

// the binary reference list of a BAM header (n_ref entries of l_name, name with its NUL, l_ref); false when cut short
inline bool parse_ref_list(const uint8_t *p, uint64_t n, uint32_t n_ref, std::vector<Ref> *out) {
    uint64_t o = 0;
    for (uint32_t r = 0; r < n_ref; ++r) {
        if (o + 4 > n) return false;
        const uint64_t l = rd32(p + o);
        if (o + 4 + l + 4 > n) return false;
        Ref ref;
        ref.name.assign(reinterpret_cast<const char *>(p + o + 4), l);
        const size_t nul = ref.name.find('\0');
        if (nul != std::string::npos) ref.name.resize(nul);
        ref.len = rd32(p + o + 4 + l);
        out->push_back(ref);
        o += 4 + l + 4;
    }
    return true;
}

// the lines of a header text, without their '\n' (and without a '\r' in front of it, or NULs that pad the text)
inline std::vector<std::string> text_lines(const std::string &text) {
    std::vector<std::string> out;
    size_t a = 0;
    while (a < text.size()) {
        size_t b = text.find('\n', a);
        if (b == std::string::npos) b = text.size();
        std::string line = text.substr(a, b - a);
        while (!line.empty() && (line.back() == '\r' || line.back() == '\0')) line.pop_back();
        if (!line.empty()) out.push_back(line);
        a = b + 1;
    }
    return out;
}

inline bool is_line(const std::string &line, const char *type) {
    return line.compare(0, 3, type) == 0 && (line.size() == 3 || line[3] == '\t');
}

// the value of field "XX:" of a header line, or "" (the first one counts)
inline std::string line_field(const std::string &line, const char *key) {
    for (size_t a = line.find('\t'); a != std::string::npos; a = line.find('\t', a + 1)) {
        if (line.compare(a + 1, 3, key) != 0) continue;
        const size_t e = line.find('\t', a + 1);
        return line.substr(a + 4, e == std::string::npos ? std::string::npos : e - a - 4);
    }
    return std::string();
}

// the reference list a SAM header's @SQ lines give (SN, LN), in line order: what the BAM made from it holds
inline std::vector<Ref> refs_from_text(const std::string &text) {
    std::vector<Ref> out;
    for (const std::string &line : text_lines(text)) {
        if (!is_line(line, "@SQ")) continue;
        Ref r;
        r.name = line_field(line, "SN:");
        r.len = uint32_t(std::strtoull(line_field(line, "LN:").c_str(), nullptr, 10));
        out.push_back(r);
    }
    return out;
}

// Why file f's reference list is not the first file's ("" when it is): the count, or the first entry that differs.
inline std::string refs_differ(const std::vector<Ref> &first, const std::vector<Ref> &other) {
    if (first.size() != other.size())
        return std::to_string(other.size()) + " references, the first file has " + std::to_string(first.size());
    for (size_t r = 0; r < first.size(); ++r)
        if (!(first[r] == other[r]))
            return "reference " + std::to_string(r) + " is " + other[r].name + " of length " +
                   std::to_string(other[r].len) + ", in the first file " + first[r].name + " of length " +
                   std::to_string(first[r].len);
    return std::string();
}

// The @RG lines of all inputs, distinct whole lines in order of first appearance (files in list order, lines in header
// order). Two different lines with one ID: false, *clash_a < *clash_b the two files and *clash_id the ID.
struct RgMerge {
    std::vector<std::string> lines;
    std::vector<size_t> file;  // where each was seen first
};

inline bool merge_rg(const std::vector<std::string> &texts, RgMerge *out, size_t *clash_a, size_t *clash_b,
                     std::string *clash_id) {
    for (size_t f = 0; f < texts.size(); ++f)
        for (const std::string &line : text_lines(texts[f])) {
            if (!is_line(line, "@RG")) continue;
            const std::string id = line_field(line, "ID:");
            bool known = false;
            for (size_t k = 0; k < out->lines.size() && !known; ++k) {
                if (out->lines[k] == line) known = true;
                else if (line_field(out->lines[k], "ID:") == id) {
                    *clash_a = out->file[k];
                    *clash_b = f;
                    *clash_id = id;
                    return false;
                }
            }
            if (known) continue;
            out->lines.push_back(line);
            out->file.push_back(f);
        }
    return true;
}

// the text of cluster k's header: m of the n cells are in the cluster
inline std::string header_text(const std::vector<Ref> &refs, const std::vector<std::string> &rg, uint32_t k, uint32_t m,
                               uint32_t n) {
    std::string t = "@HD\tVN:1.6\tSO:coordinate\n";
    for (const Ref &r : refs) t += "@SQ\tSN:" + r.name + "\tLN:" + std::to_string(r.len) + "\n";
    for (const std::string &line : rg) t += line + "\n";
    t += "@PG\tID:secedo_amd.split\tPN:secedo_amd\n";
    t += "@CO\tsecedo_amd cluster " + std::to_string(k) + ": " + std::to_string(m) + " of " + std::to_string(n) +
         " cells\n";
    return t;
}

// "BAM\1", l_text, the text, n_ref and the first file's binary reference list as it stands
inline std::vector<uint8_t> header_bytes(const std::string &text, uint32_t n_ref, const std::vector<uint8_t> &ref_list) {
    std::vector<uint8_t> out{'B', 'A', 'M', 1};
    const auto put32 = [&](uint32_t v) {
        for (int k = 0; k < 4; ++k) out.push_back(uint8_t(v >> (8 * k)));
    };
    put32(uint32_t(text.size()));
    out.insert(out.end(), text.begin(), text.end());
    put32(n_ref);
    out.insert(out.end(), ref_list.begin(), ref_list.end());
    return out;
}

// the binary reference list of `refs` (SAM inputs have none of their own)
inline std::vector<uint8_t> ref_list_bytes(const std::vector<Ref> &refs) {
    std::vector<uint8_t> out;
    const auto put32 = [&](uint32_t v) {
        for (int k = 0; k < 4; ++k) out.push_back(uint8_t(v >> (8 * k)));
    };
    for (const Ref &r : refs) {
        put32(uint32_t(r.name.size() + 1));
        out.insert(out.end(), r.name.begin(), r.name.end());
        out.push_back(0);
        put32(r.len);
    }
    return out;
}

// ---- read groups (secedo_bam_split_clusters_rg): every written record gets RG:Z:<its cell's name> as its
// last field, and the RG field it had is removed. What follows decides the edited bytes; the plan and gather kernels
// compile it as device code.

// The strict walk of a record's aux area. `rec` is the whole record, block_size word included, `len` = 4 + block_size.
// A field is a two-byte tag, a type byte and a value: A c C 1 byte, s S 2, i I f 4, Z H up to and including the NUL,
// B a subtype byte, a u32 count and count elements of the subtype's size. The walk succeeds when every field ends
// within the record and the last one ends exactly at len; an unknown type or subtype, a field that runs past the end
// and one or two bytes left over fail it. parsed: the walk succeeded. [hole_off, hole_off + hole_len) is then the
// first field named RG, whole, whatever its type; without one, and after a failed walk, hole_off = len, hole_len = 0.
// A B array is skipped by its count, so a long array costs a few loads.
struct AuxHole {
    uint32_t hole_off, hole_len;
    bool parsed;
};

SPLIT_HD uint32_t aux_elem_size(uint8_t type) {
    switch (type) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
    }
}

SPLIT_HD AuxHole aux_walk(const uint8_t *rec, uint32_t len) {
    const AuxHole failed{len, 0, false};
    if (len < 36) return failed;
    const uint64_t l_name = rec[12];
    const uint64_t n_cigar = uint32_t(rec[16]) | uint32_t(rec[17]) << 8;
    const uint64_t l_seq = uint32_t(rec[20]) | uint32_t(rec[21]) << 8 | uint32_t(rec[22]) << 16 | uint32_t(rec[23]) << 24;
    uint64_t p = 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
    AuxHole out{len, 0, true};
    while (p < len) {
        if (len - p < 3) return failed;
        const uint8_t type = rec[p + 2];
        uint64_t q = p + 3;
        if (type == 'Z' || type == 'H') {
            while (q < len && rec[q] != 0) ++q;
            if (q >= len) return failed;
            ++q;
        } else if (type == 'B') {
            if (len - q < 5) return failed;
            const uint64_t size = aux_elem_size(rec[q]);
            if (size == 0 || rec[q] == 'A') return failed;
            const uint64_t count = uint32_t(rec[q + 1]) | uint32_t(rec[q + 2]) << 8 | uint32_t(rec[q + 3]) << 16 |
                                   uint32_t(rec[q + 4]) << 24;
            q += 5 + count * size;
        } else {
            const uint64_t size = aux_elem_size(type);
            if (size == 0) return failed;
            q += size;
        }
        if (q > len) return failed;
        if (out.hole_len == 0 && rec[p] == 'R' && rec[p + 1] == 'G') {
            out.hole_off = uint32_t(p);
            out.hole_len = uint32_t(q - p);
        }
        p = q;
    }
    if (p != len) return failed;  // the fixed part alone runs past the record
    return out;
}

// The bytes a record of the cell named N gets at its end: 'R' 'G' 'Z' N '\0'.
inline std::string rg_suffix(const std::string &name) { return "RGZ" + name + std::string(1, '\0'); }

// One record's edit: its length, the hole and the length of its cell's suffix. The edited record is the record's
// bytes without the hole, then the suffix; its first four bytes are the new block_size.
struct Edit {
    uint32_t len, hole_off, hole_len, suf_len;
};

SPLIT_HD uint32_t edited_len(const Edit &e) { return e.len - e.hole_len + e.suf_len; }

// the byte at offset o < edited_len(e) of the edited record
SPLIT_HD uint8_t edited_byte(const uint8_t *rec, const Edit &e, const uint8_t *suffix, uint32_t o) {
    if (o < 4) return uint8_t((edited_len(e) - 4) >> (8 * o));
    if (o < e.hole_off) return rec[o];
    const uint32_t kept = e.len - e.hole_len;
    if (o < kept) return rec[o + e.hole_len];
    return suffix[o - kept];
}

// ---- record selection (secedo_bam_split_clusters_select): the flag filter, and duplicates marked or
// removed per cell. Which records are chosen is rule 3d of bam_kernels.hip; what follows decides the bytes of a marked
// record and how the mark reaches the gather.

// Why the masks are refused ("" when they are not): a SAM flag has 16 bits, and a bit in both masks passes no record.
inline std::string masks_fault(uint64_t require, uint64_t exclude) {
    if (require > 0xFFFF || exclude > 0xFFFF) return "a SAM flag mask is at most 0xFFFF";
    if (require & exclude)
        return "require " + std::to_string(require) + " and exclude " + std::to_string(exclude) +
               " share a bit, no record could pass";
    return std::string();
}

// A marked record is the record with 0x400 set in its FLAG: the u16 at bytes 18..19 counting from block_size, so byte
// kDupByte |= kDupBits. No other byte changes and no bit is cleared.
constexpr uint32_t kDupByte = 19;
constexpr uint8_t kDupBits = 0x04;

// byte `value` at offset o of a record, marked or not
SPLIT_HD uint8_t marked_byte(uint8_t value, uint32_t o, bool marked) {
    return (marked && o == kDupByte) ? uint8_t(value | kDupBits) : value;
}

// The mark travels to the gather in the top bit of the record's source offset (offsets are far below 2^63), so a lane
// that loads src[j] has it without another load.
constexpr uint64_t kMarkBit = 1ull << 63;
SPLIT_HD uint64_t pack_src(uint64_t off, bool marked) { return marked ? off | kMarkBit : off; }
SPLIT_HD uint64_t src_off(uint64_t src) { return src & ~kMarkBit; }
SPLIT_HD bool src_marked(uint64_t src) { return (src & kMarkBit) != 0; }

// The 16 bytes v[0..3] (little-endian dwords) of a gather lane that start at offset r of a marked record and lie
// wholly inside it: the lane that holds byte kDupByte sets the bits.
SPLIT_HD void mark_vector(uint32_t v[4], uint64_t r) {
    if (r <= kDupByte && kDupByte - r < kGatherVec) {
        const uint32_t at = kDupByte - uint32_t(r);
        const uint32_t bits = uint32_t(kDupBits) << (8 * (at & 3));
        const uint32_t word = at >> 2;  // constant indices only: v stays in registers
        v[0] |= word == 0 ? bits : 0u;
        v[1] |= word == 1 ? bits : 0u;
        v[2] |= word == 2 ? bits : 0u;
        v[3] |= word == 3 ? bits : 0u;
    }
}
// Only such lanes are patched, and no other lane holds the byte. A lane of the plain gather that is not wholly inside
// one record starts in a record j at offset r and reaches past its end: r + 16 > len >= kMinRecord, so r > kDupByte,
// and byte kDupByte of record j + 1 lies more than kDupByte >= 16 bytes past the lane's first byte. In the editing
// gather a lane that holds byte kDupByte starts at offset r in 4..19 (r + 15 >= 19) and ends at r + 16 <= 35, in front
// of any hole (hole_off >= 36 + l_name >= kMinRecord) and inside the edited record, which is no shorter than
// kMinRecord: it lies in the copied segment in front of the hole and takes the five-dword path.
static_assert(kMinRecord >= kDupByte + 1 + kGatherVec, "a lane on a record boundary never holds the FLAG's high byte");
static_assert(kDupByte >= kGatherVec, "a lane never reaches the next record's FLAG");
static_assert(kDupByte + kGatherVec <= kMinRecord, "a lane that holds the FLAG's high byte ends before any hole");
static_assert(kDupByte + 1 >= 4 + kGatherVec, "a lane that holds the FLAG's high byte starts behind block_size");

// what the plan pass leaves the gather of a sorted record: the hole, the record's length and its cell
struct RecordPlan {
    uint32_t hole_off, hole_len, len, cell;
};
static_assert(sizeof(RecordPlan) == 16, "one 16-byte load per record");

// The gather's tile bound holds for edited records too: the hole lies in the aux area, behind the 36 fixed bytes and
// the name, so what is kept of a record of at least kMinRecord bytes is at least kMinRecord bytes, and a suffix
// (at least 5 bytes) is added to it.
constexpr uint32_t kMaxName = 254;

// Why `name` cannot name a read group ("" when it can): 1 to 254 bytes, each in 0x21..0x7E.
inline std::string name_fault(const std::string &name) {
    if (name.empty()) return "is empty";
    if (name.size() > kMaxName) return "is " + std::to_string(name.size()) + " bytes long, at most 254 are allowed";
    for (size_t k = 0; k < name.size(); ++k) {
        const unsigned char ch = static_cast<unsigned char>(name[k]);
        if (ch < 0x21 || ch > 0x7E) return "has byte " + std::to_string(unsigned(ch)) + " at offset " + std::to_string(k) +
                                           ", only 0x21 to 0x7E are allowed";
    }
    return std::string();
}

// Why the cells cannot be named `names` ("" when they can): the first cell whose name breaks the rule, else the first
// two cells that share a name.
inline std::string names_fault(const std::vector<std::string> &names) {
    for (size_t c = 0; c < names.size(); ++c) {
        const std::string why = name_fault(names[c]);
        if (!why.empty()) return "the name of cell " + std::to_string(c) + " " + why;
    }
    std::map<std::string, size_t> first;
    for (size_t c = 0; c < names.size(); ++c) {
        const auto seen = first.emplace(names[c], c);
        if (!seen.second)
            return "cells " + std::to_string(seen.first->second) + " and " + std::to_string(c) + " share the name " +
                   names[c];
    }
    return std::string();
}

// the default name of a per-file cell: the file's base name without the first of .sam.gz, .bam, .sam that it ends in
inline std::string default_name(const std::string &path) {
    const size_t slash = path.rfind('/');
    std::string base = slash == std::string::npos ? path : path.substr(slash + 1);
    for (const char *ext : {".sam.gz", ".bam", ".sam"}) {
        const size_t n = std::strlen(ext);
        if (base.size() >= n && base.compare(base.size() - n, n, ext) == 0) {
            base.resize(base.size() - n);
            break;
        }
    }
    return base;
}

// the @RG lines of cluster k's file: one per cell of the cluster, in cell order
inline std::vector<std::string> rg_header_lines(const std::vector<std::string> &names,
                                                const std::vector<uint16_t> &cell_cluster, uint32_t k) {
    std::vector<std::string> out;
    for (size_t c = 0; c < names.size() && c < cell_cluster.size(); ++c)
        if (cell_cluster[c] == k) out.push_back("@RG\tID:" + names[c] + "\tSM:cluster_" + std::to_string(k));
    return out;
}

}  // namespace bamsplit
}  // namespace secedo
