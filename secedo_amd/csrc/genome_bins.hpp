// genome_bins.hpp -- everything that decides the numbers and the bytes of secedo_variant_genome_bins
// (include/secedo_variant.h), header-only, in plain C++ that g++ compiles alone
// (tests/cpp/genome_bins_test.cpp runs it under the sanitizers) and that genome_bins_kernels.hip compiles as device
// code: the class of a sequence byte, the cut of a contig's name out of its header line, the selection of contigs by
// name, the mapping of a piece of a contig to global bins, the line of the output file and its longest length. The
// bin arithmetic is bam_depth.hpp's. Failures come back as the reason's text.
#pragma once

#include "bam_depth.hpp"

#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace secedo {
namespace genomebins {

namespace bd = secedo::bamdepth;

// ---- the class of a sequence byte: the columns of a bin's row

constexpr uint32_t kA = 0, kC = 1, kG = 2, kT = 3, kOther = 4, kMasked = 5, kColumns = 6;

// A a -> 0, C c -> 1, G g -> 2, T t U u -> 3 (char_to_int of fasta_lines.hpp), every other byte -> kOther
DEPTH_HD uint32_t byte_class(uint8_t b) {
    switch (b) {
        case 'A': case 'a': return kA;
        case 'C': case 'c': return kC;
        case 'G': case 'g': return kG;
        case 'T': case 't': case 'U': case 'u': return kT;
        default: return kOther;
    }
}
// counted in addition to the class
DEPTH_HD bool byte_masked(uint8_t b) { return b >= 'a' && b <= 'z'; }

// ---- the name of a contig: the header line's bytes after its first, up to the first space, tab or '\r'

constexpr uint32_t kMaxName = 4096;
// what of a header line decides its name, at the most: its first byte, kMaxName name bytes and one more
constexpr uint32_t kHeaderPrefix = kMaxName + 2;

DEPTH_HD bool name_stop(uint8_t b) { return b == ' ' || b == '\t' || b == '\r'; }

// The name inside header[0, n): the line without its '\n', or its first kHeaderPrefix bytes where it is longer.
// *len = its length (it begins at header + 1); false when it is longer than kMaxName.
DEPTH_HD bool cut_name(const uint8_t *header, uint64_t n, uint32_t *len) {
    uint64_t e = 1;
    while (e < n && !name_stop(header[e])) ++e;
    const uint64_t l = n > 1 ? e - 1 : 0;
    *len = uint32_t(l <= kMaxName ? l : kMaxName + 1);
    return l <= kMaxName;
}

inline std::string too_long(uint64_t contig) {
    return "contig " + std::to_string(contig) + ": its name is longer than " + std::to_string(kMaxName) + " bytes";
}

// ---- the mapping of sequence to bins

constexpr uint64_t kNotSelected = ~0ull;

// A piece of one contig's sequence inside a range of text (Table::Piece of fasta_lines.hpp with the contig's bins):
// sequence ordinals [code_off, code_off + count) of the range are the contig's positions from q0 on; bin0 is the
// contig's first bin in the table that is counted into, or kNotSelected.
struct Piece {
    uint64_t q0, bin0;
    uint32_t code_off, count;
};

// the piece that holds ordinal o: the last one with code_off <= o (pieces ascending, n >= 1, pieces[0].code_off <= o)
DEPTH_HD uint32_t piece_of(const Piece *pieces, uint32_t n, uint32_t o) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pieces[mid].code_off <= o) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the table's bin of ordinal o inside piece p (o in the piece, the piece selected) and the position's offset in it
DEPTH_HD uint64_t bin_of_ordinal(const Piece &p, uint32_t o, uint32_t S, uint32_t *rem) {
    const uint64_t pos = p.q0 + (o - p.code_off);
    *rem = uint32_t(pos % S);
    return p.bin0 + pos / S;
}

// ---- the selection. contigs in file order, each with its name and length; `listed` null: all of them (the first of
// each name), else the listed names in their order.

constexpr uint64_t kMaxContigLen = 0xFFFFFFFFull;  // bin_start / bin_end are u32, as in bam_depth.hpp

struct Selection {
    std::vector<uint64_t> contig;  // per selected contig its number in the file
    uint64_t duplicate_names = 0;
};

// The first contig of each name, in file order; *duplicates = the others.
inline std::map<std::string, uint64_t> first_of_name(const std::vector<std::string> &names, uint64_t *duplicates) {
    std::map<std::string, uint64_t> first;
    *duplicates = 0;
    for (uint64_t k = 0; k < names.size(); ++k)
        if (!first.emplace(names[k], k).second) ++*duplicates;
    return first;
}

// Why the selection cannot be made ("" when it can). lengths (may be null): the expected length of each listed name.
inline std::string select(const std::vector<std::string> &names, const std::vector<uint64_t> &len,
                          const std::vector<std::string> *listed, const uint64_t *lengths, Selection *out) {
    const std::map<std::string, uint64_t> first = first_of_name(names, &out->duplicate_names);
    out->contig.clear();
    if (!listed) {
        for (uint64_t k = 0; k < names.size(); ++k)
            if (first.at(names[k]) == k) out->contig.push_back(k);
        return std::string();
    }
    if (listed->empty()) return "no contig is selected: the list of names is empty";
    std::map<std::string, size_t> seen;
    for (size_t i = 0; i < listed->size(); ++i) {
        const std::string &n = (*listed)[i];
        if (!seen.emplace(n, i).second) return "contig name '" + n + "' is listed twice";
        const auto it = first.find(n);
        if (it == first.end())
            return "the genome has no contig named '" + n + "' (names are matched exactly: no chr prefix is added or "
                   "removed)";
        out->contig.push_back(it->second);
    }
    if (lengths)
        for (size_t i = 0; i < listed->size(); ++i)
            if (len[out->contig[i]] != lengths[i])
                return (*listed)[i] + ": the genome has " + std::to_string(len[out->contig[i]]) + " bases, expected " +
                       std::to_string(lengths[i]);
    return std::string();
}

// The bin layout of the selected contigs (bam_depth.hpp's, chr = the position in the selection).
inline std::string make_layout(const std::vector<std::string> &names, const std::vector<uint64_t> &len,
                               const Selection &sel, uint32_t S, bd::Layout *out, bool *limit) {
    std::vector<uint32_t> ref_len, ids;
    *limit = false;
    for (size_t i = 0; i < sel.contig.size(); ++i) {
        const uint64_t l = len[sel.contig[i]];
        if (l > kMaxContigLen) {
            *limit = true;
            return names[sel.contig[i]] + ": " + std::to_string(l) + " bases, more than the 2^32 - 1 a contig may have";
        }
        ref_len.push_back(uint32_t(l));
        ids.push_back(uint32_t(i));
    }
    std::string why = bd::make_layout(ref_len, ids, S, out, limit);
    if (!why.empty() && *limit) {  // the id in bam_depth.hpp's words is the position in the selection
        const uint64_t n = out->base.back();
        why = std::to_string(n) + " bins up to contig '" + names[sel.contig[out->chr.size() - 1]] +
              "', more than the 2^32 - 1 a call numbers; use a larger bin_size";
    }
    return why;
}

// ---- the file

inline std::string header_line() { return "chrom\tstart\tend\ta\tc\tg\tt\tother\tmasked\n"; }

// "<name>\t<start>\t<end>\t<a>\t<c>\t<g>\t<t>\t<other>\t<masked>\n"
template <class Sink>
DEPTH_HD void put_line(Sink &s, const uint8_t *name, uint32_t name_len, uint32_t start, uint32_t end,
                       const uint32_t *counts) {
    bd::put_bin(s, name, name_len, start, end);
    for (uint32_t k = 0; k < kColumns; ++k) {
        s.put('\t');
        bd::put_u64(s, counts[k]);
    }
    s.put('\n');
}

// the longest a line can be (a u32 has at most 10 digits)
inline uint64_t max_line(uint64_t name_len) { return name_len + 2 * 11 + kColumns * 11 + 1; }

inline std::string line(const std::string &name, uint32_t start, uint32_t end, const uint32_t *counts) {
    bd::StringSink s;
    put_line(s, reinterpret_cast<const uint8_t *>(name.data()), uint32_t(name.size()), start, end, counts);
    return s.out;
}

}  // namespace genomebins
}  // namespace secedo
