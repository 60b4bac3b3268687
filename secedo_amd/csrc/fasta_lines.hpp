// fasta_lines.hpp -- what the host and the device side of the FASTA device route share (include/secedo_variant.h):
// the line roles of get_next_chromosome / read_contig as a five-state machine over bytes, the composition of its
// transfer functions (what the device scans), the walk of one chunk from a known entry state, and the assignment of
// contigs to chromosomes from the header table. Compiles with g++ (tests/cpp/fasta_lines_test.cpp) and with hipcc.
//
// Line roles. The text is cut into lines at '\n'; a last line without '\n' counts, a trailing '\n' adds no line.
// Line 0 is a header whatever it starts with; line i >= 1 is a header iff it starts with '>' and line i - 1 is not a
// header; every other line is sequence. That is the reference's getline / peek order: the line after a header is
// read as sequence even when it starts with '>', and a run of '>' lines alternates. A machine that knows, at a line
// start, the role of the line before needs no look-back further than that, so a range of text can be cut anywhere:
// the state after its last byte is all the next range needs.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define SECEDO_FASTA_HD __host__ __device__
#else
#define SECEDO_FASTA_HD
#endif

namespace secedo {
namespace fasta {

// CharToInt (util/util.hpp:17-22): A/a 0, C/c 1, G/g 2, T/t/U/u 3, anything else 5
SECEDO_FASTA_HD inline uint8_t char_to_int(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 5;
    }
}

// The state in front of a byte.
constexpr uint32_t kLine0 = 0;        // at the start of line 0 (the start of the file)
constexpr uint32_t kAfterHeader = 1;  // at a line start, the line before was a header
constexpr uint32_t kAfterSeq = 2;     // at a line start, the line before was sequence
constexpr uint32_t kInHeader = 3;     // inside a header line
constexpr uint32_t kInSeq = 4;        // inside a sequence line
constexpr uint32_t kStates = 5;

// What a byte is, as flags.
constexpr uint32_t kSeqByte = 1;      // a base: it gets a code and an ordinal in its contig
constexpr uint32_t kHeaderStart = 2;  // the first byte of a header line (the '\n' itself for an empty line 0)
constexpr uint32_t kHeaderEnd = 4;    // the '\n' that ends a header line

// The state after byte b read in state s; *kind = what b is.
SECEDO_FASTA_HD inline uint32_t step(uint32_t s, uint8_t b, uint32_t *kind) {
    const bool nl = b == '\n';
    if (s == kInSeq) {
        *kind = nl ? 0 : kSeqByte;
        return nl ? kAfterSeq : kInSeq;
    }
    if (s == kInHeader) {
        *kind = nl ? kHeaderEnd : 0;
        return nl ? kAfterHeader : kInHeader;
    }
    const bool header = s == kLine0 || (s == kAfterSeq && b == '>');
    if (header) {
        *kind = kHeaderStart | (nl ? kHeaderEnd : 0);
        return nl ? kAfterHeader : kInHeader;
    }
    *kind = nl ? 0 : kSeqByte;
    return nl ? kAfterSeq : kInSeq;
}

// A transfer function of the machine: exit state per entry state, 3 bits each.
using Transfer = uint16_t;
constexpr Transfer kIdentity = Transfer(0 | 1 << 3 | 2 << 6 | 3 << 9 | 4 << 12);

SECEDO_FASTA_HD inline uint32_t apply(Transfer t, uint32_t s) { return (uint32_t(t) >> (3 * s)) & 7u; }

// first a, then b
SECEDO_FASTA_HD inline Transfer compose(Transfer a, Transfer b) {
    uint32_t r = 0;
    for (uint32_t s = 0; s < kStates; ++s) r |= apply(b, apply(a, s)) << (3 * s);
    return Transfer(r);
}

// bytes [at, at + n) of `text` as one function
template <class Text>
SECEDO_FASTA_HD inline Transfer transfer_of(const Text &text, uint32_t at, uint32_t n) {
    uint32_t st[kStates] = {0, 1, 2, 3, 4};
    for (uint32_t i = at; i < at + n; ++i) {
        const uint8_t b = text[i];
        uint32_t kind;
        for (uint32_t s = 0; s < kStates; ++s) st[s] = step(st[s], b, &kind);
    }
    return Transfer(st[0] | st[1] << 3 | st[2] << 6 | st[3] << 9 | st[4] << 12);
}

// One header of a range's table. Slot 0 stands for the header that was open or last seen when the range began;
// slot s >= 1 is the s-th header that starts in the range. Offsets count the range's bytes.
struct HeaderSlot {
    uint32_t start;  // its first byte
    uint32_t seq;    // sequence bytes of the range in front of it
    uint32_t end;    // the '\n' that ends it; kNone while the line is open at the range's end (slot 0: when it ends here)
    uint32_t b1;     // its byte 1, 0 when the line has no byte 1 in this range (slot 0: byte 0 of the range, 0 for '\n')
};
constexpr uint32_t kNone = 0xFFFFFFFFu;

// What a range's passes leave beside the slots.
struct RangeTotals {
    uint32_t headers;  // header lines that start in the range
    uint32_t seq;      // sequence bytes of the range
    uint32_t state;    // the state after its last byte
    uint32_t reserved;
};

// The walk of bytes [at, at + n) of a range of `len` bytes from entry state `s`, `seq` sequence bytes and `headers`
// header starts of the range in front: codes[ordinal] for every base, slot entries for the headers below `cap`.
// Used by the device's last pass (one chunk per lane) and by the host test (one chunk per range).
template <class Text>
SECEDO_FASTA_HD inline uint32_t walk(const Text &text, uint32_t len, uint32_t at, uint32_t n, uint32_t s, uint32_t *seq,
                                     uint32_t *headers, uint8_t *codes, HeaderSlot *slots, uint32_t cap) {
    for (uint32_t i = at; i < at + n; ++i) {
        const uint8_t b = text[i];
        uint32_t kind;
        s = step(s, b, &kind);
        if (slots && i == 0) slots[0].b1 = b == '\n' ? 0 : b;
        if (kind & kSeqByte) {
            if (codes) codes[*seq] = char_to_int(b);
            ++*seq;
        }
        if (kind & kHeaderStart) {
            ++*headers;
            if (slots && *headers < cap) {
                uint32_t b1 = 0;
                if (b != '\n' && i + 1 < len && text[i + 1] != '\n') b1 = text[i + 1];
                slots[*headers].start = i;
                slots[*headers].seq = *seq;
                slots[*headers].b1 = b1;
            }
        }
        if ((kind & kHeaderEnd) && slots && *headers < cap) slots[*headers].end = i;
    }
    return s;
}

// ---- the assignment of contigs to chromosomes (get_next_chromosome, variant_calling.cpp:155-224), host only

struct Role {
    uint32_t chr;
    uint32_t slot;  // 0: the maternal (or only) contig, 1: the paternal one
};

struct Chrom {
    int64_t mat = -1, pat = -1;  // contig indices; pat -1: none (haploid, or missing)
    bool hap = true;
};

// Contig k's role is known once its own header's byte 1 is: whether contig k - 1 was a whole chromosome or a maternal
// half depends on it ('X' followed by 'Y'). push() takes the headers in file order, finish() says none follows.
class Assigner {
 public:
    explicit Assigner(bool diploid) : diploid_(diploid) {}
    Role push(uint8_t b1) {
        const int64_t k = n_++;
        if (pending_) {
            pending_ = false;
            Chrom &c = chroms.back();
            c.hap = !diploid_ || pend_b1_ == 'Y' || (pend_b1_ == 'X' && b1 == 'Y');
            if (!c.hap) {
                c.pat = k;
                return Role{uint32_t(chroms.size() - 1), 1};
            }
        }
        Chrom c;
        c.mat = k;
        chroms.push_back(c);
        pending_ = true;
        pend_b1_ = b1;
        return Role{uint32_t(chroms.size() - 1), 0};
    }
    void finish() {
        if (!pending_) return;
        pending_ = false;
        chroms.back().hap = !diploid_ || pend_b1_ == 'Y';  // 'X' at the end of the file: the paternal contig is missing
    }
    int64_t contigs() const { return n_; }
    std::vector<Chrom> chroms;

 private:
    bool diploid_, pending_ = false;
    uint8_t pend_b1_ = 0;
    int64_t n_ = 0;
};

struct Contig {
    uint64_t header_len = 0;
    uint64_t seq_len = 0;
    uint8_t b1 = 0;
};

// Per chromosome c < n_chr its length and whether it is haploid, from the finished assignment; the error of the first
// chromosome that has one (the messages of the host route, word for word), empty when none. A chromosome past the
// last contig keeps the data of the one before (variant_calling.cpp:161-163); chromosome 0 of an empty file is empty.
inline std::string resolve(const std::vector<Chrom> &chroms, const std::vector<Contig> &contigs, uint32_t n_chr,
                           std::vector<uint64_t> *len, std::vector<uint8_t> *hap, std::vector<uint32_t> *source) {
    len->assign(n_chr, 0);
    hap->assign(n_chr, 1);
    source->assign(n_chr, 0);
    for (uint32_t c = 0; c < n_chr; ++c) {
        if (c >= chroms.size()) {
            if (c > 0) (*len)[c] = (*len)[c - 1], (*hap)[c] = (*hap)[c - 1], (*source)[c] = (*source)[c - 1];
            continue;
        }
        const Chrom &ch = chroms[c];
        (*source)[c] = c;
        if (c == 0 && contigs[0].header_len == 0) return "reference genome: empty line where a contig header is expected";
        const uint64_t a = contigs[size_t(ch.mat)].seq_len;
        if (!ch.hap) {
            const uint64_t b = ch.pat >= 0 ? contigs[size_t(ch.pat)].seq_len : 0;
            if (a != b)
                return "Invalid reference genome. Maternal and paternal chromosome sizes don't match (" +
                       std::to_string(a) + " vs " + std::to_string(b) + ")";
        }
        (*len)[c] = a;
        (*hap)[c] = ch.hap ? 1 : 0;
    }
    return std::string();
}

// The header table of a file, fed one range at a time with what the range's passes returned: the carried state
// between ranges on the host side. `needed`: contigs past this many are counted but not kept.
class Table {
 public:
    Table(bool diploid, uint64_t needed) : assign(diploid), needed_(needed) {}

    // A piece of one contig's sequence inside a range: codes [code_off, code_off + count) of the range are the
    // contig's bases from q0 on.
    struct Piece {
        Role role;
        uint64_t q0;
        uint32_t code_off, count;
    };

    // slots[0 .. cap) with cap >= needed + 2; len: the range's bytes
    void range(const RangeTotals &t, const HeaderSlot *slots, uint32_t len, std::vector<Piece> *pieces) {
        pieces->clear();
        if (headers_ <= needed_) {  // the contig in progress, if any, is a kept one
            // the header open across the boundary: its byte 1 when it began at the last byte before, its end
            if (open_ && len) {
                if (need_b1_) {
                    contigs.back().b1 = uint8_t(slots[0].b1);
                    need_b1_ = false;
                    roles_.push_back(assign.push(contigs.back().b1));
                }
                if (slots[0].end != kNone) {
                    contigs.back().header_len = text_ + slots[0].end - open_start_;
                    open_ = false;
                }
            }
            uint32_t seq_at = 0;  // sequence bytes of the range given to contigs so far
            bool kept = true;
            for (uint32_t s = 1; s <= t.headers; ++s) {
                const HeaderSlot &h = slots[s];
                piece(seq_at, h.seq, pieces);
                seq_at = h.seq;
                if (headers_ + s - 1 >= needed_) {
                    kept = false;
                    break;
                }
                contigs.push_back(Contig{});
                open_ = h.end == kNone;
                open_start_ = text_ + h.start;
                if (!open_) contigs.back().header_len = h.end - h.start;
                need_b1_ = open_ && h.start + 1 >= len;
                if (!need_b1_) {
                    contigs.back().b1 = uint8_t(h.b1);
                    roles_.push_back(assign.push(contigs.back().b1));
                }
            }
            if (kept) piece(seq_at, t.seq, pieces);
        }
        headers_ += t.headers;
        text_ += len;
    }

    void finish() {
        if (!contigs.empty() && open_) {
            contigs.back().header_len = text_ - open_start_;
            if (need_b1_) roles_.push_back(assign.push(0));
        }
        open_ = need_b1_ = false;
        assign.finish();
    }

    uint64_t headers() const { return headers_; }
    Assigner assign;
    std::vector<Contig> contigs;

 private:
    // sequence bytes [a, b) of the range belong to the last contig
    void piece(uint32_t a, uint32_t b, std::vector<Piece> *pieces) {
        if (contigs.empty() || b <= a) return;
        Contig &c = contigs.back();
        if (roles_.size() == contigs.size()) pieces->push_back(Piece{roles_.back(), c.seq_len, a, b - a});
        c.seq_len += b - a;
    }

    uint64_t needed_, headers_ = 0, text_ = 0, open_start_ = 0;
    bool open_ = false, need_b1_ = false;
    std::vector<Role> roles_;
};

}  // namespace fasta
}  // namespace secedo
