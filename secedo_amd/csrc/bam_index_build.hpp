// bam_index_build.hpp -- the BAI index writer (SAM spec 5.2), header-only, in plain host C++ that g++ compiles alone
// (tests/cpp/bam_index_build_test.cpp runs it under the sanitizers; bam_device_input.cpp feeds it what the device's
// index pass, bam_index_kernels.hip, found). bam_index.hpp is the reader of what this writes.
//
// Per file the builder takes, in file order, the heads of the runs of consecutive records with one (RefID, bin, flag
// 0x4), each with the virtual offset of its first record and that record's ordinal in the file, and the touched 16 kb
// windows with the virtual offset of the first record that overlaps each. A run ends where the next head starts, so
// only heads are needed; the records of a run are the difference of two ordinals, so no per-record count is either.
// The device walks a large file in ranges and starts a head at the first record of each: a head whose (RefID, bin)
// equals the run under way continues that run (one chunk), which also joins the runs that differ in flag 0x4 alone.
// A window given twice keeps the lower offset. What is written:
//   bins ascending, a bin's chunks in file order; the pseudo-bin 37450 last for every reference with records: (start of
//   its first record, end of its last), (records without flag 0x4, with it); n_intv = the last touched window + 1, an
//   untouched window takes the value of the next touched one above it (htslib's backward fill); a reference without
//   records has n_bin = n_intv = 0; the trailer n_no_coor counts the records with RefID -1.
// Whatever it is fed, the builder answers with bytes or with a reason, never with a read or write out of bounds.
#pragma once

#include "bgzf_members.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define SECEDO_BAI_HD __host__ __device__
#else
#define SECEDO_BAI_HD
#endif

namespace secedo {
namespace bamindexbuild {

constexpr uint32_t kPseudoBin = 37450;
constexpr uint64_t kMaxEnd = 1ull << 29;  // BAI's bins and windows hold positions below 2^29
constexpr uint32_t kMaxWindows = uint32_t(kMaxEnd >> 14);

// the bin of [beg, end), 0 <= beg < end <= 2^29 (SAM spec 5.3); the device's index pass calls it too
SECEDO_BAI_HD inline uint32_t reg2bin(uint64_t beg, uint64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return uint32_t(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return uint32_t(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return uint32_t(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return uint32_t(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return uint32_t(1 + (beg >> 26));
    return 0;
}

// the first record of a run of consecutive records with one (ref, bin, unmapped)
struct Head {
    int32_t ref;        // -1: the records without a reference (bin and unmapped are not read)
    uint32_t bin;
    uint32_t unmapped;  // flag 0x4
    uint64_t start;     // virtual offset of the record
    uint64_t ordinal;   // of the record in the file
};

struct Window {
    int32_t ref;
    uint32_t w;      // positions [w << 14, (w + 1) << 14)
    uint64_t start;  // virtual offset of a record that overlaps it; the lowest one given stays
};

struct Stats {
    uint64_t chunks = 0, bins = 0;  // written, the pseudo-bins and their chunks not counted
    uint64_t joined = 0;            // heads that continued the run under way with the same flag: range boundaries
    uint64_t windows = 0;           // n_intv summed
};

class Builder {
public:
    explicit Builder(uint32_t n_ref) : refs_(n_ref) {}

    // Heads in file order. Empty on success, else why the head cannot follow the ones before it.
    std::string add_head(const Head &h) {
        if (h.ref < -1 || (h.ref >= 0 && uint32_t(h.ref) >= refs_.size())) return "a RefID outside the reference list";
        if (h.ref >= 0 && h.bin >= kPseudoBin) return "a bin past 37449";
        if (open_) {
            if (h.ordinal <= ord_) return "record ordinals do not ascend";
            if (ref_ < 0 ? h.ref >= 0 : (h.ref >= 0 && h.ref < ref_)) return "RefIDs do not ascend";
            if (h.start < start_) return "offsets do not ascend";
            count(h.ordinal - ord_);
            ord_ = h.ordinal;
            if (h.ref == ref_ && (h.ref < 0 || h.bin == bin_)) {
                if (h.ref < 0 || (h.unmapped != 0) == unmapped_) ++stats_.joined;
                unmapped_ = h.unmapped != 0;
                return std::string();
            }
            close(h.start);
        }
        open_ = true;
        ref_ = h.ref;
        bin_ = h.bin;
        unmapped_ = h.unmapped != 0;
        start_ = h.start;
        ord_ = h.ordinal;
        return std::string();
    }

    std::string add_window(const Window &w) {
        if (w.ref < 0 || uint32_t(w.ref) >= refs_.size()) return "a window of a RefID outside the reference list";
        if (w.w >= kMaxWindows) return "a window past 2^29";
        if (w.start == 0 && !zero_ok_) return "a window at virtual offset 0";
        if (w.start == UINT64_MAX) return "a window at the last virtual offset";
        // held as offset + 1: 0 is an untouched window
        std::vector<uint64_t> &lin = refs_[w.ref].linear;
        if (lin.size() <= w.w) lin.resize(size_t(w.w) + 1, 0);
        if (lin[w.w] == 0 || w.start + 1 < lin[w.w]) lin[w.w] = w.start + 1;
        return std::string();
    }

    // One more reference behind the last (a reader that meets its names as it goes: tabix_build.hpp) -> its number.
    uint32_t add_ref() {
        refs_.emplace_back();
        return uint32_t(refs_.size() - 1);
    }
    uint32_t n_ref() const { return uint32_t(refs_.size()); }
    // A text file's first line may lie at virtual offset 0; a BAM's first record never does, and there a window at 0
    // stays refused.
    void allow_offset_zero() { zero_ok_ = true; }

    // Ends the run under way. end: the virtual offset behind the last record; n_records: the file's.
    std::string close_runs(uint64_t end, uint64_t n_records) {
        if (!open_) return std::string();
        if (n_records <= ord_) return "fewer records than the last head's ordinal";
        if (end < start_) return "the end lies before the last head";
        count(n_records - ord_);
        close(end);
        open_ = false;
        return std::string();
    }

    // After close_runs: the body of reference `ref` (n_bin, the bins, n_intv, the windows) appended to *out. A BAI and
    // a TBI hold the same body behind different headers.
    std::string append_ref(uint32_t ref, std::vector<uint8_t> *out) {
        if (ref >= refs_.size()) return "a RefID outside the reference list";
        Ref &r = refs_[ref];
        if (r.chunks.empty() && !r.linear.empty()) return "windows of a reference without records";
        // file order within a bin: the sort is stable
        std::stable_sort(r.chunks.begin(), r.chunks.end(), [](const Chunk &a, const Chunk &b) { return a.bin < b.bin; });
        uint32_t n_bin = 0;
        for (size_t c = 0; c < r.chunks.size(); ++c) n_bin += c == 0 || r.chunks[c].bin != r.chunks[c - 1].bin;
        stats_.bins += n_bin;
        stats_.chunks += r.chunks.size();
        put32(out, n_bin + (r.chunks.empty() ? 0 : 1));
        for (size_t c = 0; c < r.chunks.size();) {
            size_t e = c;
            while (e < r.chunks.size() && r.chunks[e].bin == r.chunks[c].bin) ++e;
            put32(out, r.chunks[c].bin);
            put32(out, uint32_t(e - c));
            for (; c < e; ++c) put64(out, r.chunks[c].beg), put64(out, r.chunks[c].end);
        }
        if (!r.chunks.empty()) {
            put32(out, kPseudoBin);
            put32(out, 2);
            put64(out, r.first), put64(out, r.last);
            put64(out, r.mapped), put64(out, r.unmapped);
        }
        for (size_t w = r.linear.size(); w-- > 1;)
            if (r.linear[w - 1] == 0) r.linear[w - 1] = r.linear[w];
        stats_.windows += r.linear.size();
        put32(out, uint32_t(r.linear.size()));
        for (const uint64_t v : r.linear) put64(out, v - 1);
        return std::string();
    }
    const Stats &stats() const { return stats_; }

    // end: the virtual offset behind the last record; n_records: the file's. The index bytes to *out.
    std::string finish(uint64_t end, uint64_t n_records, std::vector<uint8_t> *out, Stats *stats) {
        const std::string why = close_runs(end, n_records);
        if (!why.empty()) return why;
        out->clear();
        put(out, "BAI\1", 4);
        put32(out, uint32_t(refs_.size()));
        for (uint32_t r = 0; r < refs_.size(); ++r) {
            const std::string bad = append_ref(r, out);
            if (!bad.empty()) return bad;
        }
        put64(out, no_coor_);
        *stats = stats_;
        return std::string();
    }

    static void put(std::vector<uint8_t> *out, const void *p, size_t n) {
        const uint8_t *b = static_cast<const uint8_t *>(p);
        out->insert(out->end(), b, b + n);
    }
    static void put32(std::vector<uint8_t> *out, uint32_t v) { put(out, &v, 4); }
    static void put64(std::vector<uint8_t> *out, uint64_t v) { put(out, &v, 8); }

private:
    struct Chunk {
        uint32_t bin;
        uint64_t beg, end;
    };
    struct Ref {
        std::vector<Chunk> chunks;  // in file order until finish()
        std::vector<uint64_t> linear;
        uint64_t first = 0, last = 0, mapped = 0, unmapped = 0;
    };

    // n more records of the run under way
    void count(uint64_t n) {
        if (ref_ < 0) no_coor_ += n;
        else (unmapped_ ? refs_[ref_].unmapped : refs_[ref_].mapped) += n;
    }
    // the run under way ends at virtual offset `end`
    void close(uint64_t end) {
        if (ref_ < 0) return;
        Ref &r = refs_[ref_];
        if (r.chunks.empty()) r.first = start_;
        r.last = end;
        r.chunks.push_back(Chunk{bin_, start_, end});
    }

    std::vector<Ref> refs_;
    bool open_ = false, unmapped_ = false, zero_ok_ = false;
    int32_t ref_ = -1;
    uint32_t bin_ = 0;
    uint64_t start_ = 0, ord_ = 0, no_coor_ = 0;
    Stats stats_;
};

// One BGZF member of the file: virtual offsets take its byte in the file and the inflated bytes [out, out + isize),
// which are its first three fields. A reader's list goes in as it is; a writer gives Member{coff, out, isize}.
using Member = bgzf_members::Member;

// The virtual offset of inflated byte `lin` of a file of `file_bytes` bytes and `total` inflated bytes, lin <= total:
// the first member that holds a byte at or past it; the end of the data names the first empty member behind it (the
// EOF member), else the file size.
inline uint64_t voffset(const std::vector<Member> &m, uint64_t total, uint64_t file_bytes, uint64_t lin) {
    // the first member with out + isize > lin; out + isize ascends
    size_t lo = 0, hi = m.size();
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (m[mid].out + m[mid].isize > lin) hi = mid;
        else lo = mid + 1;
    }
    if (lo < m.size()) return m[lo].coff << 16 | (lin - m[lo].out);
    for (size_t k = m.size(); k-- > 0 && m[k].isize == 0 && m[k].out == total;)
        if (k == 0 || m[k - 1].isize != 0) return m[k].coff << 16;
    return file_bytes << 16;
}

}  // namespace bamindexbuild
}  // namespace secedo
