// bam_batch.hpp -- where every kernel of the BAM device route (bam_device_input.cpp) reads and writes: the layout of
// one batch, in plain host C++ that g++ compiles alone (tests/cpp/bam_batch_test.cpp runs it under the sanitizers).
// Pure arithmetic over member tables: no HIP, no read of a file's bytes, no error string. The structures the layout
// fills live here too, so that the kernels' headers (bam_walk_kernels.hpp, bam_index_kernels.hpp) and bam_host.hpp
// take them from one HIP-free home.
//
// A batch is a list of pieces: members [b0, b1) of a file (or of a span of an indexed file), with the bytes carried
// in front of them. lay_out_batch() places them in three address spaces:
//   staging (pinned, uploaded in one copy to d_in): kBgzfInSlack bytes, then per piece its host carry and
//       kBgzfInSlack bytes, then the file bytes of its members' payloads (bgzf_members::payload_span);
//   the inflated buffer: per piece its carry and, behind it, its members' bytes one after another; pieces 16-aligned;
//       kWalkWindow bytes of room behind the last;
//   the lists: bamwalk::list_cap(bytes) entries per segment, one segment per member.
#pragma once

#include "bam_walk.hpp"
#include "bgzf_members.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace secedo {
namespace bam {

// bytes the walk may read past the last inflated byte of the buffer (its LDS window is staged in whole vectors)
constexpr uint32_t kWalkWindow = 4096;

// One file of a batch (or one range of a file): set by the host, updated by the passes, read back whole.
struct WalkFile {
    // in
    uint32_t first_seg, n_seg;  // its segments, one per BGZF member of the batch, in file order
    uint32_t data_end;          // the end of its bytes in the buffer (they start at its first segment's start)
    uint32_t final;             // the bytes end the file
    uint64_t carry_src;         // carry_len bytes at d_in + carry_src go in front of its first member's bytes
    uint32_t carry_len, has_prev;
    uint64_t rec_base;          // records of the file before this range
    int32_t prev_ref, prev_pos; // of the last of them (has_prev)
    // out
    uint32_t limit;             // in: data_end; the start of the first member that did not inflate, if lower
    uint32_t stop_off;          // where the chain stopped: the bytes from here on are carried into the next range
    unsigned long long bad;     // in: ~0; min of (member of the batch << 8 | its bgzf status) over bad members
    unsigned long long err;     // in: ~0; min of (record of the file << 8 | bamwalk::Code)
    unsigned long long unsorted;  // in: ~0; the lowest record that sorts before its predecessor
    uint64_t n_rec;             // records in these bytes
    uint32_t first_rec;         // the batch's index of the first of them
    uint32_t rewalked;          // segments joined by a walk of their own
    int32_t last_ref, last_pos; // of the last record (n_rec > 0)
};
static_assert(sizeof(WalkFile) == 104, "the kernels and the host copy it whole");

// the first run of requested chromosome u in file f, entry f * n_chr + u
struct WalkRun {
    uint32_t first, last;  // in and out: bam_walk.hpp's started / done rule (kNoRun, kNoRun for a fresh file)
    uint32_t j0, j1;       // out: its records among the batch's selected ones
    uint64_t b0, b1;       // out: its bytes among the gathered ones
};
static_assert(sizeof(WalkRun) == 32, "the kernels and the host copy it whole");

// One requested chromosome u of file f of a batch whose bytes are a span of an indexed file (or a range of one),
// entry f * n_chr + u: what the index says of it, as offsets of the batch's buffer, against the records the walk found.
// The offsets are signed: a chromosome may start or end in another range of the span.
constexpr uint32_t kSpanOn = 1;     // the chromosome lies in this span
constexpr uint32_t kSpanEntry = 2;  // beg is where the walk enters the span: the RefID there is read before the walk's
                                    // results are believed (when those 8 bytes lie below the file's limit)
constexpr uint32_t kSpanTail = 4;   // end is the span's limit and the 8 bytes at it are inflated: the RefID there
struct SpanCheck {
    // in
    long long beg, end;
    uint32_t flags;
    int32_t ref;
    // out
    uint32_t start;      // 0: beg is no record start of this range's; 1: the record there has RefID ref; 2: none has
    uint32_t entry_bad;  // kSpanEntry: the RefID at beg is not ref
    uint32_t tail_bad;   // kSpanTail: the RefID at end is ref
    uint32_t reserved;
    uint64_t count;      // records of this range that start in [beg, end)
};
static_assert(sizeof(SpanCheck) == 48, "the kernels and the host copy it whole");

// One file of the batch for the index pass (bam_index_kernels.hpp), entry k of WalkBatch::files too.
struct IndexFile {
    long long delta;         // a buffer offset + delta = the file-linear inflated offset
    uint64_t seg_base;       // the batch-wide number of its RefID 0; a file takes n_ref + 1 numbers
    uint32_t n_ref, pad;
    unsigned long long err;  // in: ~0
};
static_assert(sizeof(IndexFile) == 32, "the kernels and the host copy it whole");

}  // namespace bam

namespace bam_host __attribute__((visibility("hidden"))) {

// A BGZF block is a member of bgzf_members.hpp, which lists, describes and inflates them.
namespace bm = secedo::bgzf_members;
using Block = bm::Member;

// ---- reading through the .bai index: what a plan (bam_host.hpp's IndexPlan) says of one stretch of a file

// one requested chromosome inside a span; offsets count the span's inflated bytes from its first member's first byte
struct SpanChr {
    uint32_t chromosome;
    uint64_t beg, end;  // its records start at beg and end in front of end
    uint64_t count;     // the pseudo-bin's record count, or bamindex::kNoCount
};
static_assert(sizeof(SpanChr) == 32, "as both routes know it");

// A run of members that holds the records of one or more requested chromosomes, entered at a known record start.
struct Span {
    std::vector<Block> blocks;  // its members in file order, `out` from 0
    uint64_t entry = 0;         // the first record starts here (the start's uoffset)
    uint64_t limit = 0;         // no record of the span starts at or past this
    uint64_t bytes = 0;         // inflated bytes of its members
    uint64_t beg_v = 0;         // the virtual offset of the entry (messages)
    std::vector<SpanChr> chrs;  // in file order; chrs[0].beg == entry, chrs.back().end == limit
};
static_assert(sizeof(Span) == 2 * sizeof(std::vector<Block>) + 32, "as both routes know it");

// ---- the layout of a batch

// the slot of a requested chromosome in chr_ids (each stands there once), chr_ids.size() if it is not requested
inline size_t slot_of(const std::vector<uint32_t> &chr_ids, uint32_t chromosome) {
    size_t u = 0;
    while (u < chr_ids.size() && chr_ids[u] != chromosome) ++u;
    return u;
}

constexpr uint64_t kMaxBatchBytes = (1ull << 32) - (1u << 20);  // offsets in a batch are u32

// a file's walk state, handed from range to range and from span to span
struct FileWalk {
    uint64_t rec_base = 0;  // records so far
    bool has_prev = false;
    int32_t prev_ref = 0, prev_pos = 0;         // of the last of them
    std::vector<uint32_t> run_first, run_last;  // per requested chromosome (bam_walk.hpp's started / done rule)
};

// Members [b0, b1) of a file in one batch, and what goes in front of them. The route's own piece derives from it, so
// nothing is copied for the layout. Of `file` and `carry_bytes` only addresses are taken.
struct BatchPiece {
    const std::vector<Block> *blocks = nullptr;  // the file's members; of a span: the span's
    size_t b0 = 0, b1 = 0;
    const uint8_t *file = nullptr;  // the mapped file
    uint64_t file_bytes = 0;
    const uint8_t *carry_bytes = nullptr;  // the host carry
    uint64_t carry = 0;  // bytes in front of member b0: on the first range the host carry's (uploaded), on a later one
                         // the device carry's (they lie at the front of the buffer already)
    bool first_range = true, final = true;
    const FileWalk *walk = nullptr;
    const Span *span = nullptr;  // the members are a span's: b0, b1 count them
    uint32_t n_ref = 0;          // index build
    uint64_t lin0 = 0;           // index build: the file-linear inflated offset of member b0, or of the file's end
};

// bytes to put into staging
struct BatchCopy {
    uint64_t dst;
    const uint8_t *src;
    uint64_t n;
};
constexpr uint64_t kCopyChunk = 4u << 20;  // a range of members is staged in copies of at most this (one per thread)

// What lay_out_batch fills; the vectors keep their storage from batch to batch. files, runs, checks and ix_files are
// also where the passes' results are read back to.
struct BatchLayout {
    std::vector<BatchCopy> copies;
    std::vector<bam::BgzfDesc> desc;       // one per member, piece after piece
    std::vector<bamwalk::Seg> segs;        // one per member, then one per piece that has no member
    std::vector<bam::WalkFile> files;      // [n_pieces]
    std::vector<bam::WalkRun> runs;        // [n_pieces * n_chr]
    std::vector<bam::SpanCheck> checks;    // [n_pieces * n_chr]
    std::vector<bam::IndexFile> ix_files;  // [n_pieces] (index build)
    std::vector<uint32_t> first_member;    // [n_pieces] its first descriptor
    uint64_t in_bytes = 0;                 // of staging
    uint64_t out_bytes = 0;                // of the inflated buffer, without the window
    uint64_t buf_bytes = 0;                // out_bytes + kWalkWindow
    uint64_t n_list = 0;
    bool any_span = false;
    uint32_t overflow = UINT32_MAX;        // the piece with which the batch passed 4 GiB (lay_out_batch gave false)
};

// The layout of the batch of pieces `in`. false: with piece L->overflow the inflated bytes pass kMaxBatchBytes or the
// lists pass u32, and the layout is not to be used.
template <class Piece>  // BatchPiece, or derived from it
inline bool lay_out_batch(const std::vector<Piece> &in, const std::vector<uint32_t> &chr_ids, bool index,
                          BatchLayout *L) {
    using namespace secedo::bam;
    const uint32_t n_files = uint32_t(in.size()), n_chr = uint32_t(chr_ids.size());
    L->copies.clear();
    L->desc.clear();
    L->segs.clear();
    L->files.assign(n_files, WalkFile{});
    L->runs.assign(size_t(n_files) * n_chr, WalkRun{});
    L->checks.assign(size_t(n_files) * n_chr, SpanCheck{});
    L->first_member.assign(n_files, 0);
    L->any_span = false;
    L->overflow = UINT32_MAX;
    if (index) {  // a file's RefIDs and its unmapped records number n_ref + 1 segments of the index pass
        L->ix_files.assign(n_files, IndexFile{});
        uint64_t seg = 0;
        for (uint32_t k = 0; k < n_files; ++k) {
            L->ix_files[k] = IndexFile{0, seg, in[k].n_ref, 0, ~0ull};
            seg += uint64_t(in[k].n_ref) + 1;
        }
    }
    // Invariants, each kept by the lines under it:
    //  (1) every descriptor's 16-byte loads lie inside the upload: staging starts with kBgzfInSlack bytes, a carry is
    //      followed by as many, and a range of members takes payload_span().needed, slack on both sides included;
    //  (2) a file's bytes start 16-aligned: out_pos is rounded up behind every piece;
    //  (3) the segments tile [data_start (+ entry), data_end): the first starts at the carry's start (a span's first
    //      range: at its entry, a known record start), every other where the one before it ends;
    //  (4) the list offsets are the running sum of list_cap over the segments in their order.
    uint64_t in_pos = kBgzfInSlack, out_pos = 0, n_list = 0;
    for (uint32_t k = 0; k < n_files; ++k) {
        const BatchPiece &p = in[k];
        WalkFile &F = L->files[k];
        const uint32_t first_member = L->first_member[k] = uint32_t(L->desc.size());
        const uint64_t carry = p.carry;
        if (p.first_range && carry) {  // (1)
            F.carry_src = in_pos;
            F.carry_len = uint32_t(carry);
            L->copies.push_back({in_pos, p.carry_bytes, carry});
            in_pos += carry + kBgzfInSlack;
        }
        const uint64_t data_start = out_pos;  // (2)
        uint64_t o = data_start + carry;
        if (p.b0 < p.b1) {
            const std::vector<Block> &bl = *p.blocks;
            const bm::PayloadSpan sp = bm::payload_span(bl, p.b0, p.b1, p.file_bytes);  // (1)
            for (uint64_t c = 0; c < sp.hi - sp.lo; c += kCopyChunk)
                L->copies.push_back({in_pos + c, p.file + sp.lo + c, std::min(kCopyChunk, sp.hi - sp.lo - c)});
            L->desc.resize(first_member + (p.b1 - p.b0));
            bm::fill_desc(bl, p.b0, p.b1, sp.lo, in_pos, o, L->desc.data() + first_member);
            for (size_t b = p.b0; b < p.b1; ++b) {  // (3), (4)
                // a span is entered at its first record, a known record start
                const uint64_t start = b != p.b0 ? o : data_start + (p.span && p.first_range ? p.span->entry : 0);
                o += bl[b].isize;
                L->segs.push_back(bamwalk::Seg{uint32_t(start), uint32_t(o), k, uint32_t(n_list)});
                n_list += bamwalk::list_cap(uint32_t(o - start));
            }
            in_pos += sp.needed;
            F.n_seg = uint32_t(p.b1 - p.b0);
        }
        F.first_seg = first_member;
        F.data_end = F.limit = uint32_t(o);
        if (index)  // the byte behind the carry is the first of member b0 (of the file's end, if none is left)
            L->ix_files[k].delta = (long long)p.lin0 - (long long)(data_start + carry);
        if (p.span) {  // the span's offsets as offsets of the buffer; its last range ends at its limit
            const Span &sp = *p.span;
            const long long base = (long long)(data_start + carry) - (long long)sp.blocks[p.b0].out;
            if (p.final) F.data_end = F.limit = uint32_t(base + (long long)sp.limit);
            for (size_t c = 0; c < sp.chrs.size(); ++c) {
                SpanCheck &ck = L->checks[size_t(k) * n_chr + slot_of(chr_ids, sp.chrs[c].chromosome)];
                ck.beg = base + (long long)sp.chrs[c].beg;
                ck.end = base + (long long)sp.chrs[c].end;
                ck.ref = int32_t(sp.chrs[c].chromosome);
                ck.flags = kSpanOn | (c == 0 && p.first_range ? kSpanEntry : 0) |
                           (c + 1 == sp.chrs.size() && p.final && sp.limit + 8 <= sp.bytes ? kSpanTail : 0);
            }
            L->any_span = true;
        }
        F.final = p.final;
        F.has_prev = p.walk->has_prev;
        F.rec_base = p.walk->rec_base;
        F.prev_ref = p.walk->prev_ref;
        F.prev_pos = p.walk->prev_pos;
        F.stop_off = F.data_end;
        F.bad = F.err = F.unsorted = ~0ull;
        for (uint32_t u = 0; u < n_chr; ++u) {
            L->runs[size_t(k) * n_chr + u].first = p.walk->run_first[u];
            L->runs[size_t(k) * n_chr + u].last = p.walk->run_last[u];
        }
        out_pos = (o + 15) / 16 * 16;  // (2)
        if (out_pos > kMaxBatchBytes || n_list > UINT32_MAX) {
            L->overflow = k;
            return false;
        }
    }
    // a file without a member in the batch (its header's members held all of it) walks its carry as one segment
    for (uint32_t k = 0; k < n_files; ++k) {
        WalkFile &F = L->files[k];
        if (F.n_seg) continue;
        const uint32_t len = uint32_t(in[k].carry);  // a piece without members is a file's first range: its host carry
        F.first_seg = uint32_t(L->segs.size());
        F.n_seg = 1;
        L->segs.push_back(bamwalk::Seg{F.data_end - len, F.data_end, k, uint32_t(n_list)});  // (3), (4)
        n_list += bamwalk::list_cap(len);
    }
    L->in_bytes = in_pos;
    L->out_bytes = out_pos;
    L->buf_bytes = out_pos + kWalkWindow;
    L->n_list = n_list;
    return true;
}

}  // namespace bam_host
}  // namespace secedo
