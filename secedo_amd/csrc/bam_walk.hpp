// bam_walk.hpp -- the decisions of the BAM record walk on the device, in plain C++ that g++ compiles too
// (tests/cpp/bam_walk_test.cpp runs it under the sanitizers; bam_walk_kernels.hip runs it on gfx950).
//
// A BAM record is block_size (u32) and block_size bytes; the walk is the chain next(p) = p + 4 + block_size(p) from a
// known record start. The chain is a function of the offset alone, so two chains that meet stay together: a chain
// started at a guess (the start of a segment) is exact from the first offset it shares with the true chain. The
// segment walk follows a chain through one segment and lists the offsets it visits; the join goes through a file's
// segments in order and, where the true chain does not enter a segment at the guessed start, follows it until it
// meets the listed chain and adopts the rest of the list.
//
// Offsets are u32 positions in one buffer (a batch holds less than 4 GiB). A file's bytes end at data_end. Every
// read is of 4 bytes at an offset o with data_end - o >= kMinRecord, whatever the bytes hold.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SECEDO_HD __host__ __device__
#else
#define SECEDO_HD
#endif

namespace secedo {
namespace bamwalk {

constexpr uint32_t kMinRecord = 36;  // block_size and the 32 fixed bytes

// why a chain ended
enum Stop : uint32_t {
    kExit = 0,     // it reached the end of its segment
    kShort = 1,    // fewer than kMinRecord bytes are left of the file's bytes
    kBadSize = 2,  // block_size below 32
    kOverrun = 3,  // the record ends past the file's bytes
    kFull = 4,     // more steps than the segment can hold records (unreachable: each step is kMinRecord or more)
};

// error codes of the device walk, ordered as the host walk meets them on one record (atomicMin of index << 8 | code)
enum Code : uint32_t {
    kErrTruncated = 1,
    kErrBlockSize = 2,
    kErrLonger = 3,
    kErrUnsorted = 4,
    kErrNegative = 5,
    kErrCigarOp = 0x10,  // | the op code (9..15)
    kErrCigarSeq = 0x20,
};

// The words of a record defect, the same from the host walk and from the device walk: "<where the record is>" +
// defect_words(code), and for kErrCigarOp | op (is_cigar_op) the op's number, code & 15, behind them.
constexpr bool is_cigar_op(uint32_t code) { return (code & 0xF0) == kErrCigarOp; }
inline const char *defect_words(uint32_t code) {
    switch (code) {
        case kErrTruncated: return " is truncated";
        case kErrBlockSize: return " has a bad block_size";
        case kErrLonger: return " is longer than its block_size";
        case kErrUnsorted: return ": input is not coordinate-sorted";
        case kErrNegative: return " has a negative position";
        case kErrCigarSeq: return ": CIGAR and SEQ lengths differ";
        default: return ": invalid CIGAR op code ";
    }
}

// records a segment of `bytes` bytes can start
SECEDO_HD inline uint32_t list_cap(uint32_t bytes) { return (bytes + kMinRecord - 1) / kMinRecord; }

// One step of the chain at o < data_end: kExit and *next, or why there is none. rd(o) = the u32 at o.
template <class Rd>
SECEDO_HD inline uint32_t chain_step(Rd &rd, uint32_t o, uint32_t data_end, uint32_t *next) {
    if (data_end - o < kMinRecord) return kShort;
    const uint32_t bs = rd(o);
    if (bs < 32) return kBadSize;
    if (bs > data_end - o - 4) return kOverrun;
    *next = o + 4 + bs;
    return kExit;
}

struct Seg {
    uint32_t start, end;  // its bytes; end <= the file's data_end unless the file was cut short
    uint32_t file;
    uint32_t list;        // where its lists start (list_cap(end - start) entries each)
};

struct SegWalk {
    uint32_t n;     // offsets listed
    uint32_t exit;  // where the chain left off: the first offset at or past the end, or the offset that stopped it
    uint32_t stop;
};

// the accepted records of a segment: rewalk[0, n_rewalk) then list[from, from + n_adopt)
struct SegJoin {
    uint32_t n_rewalk, from, n_adopt;
};

struct Chain {
    uint64_t n;         // records of the file's bytes
    uint32_t stop_off;  // the offset that stopped the chain, or data_end
    uint32_t stop;
    uint32_t rewalked;  // segments entered elsewhere than at their start
};

// The chain from `start` through [start, end): visited offsets to list[] when `write` (one lane of a wave).
template <class Rd>
SECEDO_HD inline SegWalk walk_segment(Rd &rd, uint32_t start, uint32_t end, uint32_t data_end, uint32_t *list,
                                      bool write) {
    const uint32_t cap = list_cap(end - start);
    SegWalk r{0, start, kExit};
    while (r.exit < end) {
        if (r.n == cap) {
            r.stop = kFull;
            break;
        }
        uint32_t next = 0;
        r.stop = chain_step(rd, r.exit, data_end, &next);
        if (r.stop != kExit) break;
        if (write) list[r.n] = r.exit;
        ++r.n;
        r.exit = next;
    }
    return r;
}

// index of the first entry >= o of the ascending list[0, n)
SECEDO_HD inline uint32_t lower_bound(const uint32_t *list, uint32_t n, uint32_t o) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list[mid] < o) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The true chain of one file from segs[0].start, a record start, through its n_seg segments, given every segment's
// speculative walk from its own start (walk[], lists[]): join[k] says which offsets of segment k are records;
// offsets the join walked itself go to rewalk[] (laid out as lists[]). A segment whose bytes lie past data_end (the
// file cut short) has none. A record longer than a segment leaves the segments it covers empty.
template <class Rd>
SECEDO_HD inline Chain join_file(Rd &rd, const Seg *segs, const SegWalk *walk, const uint32_t *lists,
                                 uint32_t *rewalk, uint32_t n_seg, uint32_t data_end, SegJoin *join) {
    Chain c{0, data_end, kExit, 0};
    uint32_t e = n_seg ? segs[0].start : data_end;
    for (uint32_t k = 0; k < n_seg; ++k) {
        SegJoin j{0, 0, 0};
        const uint32_t end = segs[k].end < data_end ? segs[k].end : data_end;
        if (c.stop == kExit && e < end) {
            const SegWalk w = walk[k];
            if (e == segs[k].start) {
                j.n_adopt = w.n;
                e = w.exit;
                c.stop = w.stop;
            } else {
                ++c.rewalked;
                const uint32_t *list = lists + segs[k].list;
                uint32_t *mine = rewalk + segs[k].list;
                while (e < end) {
                    const uint32_t at = lower_bound(list, w.n, e);
                    if (at < w.n && list[at] == e) {  // the chains have met
                        j.from = at;
                        j.n_adopt = w.n - at;
                        e = w.exit;
                        c.stop = w.stop;
                        break;
                    }
                    uint32_t next = 0;
                    c.stop = chain_step(rd, e, data_end, &next);
                    if (c.stop != kExit) break;
                    mine[j.n_rewalk++] = e;
                    e = next;
                }
            }
        }
        join[k] = j;
        c.n += j.n_rewalk + j.n_adopt;
    }
    c.stop_off = c.stop == kExit ? data_end : e;
    return c;
}

// What a stopped chain means: 0 = the rest of the bytes is carried into the next range, else the walk's error code.
// final: the bytes end the file.
SECEDO_HD inline uint32_t stop_code(uint32_t stop, bool final) {
    if (stop == kBadSize) return kErrBlockSize;
    if (stop == kShort) return final ? uint32_t(kErrTruncated) : 0u;
    if (stop == kOverrun || stop == kFull) return final ? uint32_t(kErrBlockSize) : 0u;
    return 0;
}

// Coordinate order: a record sorts before the one in front of it. RefID < 0 sorts last; Position counts within a
// RefID >= 0 only.
SECEDO_HD inline bool sorts_before(int32_t ref, int32_t pos, int32_t prev_ref, int32_t prev_pos) {
    const uint32_t k = ref < 0 ? UINT32_MAX : uint32_t(ref), kp = prev_ref < 0 ? UINT32_MAX : uint32_t(prev_ref);
    return k < kp || (k == kp && ref >= 0 && pos < prev_pos);
}

// The started / done rule: of a chromosome only the first contiguous run of a file's records is taken. Records are
// numbered from 1 in a range (0 stands for the record before the range); a run starts at a record of the chromosome
// whose predecessor is not of it, and ends at the first record after it that is not. `first` = the lowest start,
// `last` = the lowest end above `first`; record i is taken when first <= i < last. A run open at the end of a range
// goes on with first = 0, a finished one with first = last = 0.
constexpr uint32_t kNoRun = UINT32_MAX;
SECEDO_HD inline bool run_starts(bool is_chr, bool has_prev, bool prev_is_chr) {
    return is_chr && !(has_prev && prev_is_chr);
}
SECEDO_HD inline bool run_ends(bool is_chr, bool has_prev, bool prev_is_chr) {
    return !is_chr && has_prev && prev_is_chr;
}
SECEDO_HD inline bool run_takes(uint32_t i, uint32_t first, uint32_t last) { return first <= i && i < last; }

}  // namespace bamwalk
}  // namespace secedo
