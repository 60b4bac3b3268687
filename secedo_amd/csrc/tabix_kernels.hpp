// tabix_kernels.hpp -- launch wrappers of tabix_kernels.hip (gfx950): what a .tbi index needs of the lines of VCF texts
// that lie back to back in HBM (vcf::DeviceText after format_device, or what the device inflate leaves of .vcf.gz
// files). See tabix_kernels.hip for the passes; tabix_api.cpp drives them and feeds tabix_build.hpp.
//
// The text is walked in ranges [a, a + n) that begin at line starts (a file's first byte, or the byte behind a '\n')
// and end at one or at the text's end. A range is at most the batch budget: 64 MiB of text by default, and whatever the
// environment variable SECEDO_TABIX_BATCH_BYTES says instead (read once per call, at least 64 bytes; for tests: a small
// value walks a small file in many ranges). A line longer than the budget stretches its range. The results never depend
// on the budget: a run head is started at every range start and the host builder joins a head that continues the run
// under way.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace tabix {

constexpr uint64_t kDefaultBudget = 64ull << 20, kMinBudget = 64, kMaxRange = 1ull << 30;
// Windows emitted per range at the most (1.5 GiB of Win): a line can touch 32768 windows and each (file, name) segment
// starts its windows anew, so a small crafted text asks for billions. A range past the cap is refused before anything
// is emitted. SECEDO_TABIX_MAX_WINDOWS lowers it (read once per call; for tests).
constexpr uint64_t kMaxRangeWindows = 1ull << 26;
// bytes the kernels may read beyond the text's ends (whole 16-byte vectors), as kDeflateInSlack
constexpr uint32_t kTextSlack = 16;

enum Err : uint32_t { kErrColumns = 1, kErrPos = 2, kErrEnd = 3, kErrOrder = 4 };
constexpr uint64_t kNoErr = ~0ull;

// the texts: file f is bytes [file_off[f], file_off[f + 1]) of text; kTextSlack readable bytes before and after the whole
struct Text {
    const uint8_t *text;
    const uint64_t *file_off;  // device, [n_files + 1]
    uint32_t n_files;
};

// one range: n <= kMaxRange text bytes from a; files f_lo..f_hi are those with bytes in it
struct Range {
    uint64_t a;
    uint32_t n, f_lo, f_hi;
};

// the last data line in front of a range, for the name and order rules across a range boundary
struct Carry {
    uint64_t name_at, pos;  // name_at: text offset of its first byte
    uint32_t name_len, file, valid, reserved;
};

// Segments number the (file, name) blocks of a range: seg k >= 1 starts at the range's k-th name change, seg 0 is the
// block the carry line belongs to. Ordinals and line numbers of a file count from the range's start where the file
// began in front of it, else from the file's start; the host adds what lay in front.
struct Head {
    uint64_t off;  // of the line's first byte, from its file's start
    uint32_t file, seg, bin, ord;  // ord: the line's number among the data lines
};
struct Win {
    uint64_t off;
    uint32_t file, seg, w, reserved;
};
struct Change {
    uint64_t name_at;  // text offset of the name
    uint32_t name_len, file, line, reserved;  // line: 0-based, every line counted
};

struct Tail {
    uint64_t err;  // kNoErr, else the lowest (data line of the range) << 8 | Err
    uint64_t n_wins;  // 64 bits as in the BAI pass: a line can touch 32768 windows, and every segment starts anew
    uint32_t err_file, err_line;  // of that line, as Change::line
    uint32_t n_heads, n_changes;
    Carry carry;  // the range's last data line; the one given where it has none
};

// Device arrays of one range. by_chunk: per 16 text bytes; by_line: per data line; by_file: per file of the range.
struct Work {
    uint32_t *file_bits;                    // [chunks / 2 + 1]
    uint64_t *chunk_cnt, *chunk_scan;       // [chunks + 1]: lines | data lines << 32
    uint32_t *first_line, *first_data;      // [files of the range]
    uint32_t *start, *line, *file, *name_len, *beg, *end, *bin;  // [data lines]
    uint64_t *pos, *key, *key_max;          // [data lines]
    uint32_t *change, *seg_ex, *head, *head_scan;  // [data lines + 1]
    uint64_t *n_win, *n_win_scan;           // [data lines + 1]
    uint64_t *err;
    Tail *tail;
    void *scan_tmp;
    size_t scan_bytes;
};

inline uint32_t range_chunks(const Text &t, const Range &r) {
    const uint64_t shift = (reinterpret_cast<uintptr_t>(t.text) + r.a) & 15;
    return uint32_t((shift + r.n + 15) / 16);
}

// scan_tmp bytes for a range of `chunks` chunks and `lines` data lines
size_t scan_workspace(uint64_t chunks, uint64_t lines);

// The line starts: w.chunk_scan[chunks] = lines | data lines << 32 of the range. Needs file_bits, chunk_cnt, chunk_scan.
hipError_t mark_lines(const Text &t, const Range &r, const Work &w, hipStream_t s);

// Everything per data line (n_data of them, as mark_lines counted) and *w.tail.
hipError_t index_lines(const Text &t, const Range &r, const Carry &carry, uint32_t n_data, const Work &w, hipStream_t s);

// The heads, windows and name changes, each in line order; sized by *w.tail, whose n_wins the caller has held against
// its cap: d_wins has room for all of them.
hipError_t emit(const Text &t, const Range &r, uint32_t n_data, const Work &w, Head *d_heads, Win *d_wins,
                Change *d_changes, hipStream_t s);

// name k = text bytes [name_at[k], name_at[k] + len[k]) to d_out + out_at[k]
hipError_t gather_names(const Text &t, const uint64_t *d_name_at, const uint32_t *d_len, const uint64_t *d_out_at,
                        uint32_t n, uint8_t *d_out, hipStream_t s);

}  // namespace tabix
}  // namespace secedo
