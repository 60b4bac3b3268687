// bam_depth.hpp -- everything that decides the numbers and the bytes of secedo_bam_depth (include/secedo_bam.h,
// DESIGN 12v), header-only, in plain C++ that g++ compiles alone (tests/cpp/bam_depth_test.cpp runs it under the
// sanitizers) and that bam_depth_kernels.hip compiles as device code: the bin layout of the requested chromosomes, the
// sort key global_bin * n_cells + cell, the pieces of a record in `bases` mode (how many bins its reference span
// touches, and what an M, = or X op covers of piece j), put_u64 and the lines of the output files. Failures come back
// as the reason's text.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define DEPTH_HD __host__ __device__ inline
#else
#define DEPTH_HD inline
#endif

namespace secedo {
namespace bamdepth {

constexpr int kModeReads = 0, kModeBases = 1;  // SECEDO_BAM_DEPTH_READS, _BASES

// ---- the bin layout. With bin size S >= 1 a chromosome of length ln has ceil(ln / S) bins; bin b covers
// [b * S, min((b + 1) * S, ln)). A position's bin is pos / S.

DEPTH_HD uint32_t chr_bins(uint32_t ln, uint32_t S) { return uint32_t((uint64_t(ln) + S - 1) / S); }
DEPTH_HD uint32_t bin_of(uint32_t pos, uint32_t S) { return pos / S; }
DEPTH_HD uint32_t bin_start(uint32_t b, uint32_t S) { return uint32_t(uint64_t(b) * S); }  // < ln for a bin of the chromosome
DEPTH_HD uint32_t bin_end(uint32_t b, uint32_t S, uint32_t ln) {
    const uint64_t e = (uint64_t(b) + 1) * S;
    return e < ln ? uint32_t(e) : ln;
}

constexpr uint64_t kMaxBins = 0xFFFFFFFFull;  // global bin numbers are u32

// The global bins of the requested chromosomes (ascending ids): chromosome k of the request owns the global bins
// [base[k], base[k + 1]).
struct Layout {
    uint32_t S = 0;
    std::vector<uint32_t> chr, len;  // [n] the @SQ index and LN of each requested chromosome
    std::vector<uint64_t> base;      // [n + 1]
    uint64_t n_bins() const { return base.empty() ? 0 : base.back(); }
};

// Why the layout cannot be made ("" when it can): ids ascending indexes into ref_len. *limit (may be null) = the
// reason is a limit of the call, not a fault of its arguments.
inline std::string make_layout(const std::vector<uint32_t> &ref_len, const std::vector<uint32_t> &ids, uint32_t S,
                               Layout *out, bool *limit = nullptr) {
    if (limit) *limit = false;
    if (S == 0) return "bin_size is 0, at least 1 is needed";
    out->S = S;
    out->base.assign(1, 0);
    for (uint32_t c : ids) {
        if (c >= ref_len.size())
            return "chromosome id " + std::to_string(c) + " is at or past the " + std::to_string(ref_len.size()) +
                   " references";
        out->chr.push_back(c);
        out->len.push_back(ref_len[c]);
        out->base.push_back(out->base.back() + chr_bins(ref_len[c], S));
        if (out->base.back() > kMaxBins) {
            if (limit) *limit = true;
            return std::to_string(out->base.back()) + " bins up to chromosome id " + std::to_string(c) +
                   ", more than the 2^32 - 1 a call numbers; use a larger bin_size";
        }
    }
    return std::string();
}

// the chromosome of the request that owns global bin g < base[n]: the last k with base[k] <= g (chromosomes without
// bins are skipped over)
DEPTH_HD uint32_t chr_of_bin(const uint64_t *base, uint32_t n, uint64_t g) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- the sort key of a piece: global_bin * n_cells + cell, so ascending keys are the output order (bin, then cell)

DEPTH_HD uint64_t pack_key(uint64_t global_bin, uint32_t cell, uint32_t n_cells) { return global_bin * n_cells + cell; }
DEPTH_HD uint32_t key_bin(uint64_t key, uint32_t n_cells) { return uint32_t(key / n_cells); }
DEPTH_HD uint32_t key_cell(uint64_t key, uint32_t n_cells) { return uint32_t(key % n_cells); }

// the key bits in use with n_bins >= 1 bins and n_cells >= 1 cells (at most 2^32 - 1 and 2^14: 46 bits): the radix
// sort's end bit, at least 1
inline int key_bits(uint64_t n_bins, uint32_t n_cells) {
    const uint64_t max_key = n_bins * n_cells - 1;
    int b = 1;
    while (b < 64 && (max_key >> b) != 0) ++b;
    return b;
}

// ---- `bases` mode. A BAM CIGAR op is the little-endian u32 len << 4 | op with op in MIDNSHP=X order. M, = and X
// cover reference positions; they, D and N advance the position; I, S, H and P do neither.

DEPTH_HD uint32_t cigar_word(const uint8_t *cigar, uint32_t k) {
    const uint8_t *p = cigar + 4ull * k;
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}
DEPTH_HD bool op_covers(uint32_t op) { return op == 0 || op == 7 || op == 8; }
DEPTH_HD bool op_advances(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// the reference positions a record's CIGAR spans (0 without a CIGAR)
DEPTH_HD uint64_t ref_span(const uint8_t *cigar, uint32_t n_cigar) {
    uint64_t span = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t w = cigar_word(cigar, k);
        if (op_advances(w & 15)) span += w >> 4;
    }
    return span;
}

// How many bins the span [pos, pos + span) touches inside the chromosome (pos < ln): the record's pieces. Piece j is
// bin pos / S + j. A span of 0 touches none.
DEPTH_HD uint32_t touched_bins(uint32_t pos, uint64_t span, uint32_t ln, uint32_t S) {
    if (span == 0 || pos >= ln) return 0;
    const uint64_t end = uint64_t(pos) + span < ln ? uint64_t(pos) + span : ln;
    return uint32_t((end - 1) / S) - pos / S + 1;
}

// The positions of piece j (bin pos / S + j, which touched_bins counted) that an M, = or X op covers. May be 0: an N
// or a D over the whole bin. The walk stops at the first op that starts at or behind the bin's end.
DEPTH_HD uint32_t piece_covered(const uint8_t *cigar, uint32_t n_cigar, uint32_t pos, uint32_t ln, uint32_t S,
                                uint32_t j) {
    const uint32_t b = pos / S + j;
    const uint64_t lo = bin_start(b, S), hi = bin_end(b, S, ln);
    uint64_t p = pos, covered = 0;
    for (uint32_t k = 0; k < n_cigar && p < hi; ++k) {
        const uint32_t w = cigar_word(cigar, k);
        if (!op_advances(w & 15)) continue;
        const uint64_t e = p + (w >> 4);
        if (op_covers(w & 15)) {
            const uint64_t a = p > lo ? p : lo, z = e < hi ? e : hi;
            if (z > a) covered += z - a;
        }
        p = e;
    }
    return uint32_t(covered);
}

// ---- text. A sink takes one char at a time through put(char) (text_sink.hpp's on the device).

// std::to_string of a u64: decimal, no padding, correct up to 2^64 - 1
template <class Sink>
DEPTH_HD void put_u64(Sink &s, uint64_t v) {
    uint64_t pow = 1;
    while (v / pow >= 10) pow *= 10;  // v / pow < 10 is reached at 10^19 at the latest, which a u64 holds
    for (; pow; pow /= 10) s.put(char('0' + (v / pow) % 10));
}

template <class Sink>
DEPTH_HD void put_bytes(Sink &s, const uint8_t *p, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) s.put(char(p[k]));
}

// names one after the other, as the kernels of both table writers read them (text_out.hpp uploads them):
// off[i] .. off[i + 1] is name i
struct Names {
    const uint8_t *bytes;
    const uint32_t *off;
};

// depth.counts.mtx: "<bin + 1>\t<cell + 1>\t<value>\n"
template <class Sink>
DEPTH_HD void put_mtx_line(Sink &s, uint32_t bin, uint32_t cell, uint64_t value) {
    put_u64(s, uint64_t(bin) + 1);
    s.put('\t');
    put_u64(s, uint64_t(cell) + 1);
    s.put('\t');
    put_u64(s, value);
    s.put('\n');
}

// what depth.cells.tsv says of a cell, in column order
struct CellRow {
    uint64_t records, counted, sum, nonzero_bins, max_value;
};
constexpr uint32_t kCellColumns = 5;

// depth.cells.tsv: "<cell>\t<name>\t<records>\t<counted>\t<sum>\t<nonzero_bins>\t<max_value>\n"
template <class Sink>
DEPTH_HD void put_cell_line(Sink &s, uint32_t cell, const uint8_t *name, uint32_t name_len, const CellRow &r) {
    put_u64(s, cell);
    s.put('\t');
    put_bytes(s, name, name_len);
    const uint64_t v[kCellColumns] = {r.records, r.counted, r.sum, r.nonzero_bins, r.max_value};
    for (uint32_t k = 0; k < kCellColumns; ++k) {
        s.put('\t');
        put_u64(s, v[k]);
    }
    s.put('\n');
}

// depth.bins.bed and the first three columns of depth.clusters.tsv: "<name>\t<start>\t<end>", 0-based half-open
template <class Sink>
DEPTH_HD void put_bin(Sink &s, const uint8_t *name, uint32_t name_len, uint32_t start, uint32_t end) {
    put_bytes(s, name, name_len);
    s.put('\t');
    put_u64(s, start);
    s.put('\t');
    put_u64(s, end);
}

// depth.clusters.tsv: the bin, then "\t<sum>" per cluster, then "\n"
template <class Sink>
DEPTH_HD void put_cluster_line(Sink &s, const uint8_t *name, uint32_t name_len, uint32_t start, uint32_t end,
                               const uint64_t *sums, uint32_t n_clusters) {
    put_bin(s, name, name_len, start, end);
    for (uint32_t k = 0; k < n_clusters; ++k) {
        s.put('\t');
        put_u64(s, sums[k]);
    }
    s.put('\n');
}

// the longest a line can be: what a range of lines is sized by (a u64 has at most 20 digits, a u32 10)
constexpr uint64_t kMaxMtxLine = 10 + 1 + 10 + 1 + 20 + 1;
inline uint64_t max_cell_line(uint64_t name_len) { return 10 + 1 + name_len + kCellColumns * 21 + 1; }
inline uint64_t max_cluster_line(uint64_t name_len, uint32_t n_clusters) {
    return name_len + 1 + 10 + 1 + 10 + uint64_t(n_clusters) * 21 + 1;
}
// lines per range of at most `batch` bytes: one at the least
inline uint64_t lines_per_range(uint64_t batch, uint64_t max_line) { return batch / max_line ? batch / max_line : 1; }

struct StringSink {
    std::string out;
    void put(char c) { out.push_back(c); }
};

inline std::string mtx_header(uint64_t n_bins, uint64_t n_cells, uint64_t nnz) {
    return "%%MatrixMarket matrix coordinate integer general\n%\n" + std::to_string(n_bins) + "\t" +
           std::to_string(n_cells) + "\t" + std::to_string(nnz) + "\n";
}
inline std::string cells_header() { return "cell\tname\trecords\tcounted\tsum\tnonzero_bins\tmax_value\n"; }
inline std::string clusters_header(uint32_t n_clusters) {
    std::string t = "chrom\tstart\tend";
    for (uint32_t k = 0; k < n_clusters; ++k) t += "\tcluster_" + std::to_string(k);
    return t + "\n";
}
inline std::string bed_line(const std::string &name, uint32_t start, uint32_t end) {
    StringSink s;
    put_bin(s, reinterpret_cast<const uint8_t *>(name.data()), uint32_t(name.size()), start, end);
    return s.out + "\n";
}

// Why `names` cannot name the cells ("" when they can): the rule of secedo_variant_set_cell_names.
inline std::string cell_names_fault(const std::vector<std::string> &names) {
    for (size_t c = 0; c < names.size(); ++c)
        if (names[c].empty() || names[c].find_first_of("\t\n\r") != std::string::npos)
            return "cell name " + std::to_string(c) + " is empty or holds a tab or a line break";
    return std::string();
}

}  // namespace bamdepth
}  // namespace secedo
