// bam_depth_test -- the rules of secedo_amd/csrc/bam_depth.hpp on the host, under AddressSanitizer and UBSan: the bin
// layout at LN % S == 0, LN % S == 1, S > LN and S == 1 (and its refusals), the key round trip at the largest bin and
// cell numbers with the radix sort's end bit, the piece rule on hand-made CIGARs (clips in front and behind, an I, a D
// that ends exactly on a bin border, an N that skips a whole bin, a span that runs past LN, = and X, no CIGAR) against
// a position-by-position count, put_u64 at the edges of its digit counts, and the line formats. CIGARs live in heap
// blocks of their exact size. Prints "ok <n> checks" and exits 0, or names the first check that failed.
#include "bam_depth.hpp"

#include <cstdio>
#include <memory>
#include <utility>

using namespace secedo::bamdepth;

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

using Ops = std::vector<std::pair<char, uint32_t>>;

// the BAM CIGAR words of ops, in a heap block of exactly 4 bytes per op
struct Cigar {
    std::unique_ptr<uint8_t[]> bytes;
    uint32_t n;
    explicit Cigar(const Ops &ops) : bytes(new uint8_t[4 * ops.size() + (ops.empty() ? 1 : 0)]), n(uint32_t(ops.size())) {
        const std::string codes = "MIDNSHP=X";
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t w = ops[k].second << 4 | uint32_t(codes.find(ops[k].first));
            for (int b = 0; b < 4; ++b) bytes[4 * k + b] = uint8_t(w >> (8 * b));
        }
    }
};

// position by position: what M, = and X cover of each bin, below ln
std::vector<uint32_t> by_position(const Ops &ops, uint32_t pos, uint32_t ln, uint32_t S) {
    std::vector<uint32_t> bins(chr_bins(ln, S), 0);
    uint64_t p = pos;
    for (const auto &op : ops) {
        const bool covers = op.first == 'M' || op.first == '=' || op.first == 'X';
        const bool advances = covers || op.first == 'D' || op.first == 'N';
        if (!advances) continue;
        uint32_t k = 0;
        for (; k < op.second && p < ln; ++k, ++p)
            if (covers) ++bins[p / S];
        p += op.second - k;  // past ln nothing is counted
    }
    return bins;
}

// the pieces of a record against by_position: every touched bin's value, nothing outside them
int check_pieces(const Ops &ops, uint32_t pos, uint32_t ln, uint32_t S, uint32_t want_touched) {
    const Cigar c(ops);
    const std::vector<uint32_t> want = by_position(ops, pos, ln, S);
    const uint32_t touched = touched_bins(pos, ref_span(c.bytes.get(), c.n), ln, S);
    CHECK(touched == want_touched);
    uint64_t sum = 0, want_sum = 0;
    for (uint32_t j = 0; j < touched; ++j) {
        const uint32_t b = pos / S + j;
        CHECK(b < want.size());
        CHECK(piece_covered(c.bytes.get(), c.n, pos, ln, S, j) == want[b]);
        sum += want[b];
    }
    for (uint32_t v : want) want_sum += v;
    CHECK(sum == want_sum);  // nothing is covered outside the touched bins
    return 0;
}

std::string u64_text(uint64_t v) {
    StringSink s;
    put_u64(s, v);
    return s.out;
}

int layout_checks() {
    // LN % S == 0, LN % S == 1, S > LN, S == 1
    CHECK(chr_bins(100000, 1000) == 100 && bin_end(99, 1000, 100000) == 100000 && bin_start(99, 1000) == 99000);
    CHECK(chr_bins(100001, 1000) == 101 && bin_start(100, 1000) == 100000 && bin_end(100, 1000, 100001) == 100001);
    CHECK(chr_bins(100000, 150000) == 1 && bin_start(0, 150000) == 0 && bin_end(0, 150000, 100000) == 100000);
    CHECK(chr_bins(300, 1) == 300 && bin_of(299, 1) == 299 && bin_end(299, 1, 300) == 300);
    CHECK(chr_bins(100000, 30000) == 4 && bin_end(3, 30000, 100000) == 100000 && bin_of(99999, 30000) == 3);
    CHECK(chr_bins(0, 7) == 0);
    CHECK(chr_bins(0xFFFFFFFFu, 1) == 0xFFFFFFFFu && bin_end(0xFFFFFFFEu, 1, 0xFFFFFFFFu) == 0xFFFFFFFFu);
    CHECK(chr_bins(0xFFFFFFFFu, 0xFFFFFFFFu) == 1 && bin_end(0, 0xFFFFFFFFu, 0xFFFFFFFFu) == 0xFFFFFFFFu);
    CHECK(bin_of(0, 1000) == 0 && bin_of(999, 1000) == 0 && bin_of(1000, 1000) == 1);

    const std::vector<uint32_t> lens{100000, 0, 100001, 300};
    Layout lay;
    bool limit = true;
    CHECK(make_layout(lens, {0, 1, 2, 3}, 1000, &lay, &limit).empty() && !limit);
    CHECK(lay.base == (std::vector<uint64_t>{0, 100, 100, 201, 202}) && lay.n_bins() == 202);
    CHECK(lay.chr == (std::vector<uint32_t>{0, 1, 2, 3}) && lay.len == lens);
    // the owner of a global bin; the chromosome without bins owns none
    CHECK(chr_of_bin(lay.base.data(), 4, 0) == 0 && chr_of_bin(lay.base.data(), 4, 99) == 0);
    CHECK(chr_of_bin(lay.base.data(), 4, 100) == 2 && chr_of_bin(lay.base.data(), 4, 200) == 2);
    CHECK(chr_of_bin(lay.base.data(), 4, 201) == 3);
    Layout sub;
    CHECK(make_layout(lens, {2}, 1000, &sub).empty() && sub.base == (std::vector<uint64_t>{0, 101}));
    Layout bad;
    CHECK(make_layout(lens, {0}, 0, &bad, &limit).find("bin_size is 0") == 0 && !limit);
    Layout past;
    CHECK(make_layout(lens, {4}, 10, &past, &limit).find("chromosome id 4 is at or past the 4 references") == 0 && !limit);
    Layout many;
    const std::vector<uint32_t> big{0xFFFFFFFFu, 1};
    CHECK(make_layout(big, {0}, 1, &many, &limit).empty());
    Layout over;
    CHECK(make_layout(big, {0, 1}, 1, &over, &limit).find("4294967296 bins up to chromosome id 1") == 0 && limit);
    return 0;
}

int key_checks() {
    const uint32_t max_cells = 16384;
    const uint64_t max_bin = kMaxBins - 1;
    const uint64_t k = pack_key(max_bin, max_cells - 1, max_cells);
    CHECK(key_bin(k, max_cells) == max_bin && key_cell(k, max_cells) == max_cells - 1);
    CHECK(key_bits(kMaxBins, max_cells) == 46 && (k >> 46) == 0 && (k >> 45) == 1);
    CHECK(key_bits(1, 1) == 1 && key_bits(1, 2) == 1 && key_bits(2, 2) == 2 && key_bits(3, 12) == 6);
    for (uint32_t n_cells : {1u, 3u, 12u, 16384u})
        for (uint64_t bin : {uint64_t(0), uint64_t(1), uint64_t(201), max_bin})
            for (uint32_t cell : {0u, n_cells / 2, n_cells - 1}) {
                const uint64_t key = pack_key(bin, cell, n_cells);
                CHECK(key_bin(key, n_cells) == bin && key_cell(key, n_cells) == cell);
                CHECK(bin == max_bin || pack_key(bin + 1, 0, n_cells) > key);  // bin first, then cell
                CHECK((key >> key_bits(max_bin + 1, n_cells)) == 0);
            }
    return 0;
}

int piece_checks() {
    const uint32_t LN = 100000, S = 1000;
    if (check_pieces({{'M', 50}}, 10, LN, S, 1)) return 1;
    if (check_pieces({{'M', 50}}, 980, LN, S, 2)) return 1;                                    // across a border
    if (check_pieces({{'S', 5}, {'M', 30}, {'S', 7}}, 990, LN, S, 2)) return 1;                // soft clips around
    if (check_pieces({{'H', 5}, {'M', 30}, {'H', 7}}, 990, LN, S, 2)) return 1;                // hard clips around
    if (check_pieces({{'H', 2}, {'S', 3}, {'M', 10}, {'I', 4}, {'M', 10}, {'S', 1}}, 995, LN, S, 2)) return 1;  // an I
    if (check_pieces({{'M', 10}, {'D', 10}, {'M', 10}}, 1980, LN, S, 2)) return 1;             // the D ends on the border
    if (check_pieces({{'M', 10}, {'D', 10}}, 1980, LN, S, 1)) return 1;                        // and ends the span there
    if (check_pieces({{'M', 10}, {'N', 1000}, {'M', 10}}, 2990, LN, S, 3)) return 1;           // an N skips bin 3 whole
    if (check_pieces({{'M', 10}, {'N', 2500}, {'M', 10}, {'P', 3}}, 2995, LN, S, 4)) return 1;
    if (check_pieces({{'=', 10}, {'X', 1}, {'=', 10}}, 3995, LN, S, 2)) return 1;              // = and X
    if (check_pieces({{'M', 100}}, LN - 50, LN, S, 1)) return 1;                               // past LN
    if (check_pieces({{'M', 3000}}, LN - 1500, LN, S, 2)) return 1;
    if (check_pieces({{'M', 50}}, LN - 1, LN, S, 1)) return 1;
    if (check_pieces({}, 500, LN, S, 0)) return 1;                                             // no CIGAR
    if (check_pieces({{'S', 10}, {'I', 5}}, 500, LN, S, 0)) return 1;                          // nothing on the reference
    if (check_pieces({{'M', 70000}}, 500, LN, S, 71)) return 1;                                // a long read
    if (check_pieces({{'M', 70000}}, 0, LN, S, 70)) return 1;
    if (check_pieces({{'M', 20}}, 290, 300, 1, 10)) return 1;                                  // S == 1, past LN
    if (check_pieces({{'M', 20}}, 5, 100000, 150000, 1)) return 1;                             // S > LN
    if (check_pieces({{'M', 1000}}, 29500, 100000, 30000, 2)) return 1;                        // a short last bin
    if (check_pieces({{'M', 20000}}, 85000, 100000, 30000, 2)) return 1;
    {  // many ops: 80 of alternating M and D, crossing two borders
        Ops ops;
        for (int k = 0; k < 80; ++k) ops.push_back({k % 2 ? 'D' : 'M', uint32_t(20 + k % 7)});
        if (check_pieces(ops, 500, LN, S, 3)) return 1;
    }
    // the largest op length, far past LN: no overflow
    if (check_pieces({{'M', 0x0FFFFFFF}}, LN - 10, LN, S, 1)) return 1;
    const Cigar wide({{'N', 0x0FFFFFFF}, {'N', 0x0FFFFFFF}, {'M', 5}});
    CHECK(ref_span(wide.bytes.get(), wide.n) == 2ull * 0x0FFFFFFF + 5);
    CHECK(touched_bins(0, ref_span(wide.bytes.get(), wide.n), 0xFFFFFFFFu, 0xFFFFFFFFu) == 1);
    CHECK(touched_bins(LN, 10, LN, S) == 0);  // a position at LN has no piece
    return 0;
}

int text_checks() {
    CHECK(u64_text(0) == "0" && u64_text(9) == "9" && u64_text(10) == "10");
    CHECK(u64_text(4294967295ull) == "4294967295" && u64_text(4294967296ull) == "4294967296");
    CHECK(u64_text(18446744073709551615ull) == "18446744073709551615");
    CHECK(u64_text(9999999999999999999ull) == "9999999999999999999" && u64_text(10000000000000000000ull) == "10000000000000000000");
    for (uint64_t v = 1; v < (1ull << 62); v *= 7) CHECK(u64_text(v) == std::to_string(v) && u64_text(v - 1) == std::to_string(v - 1));

    StringSink m;
    put_mtx_line(m, 0, 11, 3);
    put_mtx_line(m, 0xFFFFFFFEu, 16383, 18446744073709551615ull);
    CHECK(m.out == "1\t12\t3\n4294967295\t16384\t18446744073709551615\n");
    CHECK(m.out.size() - 7 <= kMaxMtxLine);  // the second line is as long as a line gets but for the cell
    CHECK(mtx_header(202, 12, 7) == "%%MatrixMarket matrix coordinate integer general\n%\n202\t12\t7\n");
    CHECK(cells_header() == "cell\tname\trecords\tcounted\tsum\tnonzero_bins\tmax_value\n");
    CHECK(clusters_header(3) == "chrom\tstart\tend\tcluster_0\tcluster_1\tcluster_2\n");
    CHECK(clusters_header(0) == "chrom\tstart\tend\n");
    CHECK(bed_line("chr1", 99000, 100000) == "chr1\t99000\t100000\n");

    const std::string name = "cell A";
    const uint8_t *np = reinterpret_cast<const uint8_t *>(name.data());
    StringSink c;
    put_cell_line(c, 7, np, uint32_t(name.size()), CellRow{5, 4, 40, 2, 25});
    CHECK(c.out == "7\tcell A\t5\t4\t40\t2\t25\n");
    StringSink widest;
    const uint64_t top = 18446744073709551615ull;
    put_cell_line(widest, 16383, np, uint32_t(name.size()), CellRow{top, top, top, top, top});
    CHECK(widest.out.size() <= max_cell_line(name.size()));
    const uint64_t sums[3] = {0, 12, top};
    StringSink k;
    put_cluster_line(k, np, uint32_t(name.size()), 99000, 100000, sums, 3);
    CHECK(k.out == "cell A\t99000\t100000\t0\t12\t18446744073709551615\n");
    CHECK(k.out.size() <= max_cluster_line(name.size(), 3));
    StringSink k0;
    put_cluster_line(k0, np, 0, 0, 1, sums, 0);
    CHECK(k0.out == "\t0\t1\n");
    CHECK(lines_per_range(256ull << 20, kMaxMtxLine) == (256ull << 20) / 43 && lines_per_range(1, kMaxMtxLine) == 1);

    CHECK(cell_names_fault({"a", "b c", "d"}).empty());
    CHECK(cell_names_fault({"a", ""}) == "cell name 1 is empty or holds a tab or a line break");
    CHECK(cell_names_fault({"a\tb"}) == "cell name 0 is empty or holds a tab or a line break");
    CHECK(!cell_names_fault({"a", "b", "c\n"}).empty() && !cell_names_fault({"\r"}).empty());
    return 0;
}

}  // namespace

int main() {
    if (layout_checks() || key_checks() || piece_checks() || text_checks()) return 1;
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
