// genome_bins_test -- the rules of secedo_amd/csrc/genome_bins.hpp on the host, under AddressSanitizer and UBSan: the
// class of every byte value, the name cut (empty lines, stops, the 4096 / 4097 border, a prefix of a longer line), the
// selection and the words of its refusals, the layout and its limit, the piece-to-bin mapping driven the way the
// device drives it (fasta_lines.hpp's walk and Table over ranges of 1 to 64 bytes, then piece_of and bin_of_ordinal
// per sequence byte) against a direct count per contig, and the line with its longest length. Buffers are heap blocks
// of their exact size. Prints "ok <n> checks" and exits 0, or names the first check that failed.
#include "fasta_lines.hpp"
#include "genome_bins.hpp"

#include <cstdio>
#include <cstring>
#include <memory>

using namespace secedo::genomebins;
namespace F = secedo::fasta;

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

struct Heap {  // a heap block of exactly n bytes
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Heap(const std::string &s) : p(new uint8_t[s.size() + (s.empty() ? 1 : 0)]), n(s.size()) {
        std::memcpy(p.get(), s.data(), s.size());
    }
};

bool name_is(const std::string &header, const std::string &want) {
    const Heap h(header);
    uint32_t l = 0;
    if (!cut_name(h.p.get(), h.n, &l)) return false;
    return std::string(reinterpret_cast<const char *>(h.p.get()) + (l ? 1 : 0), l) == want;
}

// the contigs of a text by the line rule, directly: names and sequences
void direct(const std::string &text, std::vector<std::string> *names, std::vector<std::string> *seqs) {
    uint32_t s = F::kLine0;
    bool in_header = false;
    std::string header;
    for (size_t i = 0; i < text.size(); ++i) {
        uint32_t kind;
        s = F::step(s, uint8_t(text[i]), &kind);
        if (kind & F::kHeaderStart) {
            header.clear();
            in_header = true;
            seqs->push_back(std::string());
        }
        if (in_header && text[i] != '\n') header.push_back(text[i]);
        if ((kind & F::kHeaderEnd) || (in_header && i + 1 == text.size())) {
            const Heap h(header);
            uint32_t l = 0;
            cut_name(h.p.get(), h.n, &l);
            names->push_back(header.substr(l ? 1 : 0, l));
            in_header = false;
        }
        if (kind & F::kSeqByte) seqs->back().push_back(text[i]);
    }
}

// The counts of all contigs in file order at bin size S, the way the device route gets them: ranges of `batch` bytes,
// each walked for its slots and then byte by byte through the piece table.
int by_pieces(const std::string &text, uint32_t S, uint32_t batch, const std::vector<std::string> &seqs,
              std::vector<uint32_t> *table) {
    std::vector<uint64_t> bin0(seqs.size() + 1, 0);
    for (size_t c = 0; c < seqs.size(); ++c) bin0[c + 1] = bin0[c] + bd::chr_bins(uint32_t(seqs[c].size()), S);
    table->assign(bin0.back() * kColumns, 0);
    F::Table tab(false, UINT64_MAX);
    uint32_t state = F::kLine0;
    std::vector<F::Table::Piece> fp;
    for (size_t a = 0; a < text.size(); a += batch) {
        const uint32_t len = uint32_t(std::min<size_t>(batch, text.size() - a));
        const Heap range(text.substr(a, len));
        std::vector<uint8_t> slot_bytes(sizeof(F::HeaderSlot) * (len + 2), 0xFF);
        F::HeaderSlot *slots = reinterpret_cast<F::HeaderSlot *>(slot_bytes.data());
        uint32_t seq = 0, headers = 0;
        const uint32_t exit = F::walk(range.p.get(), len, 0, len, state, &seq, &headers, nullptr, slots, len + 2);
        tab.range(F::RangeTotals{headers, seq, exit, 0}, slots, len, &fp);
        std::vector<Piece> pieces;
        for (const F::Table::Piece &p : fp) pieces.push_back(Piece{p.q0, bin0[p.role.chr], p.code_off, p.count});
        uint32_t s = state, o = 0;
        for (uint32_t i = 0; i < len; ++i) {
            uint32_t kind;
            s = F::step(s, range.p[i], &kind);
            if (!(kind & F::kSeqByte)) continue;
            CHECK(!pieces.empty() && pieces[0].code_off == 0);
            const Piece &p = pieces[piece_of(pieces.data(), uint32_t(pieces.size()), o)];
            CHECK(o >= p.code_off && o - p.code_off < p.count);
            uint32_t rem = 0;
            const uint64_t bin = bin_of_ordinal(p, o, S, &rem);
            CHECK(bin < bin0.back() && rem == (p.q0 + (o - p.code_off)) % S);
            (*table)[bin * kColumns + byte_class(range.p[i])] += 1;
            if (byte_masked(range.p[i])) (*table)[bin * kColumns + kMasked] += 1;
            ++o;
        }
        CHECK(o == seq);
        state = exit;
    }
    return 0;
}

int run() {
    // the class of every byte value
    for (uint32_t b = 0; b < 256; ++b) {
        const uint32_t want = std::strchr("Aa", int(b)) && b ? kA : std::strchr("Cc", int(b)) && b ? kC
                            : std::strchr("Gg", int(b)) && b ? kG : std::strchr("TtUu", int(b)) && b ? kT : kOther;
        CHECK(byte_class(uint8_t(b)) == want);
        CHECK(byte_class(uint8_t(b)) == (F::char_to_int(uint8_t(b)) == 5 ? kOther : F::char_to_int(uint8_t(b))));
        CHECK(byte_masked(uint8_t(b)) == (b >= 'a' && b <= 'z'));
    }
    // names
    CHECK(name_is("", "") && name_is(">", "") && name_is("> x", "") && name_is(">chr1", "chr1"));
    CHECK(name_is(">chr1 Homo sapiens", "chr1") && name_is(">a\tb", "a") && name_is(">a\r", "a"));
    CHECK(name_is("ACGT", "CGT") && name_is(">>x", ">x"));
    CHECK(name_is(">" + std::string(kMaxName, 'n'), std::string(kMaxName, 'n')));
    CHECK(name_is(">" + std::string(kMaxName, 'n') + " rest", std::string(kMaxName, 'n')));
    {
        uint32_t l = 0;
        const Heap longer(">" + std::string(kMaxName + 1, 'n'));
        CHECK(longer.n == kHeaderPrefix && !cut_name(longer.p.get(), longer.n, &l) && l == kMaxName + 1);
        const Heap stop_late(">" + std::string(kMaxName + 1, 'n') + " x");
        CHECK(!cut_name(stop_late.p.get(), kHeaderPrefix, &l));
        CHECK(too_long(3) == "contig 3: its name is longer than 4096 bytes");
    }
    // the selection
    {
        const std::vector<std::string> names{"1", "2", "1", "X", ""};
        const std::vector<uint64_t> len{10, 0, 7, 5, 3};
        Selection sel;
        CHECK(select(names, len, nullptr, nullptr, &sel).empty());
        CHECK((sel.contig == std::vector<uint64_t>{0, 1, 3, 4}) && sel.duplicate_names == 1);
        std::vector<std::string> listed{"X", "1"};
        const uint64_t good[2] = {5, 10}, bad[2] = {5, 7};
        CHECK(select(names, len, &listed, good, &sel).empty() && (sel.contig == std::vector<uint64_t>{3, 0}));
        CHECK(select(names, len, &listed, bad, &sel) == "1: the genome has 10 bases, expected 7");
        listed = {"X", "chr1"};
        CHECK(select(names, len, &listed, nullptr, &sel) ==
              "the genome has no contig named 'chr1' (names are matched exactly: no chr prefix is added or removed)");
        listed = {"X", "X"};
        CHECK(select(names, len, &listed, nullptr, &sel) == "contig name 'X' is listed twice");
        listed.clear();
        CHECK(select(names, len, &listed, nullptr, &sel) == "no contig is selected: the list of names is empty");
        listed = {"", "2", "X"};
        CHECK(select(names, len, &listed, nullptr, &sel).empty());
        bd::Layout lay;
        bool limit = true;
        CHECK(make_layout(names, len, sel, 2, &lay, &limit).empty() && !limit);
        CHECK((lay.base == std::vector<uint64_t>{0, 2, 2, 5}) && (lay.len == std::vector<uint32_t>{3, 0, 5}));
        bd::Layout zero;
        CHECK(!make_layout(names, len, sel, 0, &zero, &limit).empty() && !limit);
        const std::vector<uint64_t> huge{10, 0, 7, 1ull << 32, 3}, big{10, 0, 7, 0xFFFFFFFFull, 0xFFFFFFFFull};
        bd::Layout l2, l3;
        CHECK(make_layout(names, huge, sel, 1000, &l2, &limit) ==
                  "X: 4294967296 bases, more than the 2^32 - 1 a contig may have" && limit);
        listed = {"X", ""};
        CHECK(select(names, big, &listed, nullptr, &sel).empty());
        CHECK(make_layout(names, big, sel, 1, &l3, &limit) ==
                  "8589934590 bins up to contig '', more than the 2^32 - 1 a call numbers; use a larger bin_size" && limit);
    }
    // pieces to bins, against a direct count
    const std::vector<std::string> texts{
        ">a\nACGTNacgtnUuRy\nAC\r\n>b x\n>ACGT\nGG\n>c\n>d\n\nTT",
        "\nAC\n>e\nnnnnNNNN\n",
        "ACGT\nGGCC\n>b\nTT\n",
        ">" + std::string(70, 'h') + " tail\n" + std::string(130, 'g') + "\n" + std::string(5, 'N'),
    };
    for (const std::string &text : texts) {
        std::vector<std::string> names, seqs;
        direct(text, &names, &seqs);
        CHECK(names.size() == seqs.size() && !names.empty());
        for (uint32_t S : {1u, 3u, 16u, 64u, 1000u}) {
            std::vector<uint32_t> want;
            for (const std::string &q : seqs)
                for (uint32_t b = 0; b < bd::chr_bins(uint32_t(q.size()), S); ++b) {
                    uint32_t row[kColumns] = {0, 0, 0, 0, 0, 0};
                    for (uint32_t i = bd::bin_start(b, S); i < bd::bin_end(b, S, uint32_t(q.size())); ++i) {
                        row[byte_class(uint8_t(q[i]))] += 1;
                        row[kMasked] += byte_masked(uint8_t(q[i]));
                    }
                    CHECK(row[kA] + row[kC] + row[kG] + row[kT] + row[kOther] ==
                          bd::bin_end(b, S, uint32_t(q.size())) - bd::bin_start(b, S));
                    want.insert(want.end(), row, row + kColumns);
                }
            for (uint32_t batch : {1u, 2u, 7u, 16u, 64u, 100000u}) {
                std::vector<uint32_t> got;
                if (by_pieces(text, S, batch, seqs, &got)) return 1;
                CHECK(got == want);
            }
        }
    }
    // the line
    {
        const uint32_t row[kColumns] = {1, 0, 4294967295u, 7, 10, 3}, top[kColumns] = {4294967295u, 4294967295u,
            4294967295u, 4294967295u, 4294967295u, 4294967295u};
        CHECK(header_line() == "chrom\tstart\tend\ta\tc\tg\tt\tother\tmasked\n");
        CHECK(line("chr1", 0, 1000, row) == "chr1\t0\t1000\t1\t0\t4294967295\t7\t10\t3\n");
        CHECK(line("", 5, 6, row) == "\t5\t6\t1\t0\t4294967295\t7\t10\t3\n");
        CHECK(line("name", 4294967295u, 4294967295u, top).size() == max_line(4));
        CHECK(bd::lines_per_range(1, max_line(4)) == 1);
    }
    return 0;
}

}  // namespace

int main() {
    if (run()) return 1;
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
