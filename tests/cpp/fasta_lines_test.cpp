// fasta_lines_test -- the line roles, the range carry and the contig assignment of secedo_amd/csrc/fasta_lines.hpp as
// a host program (built with -fsanitize=address,undefined; tests/test_fasta_lines_cpu.py runs it). It does on the host
// what the device passes do: every range is cut into chunks, each chunk becomes a transfer function, the functions
// are composed in an exclusive scan, the chunks are counted and walked from their entry states, and the header table
// of the range goes to fasta::Table; the pieces it returns are put together into the chromosomes.
//
// usage: fasta_lines_test CASES RANGE CHUNK N_CHR
//   CASES: a file of cases, each a u32 length (little endian), a diploid byte and the text; RANGE: bytes per range
//   (0: the whole text); CHUNK: bytes per chunk. One line per case:
//     R <H or S per line> | C <header_len>:<byte 1>:<seq_len> ... | G <chromosome>;... or E <message>
//   a chromosome's genotypes as characters '0' + code.
#include "fasta_lines.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

namespace F = secedo::fasta;

namespace {

struct Text {
    const uint8_t *p;
    uint8_t operator[](uint32_t i) const { return p[i]; }
};

std::string run_case(const std::vector<uint8_t> &text, bool diploid, uint32_t range, uint32_t chunk, uint32_t n_chr) {
    std::string out = "R ";
    {  // the roles, from the machine run over the whole text
        uint32_t s = F::kLine0;
        for (uint8_t b : text) {
            uint32_t kind;
            const bool line_start = s <= F::kAfterSeq;
            s = F::step(s, b, &kind);
            if (line_start) out += (kind & F::kHeaderStart) ? 'H' : 'S';
        }
    }
    const uint32_t needed = 2 * n_chr + 1, cap = needed + 2;
    F::Table table(diploid, needed);
    std::vector<std::vector<uint8_t>> mat(n_chr), pat(n_chr);
    uint32_t state = F::kLine0;
    const uint32_t n = uint32_t(text.size());
    if (range == 0) range = n ? n : 1;
    std::vector<F::Table::Piece> pieces;
    for (uint32_t r0 = 0; r0 < n; r0 += range) {
        const uint32_t len = std::min(range, n - r0);
        // an exact-size copy: a read past the range is a read past the allocation
        std::vector<uint8_t> copy(text.begin() + r0, text.begin() + r0 + len);
        const Text t{copy.data()};
        const uint32_t chunks = (len + chunk - 1) / chunk;
        std::vector<F::Transfer> tf(chunks), tf_in(chunks);
        for (uint32_t j = 0; j < chunks; ++j) tf[j] = F::transfer_of(t, j * chunk, std::min(chunk, len - j * chunk));
        F::Transfer acc = F::kIdentity;
        for (uint32_t j = 0; j < chunks; ++j) {
            tf_in[j] = acc;
            acc = F::compose(acc, tf[j]);
        }
        std::vector<uint32_t> seq_before(chunks), hdr_before(chunks);
        uint32_t seq = 0, headers = 0;
        for (uint32_t j = 0; j < chunks; ++j) {
            seq_before[j] = seq, hdr_before[j] = headers;
            F::walk(t, len, j * chunk, std::min(chunk, len - j * chunk), F::apply(tf_in[j], state), &seq, &headers, nullptr,
                    nullptr, 0);
        }
        std::vector<uint8_t> codes(seq);  // exactly the range's bases: a store past them is a store past the allocation
        std::vector<F::HeaderSlot> slots(cap, F::HeaderSlot{F::kNone, F::kNone, F::kNone, F::kNone});
        F::RangeTotals totals{0, 0, state, 0};
        for (uint32_t j = chunks; j-- > 0;) {  // any order: the chunks are independent once their entries are known
            uint32_t s2 = seq_before[j], h2 = hdr_before[j];
            const uint32_t exit = F::walk(t, len, j * chunk, std::min(chunk, len - j * chunk), F::apply(tf_in[j], state),
                                          &s2, &h2, codes.data(), slots.data(), cap);
            if (j == chunks - 1) totals = F::RangeTotals{h2, s2, exit, 0};
        }
        if (totals.state != F::apply(acc, state)) return "E the scan and the walk disagree on the exit state";
        table.range(totals, slots.data(), len, &pieces);
        state = totals.state;
        for (const F::Table::Piece &p : pieces) {
            if (p.role.chr >= n_chr) continue;
            std::vector<uint8_t> &dst = (p.role.slot ? pat : mat)[p.role.chr];
            if (dst.size() != p.q0) return "E a piece does not continue its contig";
            dst.insert(dst.end(), codes.begin() + p.code_off, codes.begin() + p.code_off + p.count);
        }
    }
    table.finish();
    out += " | C";
    for (const F::Contig &c : table.contigs)
        out += " " + std::to_string(c.header_len) + ":" + std::to_string(c.b1) + ":" + std::to_string(c.seq_len);
    std::vector<uint64_t> len;
    std::vector<uint8_t> hap;
    std::vector<uint32_t> source;
    const std::string err = F::resolve(table.assign.chroms, table.contigs, n_chr, &len, &hap, &source);
    if (!err.empty()) return out + " | E " + err;
    out += " | G ";
    for (uint32_t c = 0; c < n_chr; ++c) {
        const std::vector<uint8_t> &m = mat[source[c]], &p = pat[source[c]];
        if (m.size() != len[c] || (!hap[c] && p.size() != len[c])) return out + " | E pieces and lengths disagree";
        for (size_t i = 0; i < m.size(); ++i) out += char('0' + (m[i] << 3 | (hap[c] ? m[i] : p[i])));
        out += ';';
    }
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s CASES RANGE CHUNK N_CHR\n", argv[0]);
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const uint32_t range = uint32_t(std::strtoul(argv[2], nullptr, 10));
    const uint32_t chunk = std::max<uint32_t>(1, uint32_t(std::strtoul(argv[3], nullptr, 10)));
    const uint32_t n_chr = uint32_t(std::strtoul(argv[4], nullptr, 10));
    size_t at = 0;
    while (at + 5 <= data.size()) {
        uint32_t n;
        std::memcpy(&n, data.data() + at, 4);
        const bool diploid = data[at + 4] != 0;
        at += 5;
        if (n > data.size() - at) return 3;
        const std::vector<uint8_t> text(data.begin() + at, data.begin() + at + n);
        at += n;
        std::printf("%s\n", run_case(text, diploid, range, chunk, n_chr).c_str());
    }
    return 0;
}
