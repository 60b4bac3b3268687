// bam_index_test -- secedo_amd/csrc/bam_index.hpp on the host, under AddressSanitizer and UBSan.
//   bam_index_test ranges <index> [<bam> <n_ref>]
//       prints "ref r beg_coffset:beg_uoffset end_coffset:end_uoffset count" per reference (count -1: no pseudo-bin),
//       or "rejected: <why>"; with a BAM the file-level checks are made too.
//   bam_index_test mutate <index> <bam> <n_ref> <seed> <rounds>
//       parses and checks the index cut at every byte and <rounds> copies with random bytes changed, each from a
//       heap block of its exact size, so a read past the bytes is a sanitizer report. Prints "parsed a rejected b".
// Exit 0 unless the arguments are wrong; whatever the bytes hold, the reader must parse or reject them.
#include "bam_index.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

using namespace secedo::bamindex;

namespace {

// parse and check a copy of exactly n bytes
std::string run(const uint8_t *d, size_t n, const std::vector<uint8_t> *bam, uint32_t n_ref, std::vector<RefRange> *refs) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(exact.get(), d, n);
    std::string why = parse(exact.get(), n, refs);
    if (why.empty() && bam) why = check(*refs, n_ref, bam->data(), bam->size());
    return why;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    std::vector<uint8_t> index, bam;
    if (mode == "ranges" && (argc == 3 || argc == 5)) {
        if (!read_file(argv[2], &index) || (argc == 5 && !read_file(argv[3], &bam))) return 2;
        std::vector<RefRange> refs;
        const std::string why = run(index.data(), index.size(), argc == 5 ? &bam : nullptr,
                                    argc == 5 ? uint32_t(std::strtoul(argv[4], nullptr, 10)) : 0, &refs);
        if (!why.empty()) {
            std::printf("rejected: %s\n", why.c_str());
            return 0;
        }
        for (size_t r = 0; r < refs.size(); ++r)
            std::printf("ref %zu %s %s %lld\n", r, voffset_str(refs[r].beg).c_str(), voffset_str(refs[r].end).c_str(),
                        refs[r].count == kNoCount ? -1ll : (long long)refs[r].count);
        return 0;
    }
    if (mode == "mutate" && argc == 7) {
        if (!read_file(argv[2], &index) || !read_file(argv[3], &bam)) return 2;
        const uint32_t n_ref = uint32_t(std::strtoul(argv[4], nullptr, 10));
        std::mt19937_64 rng(std::strtoull(argv[5], nullptr, 10));
        const unsigned long rounds = std::strtoul(argv[6], nullptr, 10);
        unsigned long parsed = 0, rejected = 0;
        std::vector<RefRange> refs;
        for (size_t n = 0; n <= index.size(); ++n) (run(index.data(), n, &bam, n_ref, &refs).empty() ? parsed : rejected)++;
        for (unsigned long k = 0; k < rounds && !index.empty(); ++k) {
            std::vector<uint8_t> m = index;
            const unsigned flips = 1 + unsigned(rng() % 4);
            for (unsigned i = 0; i < flips; ++i) {
                const size_t at = size_t(rng() % m.size());
                // counts and offsets are little-endian: high bytes set make the huge values
                m[at] = (rng() & 1) ? uint8_t(rng()) : uint8_t(0xFF);
            }
            (run(m.data(), m.size(), &bam, n_ref, &refs).empty() ? parsed : rejected)++;
        }
        std::printf("parsed %lu rejected %lu\n", parsed, rejected);
        return 0;
    }
    std::fprintf(stderr, "usage: bam_index_test ranges <index> [<bam> <n_ref>] | mutate <index> <bam> <n_ref> <seed> <rounds>\n");
    return 2;
}
