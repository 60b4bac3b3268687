/*
 * ref_variant_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * A command-line front of the UNMODIFIED reference's variant calling (variant_calling.hpp), linked by
 * oracle/Makefile into oracle/_ref/ref_variant (git-ignored). A program and not a part of
 * libsecedo_ref.so, because the reference ends its process on some inputs: unequal maternal and
 * paternal contigs call exit(1) after the preambles are written, and a line for a chromosome past the
 * 24th trips an assert of id_to_chromosome.
 *
 *   ref_variant genotypes <counts.bin> <lht> <prior> <theta> <out.bin>
 *       counts.bin: n x 4 u16 (n from the file's size). out.bin, per tuple: u8 likely_homozygous(counts,
 *       theta), u8 most_likely_genotype(counts, ..., lht != 0, prior, theta), u16 the coverage it reports.
 *
 *   ref_variant call <pileup.bin> <clusters.bin> <fasta> <map|""> <prior> <theta> <out_dir>
 *       pileup.bin: u64 n_chr, n_loci, n_entries, n_cells; u32 chr_locus_off[n_chr + 1]; u32
 *       locus_pos[n_loci]; u64 locus_entry_off[n_loci + 1]; u32 read_ids[n_entries]; id_base[n_entries]
 *       as u16 or, told by the file's size, u32 (tests/cpp/variant_calling_test.cpp reads the u16 form).
 *       clusters.bin: u64 n, then n u16. Runs variant_calling(); the reference's log goes where it sends
 *       it (spdlog's stdout sink) and its exit status passes through untouched.
 *
 * Statuses of the driver's own: 0 on return, 64 usage, 65 a file that cannot be read or is short, 66 a
 * group id that does not fit the reference's 14 bits or names no entry of clusters (the reference
 * would index past its vector).
 */
#include "variant_calling.hpp"

#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace {

constexpr int kUsage = 64, kBadFile = 65, kBadGroup = 66;

bool read_all(const char *path, std::vector<char> *out) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamoff n = f.tellg();
    out->resize(static_cast<size_t>(n));
    f.seekg(0);
    if (n > 0) f.read(out->data(), n);
    return static_cast<bool>(f);
}

template <typename T>
bool take(const std::vector<char> &buf, size_t *at, uint64_t count, std::vector<T> *out) {
    if (count > (buf.size() - *at) / sizeof(T)) return false;
    out->resize(count);
    if (count) std::memcpy(out->data(), buf.data() + *at, count * sizeof(T));
    *at += count * sizeof(T);
    return true;
}

int genotypes(char **argv) {
    std::vector<char> buf;
    if (!read_all(argv[2], &buf) || buf.size() % 8 != 0) return kBadFile;
    const bool lht = std::atoi(argv[3]) != 0;
    const double prior = std::strtod(argv[4], nullptr), theta = std::strtod(argv[5], nullptr);
    const size_t n = buf.size() / 8;
    std::vector<uint8_t> out(n * 4);
    const std::array<uint32_t, 4> unused_idx = {0, 1, 2, 3};
    for (size_t i = 0; i < n; ++i) {
        std::array<uint16_t, 4> c;
        std::memcpy(c.data(), buf.data() + i * 8, 8);
        uint16_t cov = 0;
        out[i * 4] = likely_homozygous(c, theta);
        out[i * 4 + 1] = most_likely_genotype(c, c, unused_idx, lht, prior, theta, &cov);
        std::memcpy(out.data() + i * 4 + 2, &cov, 2);
    }
    std::ofstream f(argv[6], std::ios::binary);
    f.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(out.size()));
    return f ? 0 : kBadFile;
}

int call(char **argv) {
    std::vector<char> buf, cbuf;
    if (!read_all(argv[2], &buf) || !read_all(argv[3], &cbuf)) return kBadFile;
    size_t at = 0;
    std::vector<uint64_t> head, off, n_clusters;
    std::vector<uint32_t> chr, pos, rid, idb32;
    std::vector<uint16_t> idb, clusters;
    if (!take(buf, &at, 4, &head) || !take(buf, &at, head[0] + 1, &chr) || !take(buf, &at, head[1], &pos) ||
        !take(buf, &at, head[1] + 1, &off) || !take(buf, &at, head[2], &rid))
        return kBadFile;
    if (buf.size() - at == head[2] * 4 && head[2] > 0) {
        if (!take(buf, &at, head[2], &idb32)) return kBadFile;
        idb.resize(idb32.size());
        for (size_t i = 0; i < idb32.size(); ++i) {
            if (idb32[i] > 0xFFFFu) return kBadGroup;
            idb[i] = static_cast<uint16_t>(idb32[i]);
        }
    } else if (!take(buf, &at, head[2], &idb) || at != buf.size()) {
        return kBadFile;
    }
    at = 0;
    if (!take(cbuf, &at, 1, &n_clusters) || !take(cbuf, &at, n_clusters[0], &clusters) || at != cbuf.size())
        return kBadFile;
    if (chr.front() != 0 || chr.back() != head[1] || off.front() != 0 || off.back() != head[2]) return kBadFile;
    for (uint16_t x : idb)
        if (static_cast<uint32_t>(x >> 2) >= clusters.size()) return kBadGroup;

    std::vector<std::vector<PosData>> pos_data(head[0]);
    for (uint64_t c = 0; c < head[0]; ++c) {
        if (chr[c] > chr[c + 1]) return kBadFile;
        for (uint32_t l = chr[c]; l < chr[c + 1]; ++l) {
            if (off[l] > off[l + 1] || off[l + 1] > head[2]) return kBadFile;
            std::vector<uint32_t> ids(rid.begin() + off[l], rid.begin() + off[l + 1]);
            std::vector<uint16_t> packed(idb.begin() + off[l], idb.begin() + off[l + 1]);
            pos_data[c].emplace_back(pos[l], std::move(ids), std::move(packed));
        }
    }
    variant_calling(pos_data, clusters, argv[4], argv[5], std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr),
                    argv[8]);
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc == 7 && std::strcmp(argv[1], "genotypes") == 0) return genotypes(argv);
    if (argc == 9 && std::strcmp(argv[1], "call") == 0) return call(argv);
    std::cerr << "usage: ref_variant genotypes counts.bin lht prior theta out.bin\n"
                 "       ref_variant call pileup.bin clusters.bin fasta map prior theta out_dir\n";
    return kUsage;
}
