// variant_calling_test.cpp -- the reference-shaped variant_calling of include/secedo_pipeline.hpp on real types:
//   variant_calling_test PILEUP CLUSTERS FASTA MAP HETERO_PRIOR THETA OUT_DIR
//       PILEUP: as divide_cluster_test.cpp (u64 n_chr, n_loci, n_entries, n_cells, then the flat arrays with a u16
//       id_base); CLUSTERS: u64 n, then n u16. MAP may be "-" for none. Writes the reference's files to OUT_DIR.
// Exit status 2 on a thrown exception (message on stderr).
#include "secedo_pipeline.hpp"

#include <cstdint>
#include <exception>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace {

// the reference's PosData, as far as the template reads it
struct PosData {
    uint32_t position;
    std::vector<uint32_t> read_ids;
    std::vector<uint16_t> group_ids_bases;
};

template <typename T>
std::vector<T> read_vec(std::ifstream &f, uint64_t count) {
    std::vector<T> out(count);
    f.read(reinterpret_cast<char *>(out.data()), static_cast<std::streamsize>(count * sizeof(T)));
    if (!f) throw std::runtime_error("short file");
    return out;
}

int run(char **argv) {
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint64_t> head = read_vec<uint64_t>(f, 4);
    const auto chr = read_vec<uint32_t>(f, head[0] + 1);
    const auto pos = read_vec<uint32_t>(f, head[1]);
    const auto off = read_vec<uint64_t>(f, head[1] + 1);
    const auto rid = read_vec<uint32_t>(f, head[2]);
    const auto idb = read_vec<uint16_t>(f, head[2]);
    std::vector<std::vector<PosData>> pds(head[0]);
    for (uint64_t c = 0; c < head[0]; ++c) {
        for (uint32_t l = chr[c]; l < chr[c + 1]; ++l) {
            PosData pd{pos[l], {rid.begin() + off[l], rid.begin() + off[l + 1]},
                       {idb.begin() + off[l], idb.begin() + off[l + 1]}};
            pds[c].push_back(std::move(pd));
        }
    }
    std::ifstream fc(argv[2], std::ios::binary);
    const std::vector<uint64_t> n = read_vec<uint64_t>(fc, 1);
    const std::vector<uint16_t> clusters = read_vec<uint16_t>(fc, n[0]);
    const std::string map_file = std::string(argv[4]) == "-" ? "" : argv[4];
    secedo_amd::variant_calling(pds, clusters, argv[3], map_file, std::stod(argv[5]), std::stod(argv[6]), argv[7]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 8) {
        std::cerr << "usage: variant_calling_test PILEUP CLUSTERS FASTA MAP HETERO_PRIOR THETA OUT_DIR\n";
        return 1;
    }
    try {
        return run(argv);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 2;
    }
}
