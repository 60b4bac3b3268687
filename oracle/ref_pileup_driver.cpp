/*
 * ref_pileup_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * A command-line front of the UNMODIFIED reference's pileup_bams() (pileup.hpp), linked by
 * oracle/Makefile into oracle/_ref/ref_pileup (git-ignored). It runs the deterministic call,
 * num_threads = 1 with the text file written, and leaves <out>.bin / .map / .txt behind:
 *
 *   ref_pileup <out> <chromosome_id> <max_coverage> <min_base_quality> <min_map_quality>
 *              <min_alignment_score> <min_different> <bam>...
 *
 * The reference needs <bam>.bai next to every file. Exit status 0 on return, 2 on a usage
 * error; an assert of the reference ends the process with SIGABRT, which is part of what the
 * tests compare.
 */
#include "pileup.hpp"

#include <cstdint>
#include <cstdlib>
#include <filesystem>
#include <iostream>
#include <sstream>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 9) {
        std::cerr << "usage: ref_pileup out chromosome max_cov min_bq min_mq min_as min_different bam...\n";
        return 2;
    }
    uint32_t v[6];
    for (int i = 0; i < 6; ++i) {
        v[i] = static_cast<uint32_t>(std::strtoul(argv[2 + i], nullptr, 10));
    }
    std::vector<std::filesystem::path> files(argv + 8, argv + argc);
    std::ostringstream sink; // the reference draws a progress bar on std::cout
    std::streambuf *old = std::cout.rdbuf(sink.rdbuf());
    pileup_bams(files, argv[1], true, v[0], v[1], v[2], v[3], v[4], 1, static_cast<uint16_t>(v[5]));
    std::cout.rdbuf(old);
    return 0;
}
