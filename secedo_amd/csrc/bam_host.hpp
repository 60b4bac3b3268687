// bam_host.hpp -- what the two host files of include/secedo_bam.h share: bam_input.cpp reads the BAM and SAM files
// into one ChrInput per requested chromosome, bam_pileup.cpp turns those into the pileup. Internal, nothing exported.
#pragma once

#include "host_util.hpp"
#include "secedo_bam.h"

#include <sys/mman.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace secedo {
namespace bam_host __attribute__((visibility("hidden"))) {

using namespace secedo::host;

inline uint32_t rd32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint16_t rd16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }

// Layout of a BAM record body c (after block_size): 32 fixed bytes, read name, CIGAR, packed SEQ, QUAL, aux fields.
inline uint32_t rec_l_name(const uint8_t *c) { return c[8]; }
inline uint32_t rec_n_cigar(const uint8_t *c) { return rd16(c + 12); }
inline uint32_t rec_l_seq(const uint8_t *c) { return rd32(c + 16); }
inline uint64_t rec_aux_off(const uint8_t *c) {
    return 32 + uint64_t(rec_l_name(c)) + 4ull * rec_n_cigar(c) + (uint64_t(rec_l_seq(c)) + 1) / 2 + rec_l_seq(c);
}

// the records of one chromosome, file after file in input order
struct ChrInput {
    uint32_t chromosome;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> file_base;          // [n_files] start of each file's run in bytes
    std::vector<std::vector<uint64_t>> roff;  // per file: record offsets (relative to its run)
    std::vector<std::vector<int32_t>> rpos;
    std::vector<std::vector<uint64_t>> ridx;  // record index in the file (messages)
};

// what one call read
struct Inputs {
    std::vector<std::string> paths;  // [n_files] (messages)
    std::vector<uint64_t> line0;     // [n_files] SAM: the line of record 0 (1-based); BAM: 0
    std::vector<ChrInput> chrs;      // [n_chr]
};

// Where record idx of file f is, for messages:
//   SAM (line0 != 0):        "file f (path), line line0 + idx"
//   BAM while loading:       "path: record idx"
//   BAM in the device stage: "file f, record idx"
// Known wart: the two BAM wordings name the same record differently. Both are kept as callers know them.
enum class Stage { kLoad, kDevice };
std::string record_where(const std::string &path, size_t f, uint64_t line0, uint64_t idx, Stage stage = Stage::kLoad);

// Reads the files (BAM or SAM, told apart by their first bytes) and keeps the records of the requested chromosomes.
// t: stage times are added to it; may be null.
int load_inputs(const std::vector<std::string> &files, const uint32_t *chromosome_ids, uint32_t n_chr,
                uint32_t threads, Inputs *in, secedo_bam_times *t);

// ---- what bam_input.cpp (host inflate, host walk) and bam_device_input.cpp (device inflate, device walk) share

constexpr uint32_t kMaxThreads = 16;

// f(0) .. f(n - 1) in a pool of at most kMaxThreads threads
template <class F>
void parallel_for(uint32_t threads, uint64_t n, F f) {
    threads = std::max<uint32_t>(1, std::min<uint64_t>(std::min(threads, kMaxThreads), n));
    std::atomic<uint64_t> next{0};
    auto work = [&] {
        for (uint64_t i; (i = next.fetch_add(1)) < n;) f(i);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
}

// inflated bytes per batch of files and per block range of one file; SECEDO_BAM_BATCH_BYTES overrides it (tests:
// outputs do not depend on it), read at every call
uint64_t batch_bytes();

struct Mapped {
    const uint8_t *p = nullptr;
    size_t n = 0;
    Mapped() = default;
    Mapped(const Mapped &) = delete;
    Mapped &operator=(const Mapped &) = delete;
    Mapped(Mapped &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    ~Mapped() {
        if (p && n) munmap(const_cast<uint8_t *>(p), n);
    }
};

struct Block {
    const uint8_t *cdata;
    uint32_t clen, crc, isize;
    uint64_t out;  // offset in the file's inflated buffer
};

// a file mapped and its BGZF blocks listed; *total = its inflated size
int open_bgzf(const std::string &path, Mapped *m, std::vector<Block> *blocks, uint64_t *total);
// zlib raw inflate of one block into dst[isize], ISIZE and CRC32 checked: empty on success, else the message's tail
std::string inflate_block(const Block &b, uint8_t *dst);

struct Header {
    uint32_t l_text = 0, n_ref = 0;
    uint64_t first_record = 0;
};

constexpr int kNeedMore = 1;  // parse_header / walk_range: the bytes end inside the header or a record

// final: d ends the file, so a cut header is an error; else kNeedMore
int parse_header(const std::string &path, const uint8_t *d, uint64_t n, bool final, Header *h);

// Process-wide BAM route (secedo_bam_set_inflate, SECEDO_BAM_INFLATE), read at every call: *device = the device
// route. An unknown value of the variable is SECEDO_E_INVALID_ARG.
int inflate_route(bool *device);

// What the last pileup or scan call on this thread did (secedo_bam_route_stats). Behind a function: an extern
// thread_local of a hidden namespace is reached through an init wrapper that other translation units call unchecked.
secedo_bam_route_info &route();

// The device route for BAM files [f0, f1) of in->paths (bam_device_input.cpp): device inflate and device walk; the
// records of the requested chromosomes are appended to runs[chr][file] and in->chrs as the host walk's FileSink does.
using Runs = std::vector<std::vector<std::vector<uint8_t>>>;  // [chr][file] the file's records of the chromosome
struct BamDevWork;
BamDevWork *new_bam_dev_work();
void delete_bam_dev_work(BamDevWork *w);
int load_bams_device(size_t f0, size_t f1, uint32_t threads, uint64_t batch, BamDevWork *w, Inputs *in, Runs *runs,
                     secedo_bam_times *t);

// Frees the device memory of the last secedo_bgzf_inflate result of this thread (secedo_bam_release calls it).
void release_inflated();

}  // namespace bam_host
}  // namespace secedo
