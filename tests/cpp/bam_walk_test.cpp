// bam_walk_test.cpp -- the segment walk and join of secedo_amd/csrc/bam_walk.hpp on the host, built with plain g++
// under AddressSanitizer and UBSan: the code that decides which offsets of inflated BAM bytes are records runs here,
// on valid and on hostile bytes, before it runs on a GPU.
//
//   bam_walk_test <bytes.bin> <start> <final 0|1> <segment bytes>...
// <bytes.bin> holds a file's inflated bytes, <start> is the offset of its first record. For each segment size the
// bytes from <start> on are cut into segments of that size, every segment is walked from its own start, the join
// follows the true chain, and the result is compared with a serial walk written here: the record offsets, where the
// chain stopped and the error code. The buffers are exactly as large as the header says they need to be, so a read or
// a write past them is a sanitizer error. Prints one line per segment size: records, re-walked segments, code, stop
// offset. Exit code 0, 1 on a mismatch, 3 if the file cannot be read.
#include "bam_walk.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace secedo::bamwalk;

namespace {

struct Reader {
    const uint8_t *p;
    uint32_t n;
    uint32_t operator()(uint32_t o) const {
        if (uint64_t(o) + 4 > n) {
            std::fprintf(stderr, "read of 4 bytes at %u past the %u bytes\n", o, n);
            std::abort();
        }
        uint32_t v;
        std::memcpy(&v, p + o, 4);
        return v;
    }
};

// the walk as the host route does it, one record after another
struct Serial {
    std::vector<uint32_t> starts;
    uint32_t stop_off = 0, code = 0;
};

Serial serial_walk(const uint8_t *d, uint32_t n, uint32_t start, bool final) {
    Serial s;
    uint32_t o = start;
    for (;;) {
        s.stop_off = o;
        if (o >= n) break;
        if (n - o < 4 + 32) {
            s.code = final ? uint32_t(kErrTruncated) : 0u;
            break;
        }
        uint32_t bs;
        std::memcpy(&bs, d + o, 4);
        if (bs < 32) {
            s.code = kErrBlockSize;
            break;
        }
        if (bs > n - o - 4) {
            s.code = final ? uint32_t(kErrBlockSize) : 0u;
            break;
        }
        s.starts.push_back(o);
        o += 4 + bs;
    }
    return s;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 5) return 3;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::unique_ptr<uint8_t[]> data(new uint8_t[size > 0 ? size : 1]);  // exactly the bytes: no slack to read into
    if (size > 0 && std::fread(data.get(), 1, size_t(size), f) != size_t(size)) return 3;
    std::fclose(f);
    const uint32_t n = uint32_t(size), start = uint32_t(std::strtoul(argv[2], nullptr, 10));
    const bool final = std::atoi(argv[3]) != 0;
    if (start > n) return 3;
    const Serial want = serial_walk(data.get(), n, start, final);
    Reader rd{data.get(), n};
    for (int a = 4; a < argc; ++a) {
        const uint32_t seg_bytes = uint32_t(std::strtoul(argv[a], nullptr, 10));
        if (!seg_bytes) return 3;
        std::vector<Seg> segs;
        uint32_t n_list = 0;
        for (uint32_t o = start; o < n; o += seg_bytes) {
            const uint32_t end = n - o < seg_bytes ? n : o + seg_bytes;
            segs.push_back(Seg{o, end, 0, n_list});
            n_list += list_cap(end - o);
            if (end == n) break;
        }
        // every list exactly list_cap long
        std::unique_ptr<uint32_t[]> lists(new uint32_t[n_list ? n_list : 1]), rewalk(new uint32_t[n_list ? n_list : 1]);
        std::vector<SegWalk> walk(segs.size());
        std::vector<SegJoin> join(segs.size());
        for (size_t k = 0; k < segs.size(); ++k)
            walk[k] = walk_segment(rd, segs[k].start, segs[k].end, n, lists.get() + segs[k].list, true);
        const Chain c = join_file(rd, segs.data(), walk.data(), lists.get(), rewalk.get(), uint32_t(segs.size()), n,
                                  join.data());
        std::vector<uint32_t> got;
        for (size_t k = 0; k < segs.size(); ++k) {
            for (uint32_t i = 0; i < join[k].n_rewalk; ++i) got.push_back(rewalk[segs[k].list + i]);
            for (uint32_t i = 0; i < join[k].n_adopt; ++i) got.push_back(lists[segs[k].list + join[k].from + i]);
        }
        const uint32_t code = stop_code(c.stop, final);
        // a chain that ends the bytes exactly stops at n; one that is cut stops at the cut record
        if (got != want.starts || c.n != want.starts.size() || code != want.code || c.stop_off != want.stop_off) {
            std::fprintf(stderr, "segments of %u: %zu records (serial %zu), code %u (%u), stop %u (%u)\n", seg_bytes,
                         got.size(), want.starts.size(), code, want.code, c.stop_off, want.stop_off);
            return 1;
        }
        std::printf("%u %zu %u %u %u\n", seg_bytes, got.size(), c.rewalked, code, c.stop_off);
    }
    return 0;
}
