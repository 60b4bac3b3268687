// bgzf_inflate_test.cpp -- the inflate of secedo_amd/csrc/bgzf_inflate.hpp on the host, built with plain g++ under
// AddressSanitizer and UBSan: the code that decides what a valid DEFLATE stream is runs here on hostile bytes before
// it runs on a GPU. Serial stand-ins replace the wave's copies; the CRC32 goes through the same per-lane chunks and
// x^(8 len) joins as the kernel's.
//
//   bgzf_inflate_test <in.bgzf> <out.bin> <status.txt>
// Walks the BGZF members of <in.bgzf>, inflates each, writes one status code per member (0 = inflated, ISIZE and
// CRC32 right; secedo::bgzf::Status) to <status.txt> and the bytes of the members with status 0 to <out.bin>.
// Exit code 0 unless the container itself is malformed (2) or a file cannot be opened (3).
#include "bgzf_inflate.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace secedo::bgzf;

namespace {

struct HostIn {
    const uint8_t *p;
    uint32_t n;
    uint32_t size() const { return n; }
    uint32_t load32(uint32_t pos) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if (uint64_t(pos) + k < n) v |= uint32_t(p[pos + k]) << (8 * k);
        return v;
    }
    uint32_t span(uint32_t pos) const { return n - pos; }
};

struct HostOut {
    std::vector<uint8_t> buf;
    explicit HostOut(uint32_t isize) : buf(isize) {}
    void lane_range(uint32_t, uint32_t *first, uint32_t *step) const { *first = 0, *step = 1; }
    void sync() const {}
    void put(uint32_t at, uint8_t b) { buf.at(at) = b; }
    void match(uint32_t at, uint32_t dist, uint32_t len) {
        for (uint32_t j = 0; j < len; ++j) buf.at(at + j) = buf.at(at - dist + j % dist);
    }
    uint32_t room(uint32_t) const { return 1u << 30; }
    void copy_in(HostIn &in, uint32_t pos, uint32_t at, uint32_t n) {
        for (uint32_t j = 0; j < n; ++j) buf.at(at + j) = in.p[pos + j];
    }
};

// the kernel's CRC: 16 KiB segments, 64 chunks of kCrcChunk bytes each, joined by x^(8 len)
uint32_t chunked_crc(const std::vector<uint8_t> &d) {
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = crc_table_entry(i);
    uint32_t crc = 0;
    for (size_t b = 0; b < d.size(); b += 16384) {
        const uint32_t n = uint32_t(std::min<size_t>(16384, d.size() - b));
        uint32_t seg = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t c0 = std::min(n, lane * kCrcChunk), c1 = std::min(n, (lane + 1) * kCrcChunk);
            uint32_t c = ~0u;
            for (uint32_t i = c0; i < c1; ++i) c = tab[(c ^ d[b + i]) & 0xFF] ^ (c >> 8);
            if (c1 > c0) seg ^= crc_mul(crc_x8n(n - c1), ~c);
        }
        crc = crc_join(crc, seg, n);
    }
    return crc;
}

uint32_t rd16(const uint8_t *p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }
uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) return 3;
    std::vector<uint8_t> file;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 3;
        uint8_t tmp[65536];
        for (size_t k; (k = std::fread(tmp, 1, sizeof(tmp), f)) > 0;) file.insert(file.end(), tmp, tmp + k);
        std::fclose(f);
    }
    FILE *out = std::fopen(argv[2], "wb"), *status = std::fopen(argv[3], "w");
    if (!out || !status) return 3;
    size_t off = 0;
    while (off < file.size()) {
        const uint8_t *b = file.data() + off;
        if (file.size() - off < 18 || b[0] != 31 || b[1] != 139 || b[2] != 8 || !(b[3] & 4)) return 2;
        const uint32_t xlen = rd16(b + 10);
        uint32_t bsize = ~0u;
        for (uint32_t x = 12; x + 4 <= 12 + xlen && 12 + xlen <= file.size() - off;) {
            const uint32_t slen = rd16(b + x + 2);
            if (b[x] == 'B' && b[x + 1] == 'C' && slen == 2 && x + 6 <= file.size() - off) bsize = rd16(b + x + 4);
            x += 4 + slen;
        }
        if (bsize == ~0u || size_t(bsize) + 1 > file.size() - off || bsize + 1 < 12 + xlen + 8) return 2;
        const uint32_t len = bsize + 1, isize = rd32(b + len - 4), crc = rd32(b + len - 8);
        if (isize > 65536) return 2;
        // the payload in a buffer of its exact size, so that the sanitizer sees a read one byte past it
        std::vector<uint8_t> payload(b + 12 + xlen, b + len - 8);
        HostIn in{payload.data(), uint32_t(payload.size())};
        HostOut o(isize);
        Tables T;
        std::memset(&T, 0, sizeof(T));
        uint32_t produced = 0;
        uint32_t st = inflate_member(in, o, T, isize, &produced);
        if (st == kOk && chunked_crc(o.buf) != crc) st = kCrcMismatch;
        std::fprintf(status, "%u\n", st);
        if (st == kOk && isize) std::fwrite(o.buf.data(), 1, isize, out);
        off += len;
    }
    std::fclose(out);
    std::fclose(status);
    return 0;
}
