// bgzf_deflate_test.cpp -- the encoder of secedo_amd/csrc/bgzf_deflate.hpp on the host, built with plain g++ under
// AddressSanitizer and UBSan. Serial stand-ins replace the wave: one "lane" runs every item of a loop in order, which
// is one of the orders the device may take, and the header's rules make every order give the same bytes. The text and
// the member live in buffers of their exact sizes, so that the sanitizer sees a read or write one byte past them.
//
//   bgzf_deflate_test <in.bin> <out.bgzf>
// Cuts <in.bin> every 0xFF00 bytes, encodes each piece as one BGZF member, inflates the member again with the host
// build of bgzf_inflate.hpp, compares, and writes the members and the EOF member to <out.bgzf>.
// Exit code 0; 3 when a file cannot be opened; 4 when a member does not inflate back to its text (its index on stderr).
#include "bgzf_deflate.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace secedo::bgzf;

namespace {

struct Text {
    const uint8_t *p;
    uint32_t n;
    uint32_t load32(uint32_t at) const {
        if (uint64_t(at) + 4 > n) std::abort();  // the header promises never to ask
        return uint32_t(p[at]) | uint32_t(p[at + 1]) << 8 | uint32_t(p[at + 2]) << 16 | uint32_t(p[at + 3]) << 24;
    }
    uint32_t byte(uint32_t at) const {
        if (at >= n) std::abort();
        return p[at];
    }
};

struct Member {
    std::vector<uint8_t> buf;
    Member() : buf(kMaxMember + kOverrunBytes) {}
    void byte(uint32_t at, uint32_t v) { buf.at(at) = uint8_t(v); }
    void word(uint32_t k, uint32_t v) {
        for (uint32_t j = 0; j < 4; ++j) buf.at(kHeaderBytes + 4 * k + j) = uint8_t(v >> (8 * j));
    }
};

struct Serial {
    void lane_range(uint32_t, uint32_t *first, uint32_t *step) const { *first = 0, *step = 1; }
    void sync() const {}
    void fence() const {}
    bool leader() const { return true; }
    void or32(uint32_t *p, uint32_t v) const { *p |= v; }
};

// the stand-ins of bgzf_inflate_test.cpp
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

uint32_t plain_crc(const uint8_t *p, size_t n) {
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; ++i) c = crc_table_entry((c ^ p[i]) & 0xFF) ^ (c >> 8);
    return ~c;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 3;
    std::vector<uint8_t> file;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 3;
        uint8_t tmp[65536];
        for (size_t k; (k = std::fread(tmp, 1, sizeof(tmp), f)) > 0;) file.insert(file.end(), tmp, tmp + k);
        std::fclose(f);
    }
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 3;
    uint32_t index = 0;
    for (size_t off = 0; off < file.size(); off += kCut, ++index) {
        const uint32_t n = uint32_t(std::min<size_t>(kCut, file.size() - off));
        const std::vector<uint8_t> text(file.begin() + off, file.begin() + off + n);  // exact size
        Text in{text.data(), n};
        Member m;
        Work W;
        std::memset(&W, 0xA5, sizeof(W));  // nothing may depend on what the working set held
        Serial L;
        uint32_t stored = 0;
        const uint32_t size = deflate_member(in, n, m, W, L, &stored);
        if (size > kMaxMember) return 4;
        // back through the decoder
        const std::vector<uint8_t> payload(m.buf.begin() + kHeaderBytes, m.buf.begin() + size - kTrailerBytes);
        HostIn din{payload.data(), uint32_t(payload.size())};
        HostOut dout(n);
        Tables T;
        std::memset(&T, 0, sizeof(T));
        uint32_t produced = 0;
        const uint32_t st = inflate_member(din, dout, T, n, &produced);
        const uint8_t *t = m.buf.data() + size - kTrailerBytes;
        const uint32_t crc = uint32_t(t[0]) | uint32_t(t[1]) << 8 | uint32_t(t[2]) << 16 | uint32_t(t[3]) << 24;
        if (st != kOk || produced != n || dout.buf != text || crc != plain_crc(text.data(), n)) {
            std::fprintf(stderr, "member %u: status %u, %u of %u bytes, stored %u\n", index, st, produced, n, stored);
            return 4;
        }
        std::fwrite(m.buf.data(), 1, size, out);
    }
    std::fwrite(eof_member().data(), 1, kEofBytes, out);
    return std::fclose(out) == 0 ? 0 : 3;
}
