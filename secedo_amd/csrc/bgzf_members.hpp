// bgzf_members.hpp -- what every host reader of a BGZF file shares, header-only, in plain host C++ that g++ compiles
// alone (tests/cpp/bgzf_members_test.cpp runs it under the sanitizers): the one struct for a member that is read, the
// one parse of its header, the walk that lists a file's members, the file bytes and descriptors the device inflate
// (bgzf_kernels.hpp) takes for a range of members, the zlib inflate of one member, and the words for a member that
// cannot be listed or does not inflate. Failures come back as the reason's text, without the file's name; nothing here
// knows the libraries' error string. A new BGZF consumer starts from here; so does a writer (DeflateDesc, member_cuts).
#pragma once

#include "bgzf_inflate.hpp"  // the status codes, kCut

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace secedo {
namespace bam {

// one BGZF member: its raw-DEFLATE payload at d_in + in_off (clen bytes) inflates to d_out + out_off (isize bytes)
struct BgzfDesc {
    uint64_t in_off, out_off;
    uint32_t clen, isize, crc, reserved;
};
static_assert(sizeof(BgzfDesc) == 32, "the kernel reads a descriptor as two 16-byte vectors");

// bytes the kernel may read beyond a payload's ends (whole 16-byte vectors): d_in needs that much room before the
// first payload and after the last one
constexpr uint32_t kBgzfInSlack = 16;
constexpr uint32_t kBgzfMaxIsize = 65536;

}  // namespace bam

namespace bgzf {
// one member to make (bgzf_deflate_kernels.hpp): text bytes [in_off, in_off + n) of d_text, 1 <= n <= kCut (0xFF00)
struct DeflateDesc {
    uint64_t in_off;
    uint32_t n, reserved;
};
// The one cut rule of every writer: the members of text [beg, end), one every kCut bytes from beg, appended to *out.
inline void member_cuts(uint64_t beg, uint64_t end, std::vector<DeflateDesc> *out) {
    for (uint64_t p = beg; p < end; p += kCut) out->push_back({p, uint32_t(std::min<uint64_t>(kCut, end - p)), 0});
}
}  // namespace bgzf

namespace bgzf_members __attribute__((visibility("hidden"))) {

using bam::BgzfDesc;
using bam::kBgzfInSlack;
using bam::kBgzfMaxIsize;

// One member of a file. A reader fills every field (read_member); a writer that only needs virtual offsets of what it
// laid out (bam_index_build.hpp's voffset) gives the first three and leaves the payload's at 0.
struct Member {
    uint64_t coff = 0;   // its byte in the file
    uint64_t out = 0;    // offset in the file's inflated bytes (of an indexed file: in its span's)
    uint32_t isize = 0;
    uint32_t poff = 0;   // its raw-DEFLATE payload starts at coff + poff (12 + XLEN)
    uint32_t clen = 0, crc = 0;
    uint64_t payload() const { return coff + poff; }
};

// What stands at byte off of the file bytes p[0, n): a BGZF member (its length in the file, its ISIZE and the length
// of its extra field), or why not. The one parse of a member header.
enum Header { kMember = 0, kNoMember = 1, kBadBsize = 2, kBigIsize = 3 };
inline Header member_header(const uint8_t *p, uint64_t n, uint64_t off, uint32_t *len, uint32_t *isize,
                            uint32_t *xlen_out) {
    const auto rd16 = [](const uint8_t *q) { return uint32_t(q[0]) | uint32_t(q[1]) << 8; };
    if (off >= n || n - off < 18) return kNoMember;
    const uint8_t *b = p + off;
    if (b[0] != 31 || b[1] != 139 || b[2] != 8 || !(b[3] & 4)) return kNoMember;
    const uint32_t xlen = rd16(b + 10);
    uint32_t bsize = UINT32_MAX;
    for (uint32_t x = 12; x + 4 <= 12 + xlen && 12 + uint64_t(xlen) <= n - off;) {
        const uint32_t slen = rd16(b + x + 2);
        if (b[x] == 'B' && b[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) bsize = rd16(b + x + 4);
        x += 4 + slen;
    }
    if (bsize == UINT32_MAX || uint64_t(bsize) + 1 > n - off || bsize + 1 < 12 + xlen + 8) return kBadBsize;
    *len = bsize + 1;
    std::memcpy(isize, b + *len - 4, 4);
    *xlen_out = xlen;
    return *isize > kBgzfMaxIsize ? kBigIsize : kMember;
}

// The member at byte off of p[0, n) (its `out` left 0) and its length in the file; empty, or why there is none.
inline std::string read_member(const uint8_t *p, uint64_t n, uint64_t off, Member *m, uint32_t *len) {
    uint32_t isize = 0, xlen = 0;
    switch (member_header(p, n, off, len, &isize, &xlen)) {
        case kNoMember: return "not a BGZF block at byte " + std::to_string(off);
        case kBadBsize: return "bad BGZF block size at byte " + std::to_string(off);
        case kBigIsize: return "BGZF ISIZE above 64 KiB";
        case kMember: break;
    }
    *m = Member{off, 0, isize, 12 + xlen, *len - xlen - 20, 0};
    std::memcpy(&m->crc, p + off + *len - 8, 4);
    return std::string();
}

// The members of p[0, n), found by following BSIZE from byte 0, appended to *members; *total = the inflated size.
inline std::string list_members(const uint8_t *p, uint64_t n, std::vector<Member> *members, uint64_t *total) {
    uint64_t off = 0, out = 0;
    while (off < n) {
        Member m;
        uint32_t len = 0;
        const std::string why = read_member(p, n, off, &m, &len);
        if (!why.empty()) return why;
        m.out = out;
        members->push_back(m);
        out += m.isize;
        off += len;
    }
    *total = out;
    return std::string();
}

// The file bytes [lo, hi) to upload for the device inflate of members [b0, b1), b0 < b1: their payloads as they lie in
// the file and kBgzfInSlack bytes on either side, so that the kernel's 16-byte loads stay inside the upload. A header
// is 18 bytes or more, so the bytes in front are always there (lo >= 2); those behind end with the file. `needed`:
// the device buffer's bytes, which is the length without that cut.
struct PayloadSpan {
    uint64_t lo, hi, needed;
};
inline PayloadSpan payload_span(const std::vector<Member> &m, size_t b0, size_t b1, uint64_t file_bytes) {
    const uint64_t lo = m[b0].payload() - kBgzfInSlack;
    const uint64_t end = m[b1 - 1].payload() + m[b1 - 1].clen + kBgzfInSlack;
    return PayloadSpan{lo, std::min(file_bytes, end), end - lo};
}

// One descriptor per member of [b0, b1) into desc[0, b1 - b0): file byte lo lies at in_base of the device input, the
// first member inflates to out_base and the others behind it as they follow it in the file.
inline void fill_desc(const std::vector<Member> &m, size_t b0, size_t b1, uint64_t lo, uint64_t in_base,
                      uint64_t out_base, BgzfDesc *desc) {
    for (size_t b = b0; b < b1; ++b)
        desc[b - b0] = BgzfDesc{in_base + (m[b].payload() - lo), out_base + (m[b].out - m[b0].out), m[b].clen,
                                m[b].isize, m[b].crc, 0};
}

// The one range cut of every reader that takes a file in ranges: members [b0, b1) of about `batch` inflated bytes, at
// least one; b1 is returned. fold_empty_tail_total: the list's inflated size, for a reader whose last range also takes
// a tail of only empty members (the EOF member) in place of a range of nothing; kNoFold for one that gives them a
// range of their own. The two kinds are kept apart: which one a reader is shows in its batch and range counts.
constexpr uint64_t kNoFold = UINT64_MAX;
inline size_t next_range(const std::vector<Member> &m, size_t b0, uint64_t batch,
                         uint64_t fold_empty_tail_total = kNoFold) {
    size_t b1 = b0;
    uint64_t bytes = 0;
    while (b1 < m.size() && (b1 == b0 || bytes + m[b1].isize <= batch)) bytes += m[b1++].isize;
    if (b1 < m.size() && m[b1].out == fold_empty_tail_total) b1 = m.size();
    return b1;
}
// the inflated bytes of members [b0, b1) of a list whose `out` is the running sum of `isize`
inline uint64_t range_bytes(const std::vector<Member> &m, size_t b0, size_t b1) {
    return b0 < b1 ? m[b1 - 1].out + m[b1 - 1].isize - m[b0].out : 0;
}

// ---- the words for a member that does not inflate: "<path>: " + block_where*() + ": " + status_text()

inline const char *status_text(uint32_t status) {
    return status == bgzf::kCrcMismatch ? "CRC32 mismatch" : "inflate failed or ISIZE mismatch";
}
inline std::string block_where(uint64_t k) { return "BGZF block " + std::to_string(k); }
// a member whose ordinal in the file is unknown (it was reached through an index)
inline std::string block_where_byte(uint64_t coff) { return "BGZF block at byte " + std::to_string(coff); }

// the lowest k with status[k] != kOk, or n
inline size_t first_bad(const uint32_t *status, size_t n) {
    size_t k = 0;
    while (k < n && status[k] == bgzf::kOk) ++k;
    return k;
}

// zlib raw inflate of one member, its payload at `payload`, into dst[isize], ISIZE and CRC32 checked: empty on success,
// else the message's tail
inline std::string inflate_member_zlib(const uint8_t *payload, const Member &m, uint8_t *dst) {
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) return "inflateInit2 failed";
    z.next_in = const_cast<Bytef *>(payload);
    z.avail_in = m.clen;
    uint8_t none;  // an empty member (the end-of-file marker) still needs room to be told from a full buffer
    z.next_out = m.isize ? dst : &none;
    z.avail_out = m.isize ? m.isize : 1;
    const int rc = inflate(&z, Z_FINISH);
    const uint64_t got = z.total_out;
    inflateEnd(&z);
    if (rc != Z_STREAM_END || got != m.isize) return status_text(bgzf::kSizeMismatch);
    if (uint32_t(crc32(crc32(0, nullptr, 0), dst, m.isize)) != m.crc) return status_text(bgzf::kCrcMismatch);
    return std::string();
}

}  // namespace bgzf_members
}  // namespace secedo
