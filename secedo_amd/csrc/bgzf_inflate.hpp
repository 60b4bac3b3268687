// bgzf_inflate.hpp -- RFC 1951 inflate of one BGZF member, written once for the device (bgzf_kernels.hip, one wavefront
// per member) and the host (tests/cpp/bgzf_inflate_test.cpp, plain g++ under the sanitizers). Everything that decides
// whether a stream is valid lives here: the bit reader, the code-length parse, the table construction, the symbol
// decode and the bounds checks. What moves bytes is behind two small interfaces the caller supplies:
//
//   In   uint32_t size()                       compressed bytes (clen)
//        uint32_t load32(uint32_t pos)         4 bytes at pos, little endian, for any pos; what it gives past size()
//                                              may be anything (it is never acted on) but must not fault
//        uint32_t span(uint32_t pos)           >= 1 bytes readable in one piece from pos < size()
//   Out  void put(uint32_t at, uint8_t b)      one literal at output offset `at`
//        void match(uint32_t at, uint32_t dist, uint32_t len)   out[at + j] = out[at - dist + j % dist], j < len
//        uint32_t room(uint32_t at)            >= 1 bytes copy_in may take at `at` in one piece
//        void copy_in(In &, uint32_t pos, uint32_t at, uint32_t n)   stored bytes, n <= span(pos), n <= room(at)
//        void lane_range(uint32_t n, uint32_t *first, uint32_t *step)   split of a loop of n independent items
//        void sync()                           what the lanes wrote to the tables is visible to all of them
//
// On the device all 64 lanes of the wavefront run this code with the same values (no divergence); the interfaces are
// where the lanes split the work. Every read is checked against size(), every write against the member's ISIZE
// before it happens, and every loop iteration consumes at least one input bit or produces one output byte, so
// arbitrary bytes end in a status code after a bounded number of steps.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // __forceinline__
#define BGZF_HD __host__ __device__ __forceinline__
#else
#define BGZF_HD inline
#endif

namespace secedo {
namespace bgzf {

enum Status : uint32_t {
    kOk = 0,
    kBadBlockType = 1,   // BTYPE 3
    kStoredLen = 2,      // LEN != ~NLEN
    kBadCounts = 3,      // HLIT > 286 or HDIST > 30 symbols
    kBadCodeLens = 4,    // over- or under-subscribed code-length code, or a repeat without a length before it / past the end
    kNoEndOfBlock = 5,   // the literal/length code has no code for 256
    kBadLitLen = 6,      // over- or under-subscribed literal/length code
    kBadDist = 7,        // over- or under-subscribed distance code
    kBadSymbol = 8,      // a bit pattern no code has, or length symbol 286/287, or distance symbol 30/31
    kDistTooFar = 9,     // a distance reaching before the member's first byte
    kInputEnd = 10,      // ran out of input
    kOutputFull = 11,    // more output than ISIZE
    kSizeMismatch = 12,  // stream ended with fewer bytes than ISIZE
    kCrcMismatch = 13,   // CRC32 of the output differs from the member's
    kStatusCodes = 14,
};

constexpr uint32_t kLitBits = 10, kDistBits = 8;  // primary table widths; longer codes take the canonical walk
constexpr uint32_t kMaxLit = 288, kMaxDist = 32, kMaxBits = 15;
constexpr uint32_t kCut = 0xFF00;  // text bytes per member at the most: bgzip's cut, every writer's (bgzf_members.hpp)

// one canonical Huffman code: symbols sorted by (length, value), counts per length, and the primary table
// entry = symbol << 4 | length (0 = no code of at most `bits` bits starts so)
struct Code {
    uint16_t count[kMaxBits + 1];
    uint16_t first[kMaxBits + 1];  // index in sym of the first symbol of each length
};

// the decoder's working set: LDS on the device, the stack on the host
struct Tables {
    uint8_t lens[kMaxLit + kMaxDist];
    uint16_t lit_sym[kMaxLit], dist_sym[kMaxDist];
    uint16_t lit_tab[1u << kLitBits], dist_tab[1u << kDistBits];
    Code lit, dist;
    uint16_t next[kMaxBits + 1];
};

BGZF_HD uint32_t reverse_bits(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// kOk, or `bad` for an over-subscribed set or an incomplete one (zlib's rule: an incomplete set passes only when it
// has no code at all, or one code of length 1 and allow_single)
template <class Out>
BGZF_HD uint32_t build_code(Out &out, const uint8_t *lens, uint32_t n, uint32_t bits, bool allow_single, Code *c,
                            uint16_t *next, uint16_t *sym, uint16_t *tab, uint32_t bad) {
    for (uint32_t l = 0; l <= kMaxBits; ++l) c->count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) c->count[lens[s]] = uint16_t(c->count[lens[s]] + 1);
    int32_t left = 1;
    uint32_t max_len = 0;
    for (uint32_t l = 1; l <= kMaxBits; ++l) {
        left = left * 2 - int32_t(c->count[l]);
        if (left < 0) return bad;
        if (c->count[l]) max_len = l;
    }
    if (left > 0 && max_len != 0 && !(allow_single && max_len == 1 && c->count[1] == 1)) return bad;
    uint32_t o = 0;
    for (uint32_t l = 1; l <= kMaxBits; ++l) {
        c->first[l] = next[l] = uint16_t(o);
        o += c->count[l];
    }
    const uint32_t n_coded = o;
    for (uint32_t s = 0; s < n; ++s)
        if (lens[s]) sym[next[lens[s]]++] = uint16_t(s);
    // primary table: cleared, then each coded symbol of at most `bits` bits fills its 2^(bits - len) slots
    uint32_t i0, step;
    out.lane_range(1u << bits, &i0, &step);
    for (uint32_t i = i0; i < (1u << bits); i += step) tab[i] = 0;
    out.sync();
    out.lane_range(n_coded, &i0, &step);
    for (uint32_t i = i0; i < n_coded; i += step) {
        uint32_t len = 1, code = 0, base = 0;  // canonical code of the i-th sorted symbol
        while (i >= base + c->count[len]) {
            code = (code + c->count[len]) << 1;
            base += c->count[len];
            ++len;
        }
        if (len > bits) continue;
        code += i - base;
        const uint16_t e = uint16_t(uint32_t(sym[i]) << 4 | len);
        for (uint32_t k = reverse_bits(code, len); k < (1u << bits); k += 1u << len) tab[k] = e;
    }
    out.sync();
    return kOk;
}

template <class In>
struct BitReader {
    In &in;
    uint64_t hold = 0;
    uint32_t nbits = 0, pos = 0;
    BGZF_HD explicit BitReader(In &i) : in(i) {}
    // at least 33 bits in hold (zeros or anything past the end: over() is asked before a symbol is acted on)
    BGZF_HD void refill() {
        if (nbits <= 32) {
            hold |= uint64_t(in.load32(pos)) << nbits;
            pos += 4;
            nbits += 32;
        }
    }
    BGZF_HD uint32_t peek(uint32_t n) const { return uint32_t(hold) & ((1u << n) - 1); }
    BGZF_HD void drop(uint32_t n) {
        hold >>= n;
        nbits -= n;
    }
    BGZF_HD uint32_t take(uint32_t n) {
        const uint32_t v = peek(n);
        drop(n);
        return v;
    }
    // more bits consumed than the member has
    BGZF_HD bool over() const { return uint64_t(pos) * 8 - nbits > uint64_t(in.size()) * 8; }
};

// one symbol: primary table, else the canonical walk over the longer lengths; -1 = no such code
template <class In>
BGZF_HD int32_t decode_symbol(BitReader<In> &br, const Code &c, const uint16_t *sym, const uint16_t *tab,
                              uint32_t bits) {
    const uint32_t e = tab[br.peek(bits)];
    if (e & 15) {
        br.drop(e & 15);
        return int32_t(e >> 4);
    }
    uint32_t code = 0, first = 0;
    const uint32_t h = uint32_t(br.hold);
    for (uint32_t len = 1; len <= kMaxBits; ++len) {
        code |= (h >> (len - 1)) & 1u;
        const uint32_t count = c.count[len];
        if (code < first + count) {
            br.drop(len);
            return int32_t(sym[c.first[len] + (code - first)]);
        }
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

BGZF_HD uint32_t len_base(uint32_t s) {
    return s < 8 ? 3 + s : s == 28 ? 258 : ((4 + (s & 3)) << ((s >> 2) - 1)) + 3;
}
BGZF_HD uint32_t len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
BGZF_HD uint32_t dist_base(uint32_t s) { return s < 4 ? 1 + s : ((2 + (s & 1)) << ((s >> 1) - 1)) + 1; }
BGZF_HD uint32_t dist_extra(uint32_t s) { return s < 4 ? 0 : (s >> 1) - 1; }

// the lengths of a dynamic block into T.lens[0, nlen + ndist)
template <class In, class Out>
BGZF_HD uint32_t read_dynamic(BitReader<In> &br, Out &out, Tables &T, uint32_t *nlen, uint32_t *ndist) {
    br.refill();
    *nlen = br.take(5) + 257;
    *ndist = br.take(5) + 1;
    const uint32_t ncode = br.take(4) + 4;
    if (br.over()) return kInputEnd;
    if (*nlen > 286 || *ndist > 30) return kBadCounts;
    for (uint32_t i = 0; i < 19; ++i) T.lens[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
        br.refill();
        T.lens[uint8_t("\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i])] = uint8_t(br.take(3));
    }
    if (br.over()) return kInputEnd;
    // the code-length code borrows the distance code's slots, which are rebuilt after it
    uint32_t rc = build_code(out, T.lens, 19, 7, false, &T.dist, T.next, T.dist_sym, T.dist_tab, kBadCodeLens);
    if (rc != kOk) return rc;
    bool any = false;
    for (uint32_t l = 1; l <= 7; ++l) any = any || T.dist.count[l];
    if (!any) return kBadCodeLens;
    const uint32_t total = *nlen + *ndist;
    // T.lens[0, 19) is dead once that code is built, so the symbols' lengths overwrite it
    uint8_t *lens = T.lens;
    uint32_t i = 0, prev = 0;
    while (i < total) {
        br.refill();
        const int32_t s = decode_symbol(br, T.dist, T.dist_sym, T.dist_tab, 7);
        if (br.over()) return kInputEnd;
        if (s < 0) return kBadCodeLens;
        if (s < 16) {
            lens[i++] = uint8_t(s);
            prev = uint32_t(s);
            continue;
        }
        uint32_t rep, val = 0;
        if (s == 16) {
            if (i == 0) return kBadCodeLens;
            val = prev;
            rep = 3 + br.take(2);
        } else if (s == 17) {
            rep = 3 + br.take(3);
        } else {
            rep = 11 + br.take(7);
        }
        if (br.over()) return kInputEnd;
        if (i + rep > total) return kBadCodeLens;
        for (uint32_t k = 0; k < rep; ++k) lens[i++] = uint8_t(val);
        prev = val;
    }
    return kOk;
}

// Inflates one member: kOk with *produced == isize, or the first failure. CRC32 is the caller's (it owns the bytes).
template <class In, class Out>
BGZF_HD uint32_t inflate_member(In &in, Out &out, Tables &T, uint32_t isize, uint32_t *produced) {
    BitReader<In> br(in);
    uint32_t at = 0, last;
    *produced = 0;
    do {
        br.refill();
        last = br.take(1);
        const uint32_t type = br.take(2);
        if (br.over()) return kInputEnd;
        if (type == 3) return kBadBlockType;
        if (type == 0) {
            br.drop(br.nbits & 7);
            uint32_t p = br.pos - br.nbits / 8;  // the byte after the header bits
            br.hold = 0;
            br.nbits = 0;
            if (uint64_t(p) + 4 > in.size()) return kInputEnd;
            const uint32_t w = in.load32(p);
            uint32_t len = w & 0xFFFF;
            if (len != ((w >> 16) ^ 0xFFFF)) return kStoredLen;
            p += 4;
            if (len > in.size() - p) return kInputEnd;
            if (len > isize - at) return kOutputFull;
            while (len) {
                uint32_t n = in.span(p);
                const uint32_t r = out.room(at);
                n = n < r ? n : r;
                n = n < len ? n : len;
                out.copy_in(in, p, at, n);
                p += n;
                at += n;
                len -= n;
            }
            br.pos = p;
            *produced = at;
            continue;
        }
        uint32_t nlen = 288, ndist = 32;  // the fixed codes, complete with their unused symbols (rejected when met)
        if (type == 1) {
            for (uint32_t s = 0; s < 288; ++s) T.lens[s] = uint8_t(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (uint32_t s = 0; s < 32; ++s) T.lens[288 + s] = 5;
        } else {
            const uint32_t rc = read_dynamic(br, out, T, &nlen, &ndist);
            if (rc != kOk) return rc;
            if (T.lens[256] == 0) return kNoEndOfBlock;
        }
        uint32_t rc = build_code(out, T.lens, nlen, kLitBits, false, &T.lit, T.next, T.lit_sym, T.lit_tab, kBadLitLen);
        if (rc != kOk) return rc;
        rc = build_code(out, T.lens + nlen, ndist, kDistBits, true, &T.dist, T.next, T.dist_sym, T.dist_tab, kBadDist);
        if (rc != kOk) return rc;
        for (;;) {
            br.refill();
            const int32_t s = decode_symbol(br, T.lit, T.lit_sym, T.lit_tab, kLitBits);
            if (br.over()) return kInputEnd;
            if (s < 0) return kBadSymbol;
            if (s < 256) {
                if (at >= isize) return kOutputFull;
                out.put(at++, uint8_t(s));
                continue;
            }
            if (s == 256) break;
            if (s > 285) return kBadSymbol;
            const uint32_t len = len_base(uint32_t(s) - 257) + br.take(len_extra(uint32_t(s) - 257));
            br.refill();
            const int32_t d = decode_symbol(br, T.dist, T.dist_sym, T.dist_tab, kDistBits);
            if (br.over()) return kInputEnd;
            if (d < 0 || d > 29) return kBadSymbol;
            const uint32_t dist = dist_base(uint32_t(d)) + br.take(dist_extra(uint32_t(d)));
            if (br.over()) return kInputEnd;
            if (dist > at) return kDistTooFar;
            if (len > isize - at) return kOutputFull;
            out.match(at, dist, len);
            at += len;
        }
        *produced = at;
    } while (!last);
    *produced = at;
    return at == isize ? kOk : kSizeMismatch;
}

// ---------------------------------------------------------------------------------------------------------------
// CRC32 (the gzip polynomial, reflected) in pieces: each lane takes a fixed-size chunk, the pieces are joined with
// crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B), which is linear, so the join is an xor over the lanes.

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcChunk = 260;  // bytes per lane: 65 dwords, so the 64 lanes start on 32 different LDS banks

BGZF_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}

// a(x) * b(x) mod P, bit-reflected operands
BGZF_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 n) mod P
BGZF_HD uint32_t crc_x8n(uint32_t n) {
    uint32_t p = 1u << 31, sq = 0x00800000u;  // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1) p = crc_mul(sq, p);
        sq = crc_mul(sq, sq);
    }
    return p;
}

// crc of A || B from crc(A), crc(B) and |B|
BGZF_HD uint32_t crc_join(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) {
    return crc_mul(crc_x8n(len_b), crc_a) ^ crc_b;
}

}  // namespace bgzf
}  // namespace secedo
