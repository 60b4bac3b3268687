// bgzf_deflate.hpp -- RFC 1951 deflate of one BGZF member, written once for the device (bgzf_deflate_kernels.hip, one
// wavefront per member) and the host (tests/cpp/bgzf_deflate_test.cpp, plain g++ under the sanitizers). Everything
// that decides the bytes lives here: the hash, which candidate a position sees and when it is accepted, the greedy
// parse, the fixed-Huffman codes and their bit layout, the stored fallback, the header and the trailer. The two builds
// give the same bytes because they run the same statements; only how the 64 items of a strip are spread over lanes
// differs, behind three small interfaces the caller supplies:
//
//   In     uint32_t load32(uint32_t p)          text bytes [p, p + 4), little endian; only asked with p + 4 <= n
//          uint32_t byte(uint32_t p)            text byte p < n
//   Out    void word(uint32_t k, uint32_t v)    payload bytes [4k, 4k + 4) (the payload starts at member byte 18)
//          void byte(uint32_t at, uint32_t v)   member byte `at`
//   Lanes  void lane_range(uint32_t n, uint32_t *first, uint32_t *step)   split of a loop of n independent items
//          void sync()                          what the lanes wrote to Work is visible to all of them
//          void fence()                         sync(), and what they wrote through Out is ordered before what follows
//          bool leader()                        true in exactly one lane (the serial steps)
//          void or32(uint32_t *p, uint32_t v)   *p |= v, safe against another lane's or32 on the same word
//
// The rules:
//   - position i hashes text[i, i + 4) to kHashBits bits (none for the last three positions of the member);
//   - its one candidate is the most recent earlier position of the member with the same hash: the strip's own
//     positions first (so the previous line of a VCF, 50-70 bytes back, and a run at distance 1 are seen), then
//     the table, which holds the last position of every hash over the strips before;
//   - the candidate is taken when it is at most 32768 back and matches at least 4 bytes, or 3 bytes at most 4096 back
//     (a far 3-byte match costs more bits than its literals); the match ends at 258 bytes or the member's end;
//   - the parse is greedy: a token starts where the one before ended, a match if the position has one, else a literal;
//   - one BTYPE 1 block; if its payload would not be smaller than the stored form (5 + n bytes), one BTYPE 0 block.
// Every value that reaches the output is a function of the text alone: or32 and the "last of its hash in the strip
// writes the table" rule are independent of the order in which lanes run.
#pragma once

#include "bgzf_inflate.hpp"

#include <array>

#if defined(__HIPCC__)
#define BGZF_UNROLL _Pragma("unroll")
#else
#define BGZF_UNROLL
#endif

namespace secedo {
namespace bgzf {

constexpr uint32_t kHeaderBytes = 18, kTrailerBytes = 8, kStoredHead = 5;
constexpr uint32_t kMaxMember = kHeaderBytes + kStoredHead + kCut + kTrailerBytes;
static_assert(kMaxMember <= 65536, "BSIZE is 16 bits");
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258, kMaxDistance = 32768, kFarForMin = 4096;
constexpr uint32_t kHashBits = 12, kNoHash = 0xFFFF;
constexpr uint32_t kStrip = 64;       // positions handled together; one per lane on the device
constexpr uint32_t kStageWords = 24;  // a strip starts at most 22 tokens of 31 bits (a match spans 3 positions) behind a carry of < 32 bits
// bytes per lane of the CRC32: 257 dwords, so that the 64 lanes start on different LDS banks
constexpr uint32_t kDeflateCrcChunk = 1028;
static_assert(kDeflateCrcChunk * kStrip >= kCut && kDeflateCrcChunk % 4 == 0, "one CRC chunk per lane covers a member");
// the compressed payload is given up for the stored form once it has this many bits more than the stored form; what
// it may have written by then is bounded by one strip more
constexpr uint32_t kOverrunBytes = 4 * kStageWords;

constexpr uint32_t kEofBytes = 28;
BGZF_HD uint32_t eof_member_byte(uint32_t k) {
    return uint8_t("\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"[k]);
}
inline std::array<uint8_t, kEofBytes> eof_member() {  // for the host: what every writer ends a file with
    std::array<uint8_t, kEofBytes> m;
    for (uint32_t k = 0; k < kEofBytes; ++k) m[k] = uint8_t(eof_member_byte(k));
    return m;
}

// the encoder's working set: LDS on the device, the stack on the host
struct Work {
    uint16_t table[1u << kHashBits];  // 1 + the last position with this hash in the strips before; 0 = none
    uint32_t crc_tab[256];
    uint32_t crc_part[kStrip];
    uint32_t stage[kStageWords];  // the payload's bits from the last whole dword written on
    uint32_t code[kStrip];
    uint32_t scan[2][kStrip];
    uint16_t hash[kStrip], len[kStrip], dist[kStrip];
    uint8_t start[kStrip], last[kStrip];
    uint32_t next;  // where the next token starts
};

BGZF_HD uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - kHashBits); }

// bytes that text[a, ...) and text[b, ...) share, at most `max`; a < b and b + max <= n
template <class In>
BGZF_HD uint32_t match_length(In &in, uint32_t a, uint32_t b, uint32_t max) {
    uint32_t k = 0;
    for (; k + 4 <= max; k += 4) {
        const uint32_t x = in.load32(a + k) ^ in.load32(b + k);
        if (x) return k + (uint32_t(__builtin_ctz(x)) >> 3);
    }
    while (k < max && in.byte(a + k) == in.byte(b + k)) ++k;
    return k;
}

BGZF_HD bool accept_match(uint32_t len, uint32_t dist) {
    return dist <= kMaxDistance && (len > kMinMatch || (len == kMinMatch && dist <= kFarForMin));
}

BGZF_HD uint32_t floor_log2(uint32_t v) { return 31u - uint32_t(__builtin_clz(v)); }

// the length symbol (0..28, code 257 + s) and distance symbol (0..29): the inverses of len_base and dist_base
BGZF_HD uint32_t len_symbol(uint32_t len) {
    if (len == kMaxMatch) return 28;
    const uint32_t l = len - 3;
    if (l < 8) return l;
    const uint32_t e = floor_log2(l) - 2;
    return 4 * (e + 1) + ((l >> e) - 4);
}
BGZF_HD uint32_t dist_symbol(uint32_t dist) {
    const uint32_t d = dist - 1;
    if (d < 4) return d;
    const uint32_t e = floor_log2(d) - 1;
    return 2 * (e + 1) + ((d >> e) - 2);
}

// the fixed literal/length code of symbol s < 288, ready for the LSB-first stream
BGZF_HD uint32_t fixed_litlen(uint32_t s, uint32_t *nbits) {
    const uint32_t n = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    const uint32_t code = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xC0 + (s - 280);
    *nbits = n;
    return reverse_bits(code, n);
}

// one token's bits, at most 31: a literal (len 0), or length code, length extra, distance code, distance extra
BGZF_HD uint32_t token_bits(uint32_t len, uint32_t dist, uint32_t literal, uint32_t *nbits) {
    if (len == 0) return fixed_litlen(literal, nbits);
    const uint32_t ls = len_symbol(len), ds = dist_symbol(dist);
    uint32_t n;
    uint32_t v = fixed_litlen(257 + ls, &n);
    v |= (len - len_base(ls)) << n;
    n += len_extra(ls);
    v |= reverse_bits(ds, 5) << n;
    n += 5;
    v |= (dist - dist_base(ds)) << n;
    n += dist_extra(ds);
    *nbits = n;
    return v;
}

BGZF_HD uint32_t member_head_byte(uint32_t k, uint32_t member_bytes) {
    if (k == 16) return (member_bytes - 1) & 0xFF;
    if (k == 17) return (member_bytes - 1) >> 8;
    return uint8_t("\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00"[k]);
}

// CRC32 of the member's text: a chunk per lane, joined by x^(8 len) mod P (the pieces of bgzf_inflate.hpp)
template <class In, class Lanes>
BGZF_HD uint32_t crc32_text(In &in, uint32_t n, Work &W, Lanes &L) {
    uint32_t i0, step;
    L.lane_range(256, &i0, &step);
    for (uint32_t i = i0; i < 256; i += step) W.crc_tab[i] = crc_table_entry(i);
    L.sync();
    L.lane_range(kStrip, &i0, &step);
    for (uint32_t l = i0; l < kStrip; l += step) {
        const uint32_t c0 = l * kDeflateCrcChunk < n ? l * kDeflateCrcChunk : n;
        const uint32_t c1 = (l + 1) * kDeflateCrcChunk < n ? (l + 1) * kDeflateCrcChunk : n;
        uint32_t c = ~0u, i = c0;
        for (; i + 4 <= c1; i += 4) {
            uint32_t w = in.load32(i);
            for (int k = 0; k < 4; ++k, w >>= 8) c = W.crc_tab[(c ^ w) & 0xFF] ^ (c >> 8);
        }
        for (; i < c1; ++i) c = W.crc_tab[(c ^ in.byte(i)) & 0xFF] ^ (c >> 8);
        W.crc_part[l] = c1 > c0 ? crc_mul(crc_x8n(n - c1), ~c) : 0;
    }
    L.sync();
    uint32_t crc = 0;
    for (uint32_t l = 0; l < kStrip; ++l) crc ^= W.crc_part[l];
    return crc;
}

// The member of text [0, n), n <= kCut, through `out`: its size in bytes; *stored = 1 when it fell back to BTYPE 0.
// Both are the same in every lane.
template <class In, class Out, class Lanes>
BGZF_HD uint32_t deflate_member(In &in, uint32_t n, Out &out, Work &W, Lanes &L, uint32_t *stored) {
    uint32_t i0, step;
    L.lane_range(1u << kHashBits, &i0, &step);
    for (uint32_t i = i0; i < (1u << kHashBits); i += step) W.table[i] = 0;
    L.lane_range(kStageWords, &i0, &step);
    for (uint32_t i = i0; i < kStageWords; i += step) W.stage[i] = i == 0 ? 3u : 0u;  // BFINAL 1, BTYPE 01
    if (L.leader()) W.next = 0;
    L.sync();
    uint32_t bits = 3, words_out = 0;
    const uint32_t give_up = 8 * (n + kStoredHead);
    bool over = false;

    for (uint32_t base = 0; base < n && !over; base += kStrip) {
        const uint32_t next = W.next;
        L.lane_range(kStrip, &i0, &step);
        for (uint32_t l = i0; l < kStrip; l += step)
            W.hash[l] = uint16_t(base + l + 4 <= n ? hash4(in.load32(base + l)) : kNoHash);
        L.sync();
        // the candidate and its match; positions before `next` lie inside a token already emitted
        for (uint32_t l = i0; l < kStrip; l += step) {
            const uint32_t i = base + l, h = W.hash[l];
            uint32_t len = 0, dist = 0;
            // one pass over the strip's hashes (constant indices: registers on the device): the nearest equal one
            // before this position, and whether an equal one follows
            uint32_t near = kStrip;
            bool last = true;
            BGZF_UNROLL
            for (uint32_t j = 0; j < kStrip; ++j) {
                const bool same = W.hash[j] == h;
                near = same && j < l ? j : near;
                last = last && !(same && j > l);
            }
            W.last[l] = last && h != kNoHash;
            if (i >= next && h != kNoHash) {
                uint32_t cand = ~0u;
                if (near != kStrip) cand = base + near;
                else if (W.table[h]) cand = W.table[h] - 1u;
                if (cand != ~0u && i - cand <= kMaxDistance) {
                    const uint32_t m = match_length(in, cand, i, n - i < kMaxMatch ? n - i : kMaxMatch);
                    if (accept_match(m, i - cand)) len = m, dist = i - cand;
                }
            }
            W.len[l] = uint16_t(len);
            W.dist[l] = uint16_t(dist);
            W.start[l] = 0;
        }
        L.sync();
        // the table takes each hash's last position of the strip; the leader walks the greedy parse (the serial part)
        for (uint32_t l = i0; l < kStrip; l += step)
            if (W.last[l]) W.table[W.hash[l]] = uint16_t(base + l + 1);
        if (L.leader()) {
            uint32_t p = next > base ? next : base;
            const uint32_t end = base + kStrip < n ? base + kStrip : n;
            while (p < end) {
                W.start[p - base] = 1;
                p += W.len[p - base] ? W.len[p - base] : 1u;
            }
            W.next = p;
        }
        L.sync();
        for (uint32_t l = i0; l < kStrip; l += step) {
            uint32_t nb = 0, v = 0;
            if (W.start[l]) v = token_bits(W.len[l], W.dist[l], W.len[l] ? 0 : in.byte(base + l), &nb);
            W.code[l] = v;
            W.scan[0][l] = nb;
        }
        L.sync();
        // bit offsets: the inclusive prefix sum of the bit lengths (six doubling rounds end in scan[0])
        for (uint32_t r = 0; r < 6; ++r) {
            const uint32_t a = r & 1, sh = 1u << r;
            for (uint32_t l = i0; l < kStrip; l += step) W.scan[a ^ 1][l] = W.scan[a][l] + (l >= sh ? W.scan[a][l - sh] : 0);
            L.sync();
        }
        const uint32_t bit0 = bits - 32 * words_out;
        for (uint32_t l = i0; l < kStrip; l += step) {
            const uint32_t before = l ? W.scan[0][l - 1] : 0, nb = W.scan[0][l] - before;
            if (!nb) continue;
            const uint32_t at = bit0 + before, sh = at & 31, v = W.code[l];
            L.or32(&W.stage[at >> 5], v << sh);
            if (sh + nb > 32) L.or32(&W.stage[(at >> 5) + 1], v >> (32 - sh));
        }
        bits += W.scan[0][kStrip - 1];
        L.sync();
        // whole dwords go out; the open one moves to the front
        const uint32_t full = bits / 32 - words_out;
        L.lane_range(full, &i0, &step);
        for (uint32_t k = i0; k < full; k += step) out.word(words_out + k, W.stage[k]);
        const uint32_t carry = W.stage[full];
        L.sync();
        L.lane_range(kStageWords, &i0, &step);
        for (uint32_t k = i0; k < kStageWords; k += step) W.stage[k] = k == 0 ? carry : 0u;
        L.sync();
        words_out += full;
        over = bits > give_up;
    }

    bits += 7;  // end of block: seven zero bits
    uint32_t payload = (bits + 7) / 8;
    *stored = over || payload >= n + kStoredHead;
    if (!*stored) {
        const uint32_t rest = payload - 4 * words_out;  // at most 5 bytes: under 32 open bits and the end of block
        L.lane_range(rest, &i0, &step);
        for (uint32_t k = i0; k < rest; k += step)
            out.byte(kHeaderBytes + 4 * words_out + k, (W.stage[k >> 2] >> (8 * (k & 3))) & 0xFF);
    } else {
        L.fence();  // the stored bytes overwrite what the compressed attempt wrote
        payload = n + kStoredHead;
        L.lane_range(kStoredHead, &i0, &step);
        for (uint32_t k = i0; k < kStoredHead; k += step) {
            const uint32_t len16 = k < 3 ? n : n ^ 0xFFFF;
            out.byte(kHeaderBytes + k, k == 0 ? 1u : (len16 >> (8 * ((k - 1) & 1))) & 0xFF);
        }
        L.lane_range(n, &i0, &step);
        for (uint32_t i = i0; i < n; i += step) out.byte(kHeaderBytes + kStoredHead + i, in.byte(i));
    }
    const uint32_t crc = crc32_text(in, n, W, L);
    const uint32_t member = kHeaderBytes + payload + kTrailerBytes;
    L.lane_range(kHeaderBytes + kTrailerBytes, &i0, &step);
    for (uint32_t k = i0; k < kHeaderBytes + kTrailerBytes; k += step) {
        if (k < kHeaderBytes) {
            out.byte(k, member_head_byte(k, member));
        } else {
            const uint32_t t = k - kHeaderBytes;
            out.byte(kHeaderBytes + payload + t, ((t < 4 ? crc : n) >> (8 * (t & 3))) & 0xFF);
        }
    }
    return member;
}

}  // namespace bgzf
}  // namespace secedo
