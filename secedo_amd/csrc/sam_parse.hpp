// sam_parse.hpp -- the SAM line parser of sam_kernels.hip as host/device code: one alignment line -> its BAM record,
// and the per-vector steps of the line split. The kernels of sam_kernels.hip run it a thread per vector or per line;
// tests/cpp/sam_parse_test.cpp runs the same code on the host under the sanitizers. No HIP header is needed here.
// See sam_kernels.hip for the conversion rules.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SECEDO_SAM_HD __host__ __device__
#define SECEDO_SAM_HDI __host__ __device__ __forceinline__
#define SECEDO_SAM_UNROLL _Pragma("unroll")
#else
#define SECEDO_SAM_HD
#define SECEDO_SAM_HDI inline
#define SECEDO_SAM_UNROLL
#endif

namespace secedo {
namespace bam {

// error codes of the SAM passes, reported for the lowest line that has one (u64 min of line << 8 | code)
enum SamErr : uint32_t {
    kSamOk = 0,
    kSamFields = 1,     // fewer than 11 tab-separated mandatory fields, or an empty one
    kSamName = 2,       // QNAME longer than 254 characters
    kSamFlag = 3,       // FLAG not a decimal integer in [0, 65535]
    kSamRname = 4,      // RNAME not '*' and not an @SQ name
    kSamPos = 5,        // POS not a decimal integer in [0, 2^31 - 1]
    kSamMapq = 6,       // MAPQ not a decimal integer in [0, 255]
    kSamCigar = 7,      // CIGAR not '*' and not ops MIDNSHP=X with lengths in [1, 2^28)
    kSamRnext = 8,      // RNEXT not '*', '=' or an @SQ name
    kSamPnext = 9,      // PNEXT not a decimal integer in [0, 2^31 - 1]
    kSamTlen = 10,      // TLEN not a decimal integer in [-(2^31 - 1), 2^31 - 1]
    kSamQual = 11,      // QUAL not '*', of another length than SEQ, or a character outside '!'..'~'
    kSamCigarSeq = 12,  // CIGAR query length (M/I/S/=/X) differs from the SEQ length
    kSamAux = 13,       // a malformed optional field
    kSamHeader = 14,    // an '@' line after the first alignment line
    kSamEmpty = 15,     // an empty line that does not end the file
    kSamManyOps = 16,   // more than 65535 CIGAR ops (SECEDO_E_LIMIT)
    kSamTooLong = 17,   // a record of 2^31 bytes or more (SECEDO_E_LIMIT)
    kSamCodes = 18,
};

// RefID of a line that is no record (the empty line that ends a file)
constexpr int32_t kSamNoRecord = -2147483647 - 1;

// 64-bit FNV-1a of a reference name; the host hashes the @SQ names with it, the device the RNAME / RNEXT fields
SECEDO_SAM_HD inline uint64_t sam_name_hash(const uint8_t *p, uint32_t n) {
    uint64_t h = 1469598103934665603ull;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// the @SQ names of one file: packed bytes (off[n + 1] by RefID), their hashes sorted and the RefID of each;
// sel[RefID] = 1 for the chromosomes whose records are encoded
struct SamRefs {
    const uint8_t *bytes;
    const uint32_t *off;
    const uint64_t *hash;
    const uint32_t *id;
    const uint8_t *sel;
    uint32_t n;
};

// '\n' bytes of a 32-bit word (exact zero-byte test of w ^ 0x0A0A0A0A)
SECEDO_SAM_HDI uint32_t newlines(uint32_t w) {
    const uint32_t t = w ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
    return uint32_t(__builtin_popcount(z));
}

// '\n' bytes of a 16-byte vector given as its four little-endian words
SECEDO_SAM_HDI uint32_t vector_newlines(const uint32_t w[4]) {
    return newlines(w[0]) + newlines(w[1]) + newlines(w[2]) + newlines(w[3]);
}

// the line starts of vector i: the byte after each of its '\n', at start[k + 1...], k = the '\n' before the vector
SECEDO_SAM_HDI void vector_starts(const uint32_t w[4], uint64_t i, uint32_t k, uint32_t *start) {
    SECEDO_SAM_UNROLL
    for (int j = 0; j < 16; ++j)
        if (((w[j / 4] >> (8 * (j % 4))) & 0xFF) == '\n') start[++k] = uint32_t(i * 16 + j + 1);
}

SECEDO_SAM_HDI bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
SECEDO_SAM_HDI bool is_alpha(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

SECEDO_SAM_HDI uint32_t float_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// decimal integer over [a, b), '-' allowed when neg_ok; values beyond 2^40 saturate there (out of every range)
SECEDO_SAM_HD inline bool parse_int(const uint8_t *s, uint32_t a, uint32_t b, bool neg_ok, int64_t *v) {
    bool neg = false;
    if (a < b && s[a] == '-') {
        if (!neg_ok) return false;
        neg = true;
        ++a;
    }
    if (a >= b) return false;
    int64_t x = 0;
    for (uint32_t i = a; i < b; ++i) {
        if (!is_digit(s[i])) return false;
        if (x < (int64_t(1) << 40)) x = x * 10 + (s[i] - '0');
    }
    *v = neg ? -x : x;
    return true;
}

// decimal float [-+]digits[.digits][(e|E)[-+]digits] over [a, b)
SECEDO_SAM_HD inline bool parse_float(const uint8_t *s, uint32_t a, uint32_t b, float *f) {
    bool neg = false;
    if (a < b && (s[a] == '-' || s[a] == '+')) neg = s[a++] == '-';
    double m = 0;
    int e10 = 0, nd = 0, sig = 0;
    for (; a < b && is_digit(s[a]); ++a, ++nd) {
        if (sig < 18) m = m * 10 + (s[a] - '0'), sig += m > 0;
        else ++e10;
    }
    if (a < b && s[a] == '.') {
        for (++a; a < b && is_digit(s[a]); ++a, ++nd)
            if (sig < 18) m = m * 10 + (s[a] - '0'), sig += m > 0, --e10;
    }
    if (nd == 0) return false;
    if (a < b && (s[a] == 'e' || s[a] == 'E')) {
        ++a;
        bool eneg = false;
        if (a < b && (s[a] == '-' || s[a] == '+')) eneg = s[a++] == '-';
        if (a >= b) return false;
        int x = 0;
        for (; a < b && is_digit(s[a]); ++a)
            if (x < 100000) x = x * 10 + (s[a] - '0');
        e10 += eneg ? -x : x;
    }
    if (a != b) return false;
    const int e = e10 < -400 ? -400 : e10 > 400 ? 400 : e10;
    const double v = m == 0 ? 0.0 : m * pow(10.0, double(e));
    *f = float(neg ? -v : v);
    return true;
}

// seq_nt16 code of a letter, either case
SECEDO_SAM_HDI uint32_t nt16(uint8_t c) {
    switch (c & 0xDF) {
        case 'A': return 1;
        case 'C': return 2;
        case 'M': return 3;
        case 'G': return 4;
        case 'R': return 5;
        case 'S': return 6;
        case 'V': return 7;
        case 'T': return 8;
        case 'W': return 9;
        case 'Y': return 10;
        case 'H': return 11;
        case 'K': return 12;
        case 'D': return 13;
        case 'B': return 14;
        default: return 15;
    }
}
SECEDO_SAM_HDI uint32_t seq_code(uint8_t c) { return c == '=' ? 0 : is_alpha(c) ? nt16(c) : 15; }

// RefID of a name: lower bound of its hash, exact compare over the run of equal hashes; -1 when absent
SECEDO_SAM_HD inline int32_t ref_id(const SamRefs &R, const uint8_t *p, uint32_t n) {
    const uint64_t h = sam_name_hash(p, n);
    uint32_t lo = 0, hi = R.n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (R.hash[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    for (; lo < R.n && R.hash[lo] == h; ++lo) {
        const uint32_t id = R.id[lo], b = R.off[id], e = R.off[id + 1];
        if (e - b != n) continue;
        uint32_t i = 0;
        while (i < n && R.bytes[b + i] == p[i]) ++i;
        if (i == n) return int32_t(id);
    }
    return -1;
}

// byte writer: W = false only counts
template <bool W>
struct Put {
    uint8_t *o;
    uint64_t n = 0;
    SECEDO_SAM_HD explicit Put(uint8_t *out) : o(out) {}
    SECEDO_SAM_HD void u8(uint32_t v) {
        if (W) o[n] = uint8_t(v);
        ++n;
    }
    SECEDO_SAM_HD void u16(uint32_t v) { u8(v), u8(v >> 8); }
    SECEDO_SAM_HD void u32(uint32_t v) { u8(v), u8(v >> 8), u8(v >> 16), u8(v >> 24); }
    SECEDO_SAM_HD void bytes(const uint8_t *p, uint32_t k) {
        if (W)
            for (uint32_t i = 0; i < k; ++i) o[n + i] = p[i];
        n += k;
    }
};

SECEDO_SAM_HDI uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return uint32_t(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return uint32_t(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return uint32_t(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return uint32_t(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return uint32_t(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

SECEDO_SAM_HDI int op_index(uint8_t c) {
    switch (c) {
        case 'M': return 0;
        case 'I': return 1;
        case 'D': return 2;
        case 'N': return 3;
        case 'S': return 4;
        case 'H': return 5;
        case 'P': return 6;
        case '=': return 7;
        case 'X': return 8;
        default: return -1;
    }
}

// one optional field [a, b) -> its BAM bytes; false when malformed
template <bool W>
SECEDO_SAM_HD inline bool parse_aux(const uint8_t *s, uint32_t a, uint32_t b, Put<W> &out) {
    if (b - a < 5 || s[a + 2] != ':' || s[a + 4] != ':' || !is_alpha(s[a]) ||
        !(is_alpha(s[a + 1]) || is_digit(s[a + 1])))
        return false;
    const uint8_t type = s[a + 3];
    const uint32_t v = a + 5;
    out.u8(s[a]);
    out.u8(s[a + 1]);
    switch (type) {
        case 'A':
            if (b - v != 1 || s[v] < '!' || s[v] > '~') return false;
            out.u8('A');
            out.u8(s[v]);
            return true;
        case 'i': {
            int64_t x;
            if (!parse_int(s, v, b, true, &x)) return false;
            if (x < 0) {
                if (x >= -128) out.u8('c'), out.u8(uint32_t(x));
                else if (x >= -32768) out.u8('s'), out.u16(uint32_t(x));
                else if (x >= -2147483648ll) out.u8('i'), out.u32(uint32_t(x));
                else return false;
            } else {
                if (x <= 255) out.u8('C'), out.u8(uint32_t(x));
                else if (x <= 65535) out.u8('S'), out.u16(uint32_t(x));
                else if (x <= 4294967295ll) out.u8('I'), out.u32(uint32_t(x));
                else return false;
            }
            return true;
        }
        case 'f': {
            float f;
            if (!parse_float(s, v, b, &f)) return false;
            out.u8('f');
            out.u32(float_bits(f));
            return true;
        }
        case 'Z':
        case 'H':
            out.u8(type);
            out.bytes(s + v, b - v);
            out.u8(0);
            return true;
        case 'B': {
            if (v >= b) return false;
            const uint8_t sub = s[v];
            int64_t lo, hi;
            switch (sub) {
                case 'c': lo = -128, hi = 127; break;
                case 'C': lo = 0, hi = 255; break;
                case 's': lo = -32768, hi = 32767; break;
                case 'S': lo = 0, hi = 65535; break;
                case 'i': lo = -2147483648ll, hi = 2147483647ll; break;
                case 'I': lo = 0, hi = 4294967295ll; break;
                case 'f': lo = hi = 0; break;
                default: return false;
            }
            if (v + 1 < b && s[v + 1] != ',') return false;
            uint32_t cnt = 0;
            for (uint32_t i = v + 1; i < b; ++i) cnt += s[i] == ',';
            out.u8('B');
            out.u8(sub);
            out.u32(cnt);
            for (uint32_t i = v + 1; i < b;) {
                const uint32_t e0 = i + 1;
                uint32_t e1 = e0;
                while (e1 < b && s[e1] != ',') ++e1;
                if (sub == 'f') {
                    float f;
                    if (!parse_float(s, e0, e1, &f)) return false;
                    out.u32(float_bits(f));
                } else {
                    int64_t x;
                    if (!parse_int(s, e0, e1, lo < 0, &x) || x < lo || x > hi) return false;
                    if (sub == 'c' || sub == 'C') out.u8(uint32_t(x));
                    else if (sub == 's' || sub == 'S') out.u16(uint32_t(x));
                    else out.u32(uint32_t(x));
                }
                i = e1;
            }
            return true;
        }
        default: return false;
    }
}

struct LineInfo {
    int32_t ref, pos;
    uint64_t bytes;  // the record with its block_size field
};

// One alignment line s[0, n) -> its BAM record (W: written at out). Returns a SamErr.
template <bool W>
SECEDO_SAM_HD inline uint32_t parse_line(const uint8_t *s, uint32_t n, const SamRefs &R, uint8_t *out, LineInfo *li) {
    if (n == 0) return kSamEmpty;
    if (s[0] == '@') return kSamHeader;
    uint32_t fa[11], fb[11];
    uint32_t o = 0;
    SECEDO_SAM_UNROLL
    for (int f = 0; f < 11; ++f) {
        fa[f] = o;
        while (o < n && s[o] != '\t') ++o;
        fb[f] = o;
        if (fb[f] == fa[f] || (f < 10 && o >= n)) return kSamFields;
        if (f < 10) ++o;
    }
    const uint32_t l_name = fb[0] - fa[0];
    if (l_name > 254) return kSamName;
    int64_t flag, pos, mapq, pnext, tlen;
    if (!parse_int(s, fa[1], fb[1], false, &flag) || flag > 65535) return kSamFlag;
    const bool star_ref = fb[2] - fa[2] == 1 && s[fa[2]] == '*';
    const int32_t ref = star_ref ? -1 : ref_id(R, s + fa[2], fb[2] - fa[2]);
    if (ref < 0 && !star_ref) return kSamRname;
    if (!parse_int(s, fa[3], fb[3], false, &pos) || pos > 2147483647ll) return kSamPos;
    if (!parse_int(s, fa[4], fb[4], false, &mapq) || mapq > 255) return kSamMapq;
    uint32_t n_cigar = 0;
    uint64_t qlen = 0, rlen = 0;
    if (!(fb[5] - fa[5] == 1 && s[fa[5]] == '*')) {
        for (uint32_t i = fa[5]; i < fb[5];) {
            const uint32_t d0 = i;
            uint64_t len = 0;
            for (; i < fb[5] && is_digit(s[i]); ++i)
                if (len < (1u << 28)) len = len * 10 + (s[i] - '0');
            if (i == d0 || i >= fb[5]) return kSamCigar;
            const int op = op_index(s[i++]);
            if (op < 0 || len == 0 || len >= (1u << 28)) return kSamCigar;
            ++n_cigar;
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += len;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += len;
        }
        if (n_cigar > 65535) return kSamManyOps;
    }
    int32_t next_ref;
    if (fb[6] - fa[6] == 1 && s[fa[6]] == '*') next_ref = -1;
    else if (fb[6] - fa[6] == 1 && s[fa[6]] == '=') next_ref = ref;
    else if ((next_ref = ref_id(R, s + fa[6], fb[6] - fa[6])) < 0) return kSamRnext;
    if (!parse_int(s, fa[7], fb[7], false, &pnext) || pnext > 2147483647ll) return kSamPnext;
    if (!parse_int(s, fa[8], fb[8], true, &tlen) || tlen > 2147483647ll || tlen < -2147483647ll) return kSamTlen;
    const bool no_seq = fb[9] - fa[9] == 1 && s[fa[9]] == '*';
    const uint32_t l_seq = no_seq ? 0 : fb[9] - fa[9];
    const bool no_qual = fb[10] - fa[10] == 1 && s[fa[10]] == '*';
    if (!no_qual) {
        if (fb[10] - fa[10] != l_seq) return kSamQual;
        for (uint32_t i = fa[10]; i < fb[10]; ++i)
            if (s[i] < '!' || s[i] > '~') return kSamQual;
    }
    if (n_cigar && l_seq && qlen != l_seq) return kSamCigarSeq;

    Put<W> p(out);
    const int32_t pos0 = int32_t(pos - 1);
    p.u32(0);  // block_size, written last
    p.u32(uint32_t(ref));
    p.u32(uint32_t(pos0));
    p.u8(l_name + 1);
    p.u8(uint32_t(mapq));
    const int64_t beg = pos0 < 0 ? 0 : pos0, end = int64_t(pos0) + int64_t(rlen > 0 ? rlen : 1);
    p.u16(reg2bin(beg, end < 1 ? 1 : end));
    p.u16(n_cigar);
    p.u16(uint32_t(flag));
    p.u32(l_seq);
    p.u32(uint32_t(next_ref));
    p.u32(uint32_t(int32_t(pnext - 1)));
    p.u32(uint32_t(int32_t(tlen)));
    p.bytes(s + fa[0], l_name);
    p.u8(0);
    if (n_cigar) {
        for (uint32_t i = fa[5]; i < fb[5];) {
            uint32_t len = 0;
            for (; is_digit(s[i]); ++i) len = len * 10 + (s[i] - '0');
            p.u32(len << 4 | uint32_t(op_index(s[i++])));
        }
    }
    if (W) {
        for (uint32_t k = 0; k < l_seq; k += 2)
            p.u8(seq_code(s[fa[9] + k]) << 4 | (k + 1 < l_seq ? seq_code(s[fa[9] + k + 1]) : 0));
        for (uint32_t k = 0; k < l_seq; ++k) p.u8(no_qual ? 0xFF : s[fa[10] + k] - 33);
    } else {
        p.n += (l_seq + 1) / 2 + l_seq;
    }
    for (uint32_t a = fb[10] + 1; a <= n;) {  // optional fields
        uint32_t b = a;
        while (b < n && s[b] != '\t') ++b;
        if (!parse_aux<W>(s, a, b, p)) return kSamAux;
        a = b + 1;
    }
    if (p.n - 4 >= (1ull << 31)) return kSamTooLong;
    if (W) {
        const uint32_t bs = uint32_t(p.n - 4);
        out[0] = uint8_t(bs), out[1] = uint8_t(bs >> 8), out[2] = uint8_t(bs >> 16), out[3] = uint8_t(bs >> 24);
    }
    li->ref = ref;
    li->pos = pos0;
    li->bytes = p.n;
    return kSamOk;
}

}  // namespace bam
}  // namespace secedo
