// sam_kernels.hip -- SAM text -> BAM records on gfx950, so that SAM input goes through bam_kernels.hip unchanged.
//
// The host cuts a file's alignment lines into ranges that end at a '\n' and uploads each one. Passes per range:
//   sam_newline_count (one thread per 16-byte vector: '\n' bytes, SWAR) -> exclusive scan -> sam_line_starts (the
//   byte after each '\n') -> sam_size (one thread per line: tokenise, validate, RefID, POS, record size) ->
//   exclusive scan of the sizes -> sam_encode (one thread per selected line: the BAM record at its scanned offset).
// Errors: the size pass takes the u64 min of (line << 8 | code), so the first bad line is reported whatever the
// thread order. Both passes run the same parser (parse_line<W>), counting or writing, so the sizes and the written
// records agree byte for byte. Plain C++ stores only.
//
// Conversion (htslib's sam_parse1, departures marked):
//  - 11 tab-separated mandatory fields, then optional fields. An '@' line is an error here (the header comes first),
//    so is an empty line unless it is the last line of the file. '\r' is an ordinary character.
//  - QNAME at most 254 characters, stored with its NUL. FLAG [0, 65535], POS and PNEXT [0, 2^31 - 1] stored minus
//    one, MAPQ [0, 255], TLEN [-(2^31 - 1), 2^31 - 1]: decimal integers ('-' only for TLEN).
//  - RNAME '*' -> -1, else the @SQ index found by hash (FNV-1a), lower bound in the sorted hashes and exact compare.
//    RNEXT '=' -> the record's RefID. A name missing from @SQ is an error (htslib warns and treats it as unmapped).
//  - CIGAR '*' -> no ops, else <len><op> with op in MIDNSHP=X and len in [1, 2^28); more than 65535 ops is a limit.
//  - SEQ '*' -> l_seq 0, else seq_nt16 codes (=ACMGRSVTWYHKDBN -> 0..15, case-insensitive, anything else 15).
//    QUAL '*' -> l_seq bytes 0xFF, else '!'..'~' minus 33 and exactly l_seq of them. With both CIGAR and SEQ, the
//    CIGAR query length (M/I/S/=/X) equals l_seq.
//  - bin = reg2bin(max(pos, 0), max(pos + max(reference length, 1), 1)).
//  - Optional fields TG:T:value, TG = [A-Za-z][A-Za-z0-9]. A: one char '!'..'~'. i: the smallest of c/s/i for a
//    negative value (down to -2^31), of C/S/I otherwise (up to 2^32 - 1). f: float32 from a decimal number; the
//    conversion is not correctly rounded in the last bit (no pass reads f values). Z, H: the value and a NUL.
//    B:[cCsSiIf](,v)*: subtype, count, values in the subtype's range.
#include "sam_kernels.hpp"

#include <hip/hip_runtime.h>

namespace secedo {
namespace bam {
namespace {

constexpr int kBlock = 256;

inline unsigned grid(uint64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

// '\n' bytes of a 32-bit word (exact zero-byte test of w ^ 0x0A0A0A0A)
__device__ __forceinline__ uint32_t newlines(uint32_t w) {
    const uint32_t t = w ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
    return __popc(z);
}

__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ bool is_alpha(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

// decimal integer over [a, b), '-' allowed when neg_ok; values beyond 2^40 saturate there (out of every range)
__device__ bool parse_int(const uint8_t *s, uint32_t a, uint32_t b, bool neg_ok, int64_t *v) {
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
__device__ bool parse_float(const uint8_t *s, uint32_t a, uint32_t b, float *f) {
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
    const double v = m == 0 ? 0.0 : m * pow(10.0, double(max(-400, min(400, e10))));
    *f = float(neg ? -v : v);
    return true;
}

// seq_nt16 code of a letter, either case
__device__ __forceinline__ uint32_t nt16(uint8_t c) {
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
__device__ __forceinline__ uint32_t seq_code(uint8_t c) { return c == '=' ? 0 : is_alpha(c) ? nt16(c) : 15; }

// RefID of a name: lower bound of its hash, exact compare over the run of equal hashes; -1 when absent
__device__ int32_t ref_id(const SamRefs &R, const uint8_t *p, uint32_t n) {
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
    __device__ void u8(uint32_t v) {
        if (W) o[n] = uint8_t(v);
        ++n;
    }
    __device__ void u16(uint32_t v) { u8(v), u8(v >> 8); }
    __device__ void u32(uint32_t v) { u8(v), u8(v >> 8), u8(v >> 16), u8(v >> 24); }
    __device__ void bytes(const uint8_t *p, uint32_t k) {
        if (W)
            for (uint32_t i = 0; i < k; ++i) o[n + i] = p[i];
        n += k;
    }
};

__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return uint32_t(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return uint32_t(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return uint32_t(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return uint32_t(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return uint32_t(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

__device__ __forceinline__ int op_index(uint8_t c) {
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
__device__ bool parse_aux(const uint8_t *s, uint32_t a, uint32_t b, Put<W> &out) {
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
            out.u32(__float_as_uint(f));
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
                    out.u32(__float_as_uint(f));
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
__device__ uint32_t parse_line(const uint8_t *s, uint32_t n, const SamRefs &R, uint8_t *out, LineInfo *li) {
    if (n == 0) return kSamEmpty;
    if (s[0] == '@') return kSamHeader;
    uint32_t fa[11], fb[11];
    uint32_t o = 0;
#pragma unroll
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

    Put<W> p{out};
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

__global__ void __launch_bounds__(kBlock) k_sam_newlines(const uint4 *text, uint64_t n16, uint32_t *cnt) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n16) return;
    const uint4 v = text[i];
    cnt[i] = newlines(v.x) + newlines(v.y) + newlines(v.z) + newlines(v.w);
}

__global__ void __launch_bounds__(kBlock) k_sam_starts(const uint4 *text, uint64_t n16, const uint32_t *scan,
                                                       uint32_t n_lines, uint32_t len, bool no_trailing,
                                                       uint32_t *start) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i == 0) {
        start[0] = 0;
        if (no_trailing) start[n_lines] = len + 1;
    }
    if (i >= n16) return;
    const uint4 v = text[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t k = scan[i];
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (((w[j / 4] >> (8 * (j % 4))) & 0xFF) == '\n') start[++k] = uint32_t(i * 16 + j + 1);
}

__global__ void __launch_bounds__(kBlock) k_sam_size(const uint8_t *text, const uint32_t *start, uint32_t n_lines,
                                                     uint64_t line_base, bool ends_file, SamRefs R, uint64_t *size,
                                                     int32_t *ref, int32_t *pos, unsigned long long *err) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_lines) return;
    const uint32_t b = start[k], n = start[k + 1] - 1 - b;
    LineInfo li{kSamNoRecord, 0, 0};
    uint32_t code = kSamOk;
    if (!(n == 0 && ends_file && k + 1 == n_lines)) code = parse_line<false>(text + b, n, R, nullptr, &li);
    if (code != kSamOk) {
        atomicMin(err, (unsigned long long)(line_base + k) << 8 | code);
        li = LineInfo{kSamNoRecord, 0, 0};
    }
    size[k] = li.ref >= 0 && R.sel[li.ref] ? li.bytes : 0;
    ref[k] = li.ref;
    pos[k] = li.pos;
}

__global__ void __launch_bounds__(kBlock) k_sam_encode(const uint8_t *text, const uint32_t *start, uint32_t n_lines,
                                                       SamRefs R, const uint64_t *off, uint8_t *out) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_lines || off[k + 1] == off[k]) return;
    const uint32_t b = start[k], n = start[k + 1] - 1 - b;
    LineInfo li;
    (void)parse_line<true>(text + b, n, R, out + off[k], &li);
}

}  // namespace

hipError_t sam_newline_count(const uint8_t *d_text, uint64_t n16, uint32_t *d_cnt, hipStream_t s) {
    if (n16 == 0) return hipSuccess;
    k_sam_newlines<<<grid(n16), kBlock, 0, s>>>(reinterpret_cast<const uint4 *>(d_text), n16, d_cnt);
    return hipGetLastError();
}

hipError_t sam_line_starts(const uint8_t *d_text, uint64_t n16, const uint32_t *d_scan, uint32_t n_lines,
                           uint32_t len, bool no_trailing_newline, uint32_t *d_start, hipStream_t s) {
    k_sam_starts<<<grid(n16 ? n16 : 1), kBlock, 0, s>>>(reinterpret_cast<const uint4 *>(d_text), n16, d_scan,
                                                        n_lines, len, no_trailing_newline, d_start);
    return hipGetLastError();
}

hipError_t sam_size(const uint8_t *d_text, const uint32_t *d_start, uint32_t n_lines, uint64_t line_base,
                    bool ends_file, const SamRefs &refs, uint64_t *d_size, int32_t *d_ref, int32_t *d_pos,
                    unsigned long long *d_err, hipStream_t s) {
    if (n_lines == 0) return hipSuccess;
    k_sam_size<<<grid(n_lines), kBlock, 0, s>>>(d_text, d_start, n_lines, line_base, ends_file, refs, d_size, d_ref,
                                                d_pos, d_err);
    return hipGetLastError();
}

hipError_t sam_encode(const uint8_t *d_text, const uint32_t *d_start, uint32_t n_lines, const SamRefs &refs,
                      const uint64_t *d_off, uint8_t *d_out, hipStream_t s) {
    if (n_lines == 0) return hipSuccess;
    k_sam_encode<<<grid(n_lines), kBlock, 0, s>>>(d_text, d_start, n_lines, refs, d_off, d_out);
    return hipGetLastError();
}

}  // namespace bam
}  // namespace secedo
