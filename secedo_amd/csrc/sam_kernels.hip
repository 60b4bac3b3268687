// sam_kernels.hip -- SAM text -> BAM records on gfx950, so that SAM input goes through bam_kernels.hip unchanged.
//
// The host cuts a file's alignment lines into ranges that end at a '\n' and uploads each one. Passes per range:
//   sam_newline_count (one thread per 16-byte vector: '\n' bytes, SWAR) -> exclusive scan -> sam_line_starts (the
//   byte after each '\n') -> sam_size (one thread per line: tokenise, validate, RefID, POS, record size) ->
//   exclusive scan of the sizes -> sam_encode (one thread per selected line: the BAM record at its scanned offset).
// Errors: the size pass takes the u64 min of (line << 8 | code), so the first bad line is reported whatever the
// thread order. Both passes run the same parser (parse_line<W> of sam_parse.hpp, host/device code that
// tests/cpp/sam_parse_test.cpp also runs on the host), counting or writing, so the sizes and the written records agree
// byte for byte. Plain C++ stores only.
//
// Conversion (htslib's sam_parse1, departures marked):
//  - 11 tab-separated mandatory fields, then optional fields. An '@' line is an error here (the header comes first),
//    so is an empty line unless it is the last line of the file. '\r' is an ordinary character.
//  - QNAME at most 254 characters, stored with its NUL. FLAG [0, 65535], POS and PNEXT [0, 2^31 - 1] stored minus
//    one, MAPQ [0, 255], TLEN [-(2^31 - 1), 2^31 - 1]: decimal integers ('-' only for TLEN).
//  - RNAME '*' -> -1, else the @SQ index found by hash (FNV-1a), lower bound in the sorted hashes and exact compare.
//    RNEXT '=' -> the record's RefID. A name missing from @SQ is an error (htslib warns and treats it as unmapped).
//  - CIGAR '*' -> no ops, else <len><op> with op in MIDNSHP=X and len in [1, 2^28); more than 65535 ops is a limit.
//  - SEQ '*' -> l_seq 0, else seq_nt16 codes (=ACMGRSVTWYHKDBN -> 0..15, case-insensitive, anything else 15; htslib
//    reads the digits 0..3 as A, C, G, T).
//    QUAL '*' -> l_seq bytes 0xFF, else '!'..'~' minus 33 and exactly l_seq of them. With both CIGAR and SEQ, the
//    CIGAR query length (M/I/S/=/X) equals l_seq.
//  - bin = reg2bin(max(pos, 0), max(pos + max(reference length, 1), 1)).
//  - Optional fields TG:T:value, TG = [A-Za-z][A-Za-z0-9]. A: one char '!'..'~'. i: the smallest of c/s/i for a
//    negative value (down to -2^31), of C/S/I otherwise (up to 2^32 - 1). f: float32 from a decimal number through
//    double, not correctly rounded in the last bit for every text (the pileup reads no f value; the per-cluster BAM
//    writer copies them, and tests/sam_cases.py pins texts of up to 9 digits, ties included). Z, H: the value and a
//    NUL.
//    B:[cCsSiIf](,v)*: subtype, count, values in the subtype's range.
#include "sam_kernels.hpp"

#include <hip/hip_runtime.h>

namespace secedo {
namespace bam {
namespace {

constexpr int kBlock = 256;

inline unsigned grid(uint64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

__global__ void __launch_bounds__(kBlock) k_sam_newlines(const uint4 *text, uint64_t n16, uint32_t *cnt) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n16) return;
    const uint4 v = text[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    cnt[i] = vector_newlines(w);
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
    vector_starts(w, i, scan[i], start);
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
