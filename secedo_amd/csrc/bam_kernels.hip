// bam_kernels.hip -- the device passes of the reference's pileup_bams() (pileup.cpp:49-348) for gfx950.
//
// Restated semantics (the reference run with num_threads = 1, the deterministic one):
//  1. Record selection: a file contributes the records whose RefID equals chromosome_id (the @SQ index) and
//     stops at the first later record with another RefID; input must be coordinate-sorted (the host returns
//     SECEDO_E_INVALID_ARG when (RefID, Position) decreases, RefID -1 sorting last).
//  2. Read ids: records are numbered by the first appearance of their name in the global order (chunk of
//     Position, file, record), chunks of 1,000,000 positions. The name maps are per batch slot
//     (file % 100, MAX_OPEN_FILES): files 0 and 100 share one. Every selected record takes an id before its
//     base loop, filtered or not.
//  3. Cell id = global file index, cell_base = cell << 2 | base (the host refuses more than 16384 files).
//  3b. Tag mode (secedo_pileup_bams_cells): the cell is the index of the record's barcode in the list, the barcode
//     being the value of the first aux field named by the tag (FindTag) when it is Z-typed. A record without the
//     tag, with a tag of another type or with an unlisted value is not selected: it takes no read id, is not
//     checked against rule 6 and gives nothing. The global order of rules 2 and 8 becomes (chunk of Position,
//     cell, Position, input file, record), which is per-file mode on the per-cell split files; the name maps are
//     per slot cell % 100. The host's structural checks (sortedness, CIGAR against SEQ, negative position) still
//     cover every record of the chromosome. At most 16384 barcodes.
//  4. Base walk (:94-155) over BamTools' AlignedBases (BuildCharData): M/I/=/X copy the bases, D gives '-',
//     N gives 'N', P gives '*', S/H give nothing. Only leading H/S ops are skipped; I advances `offset`; an I
//     as the last op ends the read; the quality index is i + offset - del_offset (a leading soft clip is not
//     counted, kept); CharToInt maps U to 3 and '-'/'N'/'*' to 5, and a 5 is skipped; a base is skipped when
//     (uint32_t)(quality_char - 33) < min_base_quality on the signed char, so a missing quality string (0xFF)
//     and qualities above 94 pass; P advances the position like D; SEQ '*' gives no bases but takes an id.
//  5. Read filters, checked per base, acting per read: MapQuality < min_map_quality, or the AS score below
//     min_alignment_score. The score is GetTag("AS", uint32_t&) from 0: only types A/C/S/I are read (1, 1, 2,
//     4 bytes), a signed c/s/i tag leaves 0.
//  6. The reference's asserts abort on some inputs (its Release flags keep them); here they are errors naming
//     the record: a record not paired / not a proper pair / failed QC; a base that passed the filters landing
//     >= 1000 past its chunk's end; the walk running past the CIGAR; a D op over a non-'-' character. A
//     quality index past the quality string (undefined in the reference) is an error too.
//  7. Loci: per position, coverage = the kept bases as the reference's atomic<uint16_t> (wraps at 2^16); kept
//     iff 2 <= coverage < max_coverage and coverage - max(base counts) >= min_different, the counts taken over
//     the stored entries. Written 1-based. Positions at or past the end of the last chunk that holds a record
//     are never written (the reference's loop ends there).
//  8. Entry order in a locus: (chunk of the record's Position, file, record) = the global ordinal; one record
//     gives at most one base per position. When the counter wrapped, the stored entries are the last
//     (arrivals mod 2^16) arrivals: slots 0..c-1 were overwritten by the last cycle.
//
// Tag mode first runs the front passes: cells (one thread per uploaded record, input order: FindTag walk, hash of the
// value, lower bound in the hash-sorted list, exact byte compare over the run of equal hashes) -> compaction of the
// selected records (scan) -> stable hipcub sort by chunk << 46 | cell << 32 | Position with the input ordinal as
// value -> order (byte offset, cell and input ordinal per global ordinal), which is the Records the chain below
// takes. The barcode census (secedo_bam_barcodes) hashes every Z-typed value, sorts, and splits each run of equal
// hashes by exact compare into distinct values with their record counts.
//
// Passes: decode (one thread per record) -> hipcub sort by (slot-name hash, ordinal) -> first_occurrence with
// an exact byte compare inside each run of equal hashes -> exclusive scan of first-occurrence flags = ids.
// Then per window of kWindow positions: count (CIGAR walk, u32 atomics on 4 base counts per position) ->
// select + scans -> emit (kept bases of candidate loci with key locus << 32 | ordinal) -> sort -> finalize +
// scans -> gather. Atomics only count or claim slots; every output position comes from a scan or a sort on
// unique keys, so two runs are bit-identical. Plain C++ stores only.
#include "bam_kernels.hpp"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

namespace secedo {
namespace bam {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}
__device__ __forceinline__ uint16_t ld16(const uint8_t *p) { return uint16_t(p[0] | p[1] << 8); }

// one BAM record (after its block_size field)
struct Rec {
    const uint8_t *core;
    int32_t pos;
    uint32_t l_name, mapq, n_cigar, flag, l_seq, l_aux;
    const uint8_t *name, *cigar, *seq, *qual, *aux;
};

__device__ __forceinline__ Rec parse(const uint8_t *rec) {
    Rec r;
    const uint32_t block_size = ld32(rec);
    r.core = rec + 4;
    r.pos = int32_t(ld32(r.core + 4));
    r.l_name = r.core[8];
    r.mapq = r.core[9];
    r.n_cigar = ld16(r.core + 12);
    r.flag = ld16(r.core + 14);
    r.l_seq = ld32(r.core + 16);
    r.name = r.core + 32;
    r.cigar = r.name + r.l_name;
    r.seq = r.cigar + 4 * r.n_cigar;
    r.qual = r.seq + (r.l_seq + 1) / 2;
    r.aux = r.qual + r.l_seq;
    r.l_aux = block_size - uint32_t(r.aux - r.core);
    return r;
}

// BAM op codes MIDNSHP=X
constexpr uint32_t kOpM = 0, kOpI = 1, kOpD = 2, kOpN = 3, kOpS = 4, kOpH = 5, kOpP = 6, kOpEq = 7, kOpX = 8;

__device__ __forceinline__ uint32_t op_type(const Rec &r, uint32_t i) { return ld32(r.cigar + 4 * i) & 15; }
__device__ __forceinline__ uint32_t op_len(const Rec &r, uint32_t i) { return ld32(r.cigar + 4 * i) >> 4; }
__device__ __forceinline__ bool copies_bases(uint32_t t) { return t == kOpM || t == kOpI || t == kOpEq || t == kOpX; }
__device__ __forceinline__ bool writes_char(uint32_t t) { return copies_bases(t) || t == kOpD || t == kOpN || t == kOpP; }

// BamAlignment::FindTag / SkipToNextTag: the first aux field named t0 t1. Returns its value (null when absent or
// when the walk gives up on an unknown storage type), *type its storage type, *avail the aux bytes from the value on.
__device__ const uint8_t *find_tag(const Rec &r, uint8_t t0, uint8_t t1, uint8_t *type, uint32_t *avail) {
    const uint8_t *p = r.aux;
    const uint32_t len = r.l_aux;
    uint32_t parsed = 0;
    while (parsed < len) {
        if (parsed + 3 > len) return nullptr;
        const uint8_t a = p[0], b = p[1], ty = p[2];
        p += 3;
        parsed += 3;
        if (a == t0 && b == t1) {
            *type = ty;
            *avail = len - parsed;
            return p;
        }
        uint32_t skip;
        switch (ty) {
            case 'A': case 'c': case 'C': skip = 1; break;
            case 's': case 'S': skip = 2; break;
            case 'f': case 'i': case 'I': skip = 4; break;
            case 'Z': case 'H': {
                skip = 0;
                while (parsed + skip < len && p[skip]) ++skip;
                ++skip;
                break;
            }
            case 'B': {
                if (parsed + 5 > len) return nullptr;
                const uint8_t at = p[0];
                const uint32_t cnt = ld32(p + 1);
                uint32_t es = 0;
                if (at == 'c' || at == 'C') es = 1;
                else if (at == 's' || at == 'S') es = 2;
                else if (at == 'i' || at == 'I' || at == 'f') es = 4;
                else return nullptr;
                skip = 5 + cnt * es;
                break;
            }
            default: return nullptr;  // unknown storage type: FindTag gives up
        }
        if (parsed + skip >= len) return nullptr;  // the next tag would start at the terminating NUL
        p += skip;
        parsed += skip;
        if (*p == 0) return nullptr;
    }
    return nullptr;
}

// GetTag("AS", uint32_t&) from 0 (TagTypeHelper<uint32_t>: only A/C/S/I are read)
__device__ uint32_t alignment_score(const Rec &r) {
    uint8_t type = 0;
    uint32_t avail = 0;
    const uint8_t *p = find_tag(r, 'A', 'S', &type, &avail);
    if (!p) return 0;
    uint32_t n = 0;
    if (type == 'A' || type == 'C') n = 1;
    else if (type == 'S') n = 2;
    else if (type == 'I') n = 4;
    if (n == 0 || n > avail) return 0;
    uint32_t v = 0;
    for (uint32_t k = 0; k < n; ++k) v |= uint32_t(p[k]) << (8 * k);
    return v;
}

// The Z-typed value of tag t0 t1 (its bytes up to the NUL or the record's end), or null when the record has no such
// tag or it is not Z-typed (rule 3b).
__device__ const uint8_t *tag_value(const Rec &r, uint8_t t0, uint8_t t1, uint32_t *len) {
    uint8_t type = 0;
    uint32_t avail = 0;
    const uint8_t *p = find_tag(r, t0, t1, &type, &avail);
    if (!p || type != 'Z') return nullptr;
    uint32_t k = 0;
    while (k < avail && p[k]) ++k;
    *len = k;
    return p;
}

__device__ __forceinline__ uint64_t value_hash(const uint8_t *v, uint32_t len) {
    uint64_t h = 1469598103934665603ull;
    for (uint32_t k = 0; k < len; ++k) {
        h ^= v[k];
        h *= 1099511628211ull;
    }
    h ^= uint64_t(len) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}

__device__ __forceinline__ bool same_bytes(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) {
    if (la != lb) return false;
    for (uint32_t k = 0; k < la; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

// CharToInt of a 4-bit SEQ code ("=ACMGRSVTWYHKDBN"): A 0, C 1, G 2, T 3, else 5
__device__ __forceinline__ uint32_t seq_code(const Rec &r, uint32_t k) {
    const uint32_t c = (r.seq[k >> 1] >> (4 * (1 - (k & 1)))) & 15;
    return c == 1 ? 0 : c == 2 ? 1 : c == 4 ? 2 : c == 8 ? 3 : 5;
}

// Cursor over AlignedBases without materialising it; the current op is cached in registers, so a base costs one
// SEQ byte unless it crosses into the next op.
struct Aligned {
    uint32_t op = 0, t = 0, start = 0, end = 0, qk = 0;  // char-writing op, type, its AlignedBases range, query index
    __device__ void first(const Rec &r) {
        t = op_type(r, 0);
        end = writes_char(t) ? op_len(r, 0) : 0;
    }
    __device__ void seek(const Rec &r, uint32_t k) {
        while (k >= end) {
            if (copies_bases(t) || t == kOpS) qk += op_len(r, op);
            start = end;
            ++op;
            t = op_type(r, op);
            end = start + (writes_char(t) ? op_len(r, op) : 0);
        }
    }
    // code of AlignedBases[k] (CharToInt) and whether it is a '-'
    __device__ uint32_t code(const Rec &r, uint32_t k, bool *dash) {
        seek(r, k);
        *dash = t == kOpD;
        if (copies_bases(t)) return seq_code(r, qk + (k - start));
        return 5;
    }
};

// The reference's loop (:93-161) over one record. on_base(position, base) for every base that passes the
// base and read filters; returns an Err. *last = one past the largest position the walk reached.
template <class F>
__device__ uint32_t walk(const Rec &r, const Params &p, bool read_pass, uint32_t end_pos, uint32_t *last, F on_base) {
    *last = uint32_t(r.pos);
    if (r.l_seq == 0 || r.n_cigar == 0) return kErrNone;
    uint32_t size = 0;
    for (uint32_t c = 0; c < r.n_cigar; ++c)
        if (writes_char(op_type(r, c))) size += op_len(r, c);
    if (size == 0) return kErrNone;
    const bool no_qual = r.qual[0] == 0xFF;
    uint32_t ci = 0;
    while (op_type(r, ci) == kOpH || op_type(r, ci) == kOpS) ++ci;
    uint32_t ct = op_type(r, ci);  // type of op ci
    uint32_t cigar_end = op_len(r, ci), offset = 0, del_offset = 0;
    Aligned ab;
    ab.first(r);
    for (uint32_t i = 0; i + offset < size; ++i) {
        while (i >= cigar_end) {
            ++ci;
            if (ci >= r.n_cigar) return kErrCigarEnd;
            ct = op_type(r, ci);
            if (ct == kOpI) {
                offset += op_len(r, ci);
                if (i + offset >= size) break;
                continue;
            } else if (ct == kOpD) {
                del_offset += op_len(r, ci);
            }
            cigar_end += op_len(r, ci);
        }
        if (i + offset >= size) {
            if (ci != r.n_cigar - 1) return kErrCigarEnd;
            break;
        }
        const uint32_t k = i + offset;
        bool dash;
        const uint32_t base = ab.code(r, k, &dash);
        if (ct == kOpD && !dash) return kErrDeletion;
        *last = uint32_t(r.pos) + i + 1;
        if (base == 5) continue;
        const uint32_t qi = k - del_offset;
        if (qi >= r.l_seq) return kErrQuality;
        const int qc = no_qual ? -1 : int(int8_t(uint8_t(r.qual[qi] + 33)));
        if (uint32_t(qc) - 33u < p.min_base_quality) continue;
        if (!read_pass) continue;
        if (uint32_t(r.pos) + i >= end_pos + kMaxInsert) return kErrInsert;
        on_base(uint32_t(r.pos) + i, base);
    }
    return kErrNone;
}

__device__ __forceinline__ uint32_t end_of_chunk(int32_t pos) { return (uint32_t(pos) / kChunk + 1) * kChunk; }

__device__ __forceinline__ uint64_t name_key(const Rec &r, uint32_t slot) {
    uint64_t h = 1469598103934665603ull ^ (uint64_t(slot) * 0x9E3779B97F4A7C15ull);
    for (uint32_t k = 0; k < r.l_name && r.name[k]; ++k) {
        h ^= r.name[k];
        h *= 1099511628211ull;
    }
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}

__global__ void __launch_bounds__(kBlock) k_decode(Records rs, Params p, uint64_t *key, uint32_t *val, uint8_t *pass,
                                                   uint32_t *span_end, unsigned long long *err) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= rs.n) return;
    const Rec r = parse(rs.bytes + rs.off[o]);
    const uint32_t file = rs.file[o];
    key[o] = name_key(r, file % kSlots);
    val[o] = o;
    uint32_t e = kErrNone, last = 0;
    bool ok = false;
    if (r.pos < 0) {
        e = kErrPosition;
    } else if (!(r.flag & 0x1) || !(r.flag & 0x2) || (r.flag & 0x200)) {
        e = kErrFlags;
    } else {
        ok = r.mapq >= p.min_map_quality && alignment_score(r) >= p.min_alignment_score;
        e = walk(r, p, ok, end_of_chunk(r.pos), &last, [](uint32_t, uint32_t) {});
    }
    pass[o] = ok ? 1 : 0;
    span_end[o] = last;
    if (e != kErrNone) atomicMin(err, (unsigned long long)o << 8 | e);
}

__global__ void __launch_bounds__(kBlock) k_run_head(const uint64_t *key, uint32_t *head, uint32_t n) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    head[j] = (j == 0 || key[j] != key[j - 1]) ? j : 0;
}

__device__ bool same_name(const Records &rs, uint32_t a, uint32_t b) {
    if (rs.file[a] % kSlots != rs.file[b] % kSlots) return false;
    const Rec x = parse(rs.bytes + rs.off[a]), y = parse(rs.bytes + rs.off[b]);
    for (uint32_t k = 0;; ++k) {
        const uint8_t cx = k < x.l_name ? x.name[k] : 0, cy = k < y.l_name ? y.name[k] : 0;
        if (cx != cy) return false;
        if (cx == 0) return true;
    }
}

__global__ void __launch_bounds__(kBlock) k_first(Records rs, const uint32_t *val, const uint32_t *run,
                                                  uint32_t *rep, uint32_t *flag) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= rs.n) return;
    const uint32_t o = val[j];
    uint32_t first = o;
    for (uint32_t q = run[j]; q < j; ++q)  // equal keys are in ordinal order (stable sort)
        if (same_name(rs, val[q], o)) {
            first = val[q];
            break;
        }
    rep[o] = first;
    flag[o] = first == o ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_ids(const uint32_t *rep, const uint32_t *scan, uint32_t *id, uint32_t n) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o < n) id[o] = scan[rep[o]];
}

__global__ void __launch_bounds__(kBlock) k_count(Records rs, Params p, const uint8_t *pass, const uint32_t *span_end,
                                                  uint32_t w0, uint32_t w1, uint32_t *cnt) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= rs.n || !pass[o]) return;
    const Rec r = parse(rs.bytes + rs.off[o]);
    if (span_end[o] <= w0 || uint32_t(r.pos) >= w1) return;
    uint32_t last;
    walk(r, p, true, end_of_chunk(r.pos), &last, [&](uint32_t pos, uint32_t base) {
        if (pos >= w0 && pos < w1) atomicAdd(&cnt[uint64_t(pos - w0) * 4 + base], 1u);
    });
}

__global__ void __launch_bounds__(kBlock) k_select(const uint4 *cnt, Params p, uint32_t n_pos, uint32_t *cand,
                                                   uint64_t *arr) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pos) return;
    const uint4 c = cnt[i];
    const uint32_t total = c.x + c.y + c.z + c.w;
    const uint32_t cov = total & 0xFFFF;
    const uint32_t mx = max(max(c.x, c.y), max(c.z, c.w));
    const bool wrapped = total >= 65536;
    const bool ok = cov >= 2 && cov < p.max_coverage && (wrapped || int32_t(cov) - int32_t(mx) >= p.min_different);
    cand[i] = ok ? 1 : 0;
    arr[i] = ok ? total : 0;
}

__global__ void __launch_bounds__(kBlock) k_compact(const uint4 *cnt, const uint32_t *cand, const uint32_t *cscan,
                                                    const uint64_t *ascan, uint32_t w0, uint32_t n_pos, uint32_t *cpos,
                                                    uint64_t *carr, uint32_t *ctot) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pos || !cand[i]) return;
    const uint4 c = cnt[i];
    const uint32_t l = cscan[i];
    cpos[l] = w0 + i + 1;
    carr[l] = ascan[i];
    ctot[l] = c.x + c.y + c.z + c.w;
}

__global__ void __launch_bounds__(kBlock) k_emit(Records rs, Params p, const uint8_t *pass, const uint32_t *span_end,
                                                 const uint32_t *id, uint32_t w0, uint32_t w1, const uint32_t *cand,
                                                 const uint32_t *cscan, const uint64_t *ascan, uint32_t *fill,
                                                 uint64_t *key, uint64_t *val) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= rs.n || !pass[o]) return;
    const Rec r = parse(rs.bytes + rs.off[o]);
    if (span_end[o] <= w0 || uint32_t(r.pos) >= w1) return;
    const uint64_t payload = uint64_t(id[o]) << 16 | uint64_t(rs.file[o]) << 2;
    uint32_t last;
    walk(r, p, true, end_of_chunk(r.pos), &last, [&](uint32_t pos, uint32_t base) {
        if (pos < w0 || pos >= w1) return;
        const uint32_t i = pos - w0;
        if (!cand[i]) return;
        const uint32_t l = cscan[i];
        const uint64_t at = ascan[i] + atomicAdd(&fill[l], 1u);  // a slot only; the sort fixes the order
        key[at] = uint64_t(l) << 32 | o;
        val[at] = payload | base;
    });
}

__global__ void __launch_bounds__(kBlock) k_finalize(const uint64_t *val, const uint64_t *carr, const uint32_t *ctot,
                                                     Params p, uint32_t n_cand, uint32_t *keep, uint64_t *kept) {
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= n_cand) return;
    const uint32_t total = ctot[l], cov = total & 0xFFFF;
    bool ok = true;
    if (total >= 65536) {  // the stored entries are the last cycle of the u16 counter
        uint32_t nb[4] = {0, 0, 0, 0};
        const uint64_t beg = carr[l] + total - cov;
        for (uint32_t k = 0; k < cov; ++k) ++nb[val[beg + k] & 3];
        const uint32_t mx = max(max(nb[0], nb[1]), max(nb[2], nb[3]));
        ok = int32_t(cov) - int32_t(mx) >= p.min_different;
    }
    keep[l] = ok ? 1 : 0;
    kept[l] = ok ? cov : 0;
}

__global__ void __launch_bounds__(kBlock) k_gather(const uint64_t *val, const uint32_t *cpos, const uint64_t *carr,
                                                   const uint32_t *ctot, const uint32_t *keep, const uint32_t *kscan,
                                                   const uint64_t *escan, uint32_t n_cand, const uint16_t *i2g,
                                                   uint32_t n_ids, uint32_t *opos, uint64_t *ooff, uint32_t *orid,
                                                   uint16_t *oidb, uint64_t entry_base, uint32_t *bad) {
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= n_cand || !keep[l]) return;
    const uint32_t total = ctot[l], cov = total & 0xFFFF;
    const uint32_t at = kscan[l];
    const uint64_t e0 = escan[l];
    opos[at] = cpos[l];
    ooff[at + 1] = entry_base + e0 + cov;
    const uint64_t beg = carr[l] + total - cov;
    uint32_t max_cell = 0;
    for (uint32_t k = 0; k < cov; ++k) {
        const uint64_t v = val[beg + k];
        const uint32_t cell = uint32_t(v >> 2) & 0x3FFF, base = uint32_t(v) & 3;
        max_cell = max(max_cell, cell);
        uint32_t g = cell;
        if (i2g) {
            if (cell >= n_ids) {
                *bad = 1;
                g = 0;
            } else {
                g = i2g[cell];
            }
        }
        orid[e0 + k] = uint32_t(v >> 16);
        oidb[e0 + k] = uint16_t(g << 2 | base);
    }
    atomicMax(&bad[1], max_cell);
}

__global__ void __launch_bounds__(kBlock) k_stats(const uint32_t *pos, const uint64_t *off, const uint32_t *rid,
                                                  uint32_t n_loci, uint32_t *minpos, uint32_t *maxpos,
                                                  uint32_t n_ids) {
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= n_loci) return;
    for (uint64_t e = off[l]; e < off[l + 1]; ++e) {
        const uint32_t id = rid[e];
        if (id < n_ids) {
            atomicMin(&minpos[id], pos[l]);
            atomicMax(&maxpos[id], pos[l]);
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_span(const uint32_t *minpos, const uint32_t *maxpos, uint32_t n_ids,
                                                 uint32_t *max_len) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= n_ids || minpos[id] > maxpos[id]) return;
    atomicMax(max_len, maxpos[id] - minpos[id]);
}

// --- tag mode (rule 3b): the cell of a record from its barcode tag, and the global order built on the device ---

// a listed barcode's hash and index, to be sorted by hash
__global__ void __launch_bounds__(kBlock) k_list_hash(const uint8_t *bytes, const uint32_t *off, uint32_t n,
                                                      uint64_t *hash, uint32_t *idx) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= n) return;
    hash[c] = value_hash(bytes + off[c], off[c + 1] - off[c]);
    idx[c] = c;
}

// the listed cell of a barcode value, or ~0: lower bound in the hash-sorted table, then an exact compare over the run
// of equal hashes, so a collision never merges two cells
__device__ uint32_t find_cell(const CellList &L, const uint8_t *v, uint32_t len) {
    const uint64_t h = value_hash(v, len);
    uint32_t lo = 0, hi = L.n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (L.hash[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    for (uint32_t k = lo; k < L.n && L.hash[k] == h; ++k) {
        const uint32_t c = L.cell[k];
        if (same_bytes(v, len, L.bytes + L.off[c], L.off[c + 1] - L.off[c])) return c;
    }
    return ~0u;
}

// one thread per uploaded record (input order): sel = 1 and key = chunk << 46 | cell << 32 | Position for a record
// of a listed cell
__global__ void __launch_bounds__(kBlock) k_cells(const uint8_t *bytes, const uint64_t *in_off, uint32_t n,
                                                  CellList L, uint64_t *key, uint32_t *sel) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= n) return;
    const Rec r = parse(bytes + in_off[o]);
    uint32_t len = 0, cell = ~0u;
    const uint8_t *v = tag_value(r, L.t0, L.t1, &len);
    if (v) cell = find_cell(L, v, len);
    const uint32_t pos = uint32_t(r.pos);  // >= 0: the host refuses negative positions
    key[o] = cell == ~0u ? 0 : (uint64_t(pos / kChunk) << 46 | uint64_t(cell) << 32 | pos);
    sel[o] = cell == ~0u ? 0 : 1;
}

// one thread per record with a Z-typed tag value: sel = 1, key = the value's hash
__global__ void __launch_bounds__(kBlock) k_tag_keys(const uint8_t *bytes, const uint64_t *in_off, uint32_t n,
                                                     uint8_t t0, uint8_t t1, uint64_t *key, uint32_t *sel) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= n) return;
    const Rec r = parse(bytes + in_off[o]);
    uint32_t len = 0;
    const uint8_t *v = tag_value(r, t0, t1, &len);
    key[o] = v ? value_hash(v, len) : 0;
    sel[o] = v ? 1 : 0;
}

// the selected (key, input ordinal) pairs, in input order
__global__ void __launch_bounds__(kBlock) k_compact_keys(const uint64_t *key, const uint32_t *sel,
                                                         const uint32_t *scan, uint32_t n, uint64_t *key_out,
                                                         uint32_t *val_out) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= n || !sel[o]) return;
    key_out[scan[o]] = key[o];
    val_out[scan[o]] = o;
}

// the Records of the global order: byte offset, cell and input ordinal of ordinal j
__global__ void __launch_bounds__(kBlock) k_order(const uint64_t *key, const uint32_t *val, const uint64_t *in_off,
                                                  uint32_t n, uint64_t *off, uint16_t *cell, uint32_t *ord) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t o = val[j];
    off[j] = in_off[o];
    cell[j] = uint16_t((key[j] >> 32) & 0x3FFF);
    ord[j] = o;
}

// distinct values: within a run of equal hashes (sorted, input order inside) the first position holding the same
// value counts the record
__global__ void __launch_bounds__(kBlock) k_tag_count(const uint8_t *bytes, const uint64_t *in_off, uint8_t t0,
                                                      uint8_t t1, const uint32_t *val, const uint32_t *run, uint32_t n,
                                                      uint32_t *cnt) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    uint32_t len = 0;
    const uint8_t *v = tag_value(parse(bytes + in_off[val[j]]), t0, t1, &len);
    uint32_t first = j;
    for (uint32_t q = run[j]; q < j; ++q) {
        uint32_t lq = 0;
        const uint8_t *w = tag_value(parse(bytes + in_off[val[q]]), t0, t1, &lq);
        if (same_bytes(v, len, w, lq)) {
            first = q;
            break;
        }
    }
    atomicAdd(&cnt[first], 1u);
}

inline uint32_t grid(uint64_t n) { return uint32_t((n + kBlock - 1) / kBlock); }

struct MaxOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};

}  // namespace

hipError_t decode(const Records &r, const Params &p, uint64_t *d_key, uint32_t *d_val, uint8_t *d_pass,
                  uint32_t *d_span_end, unsigned long long *d_err, hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_decode<<<grid(r.n), kBlock, 0, s>>>(r, p, d_key, d_val, d_pass, d_span_end, d_err);
    return hipGetLastError();
}

hipError_t first_occurrence(const Records &r, const uint64_t *d_key_sorted, const uint32_t *d_val_sorted,
                            uint32_t *d_run, uint32_t *d_rep, uint32_t *d_flag, void *tmp, size_t tmp_bytes,
                            hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_run_head<<<grid(r.n), kBlock, 0, s>>>(d_key_sorted, d_run, r.n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, d_run, d_run, MaxOp(), r.n, s);
    if (e != hipSuccess) return e;
    k_first<<<grid(r.n), kBlock, 0, s>>>(r, d_val_sorted, d_run, d_rep, d_flag);
    return hipGetLastError();
}

hipError_t assign_ids(const uint32_t *d_rep, const uint32_t *d_scan, uint32_t *d_id, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_ids<<<grid(n), kBlock, 0, s>>>(d_rep, d_scan, d_id, n);
    return hipGetLastError();
}

hipError_t count(const Records &r, const Params &p, const uint8_t *d_pass, const uint32_t *d_span_end, uint32_t w0,
                 uint32_t w1, uint32_t *d_cnt, hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_count<<<grid(r.n), kBlock, 0, s>>>(r, p, d_pass, d_span_end, w0, w1, d_cnt);
    return hipGetLastError();
}

hipError_t select(const uint32_t *d_cnt, const Params &p, uint32_t n_pos, uint32_t *d_cand, uint64_t *d_arr,
                  hipStream_t s) {
    k_select<<<grid(n_pos), kBlock, 0, s>>>(reinterpret_cast<const uint4 *>(d_cnt), p, n_pos, d_cand, d_arr);
    return hipGetLastError();
}

hipError_t compact_candidates(const uint32_t *d_cnt, const uint32_t *d_cand, const uint32_t *d_cand_scan,
                              const uint64_t *d_arr_scan, uint32_t w0, uint32_t n_pos, uint32_t *d_cpos,
                              uint64_t *d_carr, uint32_t *d_ctot, hipStream_t s) {
    k_compact<<<grid(n_pos), kBlock, 0, s>>>(reinterpret_cast<const uint4 *>(d_cnt), d_cand, d_cand_scan,
                                             d_arr_scan, w0, n_pos, d_cpos, d_carr, d_ctot);
    return hipGetLastError();
}

hipError_t emit(const Records &r, const Params &p, const uint8_t *d_pass, const uint32_t *d_span_end,
                const uint32_t *d_id, uint32_t w0, uint32_t w1, const uint32_t *d_cand, const uint32_t *d_cand_scan,
                const uint64_t *d_arr_scan, uint32_t *d_fill, uint64_t *d_key, uint64_t *d_val, hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_emit<<<grid(r.n), kBlock, 0, s>>>(r, p, d_pass, d_span_end, d_id, w0, w1, d_cand, d_cand_scan, d_arr_scan,
                                        d_fill, d_key, d_val);
    return hipGetLastError();
}

hipError_t finalize(const uint64_t *d_val_sorted, const uint64_t *d_carr, const uint32_t *d_ctot, const Params &p,
                    uint32_t n_cand, uint32_t *d_keep, uint64_t *d_kept_entries, hipStream_t s) {
    if (n_cand == 0) return hipSuccess;
    k_finalize<<<grid(n_cand), kBlock, 0, s>>>(d_val_sorted, d_carr, d_ctot, p, n_cand, d_keep, d_kept_entries);
    return hipGetLastError();
}

hipError_t gather(const uint64_t *d_val_sorted, const uint32_t *d_cpos, const uint64_t *d_carr,
                  const uint32_t *d_ctot, const uint32_t *d_keep, const uint32_t *d_keep_scan,
                  const uint64_t *d_entry_scan, uint32_t n_cand, const uint16_t *d_id_to_group, uint32_t n_ids,
                  uint32_t *d_out_pos, uint64_t *d_out_off, uint32_t *d_out_rid, uint16_t *d_out_idb,
                  uint64_t entry_base, uint32_t *d_flags, hipStream_t s) {
    if (n_cand == 0) return hipSuccess;
    k_gather<<<grid(n_cand), kBlock, 0, s>>>(d_val_sorted, d_cpos, d_carr, d_ctot, d_keep, d_keep_scan,
                                             d_entry_scan, n_cand, d_id_to_group, n_ids, d_out_pos, d_out_off,
                                             d_out_rid, d_out_idb, entry_base, d_flags);
    return hipGetLastError();
}

hipError_t read_stats(const uint32_t *d_pos, const uint64_t *d_off, const uint32_t *d_rid, uint32_t n_loci,
                      uint32_t *d_minpos, uint32_t *d_maxpos, uint32_t n_ids, uint32_t *d_max_len, hipStream_t s) {
    if (n_loci) k_stats<<<grid(n_loci), kBlock, 0, s>>>(d_pos, d_off, d_rid, n_loci, d_minpos, d_maxpos, n_ids);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_ids == 0) return e;
    k_span<<<grid(n_ids), kBlock, 0, s>>>(d_minpos, d_maxpos, n_ids, d_max_len);
    return hipGetLastError();
}

hipError_t list_hash(const uint8_t *d_bytes, const uint32_t *d_off, uint32_t n, uint64_t *d_hash, uint32_t *d_idx,
                     hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_list_hash<<<grid(n), kBlock, 0, s>>>(d_bytes, d_off, n, d_hash, d_idx);
    return hipGetLastError();
}

hipError_t cells(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, const CellList &L, uint64_t *d_key,
                 uint32_t *d_sel, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_cells<<<grid(n), kBlock, 0, s>>>(d_bytes, d_in_off, n, L, d_key, d_sel);
    return hipGetLastError();
}

hipError_t tag_keys(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, uint8_t t0, uint8_t t1,
                    uint64_t *d_key, uint32_t *d_sel, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_tag_keys<<<grid(n), kBlock, 0, s>>>(d_bytes, d_in_off, n, t0, t1, d_key, d_sel);
    return hipGetLastError();
}

hipError_t compact_keys(const uint64_t *d_key, const uint32_t *d_sel, const uint32_t *d_scan, uint32_t n,
                        uint64_t *d_key_out, uint32_t *d_val_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_compact_keys<<<grid(n), kBlock, 0, s>>>(d_key, d_sel, d_scan, n, d_key_out, d_val_out);
    return hipGetLastError();
}

hipError_t order_records(const uint64_t *d_key_sorted, const uint32_t *d_val_sorted, const uint64_t *d_in_off,
                         uint32_t n, uint64_t *d_off, uint16_t *d_cell, uint32_t *d_ord, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_order<<<grid(n), kBlock, 0, s>>>(d_key_sorted, d_val_sorted, d_in_off, n, d_off, d_cell, d_ord);
    return hipGetLastError();
}

hipError_t tag_count(const uint8_t *d_bytes, const uint64_t *d_in_off, uint8_t t0, uint8_t t1,
                     const uint64_t *d_key_sorted, const uint32_t *d_val_sorted, uint32_t *d_run, uint32_t n,
                     uint32_t *d_cnt, void *tmp, size_t tmp_bytes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_run_head<<<grid(n), kBlock, 0, s>>>(d_key_sorted, d_run, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, d_run, d_run, MaxOp(), n, s);
    if (e != hipSuccess) return e;
    k_tag_count<<<grid(n), kBlock, 0, s>>>(d_bytes, d_in_off, t0, t1, d_val_sorted, d_run, n, d_cnt);
    return hipGetLastError();
}

size_t sort_pairs_bytes(uint32_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                       (const uint32_t *)nullptr, (uint32_t *)nullptr, int(n));
    return b;
}

hipError_t sort_pairs(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in,
                      uint32_t *v_out, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k_in, k_out, v_in, v_out, int(n), 0, 64, s);
}

size_t sort_pairs64_bytes(uint64_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                       (const uint64_t *)nullptr, (uint64_t *)nullptr, n);
    return b;
}

hipError_t sort_pairs64(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint64_t *v_in,
                        uint64_t *v_out, uint64_t n, int end_bit, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k_in, k_out, v_in, v_out, n, 0, end_bit, s);
}

size_t scan_bytes(uint64_t n) {
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr, n);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, n);
    (void)hipcub::DeviceScan::InclusiveScan(nullptr, c, (const uint32_t *)nullptr, (uint32_t *)nullptr, MaxOp(), n);
    return std::max(a, std::max(b, c));
}

hipError_t exclusive_sum(void *tmp, size_t bytes, const uint32_t *in, uint32_t *out, uint64_t n, hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, n, s);
}

hipError_t exclusive_sum64(void *tmp, size_t bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, n, s);
}

}  // namespace bam
}  // namespace secedo
