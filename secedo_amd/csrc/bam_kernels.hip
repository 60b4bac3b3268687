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
//  3c. Flag filter (opt-in: secedo_bam_set_read_filter; not in the reference). After the structural walk and, in tag
//     mode, after the barcode selection of 3b, a record is kept iff (flag & require) == require && (flag & exclude)
//     == 0, both u16 masks, default 0 = off. require & exclude != 0 is SECEDO_E_INVALID_ARG: nothing could pass. The
//     structural walk is unchanged: block-size chain, sortedness, negative position and the CIGAR checks still cover
//     every record.
//  3d. Duplicate removal (opt-in: secedo_bam_set_duplicates; not in the reference), over the records 3c kept, per cell
//     and over the whole chromosome (not per chunk: mates in different chunks still pair).
//     5' end of a record: e = (u, strand), strand = flag 0x10, u a signed 64-bit value: forward u = Position - (total
//     length of the leading S and H ops), reverse u = Position + reflen - 1 + (total length of the trailing S and H
//     ops), reflen = the sum of the M, D, N, = and X lengths, Position the 0-based BAM field.
//     Template: the records of one cell (file index, or barcode index in tag mode: files 0 and 100 share a name map
//     for ids but are different cells here) with the same read name, compared as exact bytes. One record: a single;
//     two: a pair; three or more: never a duplicate, never makes another one a duplicate, counted in the stats.
//     Key: (cell, e) of a single; (cell, e_lo, e_hi) of a pair, its ends ordered by (u, strand); a single's key never
//     equals a pair's. Score: the sum over the template's records of the quality bytes >= 15 and != 0xFF.
//     Among templates with equal keys the highest score is kept, on a tie the template that holds the record with the
//     smallest global ordinal; all records of every other template are dropped.
//     A record dropped by 3c or 3d is "not selected" in 3b's sense: no read id, no .map line, no check of rule 6 or
//     any other decode error, no base; rule 7's last chunk is counted over the survivors. So the outputs equal those
//     of the same call with the options off on the input without the dropped records, byte for byte.
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
// Rules 3c and 3d are front passes too, from one Records to a compacted Records that the chain below takes unchanged;
// with both off nothing is launched or allocated. 3c: in tag mode the flag test is part of `cells` (ANDed into its
// selection in front of the compaction that mode already does); in per-file mode flag_test -> scan -> compact_records.
// 3d: ends_and_scores (16 lanes per record: the quality and name bytes strided over the lanes and summed by shuffles,
// the CIGAR words read by all lanes at one address) -> hipcub sort by hash(cell, name) with the ordinal -> templates
// (run heads, then the first record of the run with the same cell and name bytes is the template's leader: a collision
// splits the run exactly; the other records add their count, score and ordinal to the leader) -> the leaders of singles
// and pairs compacted and sorted by hash(key) -> mark_duplicates (the first leader of the run with exactly the same
// key heads the group, its best rank score << 32 | ~leader is an atomicMax; every template that is not its group's
// best clears the keep flag of its records) -> scan -> compact_records. The atomics are integer sums and maxima,
// whose results do not depend on their order, and every thread stops at its run's head unless hashes collide, so a
// group of any length costs each of its members one compare. Device counters (Sel) feed secedo_bam_select_stats.
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

__device__ __forceinline__ bool flag_require(uint32_t flag, uint32_t require) { return (flag & require) == require; }
__device__ __forceinline__ bool flag_exclude(uint32_t flag, uint32_t exclude) { return (flag & exclude) == 0; }

// Block-wide count of `yes` into *slot (one atomic per block; a sum of integers, so the order does not matter).
// Every thread of the block calls it.
__device__ __forceinline__ void block_count(bool yes, unsigned long long *slot) {
    const int c = __syncthreads_count(yes ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(slot, (unsigned long long)c);
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
// of a listed cell that passes the flag filter of rule 3c (stat: null when the filter is off, else the counts of
// k_flag_test over the records of listed cells)
__global__ void __launch_bounds__(kBlock) k_cells(const uint8_t *bytes, const uint64_t *in_off, uint32_t n,
                                                  CellList L, uint32_t require, uint32_t exclude, uint64_t *key,
                                                  uint32_t *sel, unsigned long long *stat) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    bool listed = false, req = false, exc = false;
    if (o < n) {
        const Rec r = parse(bytes + in_off[o]);
        uint32_t len = 0, cell = ~0u;
        const uint8_t *v = tag_value(r, L.t0, L.t1, &len);
        if (v) cell = find_cell(L, v, len);
        listed = cell != ~0u;
        req = listed && !flag_require(r.flag, require);
        exc = listed && !req && !flag_exclude(r.flag, exclude);
        const bool ok = listed && !req && !exc;
        const uint32_t pos = uint32_t(r.pos);  // >= 0: the host refuses negative positions
        key[o] = ok ? (uint64_t(pos / kChunk) << 46 | uint64_t(cell) << 32 | pos) : 0;
        sel[o] = ok ? 1 : 0;
    }
    if (!stat) return;  // uniform over the grid
    block_count(listed, stat + kSelRecords);
    block_count(req, stat + kSelRequire);
    block_count(exc, stat + kSelExclude);
}

// one thread per record with a Z-typed tag value that passes the flag filter of rule 3c: sel = 1, key = the value's
// hash
__global__ void __launch_bounds__(kBlock) k_tag_keys(const uint8_t *bytes, const uint64_t *in_off, uint32_t n,
                                                     uint8_t t0, uint8_t t1, uint32_t require, uint32_t exclude,
                                                     uint64_t *key, uint32_t *sel, unsigned long long *stat) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    bool tagged = false, req = false, exc = false;
    if (o < n) {
        const Rec r = parse(bytes + in_off[o]);
        uint32_t len = 0;
        const uint8_t *v = tag_value(r, t0, t1, &len);
        tagged = v != nullptr;
        req = tagged && !flag_require(r.flag, require);
        exc = tagged && !req && !flag_exclude(r.flag, exclude);
        const bool ok = tagged && !req && !exc;
        key[o] = ok ? value_hash(v, len) : 0;
        sel[o] = ok ? 1 : 0;
    }
    if (!stat) return;  // uniform over the grid
    block_count(tagged, stat + kSelRecords);
    block_count(req, stat + kSelRequire);
    block_count(exc, stat + kSelExclude);
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

// --- rules 3c and 3d: the flag filter and the duplicate removal, front passes over the Records of the global order ---

// rule 3c per record of the global order: keep[o], and stat[kSelRecords / kSelRequire / kSelExclude]
__global__ void __launch_bounds__(kBlock) k_flag_test(Records rs, uint32_t require, uint32_t exclude, uint32_t *keep,
                                                      unsigned long long *stat) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    const bool in = o < rs.n;
    bool req = false, exc = false;
    if (in) {
        const uint32_t flag = ld16(rs.bytes + rs.off[o] + 4 + 14);
        req = !flag_require(flag, require);
        exc = !req && !flag_exclude(flag, exclude);
        keep[o] = (req || exc) ? 0 : 1;
    }
    block_count(in, stat + kSelRecords);
    block_count(req, stat + kSelRequire);
    block_count(exc, stat + kSelExclude);
}

// the survivors of keep (scan = its exclusive sum) in the same order; ord_out = the ordinal each had before (through
// ord when an earlier compaction or tag mode's sort already renumbered them)
__global__ void __launch_bounds__(kBlock) k_compact_records(const uint64_t *off, const uint16_t *file,
                                                            const uint32_t *ord, const uint32_t *keep,
                                                            const uint32_t *scan, uint32_t n, uint64_t *off_out,
                                                            uint16_t *file_out, uint32_t *ord_out) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    if (o >= n || !keep[o]) return;
    const uint32_t at = scan[o];
    off_out[at] = off[o];
    file_out[at] = file[o];
    ord_out[at] = ord ? ord[o] : o;
}

constexpr uint32_t kSub = 16;                 // lanes per record in k_ends
constexpr uint64_t kEndBias = 1ull << 62;     // u + kEndBias > 0: an end (u, strand) orders as (u + bias) << 1 | strand
constexpr uint64_t kNoEnd = ~0ull;            // e_hi of a single: no pair has it
constexpr uint64_t kNamePrime = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t mix64(uint64_t h) {
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    h *= 0x94D049BB133111EBull;
    return h ^ (h >> 29);
}

// Rule 3d per record, kSub lanes per record: the lanes stride over the quality bytes and the name bytes (coalesced
// within the group) and are summed by shuffles; the CIGAR words are read by every lane at the same address.
// -> end[o] = its 5' end, score[o] = its quality sum, key[o] = hash of (cell, name), val[o] = o.
__global__ void __launch_bounds__(kBlock) k_ends(Records rs, uint64_t *key, uint32_t *val, uint64_t *end,
                                                 uint32_t *score) {
    const uint32_t o = uint32_t((uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kSub), lane = threadIdx.x % kSub;
    if (o >= rs.n) return;  // whole groups leave together: kBlock is a multiple of kSub
    const Rec r = parse(rs.bytes + rs.off[o]);
    uint32_t sum = 0;
    for (uint32_t k = lane; k < r.l_seq; k += kSub) {
        const uint32_t q = r.qual[k];
        if (q >= 15 && q != 0xFF) sum += q;
    }
    uint32_t len = r.l_name;  // the name ends at its first NUL
    for (uint32_t k = lane; k < r.l_name; k += kSub)
        if (r.name[k] == 0) {
            len = k;
            break;
        }
    for (uint32_t d = kSub / 2; d; d >>= 1) {
        sum += __shfl_xor(sum, d, kSub);
        len = min(len, uint32_t(__shfl_xor(len, d, kSub)));
    }
    uint64_t h = 0, pw = 1;
    for (uint32_t k = 0; k < lane; ++k) pw *= kNamePrime;
    uint64_t step = 1;
    for (uint32_t k = 0; k < kSub; ++k) step *= kNamePrime;
    for (uint32_t k = lane; k < len; k += kSub) {
        h += (uint64_t(r.name[k]) + 1) * pw;
        pw *= step;
    }
    for (uint32_t d = kSub / 2; d; d >>= 1) h += __shfl_xor(h, d, kSub);
    if (lane) return;
    // leading and trailing S/H runs, and the reference length
    uint64_t lead = 0, trail = 0, reflen = 0;
    bool in_lead = true;
    for (uint32_t c = 0; c < r.n_cigar; ++c) {
        const uint32_t t = op_type(r, c), l = op_len(r, c);
        if (t == kOpS || t == kOpH) {
            if (in_lead) lead += l;
            else trail += l;
        } else {
            in_lead = false;
            trail = 0;
            if (t == kOpM || t == kOpD || t == kOpN || t == kOpEq || t == kOpX) reflen += l;
        }
    }
    const bool rev = (r.flag & 0x10) != 0;
    const int64_t u = rev ? int64_t(r.pos) + int64_t(reflen) - 1 + int64_t(trail) : int64_t(r.pos) - int64_t(lead);
    end[o] = (uint64_t(u) + kEndBias) << 1 | (rev ? 1 : 0);
    score[o] = sum;
    key[o] = mix64(h ^ mix64(uint64_t(rs.file[o]) << 32 | len));
    val[o] = o;
}

// same cell and same name bytes
__device__ bool same_template(const Records &rs, uint32_t a, uint32_t b) {
    if (rs.file[a] != rs.file[b]) return false;
    const Rec x = parse(rs.bytes + rs.off[a]), y = parse(rs.bytes + rs.off[b]);
    for (uint32_t k = 0;; ++k) {
        const uint8_t cx = k < x.l_name ? x.name[k] : 0, cy = k < y.l_name ? y.name[k] : 0;
        if (cx != cy) return false;
        if (cx == 0) return true;
    }
}

// Template assembly over the hash-sorted (key, ordinal) pairs: rep[o] = the lowest ordinal of o's template (the first
// record of the run of equal hashes that compares equal; without a collision that is the run's head). The other
// records add themselves to their leader: extra[rep] counts them, tscore[rep] sums the scores, mate[rep] = max of
// their ordinals (the one mate of a pair). Integer sums and maxima: any order of the atomics gives the same values.
__global__ void __launch_bounds__(kBlock) k_tmpl_rep(Records rs, const uint32_t *val, const uint32_t *run,
                                                     const uint32_t *score, uint32_t *rep, uint32_t *extra,
                                                     uint32_t *tscore, uint32_t *mate) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= rs.n) return;
    const uint32_t o = val[j];
    uint32_t first = o;
    for (uint32_t q = run[j]; q < j; ++q)  // equal keys are in ordinal order (stable sort)
        if (same_template(rs, val[q], o)) {
            first = val[q];
            break;
        }
    rep[o] = first;
    atomicAdd(&tscore[first], score[o]);
    if (first != o) {
        atomicAdd(&extra[first], 1u);
        atomicMax(&mate[first], o);
    }
}

struct DupKey {
    uint64_t lo, hi;  // the ends in order; hi = kNoEnd for a single
};

__device__ __forceinline__ DupKey dup_key(const uint64_t *end, const uint32_t *extra, const uint32_t *mate,
                                          uint32_t o) {
    DupKey k{end[o], kNoEnd};
    if (extra[o] == 1) {
        const uint64_t e2 = end[mate[o]];
        k.hi = max(k.lo, e2);
        k.lo = min(k.lo, e2);
    }
    return k;
}

// per record: sel[o] = 1 for the leader of a single or a pair, gkey[o] = hash of its key (cell, e_lo, e_hi);
// stat[kSelTemplates / kSelLarge]
__global__ void __launch_bounds__(kBlock) k_tmpl_key(Records rs, const uint32_t *rep, const uint32_t *extra,
                                                     const uint32_t *mate, const uint64_t *end, uint64_t *gkey,
                                                     uint32_t *sel, unsigned long long *stat) {
    const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
    const bool leader = o < rs.n && rep[o] == o;
    const bool large = leader && extra[o] >= 2;
    if (o < rs.n) {
        const bool ok = leader && !large;
        uint64_t h = 0;
        if (ok) {
            const DupKey k = dup_key(end, extra, mate, o);
            h = mix64(mix64(k.lo ^ uint64_t(rs.file[o]) << 48) + mix64(k.hi) * kNamePrime);
        }
        gkey[o] = h;
        sel[o] = ok ? 1 : 0;
    }
    block_count(leader, stat + kSelTemplates);
    block_count(large, stat + kSelLarge);
}

// what a template competes with inside its key: the higher score wins, then the lower leading ordinal
__device__ __forceinline__ unsigned long long dup_rank(const uint32_t *tscore, uint32_t o) {
    return (unsigned long long)tscore[o] << 32 | (~o & 0xFFFFFFFFu);
}

// Grouping over the hash-sorted (gkey, leader ordinal) pairs: grp[o] = the lowest leader of the run of equal hashes
// with exactly o's key, and best[grp] = max of the ranks of that key's templates (atomicMax on exact integers: the
// maximum is the same in any order). A run may be of any length; without a collision every thread stops at its head.
__global__ void __launch_bounds__(kBlock) k_group(Records rs, const uint32_t *val, const uint32_t *run, uint32_t m,
                                                  const uint32_t *extra, const uint32_t *mate, const uint64_t *end,
                                                  const uint32_t *tscore, uint32_t *grp, unsigned long long *best) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t o = val[j];
    const DupKey k = dup_key(end, extra, mate, o);
    uint32_t g = o;
    for (uint32_t q = run[j]; q < j; ++q) {
        const uint32_t p = val[q];
        if (rs.file[p] != rs.file[o]) continue;
        const DupKey kp = dup_key(end, extra, mate, p);
        if (kp.lo == k.lo && kp.hi == k.hi) {
            g = p;
            break;
        }
    }
    grp[o] = g;
    atomicMax(&best[g], dup_rank(tscore, o));
}

// every template but its key's best is a duplicate: keep = 0 for its records (keep is 1 everywhere on entry);
// stat[kSelDupTemplates / kSelDupRecords]
__global__ void __launch_bounds__(kBlock) k_dup_mark(const uint32_t *val, uint32_t m, const uint32_t *grp,
                                                     const unsigned long long *best, const uint32_t *extra,
                                                     const uint32_t *mate, const uint32_t *tscore, uint32_t *keep,
                                                     unsigned long long *stat) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool dup = false, pair = false;
    if (j < m) {
        const uint32_t o = val[j];
        dup = best[grp[o]] != dup_rank(tscore, o);
        pair = dup && extra[o] == 1;
        if (dup) keep[o] = 0;
        if (pair) keep[mate[o]] = 0;
    }
    block_count(dup, stat + kSelDupTemplates);
    block_count(dup, stat + kSelDupRecords);
    block_count(pair, stat + kSelDupRecords);
}

__global__ void __launch_bounds__(kBlock) k_fill(uint32_t *p, uint32_t v, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = v;
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

hipError_t cells(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, const CellList &L, uint32_t require,
                 uint32_t exclude, uint64_t *d_key, uint32_t *d_sel, unsigned long long *d_stat, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_cells<<<grid(n), kBlock, 0, s>>>(d_bytes, d_in_off, n, L, require, exclude, d_key, d_sel, d_stat);
    return hipGetLastError();
}

hipError_t tag_keys(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, uint8_t t0, uint8_t t1,
                    uint32_t require, uint32_t exclude, uint64_t *d_key, uint32_t *d_sel, unsigned long long *d_stat,
                    hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_tag_keys<<<grid(n), kBlock, 0, s>>>(d_bytes, d_in_off, n, t0, t1, require, exclude, d_key, d_sel, d_stat);
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

hipError_t flag_test(const Records &r, uint32_t require, uint32_t exclude, uint32_t *d_keep,
                     unsigned long long *d_stat, hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_flag_test<<<grid(r.n), kBlock, 0, s>>>(r, require, exclude, d_keep, d_stat);
    return hipGetLastError();
}

hipError_t compact_records(const Records &r, const uint32_t *d_ord, const uint32_t *d_keep, const uint32_t *d_scan,
                           uint64_t *d_off_out, uint16_t *d_file_out, uint32_t *d_ord_out, hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_compact_records<<<grid(r.n), kBlock, 0, s>>>(r.off, r.file, d_ord, d_keep, d_scan, r.n, d_off_out, d_file_out,
                                                   d_ord_out);
    return hipGetLastError();
}

hipError_t ends_and_scores(const Records &r, uint64_t *d_key, uint32_t *d_val, uint64_t *d_end, uint32_t *d_score,
                           hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_ends<<<grid(uint64_t(r.n) * kSub), kBlock, 0, s>>>(r, d_key, d_val, d_end, d_score);
    return hipGetLastError();
}

hipError_t templates(const Records &r, const uint64_t *d_key_sorted, const uint32_t *d_val_sorted,
                     const uint32_t *d_score, const uint64_t *d_end, uint32_t *d_run, uint32_t *d_rep,
                     uint32_t *d_extra, uint32_t *d_tscore, uint32_t *d_mate, uint64_t *d_gkey, uint32_t *d_sel,
                     unsigned long long *d_stat, void *tmp, size_t tmp_bytes, hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_run_head<<<grid(r.n), kBlock, 0, s>>>(d_key_sorted, d_run, r.n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, d_run, d_run, MaxOp(), r.n, s);
    if (e != hipSuccess) return e;
    k_tmpl_rep<<<grid(r.n), kBlock, 0, s>>>(r, d_val_sorted, d_run, d_score, d_rep, d_extra, d_tscore, d_mate);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_tmpl_key<<<grid(r.n), kBlock, 0, s>>>(r, d_rep, d_extra, d_mate, d_end, d_gkey, d_sel, d_stat);
    return hipGetLastError();
}

hipError_t mark_duplicates(const Records &r, const uint64_t *d_gkey_sorted, const uint32_t *d_val_sorted, uint32_t m,
                           const uint32_t *d_extra, const uint32_t *d_mate, const uint64_t *d_end,
                           const uint32_t *d_tscore, uint32_t *d_run, uint32_t *d_grp, unsigned long long *d_best,
                           uint32_t *d_keep, unsigned long long *d_stat, void *tmp, size_t tmp_bytes, hipStream_t s) {
    if (r.n == 0) return hipSuccess;
    k_fill<<<grid(r.n), kBlock, 0, s>>>(d_keep, 1u, r.n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || m == 0) return e;
    k_run_head<<<grid(m), kBlock, 0, s>>>(d_gkey_sorted, d_run, m);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, d_run, d_run, MaxOp(), m, s);
    if (e != hipSuccess) return e;
    k_group<<<grid(m), kBlock, 0, s>>>(r, d_val_sorted, d_run, m, d_extra, d_mate, d_end, d_tscore, d_grp, d_best);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_dup_mark<<<grid(m), kBlock, 0, s>>>(d_val_sorted, m, d_grp, d_best, d_extra, d_mate, d_tscore, d_keep, d_stat);
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
