// bam_kernels.hpp -- launch wrappers of bam_kernels.hip (gfx950): the per-record and per-position passes of the
// reference's pileup_bams() (pileup.cpp:49-348). See bam_kernels.hip for the restated semantics.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace bam {

constexpr uint32_t kChunk = 1000000;      // CHUNK_SIZE: positions per reference chunk
constexpr uint32_t kMaxInsert = 1000;     // MAX_INSERT_SIZE
constexpr uint32_t kSlots = 100;          // MAX_OPEN_FILES: files f and f + 100 share a read-name map
constexpr uint32_t kWindow = 1u << 24;    // positions counted per device window (4 x u32 each)

// error codes of the decode pass (the reference's asserts and undefined reads), reported for the lowest
// record ordinal that has one
enum Err : uint32_t {
    kErrNone = 0,
    kErrFlags = 1,        // not paired, not a proper pair or failed QC (pileup.cpp:74-76)
    kErrInsert = 2,       // a kept base >= MAX_INSERT_SIZE past its chunk's end (:152)
    kErrCigarEnd = 3,     // the walk ran past the last CIGAR op (:106, :116, :128)
    kErrDeletion = 4,     // a D op over a character other than '-' (:134)
    kErrQuality = 5,      // the quality index i + offset - del_offset is past the quality string (:137)
    kErrPosition = 6,     // negative Position
    kErrCodes
};

struct Params {
    uint32_t chromosome;
    uint32_t min_base_quality;
    uint32_t min_map_quality;
    uint32_t min_alignment_score;
    uint32_t max_coverage;
    int32_t min_different;
};

struct Records {
    const uint8_t *bytes;   // uploaded records (block_size field first), host-validated structure
    const uint64_t *off;    // [n] byte offset of record ordinal r, in global order (chunk, file, record)
    const uint16_t *file;   // [n] file index (cell id) of record r; in tag mode its cell (rule 3b)
    uint32_t n;
};

// the barcode list of tag mode (rule 3b): packed values (off[n + 1]), their hashes sorted and the cell of each
struct CellList {
    const uint8_t *bytes;
    const uint32_t *off;   // [n + 1] by cell
    const uint64_t *hash;  // [n] sorted
    const uint32_t *cell;  // [n] cell of hash[k]
    uint32_t n;
    uint8_t t0, t1;        // the tag
};

// hash[c], idx[c] = c of each listed value (to be sorted by hash into CellList)
hipError_t list_hash(const uint8_t *d_bytes, const uint32_t *d_off, uint32_t n, uint64_t *d_hash, uint32_t *d_idx,
                     hipStream_t s);
// cells: per uploaded record (input order) d_sel = 1 for a listed barcode whose flag passes rule 3c (require,
// exclude; 0, 0 = off), d_key = chunk << 46 | cell << 32 | Position. d_stat: null, or Sel counters (zeroed by the
// caller) that take kSelRecords (records of listed barcodes), kSelRequire and kSelExclude.
hipError_t cells(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, const CellList &L, uint32_t require,
                 uint32_t exclude, uint64_t *d_key, uint32_t *d_sel, unsigned long long *d_stat, hipStream_t s);
// tag_keys: d_sel = 1 for a Z-typed value of tag t0 t1 on a record that passes rule 3c, d_key = its hash; d_stat as
// for cells, over the records with a Z-typed value
hipError_t tag_keys(const uint8_t *d_bytes, const uint64_t *d_in_off, uint32_t n, uint8_t t0, uint8_t t1,
                    uint32_t require, uint32_t exclude, uint64_t *d_key, uint32_t *d_sel, unsigned long long *d_stat,
                    hipStream_t s);
// selected (key, input ordinal) pairs at d_scan (exclusive sum of d_sel)
hipError_t compact_keys(const uint64_t *d_key, const uint32_t *d_sel, const uint32_t *d_scan, uint32_t n,
                        uint64_t *d_key_out, uint32_t *d_val_out, hipStream_t s);
// Records of the sorted order: d_off[j] = d_in_off[val[j]], d_cell[j] = the key's cell, d_ord[j] = val[j]
hipError_t order_records(const uint64_t *d_key_sorted, const uint32_t *d_val_sorted, const uint64_t *d_in_off,
                         uint32_t n, uint64_t *d_off, uint16_t *d_cell, uint32_t *d_ord, hipStream_t s);
// distinct values of hash-sorted (key, input ordinal) pairs: d_cnt[j] (zeroed by the caller) = records of the value
// first seen at sorted position j, 0 elsewhere. d_run: workspace [n]; tmp: scan_bytes(n)
hipError_t tag_count(const uint8_t *d_bytes, const uint64_t *d_in_off, uint8_t t0, uint8_t t1,
                     const uint64_t *d_key_sorted, const uint32_t *d_val_sorted, uint32_t *d_run, uint32_t n,
                     uint32_t *d_cnt, void *tmp, size_t tmp_bytes, hipStream_t s);

// --- rules 3c and 3d: front passes from one Records to a compacted Records ---

// slots of the device counters behind secedo_bam_select_info
enum Sel : uint32_t {
    kSelRecords = 0, kSelRequire, kSelExclude, kSelTemplates, kSelLarge, kSelDupTemplates, kSelDupRecords, kSelSlots
};

// rule 3c: d_keep[o] = 1 iff (flag & require) == require && (flag & exclude) == 0; counts into d_stat
hipError_t flag_test(const Records &r, uint32_t require, uint32_t exclude, uint32_t *d_keep,
                     unsigned long long *d_stat, hipStream_t s);
// the records with d_keep at d_scan (its exclusive sum), order kept; d_ord_out = d_ord[o], or o where d_ord is null
hipError_t compact_records(const Records &r, const uint32_t *d_ord, const uint32_t *d_keep, const uint32_t *d_scan,
                           uint64_t *d_off_out, uint16_t *d_file_out, uint32_t *d_ord_out, hipStream_t s);
// rule 3d per record: d_end = (u + 2^62) << 1 | strand of its 5' end, d_score = its quality sum, d_key = hash of
// (cell, name), d_val = ordinal; to be sorted by key
hipError_t ends_and_scores(const Records &r, uint64_t *d_key, uint32_t *d_val, uint64_t *d_end, uint32_t *d_score,
                           hipStream_t s);
// templates from the sorted pairs: d_rep[o] = lowest ordinal of o's template; per leader d_extra (records besides
// it), d_tscore (summed score), d_mate (a pair's other record), all three zeroed by the caller; d_sel[o] = 1 for the
// leader of a single or a pair and d_gkey[o] = hash of its key. d_run: workspace [n]; tmp: scan_bytes(n)
hipError_t templates(const Records &r, const uint64_t *d_key_sorted, const uint32_t *d_val_sorted,
                     const uint32_t *d_score, const uint64_t *d_end, uint32_t *d_run, uint32_t *d_rep,
                     uint32_t *d_extra, uint32_t *d_tscore, uint32_t *d_mate, uint64_t *d_gkey, uint32_t *d_sel,
                     unsigned long long *d_stat, void *tmp, size_t tmp_bytes, hipStream_t s);
// the m selected leaders sorted by gkey (value = leader ordinal): d_keep[o] = 0 for every record of a template that
// is not the best of its exact key, 1 elsewhere. d_best [n] zeroed by the caller; d_run, d_grp: workspace [n]
hipError_t mark_duplicates(const Records &r, const uint64_t *d_gkey_sorted, const uint32_t *d_val_sorted, uint32_t m,
                           const uint32_t *d_extra, const uint32_t *d_mate, const uint64_t *d_end,
                           const uint32_t *d_tscore, uint32_t *d_run, uint32_t *d_grp, unsigned long long *d_best,
                           uint32_t *d_keep, unsigned long long *d_stat, void *tmp, size_t tmp_bytes, hipStream_t s);

// decode: per record the read filter, the name key, the walk's error checks and the end of its touched span.
// d_err: u64 min of (ordinal << 8 | code), initialised to ~0 by the caller.
hipError_t decode(const Records &r, const Params &p, uint64_t *d_key, uint32_t *d_val, uint8_t *d_pass,
                  uint32_t *d_span_end, unsigned long long *d_err, hipStream_t s);

// name numbering: sorted (key, ordinal) pairs -> d_rep[ordinal] = first ordinal with the same (slot, name);
// d_flag[ordinal] = 1 on a first occurrence. d_run: workspace [n].
hipError_t first_occurrence(const Records &r, const uint64_t *d_key_sorted, const uint32_t *d_val_sorted,
                            uint32_t *d_run, uint32_t *d_rep, uint32_t *d_flag, void *tmp, size_t tmp_bytes,
                            hipStream_t s);
// d_id[r] = d_scan[d_rep[r]]
hipError_t assign_ids(const uint32_t *d_rep, const uint32_t *d_scan, uint32_t *d_id, uint32_t n, hipStream_t s);

// count: 4 u32 base counts per position of [w0, w1) (d_cnt zeroed by the caller, [W][4])
hipError_t count(const Records &r, const Params &p, const uint8_t *d_pass, const uint32_t *d_span_end, uint32_t w0,
                 uint32_t w1, uint32_t *d_cnt, hipStream_t s);
// select: d_cand[i] = candidate locus, d_arr[i] = its arrivals (all kept bases)
hipError_t select(const uint32_t *d_cnt, const Params &p, uint32_t n_pos, uint32_t *d_cand, uint64_t *d_arr,
                  hipStream_t s);
// per candidate: position (1-based), arrival offset, arrivals
hipError_t compact_candidates(const uint32_t *d_cnt, const uint32_t *d_cand, const uint32_t *d_cand_scan,
                              const uint64_t *d_arr_scan, uint32_t w0, uint32_t n_pos, uint32_t *d_cpos,
                              uint64_t *d_carr, uint32_t *d_ctot, hipStream_t s);
// emit: every kept base at a candidate position -> (locus << 32 | ordinal, read_id << 16 | cell << 2 | base)
hipError_t emit(const Records &r, const Params &p, const uint8_t *d_pass, const uint32_t *d_span_end,
                const uint32_t *d_id, uint32_t w0, uint32_t w1, const uint32_t *d_cand, const uint32_t *d_cand_scan,
                const uint64_t *d_arr_scan, uint32_t *d_fill, uint64_t *d_key, uint64_t *d_val, hipStream_t s);
// finalize: the entries a locus keeps (the last coverage = arrivals mod 2^16 arrivals) and the locus rule for
// loci whose counter wrapped
hipError_t finalize(const uint64_t *d_val_sorted, const uint64_t *d_carr, const uint32_t *d_ctot, const Params &p,
                    uint32_t n_cand, uint32_t *d_keep, uint64_t *d_kept_entries, hipStream_t s);
// gather into the output at (locus_base, entry_base); id_to_group may be null (identity). d_flags[0] = 1 on a
// cell outside it, d_flags[1] = max of the raw cell ids (atomicMax)
hipError_t gather(const uint64_t *d_val_sorted, const uint32_t *d_cpos, const uint64_t *d_carr,
                  const uint32_t *d_ctot, const uint32_t *d_keep, const uint32_t *d_keep_scan,
                  const uint64_t *d_entry_scan, uint32_t n_cand, const uint16_t *d_id_to_group, uint32_t n_ids,
                  uint32_t *d_out_pos, uint64_t *d_out_off, uint32_t *d_out_rid, uint16_t *d_out_idb,
                  uint64_t entry_base, uint32_t *d_flags, hipStream_t s);
// the reader's max_read_length over one chromosome's output: per read id the first and last locus position
// (d_minpos = ~0, d_maxpos = 0 on entry), then *d_max_len = max of last - first (atomicMax)
hipError_t read_stats(const uint32_t *d_pos, const uint64_t *d_off, const uint32_t *d_rid, uint32_t n_loci,
                      uint32_t *d_minpos, uint32_t *d_maxpos, uint32_t n_ids, uint32_t *d_max_len, hipStream_t s);

// hipcub wrappers
size_t sort_pairs_bytes(uint32_t n);
hipError_t sort_pairs(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in,
                      uint32_t *v_out, uint32_t n, hipStream_t s);
size_t sort_pairs64_bytes(uint64_t n);
hipError_t sort_pairs64(void *tmp, size_t bytes, const uint64_t *k_in, uint64_t *k_out, const uint64_t *v_in,
                        uint64_t *v_out, uint64_t n, int end_bit, hipStream_t s);
size_t scan_bytes(uint64_t n);
hipError_t exclusive_sum(void *tmp, size_t bytes, const uint32_t *in, uint32_t *out, uint64_t n, hipStream_t s);
hipError_t exclusive_sum64(void *tmp, size_t bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

}  // namespace bam
}  // namespace secedo
