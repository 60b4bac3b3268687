// bam_host.hpp -- what the host files of include/secedo_bam.h share: bam_input.cpp reads the BAM and SAM files
// into one ChrInput per requested chromosome, bam_pileup.cpp turns those into the pileup, bam_split.cpp into the
// per-cluster BAMs and bam_depth.cpp into the depth tables; the three take a chromosome's records to the device and
// compact the selected ones through the functions declared here (bam_pileup.cpp defines them). Internal, nothing
// exported.
#pragma once

#include "bam_batch.hpp"
#include "bam_kernels.hpp"
#include "bam_split.hpp"
#include "bgzf_members.hpp"
#include "host_util.hpp"
#include "secedo_bam.h"

#include <sys/mman.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace secedo {
namespace bam_host __attribute__((visibility("hidden"))) {

using namespace secedo::host;

inline uint32_t rd32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint16_t rd16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }

// Layout of a BAM record body c (after block_size): 32 fixed bytes, read name, CIGAR, packed SEQ, QUAL, aux fields.
inline uint32_t rec_l_name(const uint8_t *c) { return c[8]; }
inline uint32_t rec_n_cigar(const uint8_t *c) { return rd16(c + 12); }
inline uint32_t rec_l_seq(const uint8_t *c) { return rd32(c + 16); }
inline uint64_t rec_aux_off(const uint8_t *c) {
    return 32 + uint64_t(rec_l_name(c)) + 4ull * rec_n_cigar(c) + (uint64_t(rec_l_seq(c)) + 1) / 2 + rec_l_seq(c);
}

// the records of one chromosome, file after file in input order
struct ChrInput {
    uint32_t chromosome;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> file_base;          // [n_files] start of each file's run in bytes
    std::vector<std::vector<uint64_t>> roff;  // per file: record offsets (relative to its run)
    std::vector<std::vector<int32_t>> rpos;
    std::vector<std::vector<uint64_t>> ridx;  // record index in the file (messages)
};

// what one call read
struct Inputs {
    std::vector<std::string> paths;  // [n_files] (messages)
    std::vector<uint64_t> line0;     // [n_files] SAM: the line of record 0 (1-based); BAM: 0
    std::vector<char> indexed;       // [n_files] BAM read through its index: record 0 is the first span's first
    std::vector<ChrInput> chrs;      // [n_chr]
};

// Where record idx of file f is, for messages:
//   SAM (line0 != 0):        "file f (path), line line0 + idx"
//   BAM while loading:       "path: record idx"
//   BAM in the device stage: "file f, record idx"
// Known wart: the two BAM wordings name the same record differently. Both are kept as callers know them.
// indexed: the file was read through its index, its whole-file ordinals are unknown: "indexed record idx" in both.
enum class Stage { kLoad, kDevice };
std::string record_where(const std::string &path, size_t f, uint64_t line0, uint64_t idx, Stage stage = Stage::kLoad,
                         bool indexed = false);

// Reads the files (BAM or SAM, told apart by their first bytes) and keeps the records of the requested chromosomes.
// t: stage times are added to it; may be null.
int load_inputs(const std::vector<std::string> &files, const uint32_t *chromosome_ids, uint32_t n_chr,
                uint32_t threads, Inputs *in, secedo_bam_times *t);

// The header of one input file as a BAM holds it (bam_split.cpp writes headers from it): the text, and the binary
// reference list (n_ref entries of l_name, name, l_ref). Of a SAM or BGZF SAM file the text is its leading '@' lines
// and ref_list stays empty: its @SQ lines are the list. Host only; meant for files load_inputs has read already.
struct FileHeader {
    std::string text;
    uint32_t n_ref = 0;
    std::vector<uint8_t> ref_list;
    bool sam = false;
};
int read_file_header(const std::string &path, FileHeader *h);

// The reference lists of `files` (read_file_header; a SAM file's @SQ lines are its list), checked against the first
// one's (bamsplit::refs_differ: "<path>: its reference list is not that of the first file <path>: <why>") -> *first,
// its binary form *first_list and every file's header text (bam_split.cpp defines it; bam_depth.cpp takes the bins
// from *first).
int read_reference_lists(const std::vector<std::string> &files, std::vector<bamsplit::Ref> *first,
                         std::vector<uint8_t> *first_list, std::vector<std::string> *texts);

// ---- what the calls of bam_pileup.cpp, bam_split.cpp and bam_depth.cpp share of tag mode and of their argument checks

// tag: two characters [A-Za-z][A-Za-z0-9] (SAM spec 1.5)
int check_tag(const char *tag);
// the barcode list of tag mode: non-empty, at most SECEDO_BAM_MAX_FILES, no value twice
int check_cells(const char *tag, const char *const *barcodes, uint32_t n, std::vector<std::string> *values);
int check_files(const char *const *bam_files, uint32_t n_files, std::vector<std::string> *files);

// The listed barcodes of tag mode on the device: packed values, their hashes sorted, the cell of each.
struct DevCells {
    Dev<uint8_t> bytes;
    Dev<uint32_t> off, cell;
    Dev<uint64_t> hash;
    bam::CellList list{};
};
int upload_cells(const char tag[2], const std::vector<std::string> &values, hipStream_t s, DevCells *dc);

// ---- rules 3c and 3d of bam_kernels.hip, shared by the pileup calls, secedo_bam_split_clusters_select and
// secedo_bam_depth

// The device counters of the front passes (bam::Sel slots), added to a call's secedo_bam_select_info when a
// chromosome's passes are done. Stays unallocated, and adds nothing, with both rules off.
struct SelStat {
    Dev<unsigned long long> d;
    int init(hipStream_t s) {
        SECEDO_TRY(d.alloc(bam::kSelSlots));
        SECEDO_TRY(hipMemsetAsync(d.p, 0, bam::kSelSlots * 8, s));
        return SECEDO_OK;
    }
    int add_to(hipStream_t s, secedo_bam_select_info *info) {
        if (!d.p) return SECEDO_OK;
        unsigned long long h[bam::kSelSlots];
        SECEDO_TRY(hipMemcpyAsync(h, d.p, sizeof h, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        info->records += h[bam::kSelRecords];
        info->dropped_require += h[bam::kSelRequire];
        info->dropped_exclude += h[bam::kSelExclude];
        info->templates += h[bam::kSelTemplates];
        info->large_templates += h[bam::kSelLarge];
        info->duplicate_templates += h[bam::kSelDupTemplates];
        info->duplicate_records += h[bam::kSelDupRecords];
        return SECEDO_OK;
    }
};

// Rule 3d over the rs.n >= 1 records of rs, whose order within a cell is the global order: (*keep)[o] (rs.n + 1
// entries allocated) = 0 for every record of a template that is not the best of its key, 1 elsewhere. d_stat: Sel
// counters (kSelTemplates, kSelLarge, kSelDupTemplates, kSelDupRecords). The passes' arrays are freed on return.
int duplicate_keep(const bam::Records &rs, unsigned long long *d_stat, hipStream_t s, Dev<uint32_t> *keep);

// ---- what the pileup calls, bam_split.cpp and bam_depth.cpp share of a chromosome's way to the device

// Where the records of the pileup's global order come from, for error messages and the .map.
struct Order {
    uint32_t n = 0, last_chunk = 0;
    int32_t min_pos = INT32_MAX;
    std::vector<uint64_t> ord_off;  // per-file mode: per ordinal byte offset, input file, record index
    std::vector<uint16_t> ord_file;
    std::vector<uint64_t> ord_idx;
    std::vector<uint32_t> in_file;  // tag mode: per input ordinal; d_ord maps an ordinal to its input ordinal
    std::vector<uint64_t> in_idx;
    Dev<uint32_t> d_ord;  // per-file mode: null until rule 3c or 3d dropped a record, then the ordinal each had before
};

// a chromosome's records are numbered in 32 bits
inline int check_record_count(uint64_t n) {
    return n >= (1ull << 32) ? fail(SECEDO_E_LIMIT, "more than 2^32 records in one chromosome") : SECEDO_OK;
}

// zero bytes behind the last record on the device: the split's gather reads whole aligned words
constexpr size_t kRecordSlack = 16;

// The chromosome's records on the device in input order (file, record): ci.bytes and kRecordSlack zero bytes ->
// d_bytes, the byte offset of each record -> in_off / d_in_off (check_record_count holds). d_file (may be null) takes
// the input file of each record; ord (may be null) the input file and record index of each, on the host. t (may be
// null): walk_ms and upload_ms are added to. A chromosome without records is uploaded like any other.
int upload_input_order(const ChrInput &ci, hipStream_t s, std::vector<uint64_t> *in_off, Order *ord,
                       Dev<uint8_t> *d_bytes, Dev<uint64_t> *d_in_off, Dev<uint16_t> *d_file, secedo_bam_times *t);

// The selected (key, input ordinal) pairs of d_key / d_sel (n records; d_sel has n + 1 entries, the last is zeroed
// here) in input order: -> *n_sel, d_kc, d_vc.
int compact_selected(const Dev<uint64_t> &d_key, Dev<uint32_t> &d_sel, uint32_t n, hipStream_t s, uint32_t *n_sel,
                     Dev<uint64_t> *d_kc, Dev<uint32_t> *d_vc);
// compact_selected, then sorted by key (stable): -> *n_sel, d_ks, d_vs.
int compact_and_sort(const Dev<uint64_t> &d_key, Dev<uint32_t> &d_sel, uint32_t n, hipStream_t s, uint32_t *n_sel,
                     Dev<uint64_t> *d_ks, Dev<uint32_t> *d_vs);

// ---- what bam_input.cpp (host inflate, host walk) and bam_device_input.cpp (device inflate, device walk) share

constexpr uint32_t kMaxThreads = 16;

// f(0) .. f(n - 1) in a pool of at most kMaxThreads threads
template <class F>
void parallel_for(uint32_t threads, uint64_t n, F f) {
    threads = std::max<uint32_t>(1, std::min<uint64_t>(std::min(threads, kMaxThreads), n));
    std::atomic<uint64_t> next{0};
    auto work = [&] {
        for (uint64_t i; (i = next.fetch_add(1)) < n;) f(i);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
}

// inflated bytes per batch of files and per block range of one file; SECEDO_BAM_BATCH_BYTES overrides it (tests:
// outputs do not depend on it), read at every call
uint64_t batch_bytes();

struct Mapped {
    const uint8_t *p = nullptr;
    size_t n = 0;
    Mapped() = default;
    Mapped(const Mapped &) = delete;
    Mapped &operator=(const Mapped &) = delete;
    Mapped(Mapped &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    Mapped &operator=(Mapped &&o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~Mapped() {
        if (p && n) munmap(const_cast<uint8_t *>(p), n);
    }
};

// A BGZF block is a member of bgzf_members.hpp (bm::Member; Block and bm come with bam_batch.hpp), which lists,
// describes and inflates them; these two put the file's name in front of its reasons.

// "<path>: <bm::block_where*()>: <why>": the error of every route for a block that does not inflate
inline int bad_block(const std::string &path, const std::string &where, const std::string &why) {
    return fail(SECEDO_E_INVALID_ARG, path + ": " + where + ": " + why);
}

// the BGZF block at byte off < m.n of a mapped file (its `out` left 0); *len = its bytes in the file
int read_block(const std::string &path, const Mapped &m, uint64_t off, Block *blk, uint32_t *len);

// a file mapped and its BGZF blocks listed; *total = its inflated size
int open_bgzf(const std::string &path, Mapped *m, std::vector<Block> *blocks, uint64_t *total);

struct Header {
    uint32_t l_text = 0, n_ref = 0;
    uint64_t first_record = 0;
};

constexpr int kNeedMore = 1;  // parse_header / walk_range: the bytes end inside the header or a record

// final: d ends the file, so a cut header is an error; else kNeedMore
int parse_header(const std::string &path, const uint8_t *d, uint64_t n, bool final, Header *h);

// ---- reading through the .bai index (secedo_bam_set_index, SECEDO_BAM_INDEX; bam_index.hpp parses the file)

// SpanChr and Span, a run of members entered at a known record start: bam_batch.hpp

// What the index says of one BAM for the requested chromosomes.
struct IndexPlan {
    bool indexed = false;  // false: the file is read in full
    Mapped m;
    std::vector<Block> head;     // the members that hold the header and the reference list
    Header h;
    std::vector<Span> spans;     // in file order
};

// The index mode of this call: SECEDO_BAM_INDEX_OFF / AUTO / REQUIRE (secedo_bam_set_index, else SECEDO_BAM_INDEX).
int index_mode(int *mode);
// Plans the read of one BAM under AUTO or REQUIRE: its header members are inflated here, its index is read and
// checked, the members of its spans are found by following BSIZE. AUTO without a usable index: plan->indexed stays
// false and the stats count the file as read in full.
int plan_index(const std::string &path, const std::vector<uint32_t> &chromosomes, int mode, IndexPlan *plan);
// "<path>: index does not match the file (<why>); re-index it or use --index off"
int index_mismatch(const std::string &path, const std::string &why);
// "<where the record is>" + defect_tail(code): bam_walk.hpp's words of a record defect, the op's number behind them
inline std::string defect_tail(uint32_t code) {
    return bamwalk::defect_words(code) + (bamwalk::is_cigar_op(code) ? std::to_string(code & 15) : std::string());
}
// Under a span a record chain that breaks (bamwalk::kErrTruncated, kErrBlockSize at indexed record idx) means that
// the index does not fit the file: the same sentence from both routes.
inline int chain_break(const std::string &path, uint64_t idx, uint32_t code) {
    return index_mismatch(path, "the record chain breaks: indexed record " + std::to_string(idx) + defect_tail(code));
}
// The checks made after a span was read, the same words from both routes. got_count: records that start in
// [c.beg, c.end); start_ok: one starts at c.beg with the chromosome's RefID.
int check_span_chr(const std::string &path, const SpanChr &c, bool start_ok, uint64_t got_count);
int span_tail_mismatch(const std::string &path, const SpanChr &c);
secedo_bam_index_info &index_info();

// Process-wide BAM route (secedo_bam_set_inflate, SECEDO_BAM_INFLATE), read at every call: *device = the device
// route. An unknown value of the variable is SECEDO_E_INVALID_ARG.
int inflate_route(bool *device);

// What the last pileup or scan call on this thread did (secedo_bam_route_stats). Behind a function: an extern
// thread_local of a hidden namespace is reached through an init wrapper that other translation units call unchecked.
secedo_bam_route_info &route();

// The device route for BAM files [f0, f1) of in->paths (bam_device_input.cpp): device inflate and device walk; the
// records of the requested chromosomes are appended to runs[chr][file] and in->chrs as the host walk's FileSink does.
using Runs = std::vector<std::vector<std::vector<uint8_t>>>;  // [chr][file] the file's records of the chromosome
struct BamDevWork;
BamDevWork *new_bam_dev_work();
void delete_bam_dev_work(BamDevWork *w);
// (*plans)[f] (plans may be null: no index in use) says which of them go through their index.
int load_bams_device(size_t f0, size_t f1, uint32_t threads, uint64_t batch, BamDevWork *w, Inputs *in, Runs *runs,
                     secedo_bam_times *t, std::vector<IndexPlan> *plans = nullptr);

// The file is BAM by content, as load_inputs tells it: a SAM or BGZF SAM file is SECEDO_E_INVALID_ARG ("<path>: a SAM
// file <what>; ..."), a plain-gzip file is refused in load_inputs' words.
int require_bam(const std::string &path, const std::string &what);

// Frees the device memory of the last secedo_bgzf_inflate result of this thread (secedo_bam_release calls it).
void release_inflated();
// Frees the last secedo_bam_depth result of this thread (bam_depth.cpp; secedo_bam_release calls it).
void release_depth();

}  // namespace bam_host
}  // namespace secedo
