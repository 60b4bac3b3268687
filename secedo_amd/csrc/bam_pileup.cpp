// bam_pileup.cpp -- the pileup side of include/secedo_bam.h: the global record order, the launches of
// bam_kernels.hip over the ChrInput list that bam_input.cpp reads (bam_host.hpp), and the .bin / .map / .txt files of
// the reference's pileup_bams() (pileup.cpp:235-348).
//
// Tag mode (secedo_pileup_bams_cells) uploads the chromosome's records in input order and builds the global order
// on the device (bam_kernels.hip rule 3b); secedo_bam_barcodes counts the distinct tag values.
#include "bam_host.hpp"
#include "bam_kernels.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstdio>
#include <map>
#include <set>

namespace {

using namespace secedo::bam;
using namespace secedo::bam_host;

// The value of the first aux field named by the tag, which the device's census found Z-typed (FindTag's walk).
std::string first_z_value(const uint8_t *p, uint64_t len, const char *tag) {
    uint64_t o = 0;
    while (o + 3 <= len) {
        const uint8_t type = p[o + 2];
        o += 3;
        if (p[o - 3] == uint8_t(tag[0]) && p[o - 2] == uint8_t(tag[1])) {
            const uint64_t b = o;
            while (o < len && p[o]) ++o;
            return std::string(reinterpret_cast<const char *>(p + b), o - b);
        }
        uint64_t skip = 0;
        switch (type) {
            case 'A': case 'c': case 'C': skip = 1; break;
            case 's': case 'S': skip = 2; break;
            case 'f': case 'i': case 'I': skip = 4; break;
            case 'Z': case 'H': while (o + skip < len && p[o + skip]) ++skip; ++skip; break;
            case 'B': {
                const uint8_t at = p[o];
                const uint64_t es = (at == 'c' || at == 'C') ? 1 : (at == 's' || at == 'S') ? 2 : 4;
                skip = 5 + uint64_t(rd32(p + o + 1)) * es;
                break;
            }
            default: return std::string();
        }
        o += skip;
    }
    return std::string();
}

struct Result {
    std::vector<uint32_t> chr_locus_off{0};
    Dev<uint32_t> pos, rid;
    Dev<uint64_t> off;
    Dev<uint16_t> idb;
    uint64_t n_loci = 0, n_entries = 0;
    uint32_t num_cells = 1, max_read_length = 0;
};

thread_local Result *g_result = nullptr;

// Rules 3c and 3d (bam_kernels.hip): the process-wide settings, read at every call, and what the last call did.
std::atomic<int64_t> g_read_filter{-1};  // require << 16 | exclude; -1: not set, the environment decides
std::atomic<int> g_duplicates{-1};       // -1: not set by secedo_bam_set_duplicates, the environment decides
thread_local secedo_bam_select_info g_select{};

struct Select {
    uint32_t require = 0, exclude = 0;
    bool dedup = false;
    bool filter() const { return (require | exclude) != 0; }
};

int check_read_filter(const std::string &who, uint64_t require, uint64_t exclude) {
    if (require > 0xFFFF || exclude > 0xFFFF)
        return fail(SECEDO_E_INVALID_ARG, who + ": a SAM flag mask is at most 0xFFFF");
    if (require & exclude)
        return fail(SECEDO_E_INVALID_ARG, who + ": require " + std::to_string(require) + " and exclude " +
                                              std::to_string(exclude) + " share a bit, no record could pass");
    return SECEDO_OK;
}

// a flag mask of the environment: decimal or 0x hex
int env_flags(const char *name, uint64_t *v) {
    *v = 0;
    const char *e = std::getenv(name);
    if (!e || !*e) return SECEDO_OK;
    char *end = nullptr;
    const unsigned long long x = std::strtoull(e, &end, 0);
    if (end == e || *end || *e == '-' || x > 0xFFFF)
        return fail(SECEDO_E_INVALID_ARG, std::string(name) + "=" + e + ": expected a flag mask, decimal or 0x hex, at most 0xFFFF");
    *v = x;
    return SECEDO_OK;
}

int read_filter(uint32_t *require, uint32_t *exclude) {
    const int64_t f = g_read_filter.load();
    uint64_t rq = 0, ex = 0;
    if (f < 0) {
        SECEDO_CALL(env_flags("SECEDO_BAM_REQUIRE_FLAGS", &rq));
        SECEDO_CALL(env_flags("SECEDO_BAM_EXCLUDE_FLAGS", &ex));
        SECEDO_CALL(check_read_filter("SECEDO_BAM_REQUIRE_FLAGS / SECEDO_BAM_EXCLUDE_FLAGS", rq, ex));
    } else {
        rq = uint64_t(f) >> 16;
        ex = uint64_t(f) & 0xFFFF;
    }
    *require = uint32_t(rq);
    *exclude = uint32_t(ex);
    return SECEDO_OK;
}

int duplicates_mode(int *mode) {
    int m = g_duplicates.load();
    if (m < 0) {
        const char *e = std::getenv("SECEDO_BAM_DUPLICATES");
        if (!e || !*e || std::strcmp(e, "keep") == 0) m = SECEDO_BAM_DUPLICATES_KEEP;
        else if (std::strcmp(e, "remove") == 0) m = SECEDO_BAM_DUPLICATES_REMOVE;
        else return fail(SECEDO_E_INVALID_ARG, std::string("SECEDO_BAM_DUPLICATES=") + e + ": expected keep or remove");
    }
    *mode = m;
    return SECEDO_OK;
}

int current_select(Select *sel) {
    SECEDO_CALL(read_filter(&sel->require, &sel->exclude));
    int mode = SECEDO_BAM_DUPLICATES_KEEP;
    SECEDO_CALL(duplicates_mode(&mode));
    sel->dedup = mode == SECEDO_BAM_DUPLICATES_REMOVE;
    return SECEDO_OK;
}

struct ChrOut {
    std::vector<uint8_t> first;  // per ordinal: first occurrence of its name (host files only)
    std::vector<uint32_t> id;
    std::vector<uint64_t> ord_off;  // per ordinal: byte offset in ChrInput::bytes
};

}  // namespace

namespace secedo {
namespace bam_host {

// tag mode's barcode list to the device (bam_host.hpp: DevCells); bam_split.cpp uses it too
int upload_cells(const char tag[2], const std::vector<std::string> &values, hipStream_t s, DevCells *dc) {
    const uint32_t n = uint32_t(values.size());
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off{0};
    for (const auto &v : values) {
        bytes.insert(bytes.end(), v.begin(), v.end());
        off.push_back(uint32_t(bytes.size()));
    }
    Dev<uint64_t> h;
    Dev<uint32_t> idx;
    SECEDO_TRY(dc->bytes.alloc(bytes.size()));
    SECEDO_TRY(dc->off.alloc(n + 1));
    SECEDO_TRY(dc->hash.alloc(n));
    SECEDO_TRY(dc->cell.alloc(n));
    SECEDO_TRY(h.alloc(n));
    SECEDO_TRY(idx.alloc(n));
    if (!bytes.empty()) SECEDO_TRY(hipMemcpyAsync(dc->bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(dc->off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    SECEDO_TRY(bam::list_hash(dc->bytes.p, dc->off.p, n, h.p, idx.p, s));
    const size_t tb = bam::sort_pairs_bytes(n);
    Dev<uint8_t> tmp;
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(bam::sort_pairs(tmp.p, tb, h.p, dc->hash.p, idx.p, dc->cell.p, n, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    dc->list = bam::CellList{dc->bytes.p, dc->off.p, dc->hash.p, dc->cell.p, n, uint8_t(tag[0]), uint8_t(tag[1])};
    return SECEDO_OK;
}

// The chromosome's records to the device in input order (bam_host.hpp), for the pileup, the split and the depth.
int upload_input_order(const ChrInput &ci, hipStream_t s, std::vector<uint64_t> *in_off, Order *ord,
                       Dev<uint8_t> *d_bytes, Dev<uint64_t> *d_in_off, Dev<uint16_t> *d_file, secedo_bam_times *t) {
    Clock::time_point t0 = Clock::now();
    std::vector<uint16_t> in_file;
    for (size_t f = 0; f < ci.roff.size(); ++f)
        for (size_t k = 0; k < ci.roff[f].size(); ++k) {
            in_off->push_back(ci.file_base[f] + ci.roff[f][k]);
            if (d_file) in_file.push_back(uint16_t(f));
            if (ord) ord->in_file.push_back(uint32_t(f));
            if (ord) ord->in_idx.push_back(ci.ridx[f][k]);
        }
    SECEDO_CALL(check_record_count(in_off->size()));
    const uint32_t n_in = uint32_t(in_off->size());
    if (t) t->walk_ms += ms_lap(t0);
    SECEDO_TRY(d_bytes->alloc(ci.bytes.size() + kRecordSlack));
    SECEDO_TRY(d_in_off->alloc(n_in));
    if (!ci.bytes.empty())
        SECEDO_TRY(hipMemcpyAsync(d_bytes->p, ci.bytes.data(), ci.bytes.size(), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemsetAsync(d_bytes->p + ci.bytes.size(), 0, kRecordSlack, s));
    if (n_in) SECEDO_TRY(hipMemcpyAsync(d_in_off->p, in_off->data(), n_in * 8ull, hipMemcpyHostToDevice, s));
    if (d_file) {
        SECEDO_TRY(d_file->alloc(n_in));
        if (n_in) SECEDO_TRY(hipMemcpyAsync(d_file->p, in_file.data(), n_in * 2ull, hipMemcpyHostToDevice, s));
    }
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_lap(t0);
    return SECEDO_OK;
}

// The selected (key, input ordinal) pairs of d_key / d_sel in input order (bam_host.hpp).
int compact_selected(const Dev<uint64_t> &d_key, Dev<uint32_t> &d_sel, uint32_t n, hipStream_t s, uint32_t *n_sel,
                     Dev<uint64_t> *d_kc, Dev<uint32_t> *d_vc) {
    using namespace secedo::bam;
    Dev<uint32_t> scan;
    Dev<uint8_t> tmp;
    const size_t tb = scan_bytes(uint64_t(n) + 1);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(scan.alloc(size_t(n) + 1));
    SECEDO_TRY(hipMemsetAsync(d_sel.p + n, 0, 4, s));
    SECEDO_TRY(exclusive_sum(tmp.p, tb, d_sel.p, scan.p, uint64_t(n) + 1, s));
    *n_sel = 0;
    SECEDO_TRY(hipMemcpyAsync(n_sel, scan.p + n, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    SECEDO_TRY(d_kc->alloc(*n_sel));
    SECEDO_TRY(d_vc->alloc(*n_sel));
    SECEDO_TRY(compact_keys(d_key.p, d_sel.p, scan.p, n, d_kc->p, d_vc->p, s));
    SECEDO_TRY(hipStreamSynchronize(s));  // scan and tmp go with this scope
    return SECEDO_OK;
}

// compact_selected, then sorted by key: -> *n_sel, d_ks, d_vs.
int compact_and_sort(const Dev<uint64_t> &d_key, Dev<uint32_t> &d_sel, uint32_t n, hipStream_t s, uint32_t *n_sel,
                     Dev<uint64_t> *d_ks, Dev<uint32_t> *d_vs) {
    using namespace secedo::bam;
    Dev<uint32_t> vc;
    Dev<uint64_t> kc;
    Dev<uint8_t> tmp;
    SECEDO_CALL(compact_selected(d_key, d_sel, n, s, n_sel, &kc, &vc));
    const uint32_t m = *n_sel;
    SECEDO_TRY(d_ks->alloc(m));
    SECEDO_TRY(d_vs->alloc(m));
    const size_t tb = sort_pairs_bytes(m);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(sort_pairs(tmp.p, tb, kc.p, d_ks->p, vc.p, d_vs->p, m, s));  // radix sort: stable
    SECEDO_TRY(hipStreamSynchronize(s));
    return SECEDO_OK;
}

// Rule 3d over the n >= 1 records rs: ends and scores -> templates by (cell, name) -> groups by key -> the drop flags
// (bam_host.hpp: duplicate_keep; bam_split.cpp runs it over its own view of the records).
int duplicate_keep(const bam::Records &rs, unsigned long long *d_stat, hipStream_t s, Dev<uint32_t> *keep_out) {
    using namespace secedo::bam;
    const uint32_t n = rs.n;
    Dev<uint32_t> &keep = *keep_out;
    Dev<uint64_t> key, key2, end, gkey, gks;
    Dev<uint32_t> val, val2, score, run, rep, extra, tscore, mate, sel, vs, grp;
    Dev<unsigned long long> best;
    Dev<uint8_t> tmp;
    const size_t tb = std::max(sort_pairs_bytes(n), scan_bytes(uint64_t(n) + 1));
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(key.alloc(n));
    SECEDO_TRY(key2.alloc(n));
    SECEDO_TRY(val.alloc(n));
    SECEDO_TRY(val2.alloc(n));
    SECEDO_TRY(end.alloc(n));
    SECEDO_TRY(score.alloc(n));
    SECEDO_TRY(ends_and_scores(rs, key.p, val.p, end.p, score.p, s));
    SECEDO_TRY(sort_pairs(tmp.p, tb, key.p, key2.p, val.p, val2.p, n, s));  // radix sort: stable
    SECEDO_TRY(run.alloc(n));
    SECEDO_TRY(rep.alloc(n));
    SECEDO_TRY(extra.alloc(n));
    SECEDO_TRY(tscore.alloc(n));
    SECEDO_TRY(mate.alloc(n));
    SECEDO_TRY(gkey.alloc(n));
    SECEDO_TRY(sel.alloc(n + 1));
    SECEDO_TRY(hipMemsetAsync(extra.p, 0, n * 4ull, s));
    SECEDO_TRY(hipMemsetAsync(tscore.p, 0, n * 4ull, s));
    SECEDO_TRY(hipMemsetAsync(mate.p, 0, n * 4ull, s));
    SECEDO_TRY(templates(rs, key2.p, val2.p, score.p, end.p, run.p, rep.p, extra.p, tscore.p, mate.p, gkey.p, sel.p,
                         d_stat, tmp.p, tb, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    key.reset();
    key2.reset();
    val.reset();
    val2.reset();
    score.reset();
    rep.reset();
    uint32_t m = 0;
    SECEDO_CALL(compact_and_sort(gkey, sel, n, s, &m, &gks, &vs));
    gkey.reset();
    sel.reset();
    SECEDO_TRY(grp.alloc(n));
    SECEDO_TRY(best.alloc(n));
    SECEDO_TRY(keep.alloc(n + 1));
    SECEDO_TRY(hipMemsetAsync(best.p, 0, n * 8ull, s));
    SECEDO_TRY(mark_duplicates(rs, gks.p, vs.p, m, extra.p, mate.p, end.p, tscore.p, run.p, grp.p, best.p, keep.p,
                               d_stat, tmp.p, tb, s));
    SECEDO_TRY(hipStreamSynchronize(s));  // the workspace above goes with this scope
    return SECEDO_OK;
}

}  // namespace bam_host
}  // namespace secedo

namespace {

// Tag mode: the records in input order go up, the device selects the listed cells and sorts them into the global
// order (chunk, cell, Position, file, record) -> d_off / d_cell of the selected records.
int order_by_cell(const ChrInput &ci, const CellList &L, const Select &sl, unsigned long long *d_stat, hipStream_t s,
                  Dev<uint8_t> *d_bytes, Dev<uint64_t> *d_off, Dev<uint16_t> *d_cell, Order *ord,
                  secedo_bam_times *t) {
    std::vector<uint64_t> in_off;
    Dev<uint64_t> d_in_off;
    SECEDO_CALL(upload_input_order(ci, s, &in_off, ord, d_bytes, &d_in_off, nullptr, t));
    const uint32_t n_in = uint32_t(in_off.size());
    const Clock::time_point t0 = Clock::now();
    Dev<uint64_t> key, ks;
    Dev<uint32_t> sel, vs;
    SECEDO_TRY(key.alloc(n_in));
    SECEDO_TRY(sel.alloc(n_in + 1));
    SECEDO_TRY(cells(d_bytes->p, d_in_off.p, n_in, L, sl.require, sl.exclude, key.p, sel.p, d_stat, s));
    uint32_t n = 0;
    SECEDO_CALL(compact_and_sort(key, sel, n_in, s, &n, &ks, &vs));
    key.reset();
    sel.reset();
    SECEDO_TRY(d_off->alloc(n));
    SECEDO_TRY(d_cell->alloc(n));
    SECEDO_TRY(ord->d_ord.alloc(n));
    SECEDO_TRY(order_records(ks.p, vs.p, d_in_off.p, n, d_off->p, d_cell->p, ord->d_ord.p, s));
    ord->n = n;
    if (n) {
        uint64_t k0 = 0, k1 = 0;
        SECEDO_TRY(hipMemcpyAsync(&k0, ks.p, 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(&k1, ks.p + n - 1, 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        ord->min_pos = int32_t(uint32_t(k0 >> 46) * kChunk);  // the first window starts at or before it
        ord->last_chunk = uint32_t(k1 >> 46);
    }
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) t->device_ms += ms_since(t0);
    return SECEDO_OK;
}

// Per-file mode: the global order (chunk of Position, file, record) built on the host, then uploaded.
int order_by_file(const ChrInput &ci, hipStream_t s, Dev<uint8_t> *d_bytes, Dev<uint64_t> *d_off,
                  Dev<uint16_t> *d_file, Order *ord, secedo_bam_times *t) {
    const size_t n_files = ci.roff.size();
    Clock::time_point t0 = Clock::now();
    // global order: chunk of Position, file, record
    int32_t max_pos = -1, min_pos = INT32_MAX;
    uint64_t n64 = 0;
    for (size_t f = 0; f < n_files; ++f) {
        n64 += ci.rpos[f].size();
        if (!ci.rpos[f].empty()) {
            max_pos = std::max(max_pos, ci.rpos[f].back());
            min_pos = std::min(min_pos, ci.rpos[f].front());
        }
    }
    SECEDO_CALL(check_record_count(n64));
    const uint32_t n = uint32_t(n64);
    const uint32_t last_chunk = max_pos < 0 ? 0 : uint32_t(max_pos) / kChunk;
    std::vector<uint64_t> &ord_off = ord->ord_off;
    std::vector<uint16_t> &ord_file = ord->ord_file;
    std::vector<uint64_t> &ord_idx = ord->ord_idx;
    ord_off.reserve(n);
    ord_file.reserve(n);
    ord_idx.reserve(n);
    {
        std::vector<size_t> cur(n_files, 0);
        for (uint32_t c = 0; c <= last_chunk; ++c)
            for (size_t f = 0; f < n_files; ++f)
                for (size_t &k = cur[f]; k < ci.rpos[f].size() && uint32_t(ci.rpos[f][k]) / kChunk == c; ++k) {
                    ord_off.push_back(ci.file_base[f] + ci.roff[f][k]);
                    ord_file.push_back(uint16_t(f));
                    ord_idx.push_back(ci.ridx[f][k]);
                }
    }
    if (t) t->walk_ms += ms_since(t0);
    t0 = Clock::now();
    SECEDO_TRY(d_bytes->alloc(ci.bytes.size()));
    SECEDO_TRY(d_off->alloc(n));
    SECEDO_TRY(d_file->alloc(n));
    if (!ci.bytes.empty())
        SECEDO_TRY(hipMemcpyAsync(d_bytes->p, ci.bytes.data(), ci.bytes.size(), hipMemcpyHostToDevice, s));
    if (n) {
        SECEDO_TRY(hipMemcpyAsync(d_off->p, ord_off.data(), n * 8ull, hipMemcpyHostToDevice, s));
        SECEDO_TRY(hipMemcpyAsync(d_file->p, ord_file.data(), n * 2ull, hipMemcpyHostToDevice, s));
    }
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_since(t0);
    ord->n = n;
    ord->min_pos = min_pos;
    ord->last_chunk = last_chunk;
    return SECEDO_OK;
}

// One chromosome on the device: its records in the global order and what the decode pass leaves for the windows.
struct ChrDev {
    Order ord;
    Dev<uint8_t> bytes;
    Dev<uint64_t> off;
    Dev<uint16_t> file;
    Dev<uint32_t> id, span_end;  // per record: its read id, the end of the span it touches
    Dev<uint8_t> pass;           // per record: the read filter
    uint32_t n_ids = 0;
    Records records() const { return Records{bytes.p, off.p, file.p, ord.n}; }
};

const char *decode_what(uint32_t code) {
    static const char *what[kErrCodes] = {"", "is not paired, not a proper pair or failed QC",
                                          "has a kept base at or past MAX_INSERT_SIZE after its chunk's end",
                                          "walks past the end of its CIGAR", "has a D op over a base",
                                          "reads past its quality string", "has a negative position"};
    return code < kErrCodes ? what[code] : "?";
}

// the decode pass's error (ordinal << 8 | code) as a message naming the input file and record
int decode_error(const Inputs &in, const Order &ord, bool tag_mode, unsigned long long err) {
    const uint32_t o = uint32_t(err >> 8), code = uint32_t(err & 0xFF);
    uint64_t file = 0, idx = 0;
    if (tag_mode) {  // the input file and record of ordinal o
        uint32_t i = 0;
        SECEDO_TRY(hipMemcpy(&i, ord.d_ord.p + o, 4, hipMemcpyDeviceToHost));
        file = ord.in_file[i];
        idx = ord.in_idx[i];
    } else {
        uint32_t i = o;  // the ordinal it had before rules 3c and 3d dropped records
        if (ord.d_ord.p) SECEDO_TRY(hipMemcpy(&i, ord.d_ord.p + o, 4, hipMemcpyDeviceToHost));
        file = ord.ord_file[i];
        idx = ord.ord_idx[i];
    }
    return fail(SECEDO_E_INVALID_ARG,
                record_where(in.paths[file], file, in.line0[file], idx, Stage::kDevice, in.indexed[file] != 0) + ": " +
                    decode_what(code));
}

// Phase 1: the decode pass over the ordered records, then the numbering of read names (cd->id, cd->n_ids); for the
// .map, which ordinals show a name first.
int decode_and_number(const Inputs &in, const Params &prm, bool tag_mode, bool want_map, hipStream_t s, ChrDev *cd,
                      ChrOut *co) {
    const uint32_t n = cd->ord.n;
    const Records rs = cd->records();
    Dev<uint64_t> key, key2;
    Dev<uint32_t> val, val2, run, rep, flag, scan;
    Dev<unsigned long long> err;
    SECEDO_TRY(key.alloc(n));
    SECEDO_TRY(key2.alloc(n));
    SECEDO_TRY(val.alloc(n));
    SECEDO_TRY(val2.alloc(n));
    SECEDO_TRY(run.alloc(n));
    SECEDO_TRY(rep.alloc(n));
    SECEDO_TRY(flag.alloc(n + 1));
    SECEDO_TRY(scan.alloc(n + 1));
    SECEDO_TRY(cd->id.alloc(n));
    SECEDO_TRY(cd->span_end.alloc(n));
    SECEDO_TRY(cd->pass.alloc(n));
    SECEDO_TRY(err.alloc(1));
    SECEDO_TRY(hipMemsetAsync(err.p, 0xFF, 8, s));
    SECEDO_TRY(decode(rs, prm, key.p, val.p, cd->pass.p, cd->span_end.p, err.p, s));
    unsigned long long h_err = 0;
    SECEDO_TRY(hipMemcpyAsync(&h_err, err.p, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (h_err != ~0ull) return decode_error(in, cd->ord, tag_mode, h_err);
    // name numbering
    Dev<uint8_t> tmp;
    size_t tmp_bytes = std::max(sort_pairs_bytes(n), scan_bytes(uint64_t(n) + 1));
    SECEDO_TRY(tmp.alloc(tmp_bytes));
    if (n) {
        SECEDO_TRY(sort_pairs(tmp.p, tmp_bytes, key.p, key2.p, val.p, val2.p, n, s));
        SECEDO_TRY(first_occurrence(rs, key2.p, val2.p, run.p, rep.p, flag.p, tmp.p, tmp_bytes, s));
        SECEDO_TRY(hipMemsetAsync(flag.p + n, 0, 4, s));
        SECEDO_TRY(exclusive_sum(tmp.p, tmp_bytes, flag.p, scan.p, uint64_t(n) + 1, s));
        SECEDO_TRY(assign_ids(rep.p, scan.p, cd->id.p, n, s));
        SECEDO_TRY(hipMemcpyAsync(&cd->n_ids, scan.p + n, 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
    }
    key.reset();
    key2.reset();
    val.reset();
    val2.reset();
    run.reset();
    rep.reset();
    if (want_map) {
        co->first.resize(n);
        co->id.resize(n);
        std::vector<uint32_t> fl(n);
        if (n) {
            SECEDO_TRY(hipMemcpyAsync(fl.data(), flag.p, n * 4ull, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipMemcpyAsync(co->id.data(), cd->id.p, n * 4ull, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
        }
        for (uint32_t o = 0; o < n; ++o) co->first[o] = uint8_t(fl[o]);
        if (tag_mode || cd->ord.d_ord.p) {
            co->ord_off.resize(n);
            if (n) SECEDO_TRY(hipMemcpy(co->ord_off.data(), cd->off.p, n * 8ull, hipMemcpyDeviceToHost));
        } else {
            co->ord_off = cd->ord.ord_off;
        }
    }
    return SECEDO_OK;
}

// Phase 2: windows of kWindow positions over [first window start, end of the last chunk): count, select the
// candidate loci, emit and sort their bases, and gather what each locus keeps onto the end of `res`.
int pile_windows(const ChrDev &cd, const Params &prm, const uint16_t *d_i2g, uint32_t n_groups, hipStream_t s,
                 Result *res) {
    const Records rs = cd.records();
    const uint64_t locus_base = res->n_loci;
    const uint64_t limit = uint64_t(cd.ord.last_chunk + 1) * kChunk;
    Dev<uint32_t> cnt, cand, cscan, cpos, ctot, fill, keep, kscan, flags;
    Dev<uint64_t> arr, ascan, carr, ekey, eval, ekey2, eval2, kept, escan;
    const uint32_t W = kWindow;
    SECEDO_TRY(cnt.alloc(size_t(W) * 4));
    SECEDO_TRY(cand.alloc(W + 1));
    SECEDO_TRY(cscan.alloc(W + 1));
    SECEDO_TRY(arr.alloc(W + 1));
    SECEDO_TRY(ascan.alloc(W + 1));
    SECEDO_TRY(flags.alloc(2));
    SECEDO_TRY(hipMemsetAsync(flags.p, 0, 8, s));
    size_t wtmp_bytes = scan_bytes(uint64_t(W) + 1);
    Dev<uint8_t> wtmp;
    SECEDO_TRY(wtmp.alloc(wtmp_bytes));
    for (uint64_t w0 = uint64_t(cd.ord.min_pos) / W * W; w0 < limit; w0 += W) {
        const uint32_t w1 = uint32_t(std::min<uint64_t>(w0 + W, limit));
        const uint32_t n_pos = w1 - uint32_t(w0);
        SECEDO_TRY(hipMemsetAsync(cnt.p, 0, size_t(n_pos) * 16, s));
        SECEDO_TRY(count(rs, prm, cd.pass.p, cd.span_end.p, uint32_t(w0), w1, cnt.p, s));
        SECEDO_TRY(select(cnt.p, prm, n_pos, cand.p, arr.p, s));
        SECEDO_TRY(hipMemsetAsync(cand.p + n_pos, 0, 4, s));
        SECEDO_TRY(hipMemsetAsync(arr.p + n_pos, 0, 8, s));
        SECEDO_TRY(exclusive_sum(wtmp.p, wtmp_bytes, cand.p, cscan.p, uint64_t(n_pos) + 1, s));
        SECEDO_TRY(exclusive_sum64(wtmp.p, wtmp_bytes, arr.p, ascan.p, uint64_t(n_pos) + 1, s));
        uint32_t n_cand = 0;
        uint64_t n_arr = 0;
        SECEDO_TRY(hipMemcpyAsync(&n_cand, cscan.p + n_pos, 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(&n_arr, ascan.p + n_pos, 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        if (n_cand == 0) continue;
        SECEDO_TRY(cpos.alloc(n_cand));
        SECEDO_TRY(ctot.alloc(n_cand));
        SECEDO_TRY(carr.alloc(n_cand));
        SECEDO_TRY(fill.alloc(n_cand));
        SECEDO_TRY(compact_candidates(cnt.p, cand.p, cscan.p, ascan.p, uint32_t(w0), n_pos, cpos.p, carr.p,
                                   ctot.p, s));
        SECEDO_TRY(hipMemsetAsync(fill.p, 0, n_cand * 4ull, s));
        SECEDO_TRY(ekey.alloc(n_arr));
        SECEDO_TRY(eval.alloc(n_arr));
        SECEDO_TRY(ekey2.alloc(n_arr));
        SECEDO_TRY(eval2.alloc(n_arr));
        SECEDO_TRY(emit(rs, prm, cd.pass.p, cd.span_end.p, cd.id.p, uint32_t(w0), w1, cand.p, cscan.p, ascan.p, fill.p,
                     ekey.p, eval.p, s));
        int bits = 32;
        while (bits < 64 && (uint64_t(n_cand - 1) >> (bits - 32)) != 0) ++bits;
        const size_t sb = sort_pairs64_bytes(n_arr), cb = scan_bytes(uint64_t(n_cand) + 1);
        Dev<uint8_t> stmp;
        SECEDO_TRY(stmp.alloc(std::max(sb, cb)));
        SECEDO_TRY(sort_pairs64(stmp.p, sb, ekey.p, ekey2.p, eval.p, eval2.p, n_arr, bits, s));
        ekey.reset();
        eval.reset();
        ekey2.reset();
        SECEDO_TRY(keep.alloc(n_cand + 1));
        SECEDO_TRY(kscan.alloc(n_cand + 1));
        SECEDO_TRY(kept.alloc(n_cand + 1));
        SECEDO_TRY(escan.alloc(n_cand + 1));
        SECEDO_TRY(finalize(eval2.p, carr.p, ctot.p, prm, n_cand, keep.p, kept.p, s));
        SECEDO_TRY(hipMemsetAsync(keep.p + n_cand, 0, 4, s));
        SECEDO_TRY(hipMemsetAsync(kept.p + n_cand, 0, 8, s));
        SECEDO_TRY(exclusive_sum(stmp.p, cb, keep.p, kscan.p, uint64_t(n_cand) + 1, s));
        SECEDO_TRY(exclusive_sum64(stmp.p, cb, kept.p, escan.p, uint64_t(n_cand) + 1, s));
        uint32_t n_keep = 0;
        uint64_t n_kept = 0;
        SECEDO_TRY(hipMemcpyAsync(&n_keep, kscan.p + n_cand, 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(&n_kept, escan.p + n_cand, 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        if (n_keep) {
            SECEDO_TRY(res->pos.grow(res->n_loci + n_keep, res->n_loci, s));
            SECEDO_TRY(res->off.grow(res->n_loci + n_keep + 1, res->n_loci + 1, s));
            SECEDO_TRY(res->rid.grow(res->n_entries + n_kept, res->n_entries, s));
            SECEDO_TRY(res->idb.grow(res->n_entries + n_kept, res->n_entries, s));
            SECEDO_TRY(gather(eval2.p, cpos.p, carr.p, ctot.p, keep.p, kscan.p, escan.p, n_cand, d_i2g, n_groups,
                           res->pos.p + res->n_loci, res->off.p + res->n_loci, res->rid.p + res->n_entries,
                           res->idb.p + res->n_entries, res->n_entries, flags.p, s));
            res->n_loci += n_keep;
            res->n_entries += n_kept;
        }
        eval2.reset();
    }
    uint32_t h_flags[2] = {0, 0};
    SECEDO_TRY(hipMemcpyAsync(h_flags, flags.p, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (h_flags[0]) return fail(SECEDO_E_INVALID_ARG, "a cell id is too large for the id_to_group mapping");
    if (res->n_loci > locus_base) res->num_cells = std::max(res->num_cells, h_flags[1] + 1);
    return SECEDO_OK;
}

// Phase 3: the reader's max_read_length over the loci this chromosome added (those from locus_base on)
int max_read_length(const ChrDev &cd, uint64_t locus_base, hipStream_t s, Result *res) {
    const uint32_t n_ids = cd.n_ids;
    const uint64_t n_new = res->n_loci - locus_base;
    if (n_new == 0) return SECEDO_OK;
    Dev<uint32_t> mn, mx, ml;
    SECEDO_TRY(mn.alloc(n_ids));
    SECEDO_TRY(mx.alloc(n_ids));
    SECEDO_TRY(ml.alloc(1));
    SECEDO_TRY(hipMemsetAsync(mn.p, 0xFF, n_ids * 4ull, s));
    SECEDO_TRY(hipMemsetAsync(mx.p, 0, n_ids * 4ull, s));
    SECEDO_TRY(hipMemsetAsync(ml.p, 0, 4, s));
    SECEDO_TRY(read_stats(res->pos.p + locus_base, res->off.p + locus_base, res->rid.p, uint32_t(n_new), mn.p,
                       mx.p, n_ids, ml.p, s));
    uint32_t h_ml = 0;
    SECEDO_TRY(hipMemcpyAsync(&h_ml, ml.p, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    res->max_read_length = std::max(res->max_read_length, h_ml);
    return SECEDO_OK;
}

// The records with keep[o] != 0 (keep: [n + 1]) become the chromosome's Records, in the same order; Order follows:
// d_ord names the ordinal each survivor had before, the chunks are those of the first and the last survivor.
int compact_chr(const ChrInput &ci, Dev<uint32_t> &keep, hipStream_t s, ChrDev *cd) {
    const uint32_t n = cd->ord.n;
    Dev<uint32_t> scan, ord2;
    Dev<uint64_t> off2;
    Dev<uint16_t> file2;
    Dev<uint8_t> tmp;
    const size_t tb = scan_bytes(uint64_t(n) + 1);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(scan.alloc(n + 1));
    SECEDO_TRY(hipMemsetAsync(keep.p + n, 0, 4, s));
    SECEDO_TRY(exclusive_sum(tmp.p, tb, keep.p, scan.p, uint64_t(n) + 1, s));
    uint32_t m = 0;
    SECEDO_TRY(hipMemcpyAsync(&m, scan.p + n, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (m == n) return SECEDO_OK;
    SECEDO_TRY(off2.alloc(m));
    SECEDO_TRY(file2.alloc(m));
    SECEDO_TRY(ord2.alloc(m));
    SECEDO_TRY(compact_records(cd->records(), cd->ord.d_ord.p, keep.p, scan.p, off2.p, file2.p, ord2.p, s));
    uint64_t ends[2] = {0, 0};
    if (m) {
        SECEDO_TRY(hipMemcpyAsync(&ends[0], off2.p, 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(&ends[1], off2.p + m - 1, 8, hipMemcpyDeviceToHost, s));
    }
    SECEDO_TRY(hipStreamSynchronize(s));
    std::swap(cd->off.p, off2.p), std::swap(cd->off.n, off2.n);
    std::swap(cd->file.p, file2.p), std::swap(cd->file.n, file2.n);
    std::swap(cd->ord.d_ord.p, ord2.p), std::swap(cd->ord.d_ord.n, ord2.n);
    cd->ord.n = m;
    cd->ord.min_pos = INT32_MAX;
    cd->ord.last_chunk = 0;
    if (m) {  // the order starts with the chunk: the first survivor is in the first chunk, the last in the last
        const auto chunk_of = [&](uint64_t off) { return rd32(ci.bytes.data() + off + 4 + 4) / kChunk; };
        cd->ord.min_pos = int32_t(chunk_of(ends[0]) * kChunk);  // the first window starts at or before it
        cd->ord.last_chunk = chunk_of(ends[1]);
    }
    return SECEDO_OK;
}

// Rule 3c in per-file mode (tag mode folds it into the cells pass): flag test, scan, compaction.
int filter_flags(const ChrInput &ci, const Select &sl, unsigned long long *d_stat, hipStream_t s, ChrDev *cd) {
    const uint32_t n = cd->ord.n;
    if (n == 0) return SECEDO_OK;
    Dev<uint32_t> keep;
    SECEDO_TRY(keep.alloc(n + 1));
    SECEDO_TRY(flag_test(cd->records(), sl.require, sl.exclude, keep.p, d_stat, s));
    return compact_chr(ci, keep, s, cd);
}

// Rule 3d: the drop flags of duplicate_keep -> compaction.
int remove_duplicates(const ChrInput &ci, unsigned long long *d_stat, hipStream_t s, ChrDev *cd) {
    if (cd->ord.n == 0) return SECEDO_OK;
    Dev<uint32_t> keep;
    SECEDO_CALL(duplicate_keep(cd->records(), d_stat, s, &keep));
    return compact_chr(ci, keep, s, cd);
}

// The device passes of one chromosome, appended to `res`. cells: tag mode's list, or null for per-file mode.
int run_chromosome(const Inputs &in, const ChrInput &ci, const Params &prm, const CellList *cells, const Select &sl,
                   const uint16_t *d_i2g, uint32_t n_groups, bool want_map, hipStream_t s, Result *res, ChrOut *co,
                   secedo_bam_times *t) {
    ChrDev cd;
    SelStat stat;  // stays unallocated with rules 3c and 3d off
    if (sl.filter() || sl.dedup) SECEDO_CALL(stat.init(s));
    if (cells)
        SECEDO_CALL(order_by_cell(ci, *cells, sl, sl.filter() ? stat.d.p : nullptr, s, &cd.bytes, &cd.off, &cd.file,
                                  &cd.ord, t));
    else SECEDO_CALL(order_by_file(ci, s, &cd.bytes, &cd.off, &cd.file, &cd.ord, t));
    const Clock::time_point t0 = Clock::now();
    if (sl.filter() && !cells) SECEDO_CALL(filter_flags(ci, sl, stat.d.p, s, &cd));
    if (sl.dedup) SECEDO_CALL(remove_duplicates(ci, stat.d.p, s, &cd));
    SECEDO_CALL(stat.add_to(s, &g_select));
    const uint64_t locus_base = res->n_loci;
    SECEDO_CALL(decode_and_number(in, prm, cells != nullptr, want_map, s, &cd, co));
    if (cd.ord.n) SECEDO_CALL(pile_windows(cd, prm, d_i2g, n_groups, s, res));
    SECEDO_CALL(max_read_length(cd, locus_base, s, res));
    if (t) t->device_ms += ms_since(t0);
    return SECEDO_OK;
}

std::string name_at(const ChrInput &ci, uint64_t off) {
    const uint8_t *c = ci.bytes.data() + off + 4;
    const char *nm = reinterpret_cast<const char *>(c + 32);
    return std::string(nm, strnlen(nm, c[8]));
}

int write_files(const std::string &prefix, bool text, uint32_t chromosome_id, const ChrInput &ci, const ChrOut &co,
                const std::vector<uint32_t> &pos, const std::vector<uint64_t> &off, const std::vector<uint32_t> &rid,
                const std::vector<uint16_t> &idb) {
    FILE *fm = fopen((prefix + ".map").c_str(), "wb");
    if (!fm) return fail(SECEDO_E_INVALID_ARG, "Could not write " + prefix + ".map");
    std::string buf;
    for (size_t o = 0; o < co.first.size(); ++o)
        if (co.first[o]) buf += name_at(ci, co.ord_off[o]) + "\t" + std::to_string(co.id[o]) + "\n";
    fwrite(buf.data(), 1, buf.size(), fm);
    fclose(fm);
    FILE *fb = fopen((prefix + ".bin").c_str(), "wb");
    FILE *ft = fopen((prefix + ".txt").c_str(), "wb");
    if (!fb || !ft) {
        if (fb) fclose(fb);
        if (ft) fclose(ft);
        return fail(SECEDO_E_INVALID_ARG, "Could not write " + prefix + ".bin/.txt");
    }
    std::string bin, txt;
    static const char kIntToChar[4] = {'A', 'C', 'G', 'T'};
    std::vector<std::pair<uint16_t, uint32_t>> e;
    for (size_t l = 0; l < pos.size(); ++l) {
        const uint64_t b = off[l], en = off[l + 1];
        const uint16_t cov = uint16_t(en - b);
        bin.append(reinterpret_cast<const char *>(&pos[l]), 4);
        bin.append(reinterpret_cast<const char *>(&cov), 2);
        bin.append(reinterpret_cast<const char *>(&rid[b]), cov * 4ull);
        bin.append(reinterpret_cast<const char *>(&idb[b]), cov * 2ull);
        if (text) {
            e.clear();
            for (uint64_t k = b; k < en; ++k) e.emplace_back(idb[k], rid[k]);
            std::stable_sort(e.begin(), e.end(), [](const auto &x, const auto &y) { return (x.first >> 2) < (y.first >> 2); });
            txt += std::to_string(chromosome_id + 1) + "\t" + std::to_string(pos[l]) + "\t" + std::to_string(cov) + "\t";
            for (auto &x : e) txt += kIntToChar[x.first & 3];
            txt += '\t';
            for (size_t k = 0; k < e.size(); ++k) txt += (k ? "," : "") + std::to_string(e[k].first >> 2);
            txt += '\t';
            for (size_t k = 0; k < e.size(); ++k) txt += (k ? "," : "") + std::to_string(e[k].second);
            txt += '\n';
        }
        if (bin.size() > (16u << 20)) {
            fwrite(bin.data(), 1, bin.size(), fb);
            bin.clear();
        }
        if (txt.size() > (16u << 20)) {
            fwrite(txt.data(), 1, txt.size(), ft);
            txt.clear();
        }
    }
    fwrite(bin.data(), 1, bin.size(), fb);
    fwrite(txt.data(), 1, txt.size(), ft);
    const bool ok = fclose(fb) == 0;
    return (fclose(ft) == 0 && ok) ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, "Could not write " + prefix);
}

}  // namespace

namespace secedo {
namespace bam_host {

// tag: two characters [A-Za-z][A-Za-z0-9] (SAM spec 1.5)
int check_tag(const char *tag) {
    if (!tag) return fail(SECEDO_E_INVALID_ARG, "null tag");
    const auto alpha = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); };
    if (!alpha(tag[0]) || !(alpha(tag[1]) || (tag[1] >= '0' && tag[1] <= '9')))
        return fail(SECEDO_E_INVALID_ARG, "a tag is two characters [A-Za-z][A-Za-z0-9]");
    return SECEDO_OK;
}

// the barcode list of tag mode: non-empty, at most SECEDO_BAM_MAX_FILES, no value twice
int check_cells(const char *tag, const char *const *barcodes, uint32_t n, std::vector<std::string> *values) {
    SECEDO_CALL(check_tag(tag));
    if (n == 0 || !barcodes) return fail(SECEDO_E_INVALID_ARG, "an empty barcode list");
    if (n > SECEDO_BAM_MAX_FILES)
        return fail(SECEDO_E_LIMIT, "more than 16384 barcodes: cell ids do not fit cell << 2 | base in 16 bits");
    std::set<std::string> seen;
    for (uint32_t c = 0; c < n; ++c) {
        if (!barcodes[c]) return fail(SECEDO_E_INVALID_ARG, "null barcode");
        values->emplace_back(barcodes[c]);
        if (!seen.insert(values->back()).second)
            return fail(SECEDO_E_INVALID_ARG, "barcode " + values->back() + " is listed twice");
    }
    return SECEDO_OK;
}

int check_files(const char *const *bam_files, uint32_t n_files, std::vector<std::string> *files) {
    for (uint32_t f = 0; f < n_files; ++f) {
        if (!bam_files[f]) return fail(SECEDO_E_INVALID_ARG, "null file name");
        files->emplace_back(bam_files[f]);
    }
    return SECEDO_OK;
}

}  // namespace bam_host
}  // namespace secedo

namespace {

// What one pileup call asks for; the four entry points differ in the chromosome list, the output files and the tag.
struct Request {
    const char *const *bam_files;
    uint32_t n_files;
    const uint32_t *chromosome_ids;
    uint32_t n_chr;
    const char *out_pileup = nullptr;  // null: the result stays on the device only
    bool text = false;
    Params params{};  // chromosome is set per chromosome
    uint32_t num_threads = 1;
    const uint16_t *id_to_group = nullptr;
    uint32_t n_ids = 0;
    const char *tag = nullptr;  // null: per-file mode (cell = file index); else tag mode with the listed barcodes
    const char *const *barcodes = nullptr;
    uint32_t n_barcodes = 0;

    Request(const char *const *files, uint32_t nf, const uint32_t *chrs, uint32_t nc, uint32_t max_coverage,
            uint32_t min_base_quality, uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t threads,
            uint16_t min_different)
        : bam_files(files), n_files(nf), chromosome_ids(chrs), n_chr(nc), num_threads(threads) {
        params.max_coverage = max_coverage;
        params.min_base_quality = min_base_quality;
        params.min_map_quality = min_map_quality;
        params.min_alignment_score = min_alignment_score;
        params.min_different = min_different;
    }
};

// one chromosome's share of the result, fetched and written to the .bin / .map / .txt files
int write_chromosome(const Request &rq, uint32_t c, const ChrInput &ci, const ChrOut &co, const Result &res,
                     uint64_t l0, uint64_t e0) {
    const uint64_t nl = res.n_loci - l0, ne = res.n_entries - e0;
    std::vector<uint32_t> pos(nl), rid(ne);
    std::vector<uint64_t> off(nl + 1);
    std::vector<uint16_t> idb(ne);
    if (nl) {
        SECEDO_TRY(hipMemcpy(pos.data(), res.pos.p + l0, nl * 4, hipMemcpyDeviceToHost));
        SECEDO_TRY(hipMemcpy(off.data(), res.off.p + l0, (nl + 1) * 8, hipMemcpyDeviceToHost));
        SECEDO_TRY(hipMemcpy(rid.data(), res.rid.p + e0, ne * 4, hipMemcpyDeviceToHost));
        SECEDO_TRY(hipMemcpy(idb.data(), res.idb.p + e0, ne * 2, hipMemcpyDeviceToHost));
        for (auto &o : off) o -= e0;
    }
    return write_files(rq.out_pileup, rq.text, rq.chromosome_ids[c], ci, co, pos, off, rid, idb);
}

int run(const Request &rq, secedo_bam_result_info *info, secedo_bam_times *times) {
    const Clock::time_point t_all = Clock::now();
    secedo_bam_times tl{};
    if (!info || (rq.n_files && !rq.bam_files) || (rq.n_chr && !rq.chromosome_ids))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    std::vector<std::string> values;
    if (rq.tag) SECEDO_CALL(check_cells(rq.tag, rq.barcodes, rq.n_barcodes, &values));
    else if (rq.n_files > SECEDO_BAM_MAX_FILES)
        return fail(SECEDO_E_LIMIT, "more than 16384 BAM files: cell ids do not fit cell << 2 | base in 16 bits");
    std::vector<std::string> files;
    SECEDO_CALL(check_files(rq.bam_files, rq.n_files, &files));
    g_select = secedo_bam_select_info{};
    Select sl;
    SECEDO_CALL(current_select(&sl));
    delete g_result;
    g_result = new Result();
    Result *res = g_result;
    Inputs in;
    SECEDO_CALL(load_inputs(files, rq.chromosome_ids, rq.n_chr, rq.num_threads ? rq.num_threads : 1, &in, &tl));
    StreamGuard guard;
    SECEDO_TRY(hipStreamCreateWithFlags(&guard.s, hipStreamNonBlocking));
    const hipStream_t s = guard.s;
    Dev<uint16_t> d_i2g;
    if (rq.id_to_group) {
        SECEDO_TRY(d_i2g.alloc(rq.n_ids));
        if (rq.n_ids) SECEDO_TRY(hipMemcpy(d_i2g.p, rq.id_to_group, rq.n_ids * 2ull, hipMemcpyHostToDevice));
    }
    DevCells dc;
    if (rq.tag) SECEDO_CALL(upload_cells(rq.tag, values, s, &dc));
    SECEDO_TRY(res->off.grow(1, 0, s));
    SECEDO_TRY(hipMemsetAsync(res->off.p, 0, 8, s));
    for (uint32_t c = 0; c < rq.n_chr; ++c) {
        Params p = rq.params;
        p.chromosome = rq.chromosome_ids[c];
        ChrOut co;
        const uint64_t l0 = res->n_loci, e0 = res->n_entries;
        SECEDO_CALL(run_chromosome(in, in.chrs[c], p, rq.tag ? &dc.list : nullptr, sl,
                                   rq.id_to_group ? d_i2g.p : nullptr, rq.n_ids, rq.out_pileup != nullptr, s, res,
                                   &co, &tl));
        res->chr_locus_off.push_back(uint32_t(res->n_loci));
        if (rq.out_pileup) {
            const Clock::time_point t0 = Clock::now();
            SECEDO_CALL(write_chromosome(rq, c, in.chrs[c], co, *res, l0, e0));
            tl.write_ms += ms_since(t0);
        }
        std::vector<uint8_t>().swap(in.chrs[c].bytes);
    }
    info->n_loci = res->n_loci;
    info->n_entries = res->n_entries;
    info->n_chr = rq.n_chr;
    info->num_cells = res->num_cells;
    info->max_read_length = res->max_read_length;
    info->reserved = 0;
    tl.total_ms = ms_since(t_all);
    if (times) *times = tl;
    return SECEDO_OK;
}

// the distinct tag values over the requested chromosomes, sorted bytewise, and their record counts
struct Barcodes {
    std::vector<std::string> values;
    std::vector<uint64_t> counts;
};

thread_local Barcodes *g_barcodes = nullptr;

// one chromosome's distinct values (device: hash, sort, exact split of equal-hash runs) added to `acc`
int count_values(const ChrInput &ci, const char *tag, const Select &sl, hipStream_t s,
                 std::map<std::string, uint64_t> *acc) {
    std::vector<uint64_t> in_off;
    Dev<uint8_t> d_bytes, tmp;
    Dev<uint64_t> d_in_off, key, ks, voff;
    Dev<uint32_t> sel, vs, run, cnt, vlen;
    SECEDO_CALL(upload_input_order(ci, s, &in_off, nullptr, &d_bytes, &d_in_off, nullptr, nullptr));
    const uint32_t n_in = uint32_t(in_off.size());
    if (n_in == 0) return SECEDO_OK;
    SECEDO_TRY(key.alloc(n_in));
    SECEDO_TRY(sel.alloc(n_in + 1));
    const uint8_t t0 = uint8_t(tag[0]), t1 = uint8_t(tag[1]);
    SelStat stat;
    if (sl.filter()) SECEDO_CALL(stat.init(s));
    SECEDO_TRY(tag_keys(d_bytes.p, d_in_off.p, n_in, t0, t1, sl.require, sl.exclude, key.p, sel.p, stat.d.p, s));
    uint32_t n = 0;
    SECEDO_CALL(compact_and_sort(key, sel, n_in, s, &n, &ks, &vs));
    SECEDO_CALL(stat.add_to(s, &g_select));
    if (n == 0) return SECEDO_OK;
    const size_t tb = scan_bytes(n);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(run.alloc(n));
    SECEDO_TRY(cnt.alloc(n));
    SECEDO_TRY(hipMemsetAsync(cnt.p, 0, n * 4ull, s));
    SECEDO_TRY(tag_count(d_bytes.p, d_in_off.p, t0, t1, ks.p, vs.p, run.p, n, cnt.p, tmp.p, tb, s));
    std::vector<uint32_t> h_cnt(n), h_val(n);
    SECEDO_TRY(hipMemcpyAsync(h_cnt.data(), cnt.p, n * 4ull, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(h_val.data(), vs.p, n * 4ull, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    for (uint32_t j = 0; j < n; ++j) {
        if (!h_cnt[j]) continue;
        // the value of the record that first showed it: the first aux field named by the tag, Z-typed (the device
        // pass found it there)
        const uint8_t *rec = ci.bytes.data() + in_off[h_val[j]];
        const uint32_t bs = rd32(rec);
        const uint8_t *c = rec + 4;
        const uint64_t aux = rec_aux_off(c);
        const std::string v = first_z_value(c + aux, bs - aux, tag);
        (*acc)[v] += h_cnt[j];
    }
    return SECEDO_OK;
}

}  // namespace

extern "C" {

const char *secedo_bam_last_error(void) { return g_error.c_str(); }

int secedo_bam_set_read_filter(uint32_t require, uint32_t exclude) {
    SECEDO_CALL(check_read_filter("secedo_bam_set_read_filter", require, exclude));
    g_read_filter.store(int64_t(require) << 16 | exclude);
    return SECEDO_OK;
}

int secedo_bam_get_read_filter(uint32_t *require, uint32_t *exclude) {
    if (!require || !exclude) return fail(SECEDO_E_INVALID_ARG, "null argument");
    return read_filter(require, exclude);
}

int secedo_bam_set_duplicates(int mode) {
    if (mode != SECEDO_BAM_DUPLICATES_KEEP && mode != SECEDO_BAM_DUPLICATES_REMOVE)
        return fail(SECEDO_E_INVALID_ARG, "secedo_bam_set_duplicates: mode " + std::to_string(mode) +
                                              " is neither SECEDO_BAM_DUPLICATES_KEEP nor SECEDO_BAM_DUPLICATES_REMOVE");
    g_duplicates.store(mode);
    return SECEDO_OK;
}

int secedo_bam_get_duplicates(int *mode) {
    if (!mode) return fail(SECEDO_E_INVALID_ARG, "null argument");
    return duplicates_mode(mode);
}

int secedo_bam_select_stats(secedo_bam_select_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = g_select;
    return SECEDO_OK;
}

int secedo_pileup_bams(const char *const *bam_files, uint32_t n_files, const char *out_pileup, int write_text_file,
                       uint32_t chromosome_id, uint32_t max_coverage, uint32_t min_base_quality,
                       uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                       uint16_t min_different, secedo_bam_result_info *info, secedo_bam_times *times) {
    Request rq(bam_files, n_files, &chromosome_id, 1, max_coverage, min_base_quality, min_map_quality,
               min_alignment_score, num_threads, min_different);
    rq.out_pileup = out_pileup;
    rq.text = write_text_file != 0;
    return run(rq, info, times);
}

int secedo_pileup_bams_device(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                              uint32_t n_chr, uint32_t max_coverage, uint32_t min_base_quality,
                              uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                              uint16_t min_different, const uint16_t *id_to_group, uint32_t n_ids,
                              secedo_bam_result_info *info, secedo_bam_times *times) {
    Request rq(bam_files, n_files, chromosome_ids, n_chr, max_coverage, min_base_quality, min_map_quality,
               min_alignment_score, num_threads, min_different);
    rq.id_to_group = id_to_group;
    rq.n_ids = n_ids;
    return run(rq, info, times);
}

int secedo_pileup_bams_cells(const char *const *bam_files, uint32_t n_files, const char *out_pileup,
                             int write_text_file, uint32_t chromosome_id, uint32_t max_coverage,
                             uint32_t min_base_quality, uint32_t min_map_quality, uint32_t min_alignment_score,
                             uint32_t num_threads, uint16_t min_different, const char tag[2],
                             const char *const *barcodes, uint32_t n_barcodes, secedo_bam_result_info *info,
                             secedo_bam_times *times) {
    if (!tag) return fail(SECEDO_E_INVALID_ARG, "null tag");
    Request rq(bam_files, n_files, &chromosome_id, 1, max_coverage, min_base_quality, min_map_quality,
               min_alignment_score, num_threads, min_different);
    rq.out_pileup = out_pileup;
    rq.text = write_text_file != 0;
    rq.tag = tag;
    rq.barcodes = barcodes;
    rq.n_barcodes = n_barcodes;
    return run(rq, info, times);
}

int secedo_pileup_bams_cells_device(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                                    uint32_t n_chr, uint32_t max_coverage, uint32_t min_base_quality,
                                    uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                                    uint16_t min_different, const uint16_t *id_to_group, uint32_t n_ids,
                                    const char tag[2], const char *const *barcodes, uint32_t n_barcodes,
                                    secedo_bam_result_info *info, secedo_bam_times *times) {
    if (!tag) return fail(SECEDO_E_INVALID_ARG, "null tag");
    Request rq(bam_files, n_files, chromosome_ids, n_chr, max_coverage, min_base_quality, min_map_quality,
               min_alignment_score, num_threads, min_different);
    rq.id_to_group = id_to_group;
    rq.n_ids = n_ids;
    rq.tag = tag;
    rq.barcodes = barcodes;
    rq.n_barcodes = n_barcodes;
    return run(rq, info, times);
}

// the distinct tag values over the requested chromosomes and their record counts, kept for secedo_bam_barcodes_fetch
int secedo_bam_barcodes(const char *const *bam_files, uint32_t n_files, const char tag[2],
                        const uint32_t *chromosome_ids, uint32_t n_chr, uint32_t num_threads, uint32_t *n_values,
                        uint64_t *bytes) {
    if (!n_values || !bytes || (n_files && !bam_files) || (n_chr && !chromosome_ids))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    SECEDO_CALL(check_tag(tag));
    std::vector<std::string> files;
    SECEDO_CALL(check_files(bam_files, n_files, &files));
    delete g_barcodes;
    g_barcodes = nullptr;
    g_select = secedo_bam_select_info{};
    Select sl;
    SECEDO_CALL(current_select(&sl));  // the census honours rule 3c only
    Inputs in;
    SECEDO_CALL(load_inputs(files, chromosome_ids, n_chr, num_threads ? num_threads : 1, &in, nullptr));
    StreamGuard guard;
    SECEDO_TRY(hipStreamCreateWithFlags(&guard.s, hipStreamNonBlocking));
    std::map<std::string, uint64_t> acc;
    for (uint32_t c = 0; c < n_chr; ++c) {
        SECEDO_CALL(count_values(in.chrs[c], tag, sl, guard.s, &acc));
        std::vector<uint8_t>().swap(in.chrs[c].bytes);
    }
    if (acc.size() > UINT32_MAX) return fail(SECEDO_E_LIMIT, "more than 2^32 distinct values");
    Barcodes *b = new Barcodes();
    uint64_t total = 0;
    for (const auto &kv : acc) {
        b->values.push_back(kv.first);
        b->counts.push_back(kv.second);
        total += kv.first.size();
    }
    g_barcodes = b;
    *n_values = uint32_t(b->values.size());
    *bytes = total;
    return SECEDO_OK;
}

int secedo_bam_barcodes_fetch(char *values, uint64_t *value_off, uint64_t *counts) {
    const Barcodes *b = g_barcodes;
    if (!b) return fail(SECEDO_E_STATE, "no secedo_bam_barcodes result on this thread");
    uint64_t o = 0;
    for (size_t k = 0; k < b->values.size(); ++k) {
        if (values) std::memcpy(values + o, b->values[k].data(), b->values[k].size());
        if (value_off) value_off[k] = o;
        if (counts) counts[k] = b->counts[k];
        o += b->values[k].size();
    }
    if (value_off) value_off[b->values.size()] = o;
    return SECEDO_OK;
}

int secedo_bam_fetch(uint32_t *chr_locus_off, uint32_t *locus_pos, uint64_t *locus_entry_off, uint32_t *read_ids,
                     uint16_t *id_base16) {
    const Result *r = g_result;
    if (!r) return fail(SECEDO_E_STATE, "no pileup_bams result on this thread");
    if (chr_locus_off)
        SECEDO_TRY(hipMemcpy(chr_locus_off, r->chr_locus_off.data(), r->chr_locus_off.size() * 4, hipMemcpyDefault));
    if (locus_pos && r->n_loci) SECEDO_TRY(hipMemcpy(locus_pos, r->pos.p, r->n_loci * 4, hipMemcpyDefault));
    if (locus_entry_off) SECEDO_TRY(hipMemcpy(locus_entry_off, r->off.p, (r->n_loci + 1) * 8, hipMemcpyDefault));
    if (read_ids && r->n_entries) SECEDO_TRY(hipMemcpy(read_ids, r->rid.p, r->n_entries * 4, hipMemcpyDefault));
    if (id_base16 && r->n_entries) SECEDO_TRY(hipMemcpy(id_base16, r->idb.p, r->n_entries * 2, hipMemcpyDefault));
    return SECEDO_OK;
}

void secedo_bam_release(void) {
    delete g_result;
    g_result = nullptr;
    release_inflated();
    release_depth();
}

}  // extern "C"
