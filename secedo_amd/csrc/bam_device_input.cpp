// bam_device_input.cpp -- the opt-in device route for BAM input (secedo_bam_set_inflate, SECEDO_BAM_INFLATE=device):
// what bam_input.cpp's host pool and host walk give, from the device inflate (bgzf_kernels.hip) and the device walk
// (bam_walk_kernels.hip). Only compressed bytes go up; of the inflated bytes only the records of the requested
// chromosomes come back, with the roff / rpos / ridx arrays the host walk's FileSink builds.
//
// Per file the host lists the BGZF members and inflates the leading ones with zlib until the header and reference
// list are complete; what those members hold past the first record is the file's first carry. Small files go many to
// a batch: their compressed bytes are staged in one pinned buffer and go up in one copy, one descriptor table spans
// their members, one launch inflates them into one buffer, and the walk has one chain per file. A file that inflates
// to more than a batch goes alone, in ranges of members of about a batch; the cut record at a range's end is carried
// to the front of the next range, device to device. The stream is synchronised a fixed number of times per batch.
//
// A file read through its index (bam_host.hpp's IndexPlan) has one chain per span instead of one per file: the chain
// enters at the span's first record inside its first member and its bytes end at the span's limit. The spans of a
// file go one after another, span k of every file of the call in the same batches (the first spans together with the
// files read in full), so many small files still share one upload, one inflate launch and one walk; the file's walk state (record count, last record, runs) passes from span
// to span as it passes from range to range. A span larger than a batch goes alone, in ranges of members.
//
// secedo_bam_index_build (at the end of the file) sends files through the same batches and ranges with no chromosome
// requested, and after each batch's walk the index pass of bam_index_kernels.hip over its records: the heads of the
// (RefID, bin) runs and the touched windows come back with file-linear offsets, the file's member table turns them into
// virtual offsets, and bam_index_build.hpp's builder of the file takes them.
#include "bam_host.hpp"
#include "bam_index_build.hpp"
#include "bam_index_kernels.hpp"
#include "bam_kernels.hpp"  // the scan wrappers
#include "bam_walk_kernels.hpp"

#include <unistd.h>

#include <climits>
#include <cstdio>
#include <memory>

namespace secedo {
namespace bam_host {

using namespace secedo::bam;
namespace bw = secedo::bamwalk;

namespace {

// one BAM file on its way through the device route
struct DevFile {
    size_t f = 0;  // its index in the call's file list
    std::string path;
    Mapped m;
    std::vector<Block> blocks;
    uint64_t total = 0;          // inflated bytes
    size_t hb = 0;               // leading members inflated here: the header's
    Header h;
    std::vector<uint8_t> carry;  // what they hold past the first record
    // the walk's state between the ranges of a file that goes alone
    uint64_t rec_base = 0, dev_carry = 0;
    bool has_prev = false;
    int32_t prev_ref = 0, prev_pos = 0;
    std::vector<uint32_t> run_first, run_last;  // per requested chromosome (bam_walk.hpp's started / done rule)
    bool sorted = true;
    // read through its index: the plan, and of the span under way what the ranges so far found per requested chromosome
    const IndexPlan *plan = nullptr;
    std::vector<uint64_t> sp_count;
    std::vector<char> sp_start;
    // secedo_bam_index_build: the reference lengths are kept, and what the index takes from batch to batch
    bool want_refs = false;
    std::vector<uint32_t> l_ref;
    std::unique_ptr<bamindexbuild::Builder> builder;
    std::string out_path;
    uint64_t device_bytes() const { return carry.size() + (hb < blocks.size() ? total - blocks[hb].out : 0); }
};

// members [b0, b1) of a file in one batch
struct Piece {
    DevFile *df;
    size_t b0, b1;
    bool final;
    uint32_t first_member = 0;   // of the batch
    const Span *span = nullptr;  // an indexed file: b0, b1 count the span's members
    bool first_range() const { return span ? b0 == 0 : b0 == df->hb; }
    const std::vector<Block> &blocks() const { return span ? span->blocks : df->blocks; }
    const Mapped &mapped() const { return span ? df->plan->m : df->m; }
};

}  // namespace

struct BamDevWork {
    hipStream_t s = nullptr;
    uint8_t *h_in = nullptr;  // pinned staging of the compressed bytes
    size_t h_in_cap = 0;
    Dev<uint8_t> in, buf, out, tmp, carry;
    Dev<BgzfDesc> desc;
    Dev<uint32_t> status, lists, rewalk, seg_cnt, seg_base, chr, r_off, r_file, sel, sel_scan;
    Dev<bw::Seg> segs;
    Dev<bw::SegWalk> walk;
    Dev<bw::SegJoin> join;
    Dev<WalkFile> files;
    Dev<WalkRun> runs;
    Dev<SpanCheck> checks;
    std::vector<SpanCheck> h_checks;
    Dev<int32_t> r_ref, r_pos, sel_pos;
    Dev<uint64_t> size, size_scan, sel_off, sel_idx, totals;
    Dev<unsigned long long> per_ref;
    std::vector<uint32_t> chr_ids;  // the requested chromosomes, each once
    uint32_t n_ref = 0;             // scan: per_ref counts n_ref RefIDs and the unmapped records
    bool scan = false;              // scan: unsorted input is no error, nothing is taken
    // index build: the index pass follows the walk of every batch; `failed` = the piece whose error a batch returned
    bool index = false;
    uint32_t failed = UINT32_MAX;
    Dev<IndexFile> ix_files;
    Dev<uint32_t> ix_meta, ix_head, ix_head_scan;
    Dev<uint64_t> ix_key, ix_key_max, ix_n_win, ix_n_win_scan;
    Dev<IndexHead> ix_heads;
    Dev<IndexWin> ix_wins;
    std::vector<IndexFile> h_ix_files;
    std::vector<IndexHead> h_heads;
    std::vector<IndexWin> h_wins;
    std::vector<BgzfDesc> h_desc;
    std::vector<bw::Seg> h_segs;
    std::vector<WalkFile> h_files;
    std::vector<WalkRun> h_runs;
    std::vector<uint8_t> h_out;
    std::vector<uint64_t> h_sel_off, h_sel_idx;
    std::vector<int32_t> h_sel_pos;
    ~BamDevWork() {
        if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
        if (h_in) (void)hipHostFree(h_in);
    }
};

BamDevWork *new_bam_dev_work() { return new BamDevWork(); }
void delete_bam_dev_work(BamDevWork *w) { delete w; }

namespace {

int start_work(BamDevWork *w, const std::vector<ChrInput> &chrs) {
    if (!w->s) SECEDO_TRY(hipStreamCreateWithFlags(&w->s, hipStreamNonBlocking));
    if (w->chr_ids.empty() && !chrs.empty()) {
        for (const auto &ci : chrs)
            if (std::find(w->chr_ids.begin(), w->chr_ids.end(), ci.chromosome) == w->chr_ids.end())
                w->chr_ids.push_back(ci.chromosome);
        SECEDO_TRY(w->chr.grow(w->chr_ids.size(), 0, w->s));
        SECEDO_TRY(hipMemcpyAsync(w->chr.p, w->chr_ids.data(), w->chr_ids.size() * 4, hipMemcpyHostToDevice, w->s));
        SECEDO_TRY(hipStreamSynchronize(w->s));
    }
    return SECEDO_OK;
}

// The file mapped, its members listed, the header's members inflated here and the header parsed.
int open_file(size_t f, const std::string &path, size_t n_chr, DevFile *df) {
    df->f = f;
    df->path = path;
    SECEDO_CALL(open_bgzf(path, &df->m, &df->blocks, &df->total));
    std::vector<uint8_t> head;
    for (;;) {
        const bool final = df->hb == df->blocks.size();
        const int rc = parse_header(path, head.data(), head.size(), final, &df->h);
        if (rc == SECEDO_OK) break;
        if (rc != kNeedMore) return rc;
        const Block &b = df->blocks[df->hb];
        const size_t at = head.size();
        head.resize(at + b.isize);
        const std::string err = bm::inflate_member_zlib(df->m.p + b.payload(), b, head.data() + at);
        if (!err.empty()) return bad_block(path, bm::block_where(df->hb), err);
        ++df->hb;
    }
    df->carry.assign(head.begin() + df->h.first_record, head.end());
    if (df->want_refs) {  // parse_header has checked the list
        uint64_t o = 12 + uint64_t(df->h.l_text);
        for (uint32_t r = 0; r < df->h.n_ref; ++r) {
            o += 4 + uint64_t(rd32(head.data() + o));
            df->l_ref.push_back(rd32(head.data() + o));
            o += 4;
        }
    }
    df->run_first.assign(n_chr, bw::kNoRun);
    df->run_last.assign(n_chr, bw::kNoRun);
    route().host_blocks += df->hb;
    return SECEDO_OK;
}

const uint64_t kMaxBatchBytes = (1ull << 32) - (1u << 20);  // offsets in a batch are u32

// the error of one file of a finished batch, if it has one: its lowest record error, else its first bad member
int file_error(const BamDevWork &w, const Piece &p, const WalkFile &F) {
    unsigned long long e = F.err;
    if (!w.scan && F.unsorted != ~0ull) e = std::min(e, F.unsorted << 8 | bw::kErrUnsorted);
    const std::string &path = p.df->path;
    if (e != ~0ull) {
        const uint32_t code = uint32_t(e & 0xFF);
        const std::string where = record_where(path, 0, 0, e >> 8, Stage::kLoad, p.span != nullptr);
        if (p.span && (code == bw::kErrTruncated || code == bw::kErrBlockSize))  // as the host walk of a span
            return index_mismatch(path, "the record chain breaks: indexed record " + std::to_string(e >> 8) +
                                            (code == bw::kErrTruncated ? " is truncated" : " has a bad block_size"));
        std::string what;
        if (code == bw::kErrTruncated) what = " is truncated";
        else if (code == bw::kErrBlockSize) what = " has a bad block_size";
        else if (code == bw::kErrLonger) what = " is longer than its block_size";
        else if (code == bw::kErrUnsorted) what = ": input is not coordinate-sorted";
        else if (code == bw::kErrNegative) what = " has a negative position";
        else if (code == bw::kErrCigarSeq) what = ": CIGAR and SEQ lengths differ";
        else what = ": invalid CIGAR op code " + std::to_string(code & 15);
        return fail(SECEDO_E_INVALID_ARG, where + what);
    }
    if (F.bad != ~0ull) {
        const uint64_t k = p.b0 + ((F.bad >> 8) - p.first_member);
        return bad_block(path, p.span ? bm::block_where_byte(p.span->blocks[k].coff) : bm::block_where(k),
                         bm::status_text(uint32_t(F.bad & 0xFF)));
    }
    return SECEDO_OK;
}

// The index pass over the records of a walked batch whose files passed the walk's checks: its own errors first, in
// file order, then the heads and windows to each file's builder. A builder is touched only by a batch without errors.
int index_batch(BamDevWork *w, const std::vector<Piece> &pieces, const WalkBatch &wb, const WalkRecords &wr) {
    hipStream_t s = w->s;
    const uint32_t n_files = uint32_t(pieces.size()), n = wr.n;
    SECEDO_TRY(w->ix_files.grow(n_files, 0, s));
    SECEDO_TRY(w->ix_meta.grow(n, 0, s));
    SECEDO_TRY(w->ix_key.grow(n, 0, s));
    SECEDO_TRY(w->ix_key_max.grow(n, 0, s));
    SECEDO_TRY(w->ix_head.grow(uint64_t(n) + 1, 0, s));
    SECEDO_TRY(w->ix_head_scan.grow(uint64_t(n) + 1, 0, s));
    SECEDO_TRY(w->ix_n_win.grow(uint64_t(n) + 1, 0, s));
    SECEDO_TRY(w->ix_n_win_scan.grow(uint64_t(n) + 1, 0, s));
    const size_t tb = std::max(scan_bytes(uint64_t(n) + 1), index_scan_bytes(n));
    SECEDO_TRY(w->tmp.grow(tb, 0, s));
    SECEDO_TRY(hipMemcpyAsync(w->ix_files.p, w->h_ix_files.data(), n_files * sizeof(IndexFile), hipMemcpyHostToDevice,
                              s));
    const IndexRecords x{w->ix_meta.p,      w->ix_key.p,   w->ix_key_max.p,  w->ix_head.p,
                         w->ix_head_scan.p, w->ix_n_win.p, w->ix_n_win_scan.p};
    SECEDO_TRY(index_records(wb, wr, x, w->ix_files.p, w->tmp.p, tb, s));
    SECEDO_TRY(index_flags(wb, wr, x, s));
    SECEDO_TRY(exclusive_sum(w->tmp.p, tb, x.head, x.head_scan, uint64_t(n) + 1, s));
    SECEDO_TRY(exclusive_sum64(w->tmp.p, tb, x.n_win, x.n_win_scan, uint64_t(n) + 1, s));
    uint32_t n_heads = 0;
    uint64_t n_wins = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_heads, x.head_scan + n, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(&n_wins, x.n_win_scan + n, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(w->h_ix_files.data(), w->ix_files.p, n_files * sizeof(IndexFile), hipMemcpyDeviceToHost,
                              s));
    SECEDO_TRY(hipStreamSynchronize(s));
    for (uint32_t k = 0; k < n_files; ++k) {
        const unsigned long long e = w->h_ix_files[k].err;
        if (e == ~0ull) continue;
        w->failed = k;
        const std::string where = record_where(pieces[k].df->path, 0, 0, e >> 8, Stage::kLoad);
        const uint32_t code = uint32_t(e & 0xFF);
        return fail(SECEDO_E_INVALID_ARG,
                    where + (code == kIndexErrRef   ? " has a RefID outside the reference list"
                             : code == kIndexErrEnd ? " ends past position 2^29: a BAI index cannot hold it"
                                                    : " is longer than its block_size"));
    }
    // a record starts at most one run, and is the first over at most the 2^15 windows of its reference
    if (n_heads > n || n_wins > (uint64_t(n) << 15))
        return fail(SECEDO_E_STATE, pieces[0].df->path + ": the device index pass returned inconsistent results");
    SECEDO_TRY(w->ix_heads.grow(n_heads, 0, s));
    SECEDO_TRY(w->ix_wins.grow(n_wins, 0, s));
    SECEDO_TRY(index_emit(wb, wr, x, w->ix_files.p, w->ix_heads.p, w->ix_wins.p, s));
    w->h_heads.resize(n_heads);
    w->h_wins.resize(n_wins);
    if (n_heads)
        SECEDO_TRY(hipMemcpyAsync(w->h_heads.data(), w->ix_heads.p, n_heads * sizeof(IndexHead), hipMemcpyDeviceToHost,
                                  s));
    if (n_wins)
        SECEDO_TRY(hipMemcpyAsync(w->h_wins.data(), w->ix_wins.p, n_wins * sizeof(IndexWin), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    const auto bad = [&](const DevFile &df, const std::string &why) {
        return fail(SECEDO_E_STATE, df.path + ": the device index pass returned inconsistent results (" + why + ")");
    };
    for (const IndexHead &h : w->h_heads) {
        if (h.file >= n_files) return bad(*pieces[0].df, "a file outside the batch");
        DevFile &df = *pieces[h.file].df;
        if (h.lin > df.total) return bad(df, "an offset past the file's bytes");
        const std::string why = df.builder->add_head(bamindexbuild::Head{
            h.ref, h.bin, h.unmapped, bamindexbuild::voffset(df.blocks, df.total, df.m.n, h.lin), h.ord});
        if (!why.empty()) return bad(df, why);
    }
    for (const IndexWin &v : w->h_wins) {
        if (v.file >= n_files) return bad(*pieces[0].df, "a file outside the batch");
        DevFile &df = *pieces[v.file].df;
        if (v.lin > df.total) return bad(df, "an offset past the file's bytes");
        const std::string why = df.builder->add_window(
            bamindexbuild::Window{v.ref, v.w, bamindexbuild::voffset(df.blocks, df.total, df.m.n, v.lin)});
        if (!why.empty()) return bad(df, why);
    }
    return SECEDO_OK;
}

// One batch through the device: inflate, walk, the taken records back into runs / in (both may be null: scan).
int run_batch(BamDevWork *w, std::vector<Piece> &pieces, uint32_t threads, Inputs *in, Runs *runs,
              secedo_bam_times *t) {
    hipStream_t s = w->s;
    Clock::time_point t0 = Clock::now();
    const uint32_t n_files = uint32_t(pieces.size()), n_chr = uint32_t(w->chr_ids.size());
    // ---- layout: the staging buffer, the descriptors, the inflated buffer, the segments
    struct Copy {
        uint64_t dst;
        const uint8_t *src;
        uint64_t n;
    };
    std::vector<Copy> copies;
    w->h_desc.clear();
    w->h_segs.clear();
    w->h_files.assign(n_files, WalkFile{});
    w->h_runs.assign(size_t(n_files) * n_chr, WalkRun{});
    w->h_checks.assign(size_t(n_files) * n_chr, SpanCheck{});
    bool any_span = false;
    if (w->index) {
        w->failed = UINT32_MAX;
        w->h_ix_files.assign(n_files, IndexFile{});
        uint64_t seg = 0;
        for (uint32_t k = 0; k < n_files; ++k) {
            w->h_ix_files[k] = IndexFile{0, seg, pieces[k].df->h.n_ref, 0, ~0ull};
            seg += uint64_t(pieces[k].df->h.n_ref) + 1;
        }
    }
    uint64_t in_pos = kBgzfInSlack, out_pos = 0, n_list = 0;
    for (uint32_t k = 0; k < n_files; ++k) {
        Piece &p = pieces[k];
        DevFile &df = *p.df;
        WalkFile &F = w->h_files[k];
        p.first_member = uint32_t(w->h_desc.size());
        const bool first_range = p.first_range();
        const uint64_t carry = !first_range ? df.dev_carry : p.span ? 0 : df.carry.size();
        if (first_range && carry) {
            F.carry_src = in_pos;
            F.carry_len = uint32_t(carry);
            copies.push_back({in_pos, df.carry.data(), carry});
            in_pos += carry + kBgzfInSlack;
        }
        const uint64_t data_start = out_pos;
        uint64_t o = data_start + carry;
        if (p.b0 < p.b1) {
            const std::vector<Block> &bl = p.blocks();
            const bm::PayloadSpan sp = bm::payload_span(bl, p.b0, p.b1, p.mapped().n);
            const uint8_t *lo = p.mapped().p + sp.lo;
            for (uint64_t c = 0; c < sp.hi - sp.lo; c += 4u << 20)
                copies.push_back({in_pos + c, lo + c, std::min<uint64_t>(4u << 20, sp.hi - sp.lo - c)});
            w->h_desc.resize(p.first_member + (p.b1 - p.b0));
            bm::fill_desc(bl, p.b0, p.b1, sp.lo, in_pos, o, w->h_desc.data() + p.first_member);
            for (size_t b = p.b0; b < p.b1; ++b) {
                // a span is entered at its first record, a known record start
                const uint64_t start = b != p.b0 ? o : data_start + (p.span && first_range ? p.span->entry : 0);
                o += bl[b].isize;
                w->h_segs.push_back(bw::Seg{uint32_t(start), uint32_t(o), k, uint32_t(n_list)});
                n_list += bw::list_cap(uint32_t(o - start));
            }
            in_pos += sp.needed;
            F.n_seg = uint32_t(p.b1 - p.b0);
        }
        F.first_seg = p.first_member;
        F.data_end = F.limit = uint32_t(o);
        if (w->index)  // the byte behind the carry is the first of member b0 (of the file's end, if none is left)
            w->h_ix_files[k].delta = (long long)(p.b0 < df.blocks.size() ? df.blocks[p.b0].out : df.total) -
                                     (long long)(data_start + carry);
        if (p.span) {  // the span's offsets as offsets of the buffer; its last range ends at its limit
            const Span &sp = *p.span;
            const long long base = (long long)(data_start + carry) - (long long)sp.blocks[p.b0].out;
            if (p.final) F.data_end = F.limit = uint32_t(base + (long long)sp.limit);
            for (size_t c = 0; c < sp.chrs.size(); ++c) {
                const size_t u = std::find(w->chr_ids.begin(), w->chr_ids.end(), sp.chrs[c].chromosome) -
                                 w->chr_ids.begin();
                SpanCheck &ck = w->h_checks[size_t(k) * n_chr + u];
                ck.beg = base + (long long)sp.chrs[c].beg;
                ck.end = base + (long long)sp.chrs[c].end;
                ck.ref = int32_t(sp.chrs[c].chromosome);
                ck.flags = kSpanOn | (c == 0 && first_range ? kSpanEntry : 0) |
                           (c + 1 == sp.chrs.size() && p.final && sp.limit + 8 <= sp.bytes ? kSpanTail : 0);
            }
            any_span = true;
        }
        F.final = p.final;
        F.has_prev = df.has_prev;
        F.rec_base = df.rec_base;
        F.prev_ref = df.prev_ref;
        F.prev_pos = df.prev_pos;
        F.stop_off = F.data_end;
        F.bad = F.err = F.unsorted = ~0ull;
        for (uint32_t u = 0; u < n_chr; ++u) {
            w->h_runs[size_t(k) * n_chr + u].first = df.run_first[u];
            w->h_runs[size_t(k) * n_chr + u].last = df.run_last[u];
        }
        out_pos = (o + 15) / 16 * 16;
        if (out_pos > kMaxBatchBytes || n_list > UINT32_MAX)
            return fail(SECEDO_E_LIMIT, df.path + ": a batch of 4 GiB or more of inflated BAM (a record that long, or "
                                                  "SECEDO_BAM_BATCH_BYTES too large)");
    }
    const uint32_t n_members = uint32_t(w->h_desc.size());
    // a file without a member in the batch (its header's members held all of it) walks its carry as one segment
    for (uint32_t k = 0; k < n_files; ++k) {
        WalkFile &F = w->h_files[k];
        if (F.n_seg) continue;
        const uint32_t len = uint32_t(pieces[k].df->carry.size());
        F.first_seg = uint32_t(w->h_segs.size());
        F.n_seg = 1;
        w->h_segs.push_back(bw::Seg{F.data_end - len, F.data_end, k, uint32_t(n_list)});
        n_list += bw::list_cap(len);
    }
    const uint32_t n_seg = uint32_t(w->h_segs.size());
    const uint64_t buf_bytes = out_pos + kWalkWindow;
    // ---- staging and upload
    if (in_pos > w->h_in_cap) {
        if (w->h_in) SECEDO_TRY(hipHostFree(w->h_in));
        w->h_in = nullptr;
        w->h_in_cap = 0;
        const size_t cap = std::max<size_t>(in_pos + in_pos / 2, 1u << 20);
        SECEDO_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->h_in), cap, hipHostMallocDefault));
        w->h_in_cap = cap;
    }
    parallel_for(threads, copies.size(),
                 [&](uint64_t c) { std::memcpy(w->h_in + copies[c].dst, copies[c].src, copies[c].n); });
    SECEDO_TRY(w->in.grow(in_pos, 0, s));
    SECEDO_TRY(w->buf.grow(buf_bytes, pieces[0].first_range() ? 0 : pieces[0].df->dev_carry, s));
    SECEDO_TRY(w->desc.grow(n_members, 0, s));
    SECEDO_TRY(w->status.grow(n_members, 0, s));
    SECEDO_TRY(w->segs.grow(n_seg, 0, s));
    SECEDO_TRY(w->walk.grow(n_seg, 0, s));
    SECEDO_TRY(w->join.grow(n_seg, 0, s));
    SECEDO_TRY(w->seg_cnt.grow(uint64_t(n_seg) + 1, 0, s));
    SECEDO_TRY(w->seg_base.grow(uint64_t(n_seg) + 1, 0, s));
    SECEDO_TRY(w->lists.grow(n_list, 0, s));
    SECEDO_TRY(w->rewalk.grow(n_list, 0, s));
    SECEDO_TRY(w->files.grow(n_files, 0, s));
    SECEDO_TRY(w->runs.grow(w->h_runs.size(), 0, s));
    SECEDO_TRY(w->totals.grow(2, 0, s));
    if (any_span) {
        SECEDO_TRY(w->checks.grow(w->h_checks.size(), 0, s));
        SECEDO_TRY(hipMemcpyAsync(w->checks.p, w->h_checks.data(), w->h_checks.size() * sizeof(SpanCheck),
                                  hipMemcpyHostToDevice, s));
    }
    SECEDO_TRY(hipMemcpyAsync(w->in.p, w->h_in, in_pos, hipMemcpyHostToDevice, s));
    if (n_members)
        SECEDO_TRY(hipMemcpyAsync(w->desc.p, w->h_desc.data(), n_members * sizeof(BgzfDesc), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(w->segs.p, w->h_segs.data(), n_seg * sizeof(bw::Seg), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(w->files.p, w->h_files.data(), n_files * sizeof(WalkFile), hipMemcpyHostToDevice, s));
    if (!w->h_runs.empty())
        SECEDO_TRY(hipMemcpyAsync(w->runs.p, w->h_runs.data(), w->h_runs.size() * sizeof(WalkRun),
                                  hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_lap(t0);
    // ---- inflate
    SECEDO_TRY(bgzf_inflate(w->in.p, w->desc.p, n_members, w->buf.p, w->status.p, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) {
        t->inflate_ms += ms_lap(t0);
        for (const BgzfDesc &d : w->h_desc) t->inflated_bytes += double(d.isize);
    }
    // ---- walk
    const WalkBatch wb{w->buf.p,  buf_bytes / 16 * 16, w->segs.p, w->files.p,   n_seg,        n_files,
                       w->lists.p, w->rewalk.p,        w->walk.p, w->join.p,    w->seg_cnt.p, w->seg_base.p};
    SECEDO_TRY(walk_prepare(wb, w->in.p, w->desc.p, w->status.p, n_members, s));
    SECEDO_TRY(walk_segments(wb, s));
    SECEDO_TRY(hipMemsetAsync(w->seg_cnt.p + n_seg, 0, 4, s));
    size_t tb = scan_bytes(uint64_t(n_seg) + 1);
    SECEDO_TRY(w->tmp.grow(tb, 0, s));
    SECEDO_TRY(exclusive_sum(w->tmp.p, tb, w->seg_cnt.p, w->seg_base.p, uint64_t(n_seg) + 1, s));
    uint32_t n_rec = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_rec, w->seg_base.p + n_seg, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    SECEDO_TRY(w->r_off.grow(n_rec, 0, s));
    SECEDO_TRY(w->r_file.grow(n_rec, 0, s));
    SECEDO_TRY(w->r_ref.grow(n_rec, 0, s));
    SECEDO_TRY(w->r_pos.grow(n_rec, 0, s));
    SECEDO_TRY(w->sel.grow(uint64_t(n_rec) + 1, 0, s));
    SECEDO_TRY(w->sel_scan.grow(uint64_t(n_rec) + 1, 0, s));
    SECEDO_TRY(w->size.grow(uint64_t(n_rec) + 1, 0, s));
    SECEDO_TRY(w->size_scan.grow(uint64_t(n_rec) + 1, 0, s));
    const WalkRecords wr{n_rec,    w->r_off.p, w->r_file.p,   w->r_ref.p,
                         w->r_pos.p, w->sel.p,   w->size.p,     w->sel_scan.p, w->size_scan.p};
    SECEDO_TRY(walk_records(wb, wr, w->chr.p, n_chr, w->runs.p, w->scan ? w->per_ref.p : nullptr, w->n_ref, s));
    if (any_span) {
        SECEDO_TRY(walk_span_check(wb, wr, n_chr, w->checks.p, s));
        SECEDO_TRY(hipMemcpyAsync(w->h_checks.data(), w->checks.p, w->h_checks.size() * sizeof(SpanCheck),
                                  hipMemcpyDeviceToHost, s));
    }
    tb = scan_bytes(uint64_t(n_rec) + 1);
    SECEDO_TRY(w->tmp.grow(tb, 0, s));
    SECEDO_TRY(exclusive_sum(w->tmp.p, tb, w->sel.p, w->sel_scan.p, uint64_t(n_rec) + 1, s));
    SECEDO_TRY(exclusive_sum64(w->tmp.p, tb, w->size.p, w->size_scan.p, uint64_t(n_rec) + 1, s));
    SECEDO_TRY(walk_runs(wb, wr, n_chr, w->runs.p, w->totals.p, s));
    uint64_t totals[2] = {0, 0};
    SECEDO_TRY(hipMemcpyAsync(w->h_files.data(), w->files.p, n_files * sizeof(WalkFile), hipMemcpyDeviceToHost, s));
    if (!w->h_runs.empty())
        SECEDO_TRY(hipMemcpyAsync(w->h_runs.data(), w->runs.p, w->h_runs.size() * sizeof(WalkRun),
                                  hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(totals, w->totals.p, 16, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    route().device_blocks += n_members;
    route().segments += n_seg;
    route().uploaded_bytes += in_pos;
    route().batches += 1;
    for (uint32_t k = 0; k < n_files; ++k) {
        route().device_records += w->h_files[k].n_rec;
        route().rewalked_segments += w->h_files[k].rewalked;
    }
    // per file in order: the RefID at a span's entry, then the walk's own errors, then what the index says of the span
    for (uint32_t k = 0; k < n_files; ++k) {
        const Piece &p = pieces[k];
        if (p.span) {
            index_info().members += p.b1 - p.b0;
            index_info().spans += p.first_range() ? 1 : 0;
            const Span &sp = *p.span;
            const size_t u0 = std::find(w->chr_ids.begin(), w->chr_ids.end(), sp.chrs[0].chromosome) -
                              w->chr_ids.begin();
            if (w->h_checks[size_t(k) * n_chr + u0].entry_bad) return check_span_chr(p.df->path, sp.chrs[0], false, 0);
        }
        if (const int rc = file_error(*w, p, w->h_files[k])) {
            w->failed = k;
            return rc;
        }
        if (!p.span) continue;
        DevFile &df = *p.df;
        for (uint32_t u = 0; u < n_chr; ++u) {
            const SpanCheck &ck = w->h_checks[size_t(k) * n_chr + u];
            if (!(ck.flags & kSpanOn)) continue;
            df.sp_count[u] += ck.count;
            if (ck.start) df.sp_start[u] = ck.start == 1;
        }
        if (!p.final) continue;
        for (const SpanChr &sc : p.span->chrs) {
            const size_t u = std::find(w->chr_ids.begin(), w->chr_ids.end(), sc.chromosome) - w->chr_ids.begin();
            SECEDO_CALL(check_span_chr(df.path, sc, df.sp_start[u] != 0, df.sp_count[u]));
            if (w->h_checks[size_t(k) * n_chr + u].tail_bad) return span_tail_mismatch(df.path, sc);
        }
    }
    // ---- the taken records
    const uint64_t n_sel = totals[0], sel_bytes = totals[1];
    // what came back must be consistent before it is used as an index
    uint64_t sum_rec = 0;
    bool sane = n_sel <= n_rec && sel_bytes <= out_pos;
    for (uint32_t k = 0; k < n_files; ++k) {
        const WalkFile &F = w->h_files[k];
        sum_rec += F.n_rec;
        sane = sane && F.stop_off <= F.data_end;
    }
    for (const WalkRun &run : w->h_runs)
        sane = sane && run.j0 <= run.j1 && run.j1 <= n_sel && run.b0 <= run.b1 && run.b1 <= sel_bytes;
    if (!sane || sum_rec != n_rec)
        return fail(SECEDO_E_STATE, pieces[0].df->path + ": the device walk returned inconsistent results");
    if (w->index) SECEDO_CALL(index_batch(w, pieces, wb, wr));
    if (n_sel) {
        SECEDO_TRY(w->out.grow(sel_bytes, 0, s));
        SECEDO_TRY(w->sel_off.grow(n_sel, 0, s));
        SECEDO_TRY(w->sel_pos.grow(n_sel, 0, s));
        SECEDO_TRY(w->sel_idx.grow(n_sel, 0, s));
        SECEDO_TRY(walk_gather(wb, wr, w->out.p, w->sel_off.p, w->sel_pos.p, w->sel_idx.p, s));
        w->h_out.resize(sel_bytes);
        w->h_sel_off.resize(n_sel);
        w->h_sel_pos.resize(n_sel);
        w->h_sel_idx.resize(n_sel);
        SECEDO_TRY(hipMemcpyAsync(w->h_out.data(), w->out.p, sel_bytes, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(w->h_sel_off.data(), w->sel_off.p, n_sel * 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(w->h_sel_pos.data(), w->sel_pos.p, n_sel * 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(w->h_sel_idx.data(), w->sel_idx.p, n_sel * 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        route().downloaded_record_bytes += sel_bytes;
    }
    // ---- per file: its runs appended as FileSink appends them, and the state the next range starts from
    for (uint32_t k = 0; k < n_files; ++k) {
        DevFile &df = *pieces[k].df;
        const WalkFile &F = w->h_files[k];
        for (uint32_t u = 0; u < n_chr; ++u) {
            const WalkRun &run = w->h_runs[size_t(k) * n_chr + u];
            if (run.last != bw::kNoRun) df.run_first[u] = df.run_last[u] = 0;  // done
            else if (run.first != bw::kNoRun) df.run_first[u] = 0;             // open
            if (run.j1 == run.j0) continue;
            for (size_t c = 0; c < in->chrs.size(); ++c) {
                ChrInput &ci = in->chrs[c];
                if (ci.chromosome != w->chr_ids[u]) continue;
                std::vector<uint8_t> &dst = (*runs)[c][df.f];
                const uint64_t base = dst.size();
                for (uint32_t j = run.j0; j < run.j1; ++j) ci.roff[df.f].push_back(base + (w->h_sel_off[j] - run.b0));
                ci.rpos[df.f].insert(ci.rpos[df.f].end(), w->h_sel_pos.begin() + run.j0, w->h_sel_pos.begin() + run.j1);
                ci.ridx[df.f].insert(ci.ridx[df.f].end(), w->h_sel_idx.begin() + run.j0, w->h_sel_idx.begin() + run.j1);
                dst.insert(dst.end(), w->h_out.begin() + run.b0, w->h_out.begin() + run.b1);
            }
        }
        if (F.n_rec) {
            df.has_prev = true;
            df.prev_ref = F.last_ref;
            df.prev_pos = F.last_pos;
        }
        df.rec_base += F.n_rec;
        if (F.unsorted != ~0ull) df.sorted = false;
        df.dev_carry = F.data_end - F.stop_off;
        if (!pieces[k].final && df.dev_carry) {  // the cut record to the front of the buffer (one file goes alone)
            SECEDO_TRY(w->carry.grow(df.dev_carry, 0, s));
            SECEDO_TRY(hipMemcpyAsync(w->carry.p, w->buf.p + F.stop_off, df.dev_carry, hipMemcpyDeviceToDevice, s));
            SECEDO_TRY(hipMemcpyAsync(w->buf.p, w->carry.p, df.dev_carry, hipMemcpyDeviceToDevice, s));
        }
    }
    if (t) t->walk_ms += ms_lap(t0);
    return SECEDO_OK;
}

// One file that inflates to more than a batch: ranges of members of about `batch` inflated bytes.
int run_ranges(BamDevWork *w, DevFile *df, const Span *span, uint32_t threads, uint64_t batch, Inputs *in, Runs *runs,
               secedo_bam_times *t) {
    const std::vector<Block> &bl = span ? span->blocks : df->blocks;
    for (size_t b0 = span ? 0 : df->hb;;) {
        size_t b1 = b0;
        uint64_t bytes = 0;
        while (b1 < bl.size() && (b1 == b0 || bytes + bl[b1].isize <= batch)) bytes += bl[b1++].isize;
        if (!span && b1 < bl.size() && bl[b1].out == df->total) b1 = bl.size();  // only empty members follow
        std::vector<Piece> one{Piece{df, b0, b1, b1 == bl.size(), 0, span}};
        SECEDO_CALL(run_batch(w, one, threads, in, runs, t));
        if (b1 == bl.size()) return SECEDO_OK;
        b0 = b1;
    }
}

}  // namespace

int load_bams_device(size_t f0, size_t f1, uint32_t threads, uint64_t batch, BamDevWork *w, Inputs *in, Runs *runs,
                     secedo_bam_times *t, std::vector<IndexPlan> *plans) {
    SECEDO_CALL(start_work(w, in->chrs));
    std::vector<std::unique_ptr<DevFile>> open;
    std::vector<std::unique_ptr<DevFile>> indexed;  // kept over their spans
    const size_t n_chr = w->chr_ids.size();
    std::vector<Piece> pieces;
    uint64_t bytes = 0;
    const auto flush = [&]() -> int {
        if (pieces.empty()) return SECEDO_OK;
        const int rc = run_batch(w, pieces, threads, in, runs, t);
        pieces.clear();
        open.clear();
        bytes = 0;
        return rc;
    };
    for (size_t f = f0; f < f1; ++f) {
        const Clock::time_point t0 = Clock::now();
        if (plans && (*plans)[f].indexed) {  // its header is read; its spans follow below
            std::unique_ptr<DevFile> df(new DevFile());
            df->f = f;
            df->path = in->paths[f];
            df->plan = &(*plans)[f];
            df->h = df->plan->h;
            df->run_first.assign(n_chr, bw::kNoRun);
            df->run_last.assign(n_chr, bw::kNoRun);
            indexed.push_back(std::move(df));
            continue;
        }
        std::unique_ptr<DevFile> df(new DevFile());
        const int rc = open_file(f, in->paths[f], w->chr_ids.size(), df.get());
        if (t) t->inflate_ms += ms_since(t0);
        if (rc != SECEDO_OK) {  // the files in front of it come first
            const std::string msg = g_error;
            SECEDO_CALL(flush());
            return fail(rc, msg);
        }
        if (t) t->inflated_bytes += double(df->total - df->device_bytes() + df->carry.size());
        const uint64_t n = df->device_bytes();
        if (n > batch || n > kMaxBatchBytes / 2) {
            SECEDO_CALL(flush());
            SECEDO_CALL(run_ranges(w, df.get(), nullptr, threads, batch, in, runs, t));
            continue;
        }
        if (!pieces.empty() && bytes + n > batch) SECEDO_CALL(flush());
        pieces.push_back(Piece{df.get(), df->hb, df->blocks.size(), true});
        open.push_back(std::move(df));
        bytes += n;
    }
    // span k of every indexed file, k = 0, 1, ...; the first spans share the batch of the files read in full
    for (size_t k = 0;; ++k) {
        bool any = false;
        for (const auto &df : indexed) {
            if (k >= df->plan->spans.size()) continue;
            any = true;
            const Span *sp = &df->plan->spans[k];
            df->sp_count.assign(n_chr, 0);
            df->sp_start.assign(n_chr, 0);
            df->dev_carry = 0;
            if (sp->bytes > batch || sp->bytes > kMaxBatchBytes / 2) {
                SECEDO_CALL(flush());
                SECEDO_CALL(run_ranges(w, df.get(), sp, threads, batch, in, runs, t));
                continue;
            }
            if (!pieces.empty() && bytes + sp->bytes > batch) SECEDO_CALL(flush());
            pieces.push_back(Piece{df.get(), 0, sp->blocks.size(), true, 0, sp});
            bytes += sp->bytes;
        }
        SECEDO_CALL(flush());
        if (!any) break;
    }
    return SECEDO_OK;
}

}  // namespace bam_host
}  // namespace secedo

using namespace secedo::bam_host;

extern "C" int secedo_bam_scan_device(const char *path, uint32_t num_threads, secedo_bam_scan_info *info,
                                      uint64_t *records_per_ref, uint32_t capacity) {
    if (!path || !info) return fail(SECEDO_E_INVALID_ARG, "null argument");
    route() = secedo_bam_route_info{};
    std::unique_ptr<BamDevWork> w(new BamDevWork());
    w->scan = true;
    SECEDO_CALL(start_work(w.get(), {}));
    DevFile df;
    SECEDO_CALL(open_file(0, path, 0, &df));
    w->n_ref = df.h.n_ref;
    SECEDO_TRY(w->per_ref.grow(uint64_t(w->n_ref) + 1, 0, w->s));
    SECEDO_TRY(hipMemsetAsync(w->per_ref.p, 0, (uint64_t(w->n_ref) + 1) * 8, w->s));
    SECEDO_CALL(run_ranges(w.get(), &df, nullptr, num_threads ? num_threads : 1, batch_bytes(), nullptr, nullptr,
                           nullptr));
    std::vector<unsigned long long> per(uint64_t(w->n_ref) + 1);
    SECEDO_TRY(hipMemcpyAsync(per.data(), w->per_ref.p, per.size() * 8, hipMemcpyDeviceToHost, w->s));
    SECEDO_TRY(hipStreamSynchronize(w->s));
    info->n_ref = df.h.n_ref;
    info->sorted = df.sorted ? 1 : 0;
    info->n_records = df.rec_base;
    info->n_unmapped = per[w->n_ref];
    info->n_blocks = df.blocks.size();
    info->inflated_bytes = df.total;
    info->l_text = df.h.l_text;
    info->reserved = 0;
    if (records_per_ref)
        for (uint32_t r = 0; r < std::min(capacity, df.h.n_ref); ++r) records_per_ref[r] = per[r];
    return SECEDO_OK;
}

// ---- secedo_bam_index_build

namespace secedo {
namespace bam_host {
namespace {

bool exists(const std::string &path) { return access(path.c_str(), F_OK) == 0; }

// The bytes to a temporary name beside `path`, then renamed onto it: a failure leaves nothing.
int write_renamed(const std::string &path, const std::vector<uint8_t> &bytes) {
    const std::string tmp = path + ".tmp." + std::to_string((long long)getpid());
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) return fail(SECEDO_E_INVALID_ARG, "Could not create " + tmp);
    const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), path.c_str()) != 0) {
        std::remove(tmp.c_str());
        return fail(SECEDO_E_INVALID_ARG, "Could not write " + path);
    }
    return SECEDO_OK;
}

// The file's index from its builder, once its last range is through.
int finish_index(DevFile *df, secedo_bam_build_info *info) {
    std::vector<uint8_t> bytes;
    bamindexbuild::Stats st;
    const std::string why = df->builder->finish(bamindexbuild::voffset(df->blocks, df->total, df->m.n, df->total),
                                                df->rec_base, &bytes, &st);
    if (!why.empty())
        return fail(SECEDO_E_STATE, df->path + ": the device index pass returned inconsistent results (" + why + ")");
    SECEDO_CALL(write_renamed(df->out_path, bytes));
    info->files += 1;
    info->records += df->rec_base;
    info->chunks += st.chunks;
    info->bins += st.bins;
    info->windows += st.windows;
    info->index_bytes += bytes.size();
    info->joined_runs += st.joined;
    return SECEDO_OK;
}

// What must hold of a file before any of it goes to the device.
int open_for_index(size_t f, const std::string &path, const std::string &out, int overwrite, DevFile *df) {
    SECEDO_CALL(require_bam(path, "cannot be indexed"));
    if (!overwrite && exists(out))
        return fail(SECEDO_E_INVALID_ARG, path + ": the index " + out + " exists; pass overwrite to replace it");
    df->want_refs = true;
    df->out_path = out;
    SECEDO_CALL(open_file(f, path, 0, df));
    for (uint32_t r = 0; r < df->h.n_ref; ++r)
        if (df->l_ref[r] > bamindexbuild::kMaxEnd)
            return fail(SECEDO_E_INVALID_ARG, path + ": reference " + std::to_string(r) + " is " +
                                                  std::to_string(df->l_ref[r]) +
                                                  " long, past 2^29: a BAI index cannot hold it");
    df->builder.reset(new bamindexbuild::Builder(df->h.n_ref));
    return SECEDO_OK;
}

int index_build(const char *const *bam_files, uint32_t n_files, const char *const *out_paths, int overwrite,
                uint32_t threads, secedo_bam_build_info *info) {
    std::unique_ptr<BamDevWork> w(new BamDevWork());
    w->index = true;
    SECEDO_CALL(start_work(w.get(), {}));
    const uint64_t batch = batch_bytes();
    std::vector<std::unique_ptr<DevFile>> open;
    std::vector<Piece> pieces;
    uint64_t bytes = 0;
    // The batch of small files: if one of them fails, the files in front of it go through again without it and keep
    // their indexes, and the failed file's error is the call's.
    const auto flush = [&]() -> int {
        if (pieces.empty()) return SECEDO_OK;
        int rc = run_batch(w.get(), pieces, threads, nullptr, nullptr, nullptr);
        size_t n_good = pieces.size();
        std::string msg;
        if (rc != SECEDO_OK) {
            if (w->failed == UINT32_MAX) return rc;
            msg = g_error;
            n_good = w->failed;
            pieces.resize(n_good);
            if (n_good) SECEDO_CALL(run_batch(w.get(), pieces, threads, nullptr, nullptr, nullptr));
        }
        for (size_t k = 0; k < n_good; ++k) SECEDO_CALL(finish_index(pieces[k].df, info));
        pieces.clear();
        open.clear();
        bytes = 0;
        return rc == SECEDO_OK ? rc : fail(rc, msg);
    };
    for (uint32_t f = 0; f < n_files; ++f) {
        if (!bam_files[f]) return fail(SECEDO_E_INVALID_ARG, "null file name");
        const std::string path = bam_files[f];
        const std::string out = out_paths && out_paths[f] ? std::string(out_paths[f]) : path + ".bai";
        std::unique_ptr<DevFile> df(new DevFile());
        const int rc = open_for_index(f, path, out, overwrite, df.get());
        if (rc != SECEDO_OK) {  // the files in front of it come first
            const std::string msg = g_error;
            SECEDO_CALL(flush());
            return fail(rc, msg);
        }
        const uint64_t n = df->device_bytes();
        if (n > batch || n > kMaxBatchBytes / 2) {
            SECEDO_CALL(flush());
            SECEDO_CALL(run_ranges(w.get(), df.get(), nullptr, threads, batch, nullptr, nullptr, nullptr));
            SECEDO_CALL(finish_index(df.get(), info));
            continue;
        }
        if (!pieces.empty() && bytes + n > batch) SECEDO_CALL(flush());
        pieces.push_back(Piece{df.get(), df->hb, df->blocks.size(), true});
        open.push_back(std::move(df));
        bytes += n;
    }
    return flush();
}

}  // namespace
}  // namespace bam_host
}  // namespace secedo

extern "C" int secedo_bam_index_build(const char *const *bam_files, uint32_t n_files, const char *const *out_paths,
                                      int overwrite, uint32_t num_threads, secedo_bam_build_info *info) {
    if (!bam_files || !info) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *info = secedo_bam_build_info{};
    route() = secedo_bam_route_info{};
    return index_build(bam_files, n_files, out_paths, overwrite, num_threads ? num_threads : 1, info);
}
