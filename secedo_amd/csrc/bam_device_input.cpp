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
// files read in full), so many small files still share one upload, one inflate launch and one walk; the file's walk
// state (record count, last record, runs) passes from span to span as it passes from range to range. A span larger
// than a batch goes alone, in ranges of members.
//
// run_batch is a sequence of stages over BamDevWork, each a function of its own: lay_out (where everything of the
// batch lies: bam_batch.hpp's lay_out_batch, plain arithmetic that tests/cpp/bam_batch_test.cpp checks on the host),
// upload, inflate_batch, walk_and_scan, verdicts (the errors, in the host route's order and words), check_results,
// index_batch (index build only), fetch_taken, append_runs (the runs into ChrInput, the state and the device carry
// for the next range). Ranges are cut by bgzf_members.hpp's next_range.
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

// one BAM file on its way through the device route; its walk state (FileWalk) passes between its ranges and spans
struct DevFile : FileWalk {
    size_t f = 0;  // its index in the call's file list
    std::string path;
    Mapped m;
    std::vector<Block> blocks;
    uint64_t total = 0;          // inflated bytes
    size_t hb = 0;               // leading members inflated here: the header's
    Header h;
    std::vector<uint8_t> carry;  // what they hold past the first record
    uint64_t dev_carry = 0;  // the cut record's bytes at the front of the buffer, between the ranges of a file
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
    // a fresh file: no run of a requested chromosome has started
    void start(size_t file, const std::string &name, size_t n_chr) {
        f = file;
        path = name;
        run_first.assign(n_chr, bw::kNoRun);
        run_last.assign(n_chr, bw::kNoRun);
    }
};

// members [b0, b1) of a file in one batch: what the layout takes (bam_batch.hpp), and the file
struct Piece : BatchPiece {
    DevFile *df = nullptr;
};

// span: an indexed file, b0 and b1 count the span's members. Made when the piece joins its batch: a file's carries
// and its place in the file do not change until the batch has run.
Piece piece_of(DevFile *df, size_t b0, size_t b1, bool final, const Span *span = nullptr) {
    const Mapped &m = span ? df->plan->m : df->m;
    Piece p;
    p.df = df;
    p.blocks = span ? &span->blocks : &df->blocks;
    p.b0 = b0, p.b1 = b1;
    p.file = m.p, p.file_bytes = m.n;
    p.first_range = span ? b0 == 0 : b0 == df->hb;
    p.final = final;
    p.carry_bytes = df->carry.data();
    p.carry = !p.first_range ? df->dev_carry : span ? 0 : df->carry.size();
    p.walk = df;
    p.span = span;
    p.n_ref = df->h.n_ref;
    p.lin0 = b0 < df->blocks.size() ? df->blocks[b0].out : df->total;
    return p;
}

}  // namespace

// What a call keeps on the device route, grouped by who fills and who reads it.
struct BamDevWork {
    hipStream_t s = nullptr;
    // the call: set once, by start_work and the entry points
    std::vector<uint32_t> chr_ids;  // the requested chromosomes, each once
    Dev<uint32_t> chr;
    uint32_t n_ref = 0;             // scan: per_ref counts n_ref RefIDs and the unmapped records
    bool scan = false;              // scan: unsorted input is no error, nothing is taken
    Dev<unsigned long long> per_ref;
    // index build: the index pass follows the walk of every batch; `failed` = the piece whose error a batch returned
    bool index = false;
    uint32_t failed = UINT32_MAX;
    // the batch's layout (bam_batch.hpp): lay_out fills it, every stage reads it; its files, runs, checks and ix_files
    // are also where the walk's and the index pass's results come back to
    BatchLayout lay;
    // staging and inflate: upload fills them, inflate and the walk read them; carry: the cut record between ranges
    uint8_t *h_in = nullptr;  // pinned staging of the compressed bytes
    size_t h_in_cap = 0;
    Dev<uint8_t> in, buf, carry;
    Dev<BgzfDesc> desc;
    Dev<uint32_t> status;
    // the walk: per segment, per file, per record; tmp is the scans' (the index pass's too)
    Dev<bw::Seg> segs;
    Dev<bw::SegWalk> walk;
    Dev<bw::SegJoin> join;
    Dev<uint32_t> lists, rewalk, seg_cnt, seg_base;
    Dev<WalkFile> files;
    Dev<WalkRun> runs;
    Dev<SpanCheck> checks;
    Dev<uint8_t> tmp;
    Dev<uint32_t> r_off, r_file, sel, sel_scan;
    Dev<int32_t> r_ref, r_pos;
    Dev<uint64_t> size, size_scan, totals;
    uint32_t n_rec = 0;                 // records of the batch
    uint64_t n_sel = 0, sel_bytes = 0;  // the taken ones, and their bytes
    WalkBatch walk_batch() const {
        return WalkBatch{buf.p,   lay.buf_bytes / 16 * 16,    segs.p,  files.p,  uint32_t(lay.segs.size()),
                         uint32_t(lay.files.size()), lists.p, rewalk.p, walk.p, join.p, seg_cnt.p, seg_base.p};
    }
    WalkRecords walk_records() const {
        return WalkRecords{n_rec, r_off.p, r_file.p, r_ref.p, r_pos.p, sel.p, size.p, sel_scan.p, size_scan.p};
    }
    // the taken records: fetch_taken fills them, append_runs reads them
    Dev<uint8_t> out;
    Dev<uint64_t> sel_off, sel_idx;
    Dev<int32_t> sel_pos;
    std::vector<uint8_t> h_out;
    std::vector<uint64_t> h_sel_off, h_sel_idx;
    std::vector<int32_t> h_sel_pos;
    // the index pass: index_batch fills and reads them
    Dev<IndexFile> ix_files;
    Dev<uint32_t> ix_meta, ix_head, ix_head_scan;
    Dev<uint64_t> ix_key, ix_key_max, ix_n_win, ix_n_win_scan;
    Dev<IndexHead> ix_heads;
    Dev<IndexWin> ix_wins;
    std::vector<IndexHead> h_heads;
    std::vector<IndexWin> h_wins;
    IndexRecords index_records() const {
        return IndexRecords{ix_meta.p, ix_key.p, ix_key_max.p, ix_head.p, ix_head_scan.p, ix_n_win.p, ix_n_win_scan.p};
    }
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
            if (slot_of(w->chr_ids, ci.chromosome) == w->chr_ids.size()) w->chr_ids.push_back(ci.chromosome);
        SECEDO_TRY(w->chr.grow(w->chr_ids.size(), 0, w->s));
        SECEDO_TRY(hipMemcpyAsync(w->chr.p, w->chr_ids.data(), w->chr_ids.size() * 4, hipMemcpyHostToDevice, w->s));
        SECEDO_TRY(hipStreamSynchronize(w->s));
    }
    return SECEDO_OK;
}

// The file mapped, its members listed, the header's members inflated here and the header parsed.
int open_file(size_t f, const std::string &path, size_t n_chr, DevFile *df) {
    df->start(f, path, n_chr);
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
    route().host_blocks += df->hb;
    return SECEDO_OK;
}

// the error of one file of a finished batch, if it has one: its lowest record error, else its first bad member
int file_error(const BamDevWork &w, const Piece &p, uint32_t first_member, const WalkFile &F) {
    unsigned long long e = F.err;
    if (!w.scan && F.unsorted != ~0ull) e = std::min(e, F.unsorted << 8 | bw::kErrUnsorted);
    const std::string &path = p.df->path;
    if (e != ~0ull) {
        const uint32_t code = uint32_t(e & 0xFF);
        if (p.span && (code == bw::kErrTruncated || code == bw::kErrBlockSize))  // as the host walk of a span
            return chain_break(path, e >> 8, code);
        return fail(SECEDO_E_INVALID_ARG,
                    record_where(path, 0, 0, e >> 8, Stage::kLoad, p.span != nullptr) + defect_tail(code));
    }
    if (F.bad != ~0ull) {
        const uint64_t k = p.b0 + ((F.bad >> 8) - first_member);
        return bad_block(path, p.span ? bm::block_where_byte(p.span->blocks[k].coff) : bm::block_where(k),
                         bm::status_text(uint32_t(F.bad & 0xFF)));
    }
    return SECEDO_OK;
}

// The index pass over the records of a walked batch whose files passed the walk's checks: its own errors first, in
// file order, then the heads and windows to each file's builder. A builder is touched only by a batch without errors.
int index_batch(BamDevWork *w, const std::vector<Piece> &pieces) {
    hipStream_t s = w->s;
    const WalkBatch wb = w->walk_batch();
    const WalkRecords wr = w->walk_records();
    std::vector<IndexFile> &h_ix_files = w->lay.ix_files;
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
    SECEDO_TRY(hipMemcpyAsync(w->ix_files.p, h_ix_files.data(), n_files * sizeof(IndexFile), hipMemcpyHostToDevice, s));
    const IndexRecords x = w->index_records();
    SECEDO_TRY(index_records(wb, wr, x, w->ix_files.p, w->tmp.p, tb, s));
    SECEDO_TRY(index_flags(wb, wr, x, s));
    SECEDO_TRY(exclusive_sum(w->tmp.p, tb, x.head, x.head_scan, uint64_t(n) + 1, s));
    SECEDO_TRY(exclusive_sum64(w->tmp.p, tb, x.n_win, x.n_win_scan, uint64_t(n) + 1, s));
    uint32_t n_heads = 0;
    uint64_t n_wins = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_heads, x.head_scan + n, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(&n_wins, x.n_win_scan + n, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(h_ix_files.data(), w->ix_files.p, n_files * sizeof(IndexFile), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    for (uint32_t k = 0; k < n_files; ++k) {
        const unsigned long long e = h_ix_files[k].err;
        if (e == ~0ull) continue;
        w->failed = k;
        const std::string where = record_where(pieces[k].df->path, 0, 0, e >> 8, Stage::kLoad);
        const uint32_t code = uint32_t(e & 0xFF);
        return fail(SECEDO_E_INVALID_ARG,
                    where + (code == kIndexErrRef   ? " has a RefID outside the reference list"
                             : code == kIndexErrEnd ? " ends past position 2^29: a BAI index cannot hold it"
                                                    : defect_tail(bw::kErrLonger)));
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

// ---- the stages of one batch, in run_batch's order

// Stage 1: where everything of the batch lies (bam_batch.hpp).
int lay_out(BamDevWork *w, const std::vector<Piece> &pieces) {
    if (lay_out_batch(pieces, w->chr_ids, w->index, &w->lay)) return SECEDO_OK;
    return fail(SECEDO_E_LIMIT, pieces[w->lay.overflow].df->path +
                                    ": a batch of 4 GiB or more of inflated BAM (a record that long, or "
                                    "SECEDO_BAM_BATCH_BYTES too large)");
}

// Stage 2: the compressed bytes into staging, the device buffers grown, staging and the layout's tables up.
int upload(BamDevWork *w, const std::vector<Piece> &pieces, uint32_t threads) {
    hipStream_t s = w->s;
    const BatchLayout &L = w->lay;
    const uint64_t n_members = L.desc.size(), n_seg = L.segs.size();
    if (L.in_bytes > w->h_in_cap) {
        if (w->h_in) SECEDO_TRY(hipHostFree(w->h_in));
        w->h_in = nullptr;
        w->h_in_cap = 0;
        const size_t cap = std::max<size_t>(L.in_bytes + L.in_bytes / 2, 1u << 20);
        SECEDO_TRY(hipHostMalloc(reinterpret_cast<void **>(&w->h_in), cap, hipHostMallocDefault));
        w->h_in_cap = cap;
    }
    parallel_for(threads, L.copies.size(),
                 [&](uint64_t c) { std::memcpy(w->h_in + L.copies[c].dst, L.copies[c].src, L.copies[c].n); });
    SECEDO_TRY(w->in.grow(L.in_bytes, 0, s));
    SECEDO_TRY(w->buf.grow(L.buf_bytes, pieces[0].first_range ? 0 : pieces[0].df->dev_carry, s));
    SECEDO_TRY(w->desc.grow(n_members, 0, s));
    SECEDO_TRY(w->status.grow(n_members, 0, s));
    SECEDO_TRY(w->segs.grow(n_seg, 0, s));
    SECEDO_TRY(w->walk.grow(n_seg, 0, s));
    SECEDO_TRY(w->join.grow(n_seg, 0, s));
    SECEDO_TRY(w->seg_cnt.grow(n_seg + 1, 0, s));
    SECEDO_TRY(w->seg_base.grow(n_seg + 1, 0, s));
    SECEDO_TRY(w->lists.grow(L.n_list, 0, s));
    SECEDO_TRY(w->rewalk.grow(L.n_list, 0, s));
    SECEDO_TRY(w->files.grow(L.files.size(), 0, s));
    SECEDO_TRY(w->runs.grow(L.runs.size(), 0, s));
    SECEDO_TRY(w->totals.grow(2, 0, s));
    if (L.any_span) {
        SECEDO_TRY(w->checks.grow(L.checks.size(), 0, s));
        SECEDO_TRY(hipMemcpyAsync(w->checks.p, L.checks.data(), L.checks.size() * sizeof(SpanCheck),
                                  hipMemcpyHostToDevice, s));
    }
    SECEDO_TRY(hipMemcpyAsync(w->in.p, w->h_in, L.in_bytes, hipMemcpyHostToDevice, s));
    if (n_members)
        SECEDO_TRY(hipMemcpyAsync(w->desc.p, L.desc.data(), n_members * sizeof(BgzfDesc), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(w->segs.p, L.segs.data(), n_seg * sizeof(bw::Seg), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(w->files.p, L.files.data(), L.files.size() * sizeof(WalkFile), hipMemcpyHostToDevice, s));
    if (!L.runs.empty())
        SECEDO_TRY(hipMemcpyAsync(w->runs.p, L.runs.data(), L.runs.size() * sizeof(WalkRun), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    return SECEDO_OK;
}

// Stage 3: every member of the batch inflated into the buffer.
int inflate_batch(BamDevWork *w) {
    SECEDO_TRY(bgzf_inflate(w->in.p, w->desc.p, uint32_t(w->lay.desc.size()), w->buf.p, w->status.p, w->s));
    SECEDO_TRY(hipStreamSynchronize(w->s));
    return SECEDO_OK;
}

// Stage 4: the walk up to the record count, then the record passes and their scans; the files, the runs, the span
// checks and the totals come back, and the route's counters take what the batch did.
int walk_and_scan(BamDevWork *w) {
    hipStream_t s = w->s;
    BatchLayout &L = w->lay;
    const uint32_t n_members = uint32_t(L.desc.size()), n_seg = uint32_t(L.segs.size());
    const uint32_t n_chr = uint32_t(w->chr_ids.size());
    const WalkBatch wb = w->walk_batch();
    SECEDO_TRY(walk_prepare(wb, w->in.p, w->desc.p, w->status.p, n_members, s));
    SECEDO_TRY(walk_segments(wb, s));
    SECEDO_TRY(hipMemsetAsync(w->seg_cnt.p + n_seg, 0, 4, s));
    size_t tb = scan_bytes(uint64_t(n_seg) + 1);
    SECEDO_TRY(w->tmp.grow(tb, 0, s));
    SECEDO_TRY(exclusive_sum(w->tmp.p, tb, w->seg_cnt.p, w->seg_base.p, uint64_t(n_seg) + 1, s));
    SECEDO_TRY(hipMemcpyAsync(&w->n_rec, w->seg_base.p + n_seg, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    const uint64_t n_rec = w->n_rec;
    SECEDO_TRY(w->r_off.grow(n_rec, 0, s));
    SECEDO_TRY(w->r_file.grow(n_rec, 0, s));
    SECEDO_TRY(w->r_ref.grow(n_rec, 0, s));
    SECEDO_TRY(w->r_pos.grow(n_rec, 0, s));
    SECEDO_TRY(w->sel.grow(n_rec + 1, 0, s));
    SECEDO_TRY(w->sel_scan.grow(n_rec + 1, 0, s));
    SECEDO_TRY(w->size.grow(n_rec + 1, 0, s));
    SECEDO_TRY(w->size_scan.grow(n_rec + 1, 0, s));
    const WalkRecords wr = w->walk_records();
    SECEDO_TRY(walk_records(wb, wr, w->chr.p, n_chr, w->runs.p, w->scan ? w->per_ref.p : nullptr, w->n_ref, s));
    if (L.any_span) {
        SECEDO_TRY(walk_span_check(wb, wr, n_chr, w->checks.p, s));
        SECEDO_TRY(hipMemcpyAsync(L.checks.data(), w->checks.p, L.checks.size() * sizeof(SpanCheck),
                                  hipMemcpyDeviceToHost, s));
    }
    tb = scan_bytes(n_rec + 1);
    SECEDO_TRY(w->tmp.grow(tb, 0, s));
    SECEDO_TRY(exclusive_sum(w->tmp.p, tb, w->sel.p, w->sel_scan.p, n_rec + 1, s));
    SECEDO_TRY(exclusive_sum64(w->tmp.p, tb, w->size.p, w->size_scan.p, n_rec + 1, s));
    SECEDO_TRY(walk_runs(wb, wr, n_chr, w->runs.p, w->totals.p, s));
    uint64_t totals[2] = {0, 0};
    SECEDO_TRY(hipMemcpyAsync(L.files.data(), w->files.p, L.files.size() * sizeof(WalkFile), hipMemcpyDeviceToHost, s));
    if (!L.runs.empty())
        SECEDO_TRY(hipMemcpyAsync(L.runs.data(), w->runs.p, L.runs.size() * sizeof(WalkRun), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(totals, w->totals.p, 16, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    w->n_sel = totals[0];
    w->sel_bytes = totals[1];
    route().device_blocks += n_members;
    route().segments += n_seg;
    route().uploaded_bytes += L.in_bytes;
    route().batches += 1;
    for (const WalkFile &F : L.files) {
        route().device_records += F.n_rec;
        route().rewalked_segments += F.rewalked;
    }
    return SECEDO_OK;
}

// Stage 5: the verdicts, per file in order: the RefID at a span's entry, then the walk's own errors, then what the
// index says of the span (its counts summed over its ranges, its tail on the last).
int verdicts(BamDevWork *w, const std::vector<Piece> &pieces) {
    const size_t n_chr = w->chr_ids.size();
    for (size_t k = 0; k < pieces.size(); ++k) {
        const Piece &p = pieces[k];
        const SpanCheck *checks = w->lay.checks.data() + k * n_chr;
        if (p.span) {
            index_info().members += p.b1 - p.b0;
            index_info().spans += p.first_range ? 1 : 0;
            const SpanChr &c0 = p.span->chrs[0];
            if (checks[slot_of(w->chr_ids, c0.chromosome)].entry_bad) return check_span_chr(p.df->path, c0, false, 0);
        }
        if (const int rc = file_error(*w, p, w->lay.first_member[k], w->lay.files[k])) {
            w->failed = uint32_t(k);
            return rc;
        }
        if (!p.span) continue;
        DevFile &df = *p.df;
        for (size_t u = 0; u < n_chr; ++u) {
            if (!(checks[u].flags & kSpanOn)) continue;
            df.sp_count[u] += checks[u].count;
            if (checks[u].start) df.sp_start[u] = checks[u].start == 1;
        }
        if (!p.final) continue;
        for (const SpanChr &sc : p.span->chrs) {
            const size_t u = slot_of(w->chr_ids, sc.chromosome);
            SECEDO_CALL(check_span_chr(df.path, sc, df.sp_start[u] != 0, df.sp_count[u]));
            if (checks[u].tail_bad) return span_tail_mismatch(df.path, sc);
        }
    }
    return SECEDO_OK;
}

// Stage 6: what came back must be consistent before it is used as an index.
int check_results(const BamDevWork &w, const std::vector<Piece> &pieces) {
    uint64_t sum_rec = 0;
    bool sane = w.n_sel <= w.n_rec && w.sel_bytes <= w.lay.out_bytes;
    for (const WalkFile &F : w.lay.files) {
        sum_rec += F.n_rec;
        sane = sane && F.stop_off <= F.data_end;
    }
    for (const WalkRun &run : w.lay.runs)
        sane = sane && run.j0 <= run.j1 && run.j1 <= w.n_sel && run.b0 <= run.b1 && run.b1 <= w.sel_bytes;
    if (!sane || sum_rec != w.n_rec)
        return fail(SECEDO_E_STATE, pieces[0].df->path + ": the device walk returned inconsistent results");
    return SECEDO_OK;
}

// Stage 7: the taken records gathered and brought back, with their offsets, Positions and file indexes.
int fetch_taken(BamDevWork *w) {
    hipStream_t s = w->s;
    const uint64_t n_sel = w->n_sel, sel_bytes = w->sel_bytes;
    if (!n_sel) return SECEDO_OK;
    SECEDO_TRY(w->out.grow(sel_bytes, 0, s));
    SECEDO_TRY(w->sel_off.grow(n_sel, 0, s));
    SECEDO_TRY(w->sel_pos.grow(n_sel, 0, s));
    SECEDO_TRY(w->sel_idx.grow(n_sel, 0, s));
    SECEDO_TRY(walk_gather(w->walk_batch(), w->walk_records(), w->out.p, w->sel_off.p, w->sel_pos.p, w->sel_idx.p, s));
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
    return SECEDO_OK;
}

// Stage 8, per file: its runs appended as FileSink appends them, the state the next range starts from, and the cut
// record to the front of the buffer (only a file that goes alone has a next range).
int append_runs(BamDevWork *w, const std::vector<Piece> &pieces, Inputs *in, Runs *runs) {
    hipStream_t s = w->s;
    const size_t n_chr = w->chr_ids.size();
    for (size_t k = 0; k < pieces.size(); ++k) {
        DevFile &df = *pieces[k].df;
        const WalkFile &F = w->lay.files[k];
        for (size_t u = 0; u < n_chr; ++u) {
            const WalkRun &run = w->lay.runs[k * n_chr + u];
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
        if (!pieces[k].final && df.dev_carry) {
            SECEDO_TRY(w->carry.grow(df.dev_carry, 0, s));
            SECEDO_TRY(hipMemcpyAsync(w->carry.p, w->buf.p + F.stop_off, df.dev_carry, hipMemcpyDeviceToDevice, s));
            SECEDO_TRY(hipMemcpyAsync(w->buf.p, w->carry.p, df.dev_carry, hipMemcpyDeviceToDevice, s));
        }
    }
    return SECEDO_OK;
}

// One batch through the device: inflate, walk, the taken records back into runs / in (both may be null: scan).
int run_batch(BamDevWork *w, std::vector<Piece> &pieces, uint32_t threads, Inputs *in, Runs *runs,
              secedo_bam_times *t) {
    Clock::time_point t0 = Clock::now();
    w->failed = UINT32_MAX;
    SECEDO_CALL(lay_out(w, pieces));
    SECEDO_CALL(upload(w, pieces, threads));
    if (t) t->upload_ms += ms_lap(t0);
    SECEDO_CALL(inflate_batch(w));
    if (t) {
        t->inflate_ms += ms_lap(t0);
        for (const BgzfDesc &d : w->lay.desc) t->inflated_bytes += double(d.isize);
    }
    SECEDO_CALL(walk_and_scan(w));
    SECEDO_CALL(verdicts(w, pieces));
    SECEDO_CALL(check_results(*w, pieces));
    if (w->index) SECEDO_CALL(index_batch(w, pieces));
    SECEDO_CALL(fetch_taken(w));
    SECEDO_CALL(append_runs(w, pieces, in, runs));
    if (t) t->walk_ms += ms_lap(t0);
    return SECEDO_OK;
}

// One file that inflates to more than a batch: ranges of members of about `batch` inflated bytes.
int run_ranges(BamDevWork *w, DevFile *df, const Span *span, uint32_t threads, uint64_t batch, Inputs *in, Runs *runs,
               secedo_bam_times *t) {
    const std::vector<Block> &bl = span ? span->blocks : df->blocks;
    for (size_t b0 = span ? 0 : df->hb;;) {
        // a file's tail of only empty members goes with its last range; a span has none
        const size_t b1 = bm::next_range(bl, b0, batch, span ? bm::kNoFold : df->total);
        std::vector<Piece> one{piece_of(df, b0, b1, b1 == bl.size(), span)};
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
            df->start(f, in->paths[f], n_chr);
            df->plan = &(*plans)[f];
            df->h = df->plan->h;
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
        pieces.push_back(piece_of(df.get(), df->hb, df->blocks.size(), true));
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
            pieces.push_back(piece_of(df.get(), 0, sp->blocks.size(), true, sp));
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
        pieces.push_back(piece_of(df.get(), df->hb, df->blocks.size(), true));
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
