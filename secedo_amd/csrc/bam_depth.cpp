// bam_depth.cpp -- secedo_bam_depth of include/secedo_bam.h: per-cell read depth in fixed genomic bins.
// The inputs come through the pileup's input layer (bam_host.hpp: load_inputs, one ChrInput per requested chromosome);
// per chromosome the records go up in input order and bam_depth_kernels.hip selects them, cuts them into (record, bin)
// pieces, sorts the pieces by global_bin * n_cells + cell and reduces the runs to the pairs in output order. The pairs
// of all chromosomes are held until the last one (the .mtx header needs their number), then the summaries run over
// them and the text of the per-pair, per-cell and per-bin files is formatted on the GPU in ranges, downloaded as it is
// or deflated by the shared BGZF encoder. The record upload and the compaction are bam_host.hpp's, the ranged
// formatter, the way down and the name upload text_out.hpp's, the temporary files out_files.hpp's. What decides
// numbers and bytes is in bam_depth.hpp.
#include "bam_depth.hpp"
#include "bam_depth_kernels.hpp"
#include "bam_host.hpp"
#include "bam_kernels.hpp"
#include "bam_split.hpp"
#include "bam_split_kernels.hpp"
#include "text_out.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <memory>

namespace {

using namespace secedo::bam_host;
namespace bam = secedo::bam;
namespace bs = secedo::bamsplit;
namespace bd = secedo::bamdepth;
namespace bz = secedo::bgzf;

thread_local secedo_bam_depth_info g_info{};

// what secedo_bam_depth_fetch copies out
struct Result {
    std::vector<uint32_t> bin_chr, bin_start, bin_end;
    std::vector<bd::Pair> pairs;
    std::vector<bd::CellRow> rows;
    std::vector<uint64_t> table;  // [bins][clusters]
    std::vector<std::string> chr_names;  // of the requested chromosomes, ascending id
    std::vector<uint32_t> chr_len;
};
thread_local Result *g_result = nullptr;

// What one call asks for, checked.
struct Request {
    std::vector<std::string> files, values, names;
    std::vector<uint32_t> chr;  // sorted
    std::vector<uint16_t> cluster;
    const char *tag = nullptr;
    uint32_t n_cells = 0, n_clusters = 0, S = 0, min_mapq = 0, require = 0, exclude = 0, threads = 1;
    int mode = SECEDO_BAM_DEPTH_READS, dup = SECEDO_BAM_DUPLICATES_KEEP;
    bool bgzf = false, overwrite = false, write = false;
    std::string out_dir;
};

// the per-cell counters and the drop counters of the front passes, kept over the chromosomes of one call
struct Counters {
    Dev<unsigned long long> cell_records, cell_counted, stat;
    int init(uint32_t n_cells, hipStream_t s) {
        SECEDO_TRY(cell_records.alloc(n_cells));
        SECEDO_TRY(cell_counted.alloc(n_cells));
        SECEDO_TRY(stat.alloc(bd::kStatSlots));
        SECEDO_TRY(hipMemsetAsync(cell_records.p, 0, n_cells * 8ull, s));
        SECEDO_TRY(hipMemsetAsync(cell_counted.p, 0, n_cells * 8ull, s));
        SECEDO_TRY(hipMemsetAsync(stat.p, 0, bd::kStatSlots * 8ull, s));
        return SECEDO_OK;
    }
};

using PairChunks = std::vector<std::unique_ptr<Dev<bd::Pair>>>;

// One chromosome: its records in HBM in input order -> its pairs in output order, appended to `chunks`.
int depth_chromosome(const Request &rq, const ChrInput &ci, uint32_t ln, uint64_t bin_base, int end_bit,
                     const bam::CellList *cells, Counters *cnt, PairChunks *chunks, hipStream_t s,
                     secedo_bam_times *t) {
    std::vector<uint64_t> in_off;
    Dev<uint8_t> d_bytes, tmp;
    Dev<uint64_t> d_in_off;
    Dev<uint16_t> d_file;  // stays null in tag mode
    SECEDO_CALL(upload_input_order(ci, s, &in_off, nullptr, &d_bytes, &d_in_off, cells ? nullptr : &d_file, t));
    const uint32_t n_in = uint32_t(in_off.size());
    if (n_in == 0) return SECEDO_OK;
    Clock::time_point t0 = Clock::now();

    // steps 1 and 2, the compaction, and with duplicates the order rule 3d's passes need
    Dev<uint64_t> tag_key, key, kc, ks;
    Dev<uint32_t> tag_sel, sel, vc, vs, dup_keep;
    Dev<uint16_t> d_cell;
    SECEDO_TRY(key.alloc(n_in));
    SECEDO_TRY(sel.alloc(size_t(n_in) + 1));
    SECEDO_TRY(d_cell.alloc(n_in));
    if (cells) {  // rule 3b of bam_kernels.hip, its flag filter off: step 2 is k_front's, which also counts per cell
        SECEDO_TRY(tag_key.alloc(n_in));
        SECEDO_TRY(tag_sel.alloc(n_in));
        SECEDO_TRY(bam::cells(d_bytes.p, d_in_off.p, n_in, *cells, 0, 0, tag_key.p, tag_sel.p, nullptr, s));
    }
    SECEDO_TRY(bd::depth_front(d_bytes.p, d_in_off.p, n_in, d_file.p, tag_key.p, tag_sel.p, rq.n_cells, rq.require,
                               rq.exclude, d_cell.p, sel.p, key.p, cnt->cell_records.p, cnt->stat.p, s));
    uint32_t m = 0;
    SECEDO_CALL(compact_selected(key, sel, n_in, s, &m, &kc, &vc));
    if (m == 0) {
        g_info.order_ms += ms_lap(t0);
        return SECEDO_OK;
    }
    const uint32_t *d_val = vc.p;
    if (rq.dup != SECEDO_BAM_DUPLICATES_KEEP) {
        // Sorted by Position (stable over the input order) the records of a cell stand in the pileup's global order,
        // as in secedo_bam_split_clusters_select, so rule 3d's passes choose the pileup's set.
        SECEDO_TRY(ks.alloc(m));
        SECEDO_TRY(vs.alloc(m));
        size_t tb = bs::split_sort_bytes(m);
        SECEDO_TRY(tmp.alloc(tb));
        SECEDO_TRY(bs::split_sort(tmp.p, tb, kc.p, ks.p, vc.p, vs.p, m, 32, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        key.reset(), sel.reset(), kc.reset(), vc.reset(), ks.reset(), tmp.reset();
        SelStat stat;
        SECEDO_CALL(stat.init(s));
        Dev<uint64_t> v_off;
        Dev<uint16_t> v_cell;
        SECEDO_TRY(v_off.alloc(m));
        SECEDO_TRY(v_cell.alloc(m));
        SECEDO_TRY(bs::split_view(d_in_off.p, vs.p, m, d_file.p, tag_key.p, v_off.p, v_cell.p, s));
        SECEDO_CALL(duplicate_keep(bam::Records{d_bytes.p, v_off.p, v_cell.p, m}, stat.d.p, s, &dup_keep));
        SECEDO_TRY(hipStreamSynchronize(s));  // v_off, v_cell and stat go with this scope
        d_val = vs.p;
    }
    g_info.order_ms += ms_lap(t0);

    // steps 3 to 5 and the pieces
    Dev<uint64_t> pieces, piece_off;
    SECEDO_TRY(pieces.alloc(size_t(m) + 1));
    SECEDO_TRY(piece_off.alloc(size_t(m) + 1));
    SECEDO_TRY(bd::depth_count(d_bytes.p, d_in_off.p, d_val, m, d_cell.p, dup_keep.p, rq.min_mapq, ln, rq.S, rq.mode,
                               pieces.p, cnt->cell_counted.p, cnt->stat.p, s));
    size_t tb = bam::scan_bytes(uint64_t(m) + 1);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(bam::exclusive_sum64(tmp.p, tb, pieces.p, piece_off.p, uint64_t(m) + 1, s));
    uint64_t n_pieces64 = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_pieces64, piece_off.p + m, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (n_pieces64 > 0xFFFFFFFFull)
        return fail(SECEDO_E_LIMIT, "chromosome id " + std::to_string(ci.chromosome) + " has " +
                                        std::to_string(n_pieces64) + " pieces, more than the 2^32 - 1 one sort takes; "
                                        "use a larger bin_size");
    const uint32_t n_pieces = uint32_t(n_pieces64);
    if (n_pieces == 0) {
        g_info.count_ms += ms_lap(t0);
        return SECEDO_OK;
    }
    Dev<uint64_t> pk, pks;
    Dev<uint32_t> pv, pvs;
    SECEDO_TRY(pk.alloc(n_pieces));
    SECEDO_TRY(pv.alloc(n_pieces));
    SECEDO_TRY(bd::depth_emit(d_bytes.p, d_in_off.p, d_val, m, d_cell.p, piece_off.p, n_pieces, ln, rq.S, rq.mode,
                              bin_base, rq.n_cells, pk.p, pv.p, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    d_bytes.reset(), d_in_off.reset(), d_file.reset(), tag_key.reset(), tag_sel.reset(), key.reset(), sel.reset();
    kc.reset(), vc.reset(), vs.reset(), dup_keep.reset(), d_cell.reset(), pieces.reset();
    piece_off.reset();

    // sort and reduce
    SECEDO_TRY(pks.alloc(n_pieces));
    SECEDO_TRY(pvs.alloc(n_pieces));
    tb = bd::depth_sort_bytes(n_pieces);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(bd::depth_sort(tmp.p, tb, pk.p, pks.p, pv.p, pvs.p, n_pieces, end_bit, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    pk.reset(), pv.reset();
    Dev<uint32_t> head, run, start, keep, at;
    Dev<uint64_t> wide, sum;
    SECEDO_TRY(head.alloc(size_t(n_pieces) + 1));
    SECEDO_TRY(run.alloc(size_t(n_pieces) + 1));
    SECEDO_TRY(wide.alloc(size_t(n_pieces) + 1));
    SECEDO_TRY(sum.alloc(size_t(n_pieces) + 1));
    SECEDO_TRY(bd::depth_heads(pks.p, pvs.p, n_pieces, head.p, wide.p, s));
    tb = bam::scan_bytes(uint64_t(n_pieces) + 1);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(bam::exclusive_sum(tmp.p, tb, head.p, run.p, uint64_t(n_pieces) + 1, s));
    SECEDO_TRY(bam::exclusive_sum64(tmp.p, tb, wide.p, sum.p, uint64_t(n_pieces) + 1, s));
    uint32_t n_runs = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_runs, run.p + n_pieces, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    Dev<bd::Pair> all;
    SECEDO_TRY(start.alloc(size_t(n_runs) + 1));
    SECEDO_TRY(all.alloc(n_runs));
    SECEDO_TRY(keep.alloc(size_t(n_runs) + 1));
    SECEDO_TRY(at.alloc(size_t(n_runs) + 1));
    SECEDO_TRY(bd::depth_run_starts(head.p, run.p, n_pieces, start.p, s));
    SECEDO_TRY(bd::depth_run_sums(pks.p, start.p, sum.p, n_runs, rq.n_cells, all.p, keep.p, s));
    tb = bam::scan_bytes(uint64_t(n_runs) + 1);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(bam::exclusive_sum(tmp.p, tb, keep.p, at.p, uint64_t(n_runs) + 1, s));
    uint32_t n_pairs = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_pairs, at.p + n_runs, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (n_pairs) {
        std::unique_ptr<Dev<bd::Pair>> out(new Dev<bd::Pair>);
        SECEDO_TRY(out->alloc(n_pairs));
        SECEDO_TRY(bd::depth_compact(all.p, keep.p, at.p, n_runs, out->p, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        chunks->push_back(std::move(out));
    }
    g_info.pieces += n_pieces;
    g_info.pairs += n_pairs;
    g_info.count_ms += ms_lap(t0);
    return SECEDO_OK;
}

int write_files(const Request &rq, const bd::Layout &lay, const std::vector<bs::Ref> &refs, const Result &res,
                const bd::Pair *d_pairs, const bd::CellRow *d_rows, const uint64_t *d_table, OutFiles *of,
                TextCounts *tc, hipStream_t s) {
    Clock::time_point t0 = Clock::now();
    SECEDO_CALL(out_error(of->open()));
    {  // the two host-written files
        std::string bed, samples;
        for (size_t g = 0; g < res.bin_chr.size(); ++g)
            bed += bd::bed_line(refs[res.bin_chr[g]].name, res.bin_start[g], res.bin_end[g]);
        for (const std::string &n : rq.names) samples += n + "\n";
        SECEDO_CALL(out_error(of->append(0, bed.data(), bed.size())));
        SECEDO_CALL(out_error(of->append(1, samples.data(), samples.size())));
    }
    g_info.write_ms += ms_lap(t0);
    const uint64_t batch = text_batch_bytes("SECEDO_DEPTH_BATCH_BYTES");
    const Scan64 scan{bam::scan_bytes, bam::exclusive_sum64};
    bz::Encoder enc(kSlice);
    Formatter fm;
    DevNames cell_names, chr_names;
    SECEDO_CALL(upload_names(rq.names, s, &cell_names));
    {
        TextOut out{of, 2, rq.bgzf, &enc, s, tc, {}, {}};
        SECEDO_CALL(out.host(bd::mtx_header(lay.n_bins(), rq.n_cells, res.pairs.size())));
        SECEDO_CALL(fm.run(
            res.pairs.size(), bd::lines_per_range(batch, bd::kMaxMtxLine), bd::kMaxMtxLine,
            [&](uint64_t i0, uint32_t n, uint64_t *len) { return bd::mtx_measure(d_pairs, i0, n, len, s); },
            [&](uint64_t i0, uint32_t n, const uint64_t *off, uint8_t *text) {
                return bd::mtx_write(d_pairs, i0, n, off, text, s);
            },
            scan, &out, s));
        SECEDO_CALL(out.finish());
    }
    {
        TextOut out{of, 3, rq.bgzf, &enc, s, tc, {}, {}};
        SECEDO_CALL(out.host(bd::cells_header()));
        const bd::Names names = cell_names.view();
        const uint64_t max_line = bd::max_cell_line(cell_names.longest);
        SECEDO_CALL(fm.run(
            rq.n_cells, bd::lines_per_range(batch, max_line), max_line,
            [&](uint64_t i0, uint32_t n, uint64_t *len) {
                return bd::cells_measure(d_rows, names, uint32_t(i0), n, len, s);
            },
            [&](uint64_t i0, uint32_t n, const uint64_t *off, uint8_t *text) {
                return bd::cells_write(d_rows, names, uint32_t(i0), n, off, text, s);
            },
            scan, &out, s));
        SECEDO_CALL(out.finish());
    }
    if (rq.n_clusters) {
        std::vector<std::string> names;
        for (uint32_t c : lay.chr) names.push_back(refs[c].name);
        SECEDO_CALL(upload_names(names, s, &chr_names));
        Dev<uint64_t> d_base;
        Dev<uint32_t> d_len;
        SECEDO_TRY(d_base.alloc(lay.base.size()));
        SECEDO_TRY(d_len.alloc(lay.len.size()));
        SECEDO_TRY(hipMemcpyAsync(d_base.p, lay.base.data(), lay.base.size() * 8, hipMemcpyHostToDevice, s));
        if (!lay.len.empty())
            SECEDO_TRY(hipMemcpyAsync(d_len.p, lay.len.data(), lay.len.size() * 4, hipMemcpyHostToDevice, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        const bd::BinTable bt{d_base.p, d_len.p, uint32_t(lay.chr.size()), rq.S, chr_names.view(), d_table,
                              rq.n_clusters};
        const uint64_t max_line = bd::max_cluster_line(chr_names.longest, rq.n_clusters);
        TextOut out{of, 4, rq.bgzf, &enc, s, tc, {}, {}};
        SECEDO_CALL(out.host(bd::clusters_header(rq.n_clusters)));
        SECEDO_CALL(fm.run(
            lay.n_bins(), bd::lines_per_range(batch, max_line), max_line,
            [&](uint64_t i0, uint32_t n, uint64_t *len) { return bd::clusters_measure(bt, i0, n, len, s); },
            [&](uint64_t i0, uint32_t n, const uint64_t *off, uint8_t *text) {
                return bd::clusters_write(bt, i0, n, off, text, s);
            },
            scan, &out, s));
        SECEDO_CALL(out.finish());
    }
    (void)ms_lap(t0);
    SECEDO_CALL(out_error(of->commit()));
    g_info.write_ms += ms_lap(t0);
    return SECEDO_OK;
}

int depth(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids, uint32_t n_chr,
          const char *tag, const char *const *barcodes, uint32_t n_barcodes, uint32_t bin_size, int mode,
          uint32_t min_map_quality, uint32_t require, uint32_t exclude, int duplicates, const uint16_t *clustering,
          uint32_t n_clustering, const char *const *cell_names, uint32_t n_names, const char *out_dir, int output,
          int overwrite, uint32_t num_threads, secedo_bam_times *times) {
    const Clock::time_point t_all = Clock::now();
    secedo_bam_times tl{};
    if ((n_files && !bam_files) || (n_chr && !chromosome_ids)) return fail(SECEDO_E_INVALID_ARG, "null argument");
    Request rq;
    // everything that needs no input, before any is read
    if (bin_size == 0) return fail(SECEDO_E_INVALID_ARG, "secedo_bam_depth: bin_size is 0, at least 1 is needed");
    if (mode != SECEDO_BAM_DEPTH_READS && mode != SECEDO_BAM_DEPTH_BASES)
        return fail(SECEDO_E_INVALID_ARG, "secedo_bam_depth: mode " + std::to_string(mode) +
                                              " is neither SECEDO_BAM_DEPTH_READS nor SECEDO_BAM_DEPTH_BASES");
    if (output != SECEDO_BAM_DEPTH_PLAIN && output != SECEDO_BAM_DEPTH_BGZF)
        return fail(SECEDO_E_INVALID_ARG, "secedo_bam_depth: output " + std::to_string(output) +
                                              " is neither SECEDO_BAM_DEPTH_PLAIN nor SECEDO_BAM_DEPTH_BGZF");
    {
        const std::string why = bs::masks_fault(require, exclude);
        if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, "secedo_bam_depth: " + why);
    }
    if (duplicates != SECEDO_BAM_DUPLICATES_KEEP && duplicates != SECEDO_BAM_DUPLICATES_REMOVE)
        return fail(SECEDO_E_INVALID_ARG, "secedo_bam_depth: duplicates " + std::to_string(duplicates) +
                                              " is neither SECEDO_BAM_DUPLICATES_KEEP nor _REMOVE");
    if (min_map_quality > 255) return fail(SECEDO_E_INVALID_ARG, "secedo_bam_depth: min_map_quality is at most 255");
    rq.S = bin_size, rq.mode = mode, rq.min_mapq = min_map_quality, rq.require = require, rq.exclude = exclude;
    rq.dup = duplicates, rq.bgzf = output == SECEDO_BAM_DEPTH_BGZF, rq.overwrite = overwrite != 0;
    rq.tag = tag;
    rq.threads = num_threads ? num_threads : 1;
    if (n_files == 0) return fail(SECEDO_E_INVALID_ARG, "no input files");
    if (tag) {
        SECEDO_CALL(check_cells(tag, barcodes, n_barcodes, &rq.values));
        rq.n_cells = n_barcodes;
    } else {
        if (n_files > SECEDO_BAM_MAX_FILES)
            return fail(SECEDO_E_LIMIT, "more than 16384 BAM files: cell ids do not fit 14 bits");
        rq.n_cells = n_files;
    }
    SECEDO_CALL(check_files(bam_files, n_files, &rq.files));
    if (cell_names) {
        if (n_names != rq.n_cells)
            return fail(SECEDO_E_INVALID_ARG, std::to_string(n_names) + " cell names for " +
                                                  std::to_string(rq.n_cells) + " cells");
        for (uint32_t c = 0; c < n_names; ++c) rq.names.push_back(cell_names[c] ? cell_names[c] : "");
    } else if (tag) {
        rq.names = rq.values;
    } else {
        for (const std::string &f : rq.files) rq.names.push_back(bs::default_name(f));
    }
    {
        const std::string why = bd::cell_names_fault(rq.names);
        if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, why);
    }
    if (clustering) {
        if (n_clustering != rq.n_cells)
            return fail(SECEDO_E_INVALID_ARG, "the clustering has " + std::to_string(n_clustering) +
                                                  " cells, there are " + std::to_string(rq.n_cells) + " cells");
        rq.cluster.assign(clustering, clustering + n_clustering);
        rq.n_clusters = uint32_t(*std::max_element(rq.cluster.begin(), rq.cluster.end())) + 1;
    }
    rq.chr.assign(chromosome_ids, chromosome_ids + n_chr);
    std::sort(rq.chr.begin(), rq.chr.end());
    for (size_t c = 1; c < rq.chr.size(); ++c)
        if (rq.chr[c] == rq.chr[c - 1])
            return fail(SECEDO_E_INVALID_ARG, "chromosome id " + std::to_string(rq.chr[c]) + " is listed twice");
    g_info.files = n_files;
    g_info.cells = rq.n_cells;
    g_info.chromosomes = n_chr;
    g_info.clusters = rq.n_clusters;

    OutFiles of;
    if (out_dir) {
        rq.write = true;
        rq.out_dir = out_dir;
        struct stat st;
        if (stat(rq.out_dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode))
            return fail(SECEDO_E_INVALID_ARG, rq.out_dir + " is not a directory");
        of.dir = rq.out_dir + "/depth";
        const std::string gz = rq.bgzf ? ".gz" : "";
        of.target = {of.dir + "/depth.bins.bed", of.dir + "/depth.samples.tsv", of.dir + "/depth.counts.mtx" + gz,
                     of.dir + "/depth.cells.tsv" + gz};
        if (rq.n_clusters) of.target.push_back(of.dir + "/depth.clusters.tsv" + gz);
        for (const std::string &t : of.target)
            if (!rq.overwrite && stat(t.c_str(), &st) == 0)
                return fail(SECEDO_E_INVALID_ARG, t + " exists; pass overwrite to replace it");
    }

    // the bins, from the first input's reference list
    std::vector<bs::Ref> refs;
    {
        std::vector<uint8_t> list;
        std::vector<std::string> texts;
        SECEDO_CALL(read_reference_lists(rq.files, &refs, &list, &texts));
    }
    bd::Layout lay;
    {
        std::vector<uint32_t> ref_len;
        for (const bs::Ref &r : refs) ref_len.push_back(r.len);
        bool limit = false;
        const std::string why = bd::make_layout(ref_len, rq.chr, rq.S, &lay, &limit);
        if (!why.empty())
            return fail(limit ? SECEDO_E_LIMIT : SECEDO_E_INVALID_ARG, "secedo_bam_depth: " + why + " (" + rq.files[0] + ")");
    }
    g_info.bins = lay.n_bins();
    std::unique_ptr<Result> res(new Result);
    for (size_t k = 0; k < lay.chr.size(); ++k)
        for (uint64_t b = 0; b < lay.base[k + 1] - lay.base[k]; ++b) {
            res->bin_chr.push_back(lay.chr[k]);
            res->bin_start.push_back(bd::bin_start(uint32_t(b), rq.S));
            res->bin_end.push_back(bd::bin_end(uint32_t(b), rq.S, lay.len[k]));
        }

    for (size_t k = 0; k < lay.chr.size(); ++k) {
        res->chr_names.push_back(refs[lay.chr[k]].name);
        res->chr_len.push_back(lay.len[k]);
    }

    Inputs in;
    SECEDO_CALL(load_inputs(rq.files, rq.chr.data(), n_chr, rq.threads, &in, &tl));

    StreamGuard guard;
    SECEDO_TRY(hipStreamCreateWithFlags(&guard.s, hipStreamNonBlocking));
    const hipStream_t s = guard.s;
    DevCells dc;
    if (tag) SECEDO_CALL(upload_cells(tag, rq.values, s, &dc));
    Counters cnt;
    SECEDO_CALL(cnt.init(rq.n_cells, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    const int end_bit = bd::key_bits(std::max<uint64_t>(lay.n_bins(), 1), rq.n_cells);

    PairChunks chunks;
    for (uint32_t c = 0; c < n_chr; ++c) {  // in.chrs follows rq.chr: ascending ids, so the chunks are in output order
        SECEDO_CALL(depth_chromosome(rq, in.chrs[c], lay.len[c], lay.base[c], end_bit, tag ? &dc.list : nullptr, &cnt,
                                     &chunks, s, &tl));
        std::vector<uint8_t>().swap(in.chrs[c].bytes);
    }

    // the pairs of the call in one array, the counters, the summaries
    Clock::time_point t0 = Clock::now();
    const uint64_t n_pairs = g_info.pairs;
    Dev<bd::Pair> d_pairs;
    SECEDO_TRY(d_pairs.alloc(n_pairs));
    {
        uint64_t at = 0;
        for (const auto &ch : chunks) {
            SECEDO_TRY(hipMemcpyAsync(d_pairs.p + at, ch->p, ch->n * sizeof(bd::Pair), hipMemcpyDeviceToDevice, s));
            at += ch->n;
        }
        SECEDO_TRY(hipStreamSynchronize(s));
        chunks.clear();
    }
    std::vector<unsigned long long> h_rec(rq.n_cells), h_cnt(rq.n_cells), h_stat(bd::kStatSlots);
    SECEDO_TRY(hipMemcpyAsync(h_rec.data(), cnt.cell_records.p, rq.n_cells * 8ull, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(h_cnt.data(), cnt.cell_counted.p, rq.n_cells * 8ull, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(h_stat.data(), cnt.stat.p, bd::kStatSlots * 8ull, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    g_info.records = h_stat[bd::kStatRecords];
    g_info.counted = h_stat[bd::kStatCounted];
    g_info.dropped_barcode = h_stat[bd::kStatBarcode];
    g_info.dropped_require = h_stat[bd::kStatRequire];
    g_info.dropped_exclude = h_stat[bd::kStatExclude];
    g_info.dropped_duplicate = h_stat[bd::kStatDuplicate];
    g_info.dropped_mapq = h_stat[bd::kStatMapq];
    g_info.out_of_range = h_stat[bd::kStatRange];
    res->rows.assign(rq.n_cells, bd::CellRow{0, 0, 0, 0, 0});
    for (uint32_t c = 0; c < rq.n_cells; ++c) res->rows[c].records = h_rec[c], res->rows[c].counted = h_cnt[c];
    Dev<bd::CellRow> d_rows;
    Dev<uint64_t> d_table;
    Dev<uint16_t> d_cluster;
    SECEDO_TRY(d_rows.alloc(rq.n_cells));
    SECEDO_TRY(hipMemcpyAsync(d_rows.p, res->rows.data(), rq.n_cells * sizeof(bd::CellRow), hipMemcpyHostToDevice, s));
    const uint64_t table_n = lay.n_bins() * rq.n_clusters;
    if (rq.n_clusters) {
        SECEDO_TRY(d_table.alloc(table_n));
        SECEDO_TRY(hipMemsetAsync(d_table.p, 0, table_n * 8, s));
        SECEDO_TRY(d_cluster.alloc(rq.n_cells));
        SECEDO_TRY(hipMemcpyAsync(d_cluster.p, rq.cluster.data(), rq.n_cells * 2ull, hipMemcpyHostToDevice, s));
    }
    SECEDO_TRY(bd::depth_summaries(d_pairs.p, n_pairs, d_rows.p, d_cluster.p, rq.n_clusters, d_table.p, s));
    res->pairs.resize(n_pairs);
    res->table.resize(table_n);
    if (n_pairs)
        SECEDO_TRY(hipMemcpyAsync(res->pairs.data(), d_pairs.p, n_pairs * sizeof(bd::Pair), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(res->rows.data(), d_rows.p, rq.n_cells * sizeof(bd::CellRow), hipMemcpyDeviceToHost, s));
    if (table_n) SECEDO_TRY(hipMemcpyAsync(res->table.data(), d_table.p, table_n * 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    g_info.count_ms += ms_lap(t0);

    if (rq.write) {
        TextCounts tc;  // what the text layer did, also where it failed
        const int rc = write_files(rq, lay, refs, *res, d_pairs.p, d_rows.p, d_table.p, &of, &tc, s);
        g_info.text_bytes += tc.text_bytes, g_info.compressed_bytes += tc.compressed_bytes;
        g_info.members += tc.members, g_info.ranges += tc.ranges;
        g_info.format_ms += tc.format_ms, g_info.deflate_ms += tc.deflate_ms;
        g_info.download_ms += tc.download_ms, g_info.write_ms += tc.write_ms;
        SECEDO_CALL(rc);
    }
    delete g_result;
    g_result = res.release();
    tl.device_ms += g_info.order_ms + g_info.count_ms + g_info.format_ms + g_info.deflate_ms + g_info.download_ms;
    tl.write_ms += g_info.write_ms;
    tl.total_ms = ms_since(t_all);
    if (times) *times = tl;
    return SECEDO_OK;
}

}  // namespace

namespace secedo {
namespace bam_host {
void release_depth() {
    delete g_result;
    g_result = nullptr;
}
}  // namespace bam_host
}  // namespace secedo

extern "C" {

int secedo_bam_depth(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids, uint32_t n_chr,
                     const char tag[2], const char *const *barcodes, uint32_t n_barcodes, uint32_t bin_size, int mode,
                     uint32_t min_map_quality, uint32_t require, uint32_t exclude, int duplicates,
                     const uint16_t *clustering, uint32_t n_clustering, const char *const *cell_names,
                     uint32_t n_names, const char *out_dir, int output, int overwrite, uint32_t num_threads,
                     secedo_bam_depth_info *info, secedo_bam_times *times) {
    if (!info) return fail(SECEDO_E_INVALID_ARG, "null argument");
    g_info = secedo_bam_depth_info{};
    release_depth();
    const int rc = depth(bam_files, n_files, chromosome_ids, n_chr, tag, barcodes, n_barcodes, bin_size, mode,
                         min_map_quality, require, exclude, duplicates, clustering, n_clustering, cell_names, n_names,
                         out_dir, output, overwrite, num_threads, times);
    *info = g_info;
    return rc;
}

int secedo_bam_depth_fetch(uint32_t *bin_chr, uint32_t *bin_start, uint32_t *bin_end, uint32_t *pair_bin,
                           uint32_t *pair_cell, uint64_t *pair_value, uint64_t *cell_table, uint64_t *cluster_sums) {
    if (!g_result) return fail(SECEDO_E_STATE, "no depth result: call secedo_bam_depth first");
    const Result &r = *g_result;
    if (bin_chr) std::copy(r.bin_chr.begin(), r.bin_chr.end(), bin_chr);
    if (bin_start) std::copy(r.bin_start.begin(), r.bin_start.end(), bin_start);
    if (bin_end) std::copy(r.bin_end.begin(), r.bin_end.end(), bin_end);
    for (size_t i = 0; i < r.pairs.size(); ++i) {
        if (pair_bin) pair_bin[i] = r.pairs[i].bin;
        if (pair_cell) pair_cell[i] = r.pairs[i].cell;
        if (pair_value) pair_value[i] = r.pairs[i].value;
    }
    if (cell_table)
        for (size_t c = 0; c < r.rows.size(); ++c) {
            const uint64_t v[bd::kCellColumns] = {r.rows[c].records, r.rows[c].counted, r.rows[c].sum,
                                                  r.rows[c].nonzero_bins, r.rows[c].max_value};
            std::copy(v, v + bd::kCellColumns, cell_table + c * bd::kCellColumns);
        }
    if (cluster_sums) std::copy(r.table.begin(), r.table.end(), cluster_sums);
    return SECEDO_OK;
}

int secedo_bam_depth_chromosomes(char *names, uint64_t capacity, uint64_t *name_off, uint32_t *lengths,
                                 uint64_t *name_bytes) {
    if (!g_result) return fail(SECEDO_E_STATE, "no depth result: call secedo_bam_depth first");
    const Result &r = *g_result;
    uint64_t total = 0;
    for (const std::string &n : r.chr_names) total += n.size();
    if (name_bytes) *name_bytes = total;
    if (names && capacity < total)
        return fail(SECEDO_E_LIMIT, "the chromosome names take " + std::to_string(total) + " bytes");
    uint64_t at = 0;
    for (size_t k = 0; k < r.chr_names.size(); ++k) {
        if (name_off) name_off[k] = at;
        if (names) std::copy(r.chr_names[k].begin(), r.chr_names[k].end(), names + at);
        at += r.chr_names[k].size();
    }
    if (name_off) name_off[r.chr_names.size()] = at;
    if (lengths) std::copy(r.chr_len.begin(), r.chr_len.end(), lengths);
    return SECEDO_OK;
}

int secedo_bam_depth_stats(secedo_bam_depth_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = g_info;
    return SECEDO_OK;
}

}  // extern "C"
