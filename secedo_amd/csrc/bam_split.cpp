// bam_split.cpp -- secedo_bam_split_clusters of include/secedo_bam.h: one coordinate-sorted BAM per
// cluster of a clustering. The inputs come through the pileup's input layer (bam_host.hpp: load_inputs, one ChrInput
// per requested chromosome); per chromosome the records go up in input order and bam_split_kernels.hip turns them into
// one stream, cluster after cluster, which the BGZF encoder (bgzf_deflate_kernels.hip) deflates member by member. Only
// compressed bytes come back; they are appended to the clusters' temporary files (out_files.hpp, reopened per append).
// The record upload and the compaction are bam_host.hpp's. What decides bytes is in bam_split.hpp. secedo_bam_split_clusters_rg is the same call with a gather that edits the records on
// the way: every record gets RG:Z:<its cell's name>, the header one @RG line per cell of the cluster.
// secedo_bam_split_clusters_select selects records on the way: the flag filter in front of the compaction,
// rule 3d's passes (bam_host.hpp: duplicate_keep) over the sorted records, whose choice is removed before the lengths
// or carried to the gather as a mark.
#include "bam_host.hpp"
#include "bam_kernels.hpp"
#include "bam_split.hpp"
#include "bam_split_kernels.hpp"
#include "text_out.hpp"

#include <sys/stat.h>

#include <algorithm>

namespace {

using namespace secedo::bam_host;
namespace bam = secedo::bam;
namespace bs = secedo::bamsplit;
namespace bz = secedo::bgzf;

thread_local secedo_bam_split_info g_split{};
thread_local secedo_bam_split_rg_info g_rg{};
thread_local secedo_bam_select_info g_sel{};

// the gather's stream lies behind this much room (the encoder's 16-byte loads); keeps the stream 16-byte aligned
constexpr uint64_t kFront = bz::kDeflateInSlack;
static_assert(kFront % bs::kGatherVec == 0, "the gather stores whole aligned vectors");

bool exists(const std::string &path) {
    struct stat st;
    return stat(path.c_str(), &st) == 0;
}

// The members desc of the text at d_text go through the encoder (kept over the header and the chromosomes of one
// call) and member k is appended to file owner[k]; owners ascend, so every file gets its members in stream order.
int encode_to_files(bz::Encoder *enc, const uint8_t *d_text, const std::vector<bz::DeflateDesc> &desc,
                    const std::vector<uint32_t> &owner, OutFiles *of, hipStream_t s) {
    const int rc = enc->run(d_text, desc, s, [&](size_t b0, uint32_t n, const uint32_t *bytes, uint64_t *at) -> int {
        uint64_t end = 0;
        for (uint32_t k = 0; k < n; ++k) {
            at[k] = end;
            end += bytes[k];
        }
        SECEDO_CALL(enc->fetch(end, &enc->bytes, 0));
        Clock::time_point t0 = Clock::now();
        for (uint32_t k = 0; k < n;) {  // the members of one file in one write
            uint32_t e = k + 1;
            while (e < n && owner[b0 + e] == owner[b0 + k]) ++e;
            const uint64_t stop = e < n ? at[e] : end;
            SECEDO_CALL(out_error(of->append(owner[b0 + k], enc->bytes.data() + at[k], stop - at[k])));
            k = e;
        }
        g_split.compressed_bytes += end;
        g_split.write_ms += ms_since(t0);
        return SECEDO_OK;
    });
    g_split.members += enc->counts.members;
    g_split.stored_members += enc->counts.stored_members;
    g_split.deflate_ms += enc->counts.deflate_ms;
    g_split.download_ms += enc->counts.download_ms;
    enc->counts = bz::EncoderCounts{};  // taken
    return rc;
}

// What one call asks for, checked.
struct Request {
    std::vector<std::string> files, values;
    std::vector<uint32_t> chr;  // sorted
    std::vector<uint16_t> cell_cluster;
    const char *tag = nullptr;
    uint32_t n_clusters = 0;
    uint32_t threads = 1;
    bool rg = false;                 // the _rg call: records are edited, the header names the cells
    std::vector<std::string> names;  // with rg: the read group of each cell
    uint32_t require = 0, exclude = 0;  // the _select call: rule 1, 0 and 0 = off
    int dup = SECEDO_BAM_DUPLICATES_KEEP;  // the _select call: rule 2, _KEEP = off
    bool filter() const { return (require | exclude) != 0; }
    bool select() const { return filter() || dup != SECEDO_BAM_DUPLICATES_KEEP; }
};

// The suffixes RGZ<name>\0 of all cells on the device, one after the other; off[c] .. off[c + 1] is cell c's.
struct DevSuffixes {
    Dev<uint8_t> bytes;
    Dev<uint32_t> off;
};

int upload_suffixes(const std::vector<std::string> &names, hipStream_t s, DevSuffixes *ds) {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off{0};
    for (const std::string &n : names) {
        const std::string suffix = bs::rg_suffix(n);
        bytes.insert(bytes.end(), suffix.begin(), suffix.end());
        off.push_back(uint32_t(bytes.size()));
    }
    bytes.resize(bytes.size() + 16, 0);  // room behind the last suffix, as behind the last record
    SECEDO_TRY(ds->bytes.alloc(bytes.size()));
    SECEDO_TRY(ds->off.alloc(off.size()));
    SECEDO_TRY(hipMemcpyAsync(ds->bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(ds->off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    return SECEDO_OK;
}

// One chromosome: its records in HBM in input order -> the stream -> members appended to the clusters' files.
int split_chromosome(const Request &rq, const ChrInput &ci, const bam::CellList *cells, const uint16_t *d_cell_cluster,
                     const DevSuffixes *suffixes, bz::Encoder *enc, OutFiles *of, hipStream_t s, secedo_bam_times *t) {
    std::vector<uint64_t> in_off;
    Dev<uint8_t> d_bytes, tmp;
    Dev<uint64_t> d_in_off;
    Dev<uint16_t> d_file;  // stays null in tag mode
    SECEDO_CALL(upload_input_order(ci, s, &in_off, nullptr, &d_bytes, &d_in_off, cells ? nullptr : &d_file, t));
    const uint32_t n_in = uint32_t(in_off.size());
    if (n_in == 0) return SECEDO_OK;
    Clock::time_point t0 = Clock::now();

    // keys, compaction, order
    const uint32_t n_cells = uint32_t(rq.cell_cluster.size());
    Dev<uint64_t> tag_key, key, kc, ks;
    Dev<uint32_t> tag_sel, sel, scan, vc, vs;
    SelStat stat;  // stays unallocated in the plain and _rg calls
    if (rq.select()) SECEDO_CALL(stat.init(s));
    // what the selection counted goes to the call's stats; dropped_records stays the records without a cell
    const auto take_stats = [&]() -> int {
        const uint64_t before = g_sel.dropped_require + g_sel.dropped_exclude;
        SECEDO_CALL(stat.add_to(s, &g_sel));
        g_split.dropped_records -= g_sel.dropped_require + g_sel.dropped_exclude - before;
        return SECEDO_OK;
    };
    SECEDO_TRY(key.alloc(n_in));
    SECEDO_TRY(sel.alloc(size_t(n_in) + 1));
    if (cells) {  // rule 3b of bam_kernels.hip, with its flag filter (3c) in the _select call: the cell from the tag
        SECEDO_TRY(tag_key.alloc(n_in));
        SECEDO_TRY(tag_sel.alloc(n_in));
        SECEDO_TRY(bam::cells(d_bytes.p, d_in_off.p, n_in, *cells, rq.require, rq.exclude, tag_key.p, tag_sel.p,
                              rq.filter() ? stat.d.p : nullptr, s));
    }
    SECEDO_TRY(bs::split_keys(d_bytes.p, d_in_off.p, n_in, d_file.p, tag_key.p, tag_sel.p, d_cell_cluster, n_cells,
                              key.p, sel.p, s));
    if (rq.filter() && !cells) {  // rule 3c in per-file mode: the flag test joins the selection (all have a cell)
        Dev<uint32_t> pass;
        SECEDO_TRY(pass.alloc(n_in));
        SECEDO_TRY(bam::flag_test(bam::Records{d_bytes.p, d_in_off.p, d_file.p, n_in}, rq.require, rq.exclude, pass.p,
                                  stat.d.p, s));
        SECEDO_TRY(bs::split_and(sel.p, pass.p, n_in, s));
        SECEDO_TRY(hipStreamSynchronize(s));  // pass goes with this scope
    }
    uint32_t m = 0;
    SECEDO_CALL(compact_selected(key, sel, n_in, s, &m, &kc, &vc));
    g_split.dropped_records += n_in - m;
    if (m == 0) {
        SECEDO_CALL(take_stats());
        g_split.order_ms += ms_lap(t0);
        return SECEDO_OK;
    }
    SECEDO_TRY(ks.alloc(m));
    SECEDO_TRY(vs.alloc(m));
    size_t tb = bs::split_sort_bytes(m);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(bs::split_sort(tmp.p, tb, kc.p, ks.p, vc.p, vs.p, m, bs::key_bits(rq.n_clusters - 1), s));
    // Rule 2. Within a cell the sorted records stand in the pileup's global order, so rule 3d's passes over them choose
    // the pileup's set. remove: the choice leaves the order here; mark: dup_keep goes on to the sources.
    Dev<uint32_t> dup_keep;
    if (rq.dup != SECEDO_BAM_DUPLICATES_KEEP) {
        SECEDO_TRY(hipStreamSynchronize(s));
        key.reset(), sel.reset(), scan.reset(), kc.reset(), vc.reset(), tag_sel.reset(), tmp.reset();
        {
            Dev<uint64_t> v_off;
            Dev<uint16_t> v_cell;
            SECEDO_TRY(v_off.alloc(m));
            SECEDO_TRY(v_cell.alloc(m));
            SECEDO_TRY(bs::split_view(d_in_off.p, vs.p, m, d_file.p, tag_key.p, v_off.p, v_cell.p, s));
            SECEDO_CALL(duplicate_keep(bam::Records{d_bytes.p, v_off.p, v_cell.p, m}, stat.d.p, s, &dup_keep));
        }
        if (rq.dup == SECEDO_BAM_DUPLICATES_REMOVE) {
            tb = bam::scan_bytes(uint64_t(m) + 1);
            SECEDO_TRY(tmp.alloc(tb));
            SECEDO_TRY(scan.alloc(size_t(m) + 1));
            SECEDO_TRY(hipMemsetAsync(dup_keep.p + m, 0, 4, s));
            SECEDO_TRY(bam::exclusive_sum(tmp.p, tb, dup_keep.p, scan.p, uint64_t(m) + 1, s));
            uint32_t m2 = 0;
            SECEDO_TRY(hipMemcpyAsync(&m2, scan.p + m, 4, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            if (m2 != m) {  // m2 >= 1: the best template of every key stays
                SECEDO_TRY(kc.alloc(m2));
                SECEDO_TRY(vc.alloc(m2));
                SECEDO_TRY(bs::split_compact(ks.p, vs.p, dup_keep.p, scan.p, m, kc.p, vc.p, s));
                SECEDO_TRY(hipStreamSynchronize(s));
                std::swap(ks.p, kc.p), std::swap(ks.n, kc.n);
                std::swap(vs.p, vc.p), std::swap(vs.n, vc.n);
                m = m2;
            }
            dup_keep.reset();
        }
    }
    SECEDO_CALL(take_stats());
    // destinations and extents
    Dev<uint64_t> src, len, dst, beg;
    SECEDO_TRY(src.alloc(m));
    SECEDO_TRY(len.alloc(size_t(m) + 1));
    SECEDO_TRY(dst.alloc(size_t(m) + 1));
    SECEDO_TRY(beg.alloc(rq.n_clusters));
    Dev<bs::RecordPlan> plan;
    Dev<uint64_t> cnt;
    if (suffixes) {  // the edited lengths, and what the gather needs to edit
        SECEDO_TRY(plan.alloc(m));
        SECEDO_TRY(cnt.alloc(4));
        SECEDO_TRY(hipMemsetAsync(cnt.p, 0, 4 * 8, s));
        SECEDO_TRY(bs::split_plan(d_bytes.p, d_in_off.p, vs.p, m, d_file.p, tag_key.p, suffixes->off.p, src.p, len.p,
                                  plan.p, cnt.p, s));
    } else {
        SECEDO_TRY(bs::split_lengths(d_bytes.p, d_in_off.p, vs.p, m, src.p, len.p, s));
    }
    const bool marks = dup_keep.p != nullptr;
    if (marks) SECEDO_TRY(bs::split_mark(src.p, dup_keep.p, m, s));
    tb = bam::scan_bytes(uint64_t(m) + 1);
    SECEDO_TRY(tmp.alloc(tb));
    SECEDO_TRY(bam::exclusive_sum64(tmp.p, tb, len.p, dst.p, uint64_t(m) + 1, s));
    SECEDO_TRY(hipMemsetAsync(beg.p, 0xFF, rq.n_clusters * 8ull, s));
    SECEDO_TRY(bs::split_extents(ks.p, dst.p, m, beg.p, s));
    std::vector<uint64_t> h_beg(size_t(rq.n_clusters) + 1);
    uint64_t total = 0;
    SECEDO_TRY(hipMemcpyAsync(h_beg.data(), beg.p, rq.n_clusters * 8ull, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(&total, dst.p + m, 8, hipMemcpyDeviceToHost, s));
    uint64_t h_cnt[4] = {0, 0, 0, 0};  // replaced, unparsed, added, removed
    if (suffixes) SECEDO_TRY(hipMemcpyAsync(h_cnt, cnt.p, sizeof h_cnt, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (total > ci.bytes.size() + h_cnt[2])
        return fail(SECEDO_E_STATE, "split: the stream is longer than the chromosome's records");
    if (suffixes) {
        g_rg.tagged_records += m;
        g_rg.replaced_records += h_cnt[0];
        g_rg.unparsed_records += h_cnt[1];
        g_rg.added_bytes += h_cnt[2];
        g_rg.removed_bytes += h_cnt[3];
    }
    g_split.order_ms += ms_lap(t0);
    key.reset(), sel.reset(), scan.reset(), kc.reset(), vc.reset(), ks.reset(), vs.reset(), len.reset();
    tag_key.reset(), tag_sel.reset(), tmp.reset(), dup_keep.reset();

    // the gather: every byte of the stream read once and written once
    const uint64_t padded = (total + bs::kGatherVec - 1) / bs::kGatherVec * bs::kGatherVec;
    Dev<uint8_t> out;
    SECEDO_TRY(out.alloc(kFront + padded + bz::kDeflateInSlack));
    SECEDO_TRY(hipMemsetAsync(out.p, 0, kFront, s));
    SECEDO_TRY(hipMemsetAsync(out.p + kFront + padded, 0, bz::kDeflateInSlack, s));
    Events<2> ev;
    SECEDO_CALL(ev.create());
    SECEDO_TRY(hipEventRecord(ev.e[0], s));
    if (suffixes)
        SECEDO_TRY(bs::split_gather_rg(d_bytes.p, src.p, dst.p, plan.p, suffixes->off.p, suffixes->bytes.p, m, total,
                                       out.p + kFront, s, marks));
    else
        SECEDO_TRY(bs::split_gather(d_bytes.p, src.p, dst.p, m, total, out.p + kFront, s, marks));
    SECEDO_TRY(hipEventRecord(ev.e[1], s));
    SECEDO_TRY(hipStreamSynchronize(s));
    float g_ms = 0;
    SECEDO_TRY(hipEventElapsedTime(&g_ms, ev.e[0], ev.e[1]));
    g_split.gather_ms += g_ms;
    d_bytes.reset(), d_in_off.reset(), d_file.reset(), src.reset(), dst.reset(), plan.reset(), cnt.reset();
    (void)ms_lap(t0);

    // a cluster without records of this chromosome starts where the next one does
    h_beg[rq.n_clusters] = total;
    for (uint32_t c = rq.n_clusters; c-- > 0;)
        if (h_beg[c] == ~0ull) h_beg[c] = h_beg[c + 1];
    std::vector<bz::DeflateDesc> desc;
    std::vector<uint32_t> owner;
    for (uint32_t c = 0; c < rq.n_clusters; ++c) {
        bz::member_cuts(h_beg[c], h_beg[c + 1], &desc);
        owner.resize(desc.size(), c);
    }
    SECEDO_CALL(encode_to_files(enc, out.p + kFront, desc, owner, of, s));
    g_split.records += m;
    g_split.text_bytes += total;
    return SECEDO_OK;
}

// The headers of the inputs, checked against each other -> the header bytes of every cluster's file.
int make_headers(const Request &rq, std::vector<std::vector<uint8_t>> *headers) {
    std::vector<bs::Ref> first;
    std::vector<uint8_t> first_list;
    std::vector<std::string> texts;
    SECEDO_CALL(read_reference_lists(rq.files, &first, &first_list, &texts));
    for (uint32_t c : rq.chr)
        if (c >= first.size())
            return fail(SECEDO_E_INVALID_ARG, "chromosome id " + std::to_string(c) + " is at or past the " +
                                                  std::to_string(first.size()) + " references of " +
                                                  (rq.files.empty() ? std::string("the input") : rq.files[0]));
    bs::RgMerge rg;
    size_t a = 0, b = 0;
    std::string id;
    if (!rq.rg && !bs::merge_rg(texts, &rg, &a, &b, &id))
        return fail(SECEDO_E_INVALID_ARG, "@RG ID:" + id + " names different lines in " + rq.files[a] + " and " +
                                              rq.files[b]);
    std::vector<uint32_t> members(rq.n_clusters, 0);
    for (uint16_t c : rq.cell_cluster) ++members[c];
    for (uint32_t k = 0; k < rq.n_clusters; ++k)
        headers->push_back(bs::header_bytes(
            bs::header_text(first, rq.rg ? bs::rg_header_lines(rq.names, rq.cell_cluster, k) : rg.lines, k, members[k],
                            uint32_t(rq.cell_cluster.size())),
            uint32_t(first.size()), first_list));
    return SECEDO_OK;
}

// the headers' members: the same encoder, once per file
int write_headers(const std::vector<std::vector<uint8_t>> &headers, bz::Encoder *enc, OutFiles *of, hipStream_t s) {
    std::vector<uint8_t> all(kFront, 0);
    std::vector<bz::DeflateDesc> desc;
    std::vector<uint32_t> owner;
    for (size_t k = 0; k < headers.size(); ++k) {
        const uint64_t beg = all.size() - kFront;
        all.insert(all.end(), headers[k].begin(), headers[k].end());
        bz::member_cuts(beg, all.size() - kFront, &desc);
        owner.resize(desc.size(), uint32_t(k));
        g_split.text_bytes += headers[k].size();
    }
    all.resize(all.size() + bz::kDeflateInSlack, 0);
    Dev<uint8_t> d;
    SECEDO_TRY(d.alloc(all.size()));
    SECEDO_TRY(hipMemcpyAsync(d.p, all.data(), all.size(), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    return encode_to_files(enc, d.p + kFront, desc, owner, of, s);
}

int split(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids, uint32_t n_chr,
          const uint16_t *cell_cluster, uint32_t n_cells, const char *tag, const char *const *barcodes,
          uint32_t n_barcodes, const char *out_dir, int overwrite, uint32_t num_threads, secedo_bam_times *times,
          bool read_groups = false, const char *const *cell_names = nullptr, uint32_t n_names = 0,
          uint32_t require = 0, uint32_t exclude = 0, int duplicates = SECEDO_BAM_DUPLICATES_KEEP) {
    const Clock::time_point t_all = Clock::now();
    secedo_bam_times tl{};
    if ((n_files && !bam_files) || (n_chr && !chromosome_ids) || !cell_cluster || !out_dir)
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    Request rq;
    {  // the selection, before any input is read
        const std::string why = bs::masks_fault(require, exclude);
        if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, "secedo_bam_split_clusters_select: " + why);
        if (duplicates != SECEDO_BAM_DUPLICATES_KEEP && duplicates != SECEDO_BAM_DUPLICATES_REMOVE &&
            duplicates != SECEDO_BAM_DUPLICATES_MARK)
            return fail(SECEDO_E_INVALID_ARG, "secedo_bam_split_clusters_select: duplicates " +
                                                  std::to_string(duplicates) +
                                                  " is none of SECEDO_BAM_DUPLICATES_KEEP, _REMOVE and _MARK");
        rq.require = require, rq.exclude = exclude, rq.dup = duplicates;
    }
    rq.tag = tag;
    rq.threads = num_threads ? num_threads : 1;
    if (n_files == 0) return fail(SECEDO_E_INVALID_ARG, "no input files");
    if (n_cells == 0) return fail(SECEDO_E_INVALID_ARG, "an empty clustering");
    if (tag) {
        SECEDO_CALL(check_cells(tag, barcodes, n_barcodes, &rq.values));
        if (n_cells != n_barcodes)
            return fail(SECEDO_E_INVALID_ARG, "the clustering has " + std::to_string(n_cells) + " cells, the barcode "
                                                  "list " + std::to_string(n_barcodes));
    } else {
        if (n_files > SECEDO_BAM_MAX_FILES)
            return fail(SECEDO_E_LIMIT, "more than 16384 BAM files: cell ids do not fit 14 bits");
        if (n_cells != n_files)
            return fail(SECEDO_E_INVALID_ARG, "the clustering has " + std::to_string(n_cells) + " cells, there are " +
                                                  std::to_string(n_files) + " files (one cell per file)");
    }
    SECEDO_CALL(check_files(bam_files, n_files, &rq.files));
    if (read_groups) {  // the names, before any input is read
        rq.rg = true;
        if (cell_names) {
            if (n_names != n_cells)
                return fail(SECEDO_E_INVALID_ARG, "the clustering has " + std::to_string(n_cells) + " cells, the name "
                                                      "list " + std::to_string(n_names));
            for (uint32_t c = 0; c < n_names; ++c) {
                if (!cell_names[c]) return fail(SECEDO_E_INVALID_ARG, "the name of cell " + std::to_string(c) + " is null");
                rq.names.push_back(cell_names[c]);
            }
        } else if (tag) {
            rq.names = rq.values;
        } else {
            for (const std::string &f : rq.files) rq.names.push_back(bs::default_name(f));
        }
        const std::string why = bs::names_fault(rq.names);
        if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, "read groups: " + why);
    }
    rq.chr.assign(chromosome_ids, chromosome_ids + n_chr);
    std::sort(rq.chr.begin(), rq.chr.end());
    for (size_t c = 1; c < rq.chr.size(); ++c)
        if (rq.chr[c] == rq.chr[c - 1])
            return fail(SECEDO_E_INVALID_ARG, "chromosome id " + std::to_string(rq.chr[c]) + " is listed twice");
    rq.cell_cluster.assign(cell_cluster, cell_cluster + n_cells);
    rq.n_clusters = uint32_t(*std::max_element(rq.cell_cluster.begin(), rq.cell_cluster.end())) + 1;
    g_split.files = n_files;
    g_split.cells = n_cells;
    g_split.clusters = rq.n_clusters;

    const std::string dir(out_dir);
    struct stat st;
    if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode))
        return fail(SECEDO_E_INVALID_ARG, dir + " is not a directory");
    OutFiles of;
    of.keep_open = false;  // there may be more clusters than descriptors
    for (uint32_t k = 0; k < rq.n_clusters; ++k) {
        of.target.push_back(dir + "/cluster_" + std::to_string(k) + ".bam");
        if (!overwrite && exists(of.target.back()))
            return fail(SECEDO_E_INVALID_ARG, of.target.back() + " exists; pass overwrite to replace it");
    }

    Inputs in;
    SECEDO_CALL(load_inputs(rq.files, rq.chr.data(), n_chr, rq.threads, &in, &tl));
    std::vector<std::vector<uint8_t>> headers;
    SECEDO_CALL(make_headers(rq, &headers));

    StreamGuard guard;
    SECEDO_TRY(hipStreamCreateWithFlags(&guard.s, hipStreamNonBlocking));
    const hipStream_t s = guard.s;
    bz::Encoder enc(kSlice);
    Dev<uint16_t> d_cc;
    SECEDO_TRY(d_cc.alloc(n_cells));
    SECEDO_TRY(hipMemcpyAsync(d_cc.p, rq.cell_cluster.data(), n_cells * 2ull, hipMemcpyHostToDevice, s));
    DevCells dc;
    if (tag) SECEDO_CALL(upload_cells(tag, rq.values, s, &dc));
    DevSuffixes ds;
    if (rq.rg) SECEDO_CALL(upload_suffixes(rq.names, s, &ds));
    SECEDO_TRY(hipStreamSynchronize(s));

    SECEDO_CALL(out_error(of.open()));
    SECEDO_CALL(write_headers(headers, &enc, &of, s));
    for (uint32_t c = 0; c < n_chr; ++c) {
        SECEDO_CALL(split_chromosome(rq, in.chrs[c], tag ? &dc.list : nullptr, d_cc.p, rq.rg ? &ds : nullptr, &enc, &of,
                                     s, &tl));
        std::vector<uint8_t>().swap(in.chrs[c].bytes);
    }
    Clock::time_point t0 = Clock::now();
    const auto eof = bz::eof_member();
    for (uint32_t k = 0; k < rq.n_clusters; ++k) SECEDO_CALL(out_error(of.append(k, eof.data(), eof.size())));
    g_split.compressed_bytes += uint64_t(rq.n_clusters) * eof.size();
    SECEDO_CALL(out_error(of.commit()));
    g_split.write_ms += ms_since(t0);
    tl.device_ms += g_split.order_ms + g_split.gather_ms + g_split.deflate_ms + g_split.download_ms;
    tl.write_ms += g_split.write_ms;
    tl.total_ms = ms_since(t_all);
    if (times) *times = tl;
    return SECEDO_OK;
}

}  // namespace

namespace secedo {
namespace bam_host {

int read_reference_lists(const std::vector<std::string> &files, std::vector<bamsplit::Ref> *first,
                         std::vector<uint8_t> *first_list, std::vector<std::string> *texts) {
    for (size_t f = 0; f < files.size(); ++f) {
        FileHeader h;
        SECEDO_CALL(read_file_header(files[f], &h));
        std::vector<bs::Ref> refs;
        if (h.sam) refs = bs::refs_from_text(h.text);
        else if (!bs::parse_ref_list(h.ref_list.data(), h.ref_list.size(), h.n_ref, &refs))
            return fail(SECEDO_E_INVALID_ARG, files[f] + ": truncated reference list");
        if (f == 0) {
            *first = refs;
            *first_list = h.sam ? bs::ref_list_bytes(refs) : h.ref_list;
        } else {
            const std::string why = bs::refs_differ(*first, refs);
            if (!why.empty())
                return fail(SECEDO_E_INVALID_ARG, files[f] + ": its reference list is not that of the first file " +
                                                      files[0] + ": " + why);
        }
        texts->push_back(h.text);
    }
    return SECEDO_OK;
}

}  // namespace bam_host
}  // namespace secedo

extern "C" {

int secedo_bam_split_clusters(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                              uint32_t n_chr, const uint16_t *cell_cluster, uint32_t n_cells, const char tag[2],
                              const char *const *barcodes, uint32_t n_barcodes, const char *out_dir, int overwrite,
                              uint32_t num_threads, secedo_bam_split_info *info, secedo_bam_times *times) {
    if (!info) return fail(SECEDO_E_INVALID_ARG, "null argument");
    g_split = secedo_bam_split_info{};
    g_rg = secedo_bam_split_rg_info{};
    g_sel = secedo_bam_select_info{};
    const int rc = split(bam_files, n_files, chromosome_ids, n_chr, cell_cluster, n_cells, tag, barcodes, n_barcodes,
                         out_dir, overwrite, num_threads, times);
    *info = g_split;
    return rc;
}

int secedo_bam_split_clusters_rg(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                                 uint32_t n_chr, const uint16_t *cell_cluster, uint32_t n_cells, const char tag[2],
                                 const char *const *barcodes, uint32_t n_barcodes, const char *out_dir, int overwrite,
                                 uint32_t num_threads, secedo_bam_split_info *info, secedo_bam_times *times,
                                 const char *const *cell_names, uint32_t n_names, secedo_bam_split_rg_info *rg_info) {
    if (!info || !rg_info) return fail(SECEDO_E_INVALID_ARG, "null argument");
    g_split = secedo_bam_split_info{};
    g_rg = secedo_bam_split_rg_info{};
    g_sel = secedo_bam_select_info{};
    const int rc = split(bam_files, n_files, chromosome_ids, n_chr, cell_cluster, n_cells, tag, barcodes, n_barcodes,
                         out_dir, overwrite, num_threads, times, true, cell_names, n_names);
    *info = g_split;
    *rg_info = g_rg;
    return rc;
}

int secedo_bam_split_clusters_select(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                                     uint32_t n_chr, const uint16_t *cell_cluster, uint32_t n_cells, const char tag[2],
                                     const char *const *barcodes, uint32_t n_barcodes, const char *out_dir,
                                     int overwrite, uint32_t num_threads, secedo_bam_split_info *info,
                                     secedo_bam_times *times, const char *const *cell_names, uint32_t n_names,
                                     secedo_bam_split_rg_info *rg_info, int read_groups, uint32_t require,
                                     uint32_t exclude, int duplicates, secedo_bam_select_info *select_info) {
    if (!info || !select_info || (read_groups && !rg_info)) return fail(SECEDO_E_INVALID_ARG, "null argument");
    g_split = secedo_bam_split_info{};
    g_rg = secedo_bam_split_rg_info{};
    g_sel = secedo_bam_select_info{};
    const int rc = split(bam_files, n_files, chromosome_ids, n_chr, cell_cluster, n_cells, tag, barcodes, n_barcodes,
                         out_dir, overwrite, num_threads, times, read_groups != 0, read_groups ? cell_names : nullptr,
                         read_groups ? n_names : 0, require, exclude, duplicates);
    *info = g_split;
    if (rg_info) *rg_info = g_rg;
    *select_info = g_sel;
    return rc;
}

int secedo_bam_split_select_stats(secedo_bam_select_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = g_sel;
    return SECEDO_OK;
}

int secedo_bam_split_rg_stats(secedo_bam_split_rg_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = g_rg;
    return SECEDO_OK;
}

int secedo_bam_split_stats(secedo_bam_split_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = g_split;
    return SECEDO_OK;
}

}  // extern "C"
