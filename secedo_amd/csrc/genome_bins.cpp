// genome_bins.cpp -- secedo_variant_genome_bins of include/secedo_variant.h: the composition of a
// reference genome per bin, the companion of secedo_bam_depth. The file comes through the compressed-genome input
// layer (fasta_source.cpp) and the double-buffered stager (fasta_stage.hpp); per range the scans of fasta_kernels.hip
// give every chunk its entry state and sequence ordinal and the host its header slots, the host names the contigs and
// builds the piece table, and k_compose (genome_bins_kernels.hip) counts the text into the bins x 6 table. The host
// keeps what is serial and small: names, lengths, the selection. The file's lines go out through text_out.hpp (the
// ranged formatter, the way down, the name upload) into a temporary file of out_files.hpp. What decides numbers and
// bytes is in genome_bins.hpp.
//
// Which contigs are selected, and so where a contig's bins begin in selection order, is known only at the end of the
// file. The ranges therefore count into a table laid out in file order over the contigs that can still be selected
// (all first-of-their-name ones, or the listed names): a contig's first bin there is known when its header is, since
// every contig in front of it has ended. With a list of names the rows are moved into the listed order at the end,
// one device copy per contig.
#include "fasta_stage.hpp"
#include "genome_bins_kernels.hpp"
#include "text_out.hpp"

#include <sys/stat.h>

#include <cstring>
#include <memory>
#include <set>

namespace {

using namespace secedo::fasta_host;
namespace gb = secedo::genomebins;
namespace bd = secedo::bamdepth;
namespace bz = secedo::bgzf;

thread_local secedo_variant_genome_bins_info g_info{};

// what secedo_variant_genome_bins_fetch copies out
struct Result {
    std::vector<std::string> names;
    std::vector<uint64_t> lengths;
    std::vector<uint32_t> bin_contig, bin_start, bin_end, counts;
};
thread_local std::unique_ptr<Result> g_result;

constexpr uint32_t kInitialSlots = 256;  // header slots of a range before the first range that has more

// The names of the contigs, in file order, from the header slots of one range after the other. A header line that a
// range boundary cuts is joined here: `raw` holds its first bytes until its end is seen.
struct ContigNames {
    std::vector<std::string> names;
    std::vector<uint8_t> raw;
    bool open = false;

    struct Span {  // bytes [off, off + n) of the range: the part of a header line that can decide its name
        uint32_t off, n;
        bool first, ends;  // begins a header line; the line ends in this range
    };
    // the spans of a range entered with this->open, from its totals and slots (cap > t.headers)
    void spans(const F::RangeTotals &t, const F::HeaderSlot *slots, uint32_t len, std::vector<Span> *out) const {
        out->clear();
        if (open && len) {
            const bool ends = slots[0].end != F::kNone;
            const uint32_t e = ends ? slots[0].end : len;
            const uint32_t room = raw.size() < gb::kHeaderPrefix ? uint32_t(gb::kHeaderPrefix - raw.size()) : 0;
            out->push_back(Span{0, std::min(e, room), false, ends});
        }
        for (uint32_t h = 1; h <= t.headers; ++h) {
            const bool ends = slots[h].end != F::kNone;
            const uint32_t e = ends ? slots[h].end : len;
            out->push_back(Span{slots[h].start, std::min(e - slots[h].start, gb::kHeaderPrefix), true, ends});
        }
    }
    // "" or why a name is refused
    std::string take(const Span &sp, const uint8_t *bytes) {
        if (sp.first) raw.clear();
        raw.insert(raw.end(), bytes, bytes + sp.n);
        open = !sp.ends;
        return open ? std::string() : close();
    }
    std::string close() {
        open = false;
        uint32_t l = 0;
        if (!gb::cut_name(raw.data(), raw.size(), &l)) return gb::too_long(names.size());
        names.emplace_back(reinterpret_cast<const char *>(raw.data()) + (l ? 1 : 0), l);
        return std::string();
    }
};

struct Request {
    uint32_t S = 0;
    bool listed = false, bgzf = false, overwrite = false, write = false;
    std::vector<std::string> names;
    std::vector<uint64_t> lengths;  // empty: none given
    std::set<std::string> wanted;
};

// The parse and the counts of the whole file: names and lengths of all contigs, and the table in file order over the
// contigs that may be selected, bin0[c] being contig c's first bin there (kNotSelected: none).
struct Counted {
    std::vector<std::string> names;
    std::vector<uint64_t> len, bin0;
    Dev<uint32_t> table;
};

int count_file(const Source &src, const Request &rq, hipStream_t s, Counted *out) {
    const bool members = src.kind == SECEDO_FASTA_KIND_BGZF;
    Stager stager(src, members);
    SECEDO_CALL(stager.init());
    const std::vector<Range> &ranges = stager.ranges;
    g_info.ranges = ranges.size();

    const uint32_t max_len = stager.max_len();
    const uint32_t chunks = std::max<uint32_t>(F::num_chunks(max_len), 1);
    Buf b_tf, b_tf_in, b_cnt, b_cnt_before, b_table, b_scan;
    Dev<gb::Piece> d_pieces[2];
    F::RangeWork w{};
    w.cap = kInitialSlots;
    w.scan_bytes = F::scan_workspace(max_len);
    SECEDO_TRY(b_tf.alloc(size_t(chunks) * sizeof(F::Transfer)));
    SECEDO_TRY(b_tf_in.alloc(size_t(chunks) * sizeof(F::Transfer)));
    SECEDO_TRY(b_cnt.alloc(size_t(chunks) * 8));
    SECEDO_TRY(b_cnt_before.alloc(size_t(chunks) * 8));
    SECEDO_TRY(b_table.alloc(F::table_bytes(w.cap)));
    SECEDO_TRY(b_scan.alloc(w.scan_bytes));
    w.tf = b_tf.as<F::Transfer>(), w.tf_in = b_tf_in.as<F::Transfer>();
    w.cnt = b_cnt.as<uint64_t>(), w.cnt_before = b_cnt_before.as<uint64_t>();
    w.codes = nullptr;  // this call needs no codes
    w.totals = b_table.as<F::RangeTotals>(), w.scan_tmp = b_scan.p;
    Events<6> ev;  // [0, 1] a range's parse passes; per parity k [2 + 2k, 3 + 2k] its k_compose
    SECEDO_CALL(ev.create());

    F::Table table(false, UINT64_MAX);  // no pairing: every header is a contig of its own, and all are kept
    ContigNames cn;
    std::vector<uint8_t> h_table(F::table_bytes(w.cap)), h_bytes;
    std::vector<uint32_t> h_status;
    std::vector<F::Table::Piece> pieces;
    std::vector<gb::Piece> h_pieces[2];
    std::vector<ContigNames::Span> spans;
    std::set<std::string> seen;
    std::vector<uint8_t> taken;  // per named contig: it may be selected
    uint64_t next_bin = 0;       // the table's bins in front of the next taken contig, once `last_taken` is added
    int64_t last_taken = -1;
    uint32_t state = F::kLine0;
    uint64_t bad_k = UINT64_MAX;
    uint32_t bad_status = 0;
    float ms = 0;
    int timed = -1;  // the parity of the range whose k_compose events are recorded and not yet read
    auto read_timed = [&]() -> int {
        if (timed < 0) return SECEDO_OK;
        SECEDO_TRY(hipEventElapsedTime(&ms, ev.e[2 + 2 * timed], ev.e[3 + 2 * timed]));
        g_info.count_ms += ms;
        timed = -1;
        return SECEDO_OK;
    };

    if (!ranges.empty()) SECEDO_CALL(stager.stage(0, false));
    for (size_t r = 0; r < ranges.size(); ++r) {
        const int k = int(r & 1);
        const Range &x = ranges[r];
        SECEDO_TRY(hipStreamWaitEvent(s, stager.ev.e[k], 0));
        if (members) {  // a bad member's text is not parsed: the status words first
            h_status.resize(x.b - x.a);
            SECEDO_TRY(hipMemcpyAsync(h_status.data(), stager.status[k].p, h_status.size() * 4, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            SECEDO_CALL(read_timed());
            note_bad(h_status, x, &bad_k, &bad_status);
        }
        const bool parse = bad_k == UINT64_MAX;
        if (parse) {
            SECEDO_TRY(hipEventRecord(ev.e[0], s));
            SECEDO_TRY(F::parse_range(stager.text[k].p, x.len, state, w, s));
            SECEDO_TRY(hipEventRecord(ev.e[1], s));
            SECEDO_TRY(hipMemcpyAsync(h_table.data(), b_table.p, h_table.size(), hipMemcpyDeviceToHost, s));
        }
        // the next range's upload (and inflate) beside this range's passes: its slot was released by range r - 1
        if (r + 1 < ranges.size()) SECEDO_CALL(stager.stage(r + 1, r >= 1));
        if (!parse) {
            SECEDO_TRY(hipEventRecord(stager.ev.e[2 + k], s));
            continue;
        }
        SECEDO_TRY(hipStreamSynchronize(s));
        SECEDO_CALL(read_timed());
        SECEDO_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        g_info.parse_ms += ms;
        F::RangeTotals totals;
        std::memcpy(&totals, h_table.data(), sizeof totals);
        if (totals.seq > x.len || totals.headers > x.len || totals.state >= F::kStates)
            return fail(SECEDO_E_HIP, "the FASTA passes returned totals beyond their range");
        if (totals.headers >= w.cap) {  // all headers are needed: the last pass again, with slots for them
            w.cap = totals.headers + 2;
            SECEDO_TRY(b_table.alloc(F::table_bytes(w.cap)));
            w.totals = b_table.as<F::RangeTotals>();
            h_table.resize(F::table_bytes(w.cap));
            SECEDO_TRY(hipEventRecord(ev.e[0], s));
            SECEDO_TRY(F::emit_range(stager.text[k].p, x.len, state, w, s));
            SECEDO_TRY(hipEventRecord(ev.e[1], s));
            SECEDO_TRY(hipMemcpyAsync(h_table.data(), b_table.p, h_table.size(), hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            SECEDO_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
            g_info.parse_ms += ms;
            F::RangeTotals again;
            std::memcpy(&again, h_table.data(), sizeof again);
            if (std::memcmp(&again, &totals, sizeof again) != 0)
                return fail(SECEDO_E_HIP, "the FASTA passes returned other totals the second time");
        }
        const F::HeaderSlot *slots = reinterpret_cast<const F::HeaderSlot *>(h_table.data() + sizeof totals);
        for (uint32_t h = 1; h <= totals.headers; ++h)
            if (slots[h].start >= x.len || (slots[h].end != F::kNone && (slots[h].end >= x.len || slots[h].end < slots[h].start)))
                return fail(SECEDO_E_HIP, "the FASTA passes returned a header beyond its range");
        if (slots[0].end != F::kNone && slots[0].end >= x.len)
            return fail(SECEDO_E_HIP, "the FASTA passes returned a header beyond its range");

        // the names: from the host's text, or for BGZF from the header bytes the slots delimit
        cn.spans(totals, slots, x.len, &spans);
        const uint8_t *from = nullptr;
        if (members) {
            size_t all = 0;
            for (const ContigNames::Span &sp : spans) all += sp.n;
            h_bytes.resize(all);
            size_t at = 0;
            for (const ContigNames::Span &sp : spans) {
                if (sp.n)
                    SECEDO_TRY(hipMemcpyAsync(h_bytes.data() + at, stager.text[k].p + sp.off, sp.n, hipMemcpyDeviceToHost, s));
                at += sp.n;
            }
            SECEDO_TRY(hipStreamSynchronize(s));
        } else {
            from = src.text() + x.a;
        }
        {
            size_t at = 0;
            for (const ContigNames::Span &sp : spans) {
                const std::string why = cn.take(sp, members ? h_bytes.data() + at : from + sp.off);
                if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, src.path + ": " + why);
                at += sp.n;
            }
        }
        for (size_t c = taken.size(); c < cn.names.size(); ++c) {
            const bool first = seen.insert(cn.names[c]).second;
            taken.push_back(first && (!rq.listed || rq.wanted.count(cn.names[c])));
        }

        // the pieces of the range with their bins, the table grown to hold them
        table.range(totals, slots, x.len, &pieces);
        const uint32_t entry = state;
        state = totals.state;
        g_info.fasta_bytes += x.len;
        std::vector<gb::Piece> &hp = h_pieces[k];
        hp.clear();
        uint64_t bins_needed = 0;
        for (const F::Table::Piece &p : pieces) {
            const size_t c = p.role.chr;
            if (c >= taken.size() || uint64_t(p.code_off) + p.count > totals.seq)
                return fail(SECEDO_E_HIP, "the FASTA passes returned sequence in front of its header");
            out->bin0.resize(std::max(out->bin0.size(), c + 1), gb::kNotSelected);
            if (taken[c]) {
                if (p.q0 + p.count > gb::kMaxContigLen)
                    return fail(SECEDO_E_LIMIT, cn.names[c] + ": more than the 2^32 - 1 bases a contig may have");
                if (out->bin0[c] == gb::kNotSelected) {  // every contig in front of it has ended
                    if (last_taken >= 0) next_bin += bd::chr_bins(uint32_t(table.contigs[size_t(last_taken)].seq_len), rq.S);
                    out->bin0[c] = next_bin;
                    last_taken = int64_t(c);
                }
                bins_needed = out->bin0[c] + bd::chr_bins(uint32_t(p.q0 + p.count), rq.S);
                if (bins_needed > bd::kMaxBins)
                    return fail(SECEDO_E_LIMIT, "more than the 2^32 - 1 bins a call numbers; use a larger bin_size");
            }
            hp.push_back(gb::Piece{p.q0, out->bin0[c], p.code_off, p.count});
        }
        if (bins_needed * gb::kColumns > out->table.n || !out->table.p) {
            const size_t before = out->table.p ? out->table.n : 0;
            SECEDO_TRY(out->table.grow(size_t(bins_needed) * gb::kColumns, before, s));
            if (out->table.n > before)
                SECEDO_TRY(hipMemsetAsync(out->table.p + before, 0, (out->table.n - before) * 4, s));
        }
        if (!hp.empty()) {
            SECEDO_TRY(d_pieces[k].grow(hp.size(), 0, s));
            SECEDO_TRY(hipMemcpyAsync(d_pieces[k].p, hp.data(), hp.size() * sizeof(gb::Piece), hipMemcpyHostToDevice, s));
        }
        SECEDO_TRY(hipEventRecord(ev.e[2 + 2 * k], s));
        SECEDO_TRY(gb::compose(stager.text[k].p, x.len, entry, w, d_pieces[k].p,
                               uint32_t(hp.size()), rq.S, out->table.p, out->table.n / gb::kColumns, s));
        SECEDO_TRY(hipEventRecord(ev.e[3 + 2 * k], s));
        timed = k;
        SECEDO_TRY(hipEventRecord(stager.ev.e[2 + k], s));
    }
    SECEDO_TRY(hipStreamSynchronize(stager.up.s));
    SECEDO_TRY(hipStreamSynchronize(s));
    SECEDO_CALL(read_timed());
    if (bad_k != UINT64_MAX) return bad_member(src.path, bad_k, bm::status_text(bad_status));

    if (cn.open) {  // the file ends inside a header line
        const std::string why = cn.close();
        if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, src.path + ": " + why);
    }
    table.finish();
    if (cn.names.size() != table.contigs.size())
        return fail(SECEDO_E_HIP, "the FASTA passes returned " + std::to_string(table.contigs.size()) + " contigs and " +
                                      std::to_string(cn.names.size()) + " names");
    out->names = std::move(cn.names);
    out->bin0.resize(out->names.size(), gb::kNotSelected);
    for (const F::Contig &c : table.contigs) out->len.push_back(c.seq_len);
    return SECEDO_OK;
}

// The file of the selected contigs' bins: the header line, then the lines formatted on the GPU from the table in
// selection order.
int write_file(const Request &rq, const bd::Layout &lay, const std::vector<std::string> &names,
               const uint32_t *d_counts, OutFiles *of, TextCounts *tc, hipStream_t s) {
    Clock::time_point t0 = Clock::now();
    SECEDO_CALL(out_error(of->open()));
    g_info.write_ms += ms_lap(t0);
    DevNames dn;
    SECEDO_CALL(upload_names(names, s, &dn));
    Dev<uint32_t> d_len;
    Dev<uint64_t> d_base;
    SECEDO_TRY(d_base.alloc(lay.base.size()));
    SECEDO_TRY(d_len.alloc(lay.len.size()));
    SECEDO_TRY(hipMemcpyAsync(d_base.p, lay.base.data(), lay.base.size() * 8, hipMemcpyHostToDevice, s));
    if (!lay.len.empty())
        SECEDO_TRY(hipMemcpyAsync(d_len.p, lay.len.data(), lay.len.size() * 4, hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    const gb::Rows rows{d_base.p, d_len.p, uint32_t(lay.chr.size()), rq.S, dn.view(), d_counts};
    bz::Encoder enc(kSlice);
    Formatter fm;
    TextOut out{of, 0, rq.bgzf, &enc, s, tc, {}, {}};
    SECEDO_CALL(out.host(gb::header_line()));
    const uint64_t max_line = gb::max_line(dn.longest);
    SECEDO_CALL(fm.run(
        lay.n_bins(), bd::lines_per_range(text_batch_bytes("SECEDO_GENOME_BINS_BATCH_BYTES"), max_line), max_line,
        [&](uint64_t i0, uint32_t n, uint64_t *len) { return gb::lines_measure(rows, i0, n, len, s); },
        [&](uint64_t i0, uint32_t n, const uint64_t *off, uint8_t *text) {
            return gb::lines_write(rows, i0, n, off, text, s);
        },
        Scan64{gb::scan_bytes, gb::exclusive_sum64}, &out, s));
    SECEDO_CALL(out.finish());
    t0 = Clock::now();
    SECEDO_CALL(out_error(of->commit()));
    g_info.write_ms += ms_lap(t0);
    return SECEDO_OK;
}

int genome_bins(const char *fasta, uint32_t bin_size, const char *const *names, const uint64_t *lengths,
                uint32_t n_names, const char *out_path, int output, int overwrite) {
    // everything that needs no input, before any is read
    if (bin_size == 0)
        return fail(SECEDO_E_INVALID_ARG, "secedo_variant_genome_bins: bin_size is 0, at least 1 is needed");
    if (output != SECEDO_GENOME_BINS_PLAIN && output != SECEDO_GENOME_BINS_BGZF)
        return fail(SECEDO_E_INVALID_ARG, "secedo_variant_genome_bins: output " + std::to_string(output) +
                                              " is neither SECEDO_GENOME_BINS_PLAIN nor SECEDO_GENOME_BINS_BGZF");
    if (!names && (lengths || n_names))
        return fail(SECEDO_E_INVALID_ARG, "secedo_variant_genome_bins: lengths or a count without names");
    Request rq;
    rq.S = bin_size, rq.bgzf = output == SECEDO_GENOME_BINS_BGZF, rq.overwrite = overwrite != 0;
    rq.listed = names != nullptr;
    for (uint32_t i = 0; names && i < n_names; ++i) {
        rq.names.push_back(names[i] ? names[i] : "");
        rq.wanted.insert(rq.names.back());
        if (lengths) rq.lengths.push_back(lengths[i]);
    }
    g_info.output = uint32_t(output);
    OutFiles of;
    if (out_path) {
        rq.write = true;
        of.target = {std::string(out_path) + (rq.bgzf ? ".gz" : "")};
        struct stat st;
        if (!rq.overwrite && stat(of.target[0].c_str(), &st) == 0)
            return fail(SECEDO_E_INVALID_ARG, of.target[0] + " exists; pass overwrite to replace it");
    }

    Source src;
    SECEDO_CALL(open_source(fasta, &src));
    g_info.kind = src.kind;
    if ((src.kind == SECEDO_FASTA_KIND_BGZF ? src.members_text : src.text_bytes()) == 0)
        return fail(SECEDO_E_INVALID_ARG, src.path + ": the genome is empty");

    StreamGuard guard;
    SECEDO_TRY(hipStreamCreateWithFlags(&guard.s, hipStreamNonBlocking));
    const hipStream_t s = guard.s;
    Counted cnt;
    const int rc = count_file(src, rq, s, &cnt);
    {
        const secedo_variant_fasta_info &fi = info();
        g_info.uploaded_bytes = fi.uploaded_bytes, g_info.device_members = fi.device_members;
        g_info.upload_ms = fi.upload_ms;
    }
    SECEDO_CALL(rc);
    g_info.contigs = cnt.names.size();

    // the selection and its bins
    gb::Selection sel;
    std::string why = gb::select(cnt.names, cnt.len, rq.listed ? &rq.names : nullptr,
                                 rq.lengths.empty() ? nullptr : rq.lengths.data(), &sel);
    g_info.duplicate_names = sel.duplicate_names;
    if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, why);
    bd::Layout lay;
    bool limit = false;
    why = gb::make_layout(cnt.names, cnt.len, sel, rq.S, &lay, &limit);
    if (!why.empty()) return fail(limit ? SECEDO_E_LIMIT : SECEDO_E_INVALID_ARG, why);
    const uint64_t n_bins = lay.n_bins();
    g_info.selected = sel.contig.size();
    g_info.bins = n_bins;

    std::unique_ptr<Result> res(new Result);
    for (size_t i = 0; i < sel.contig.size(); ++i) {
        res->names.push_back(cnt.names[sel.contig[i]]);
        res->lengths.push_back(cnt.len[sel.contig[i]]);
        g_info.bases += res->lengths.back();
        g_info.name_bytes += res->names.back().size();
        for (uint64_t b = 0; b < lay.base[i + 1] - lay.base[i]; ++b) {
            res->bin_contig.push_back(uint32_t(i));
            res->bin_start.push_back(bd::bin_start(uint32_t(b), rq.S));
            res->bin_end.push_back(bd::bin_end(uint32_t(b), rq.S, lay.len[i]));
        }
    }

    // the table in selection order: as counted without a list, else moved contig by contig
    Dev<uint32_t> moved;
    const uint32_t *d_counts = cnt.table.p;
    if (rq.listed && n_bins) {
        SECEDO_TRY(moved.alloc(n_bins * gb::kColumns));
        for (size_t i = 0; i < sel.contig.size(); ++i) {
            const uint64_t nb = lay.base[i + 1] - lay.base[i], from = cnt.bin0[sel.contig[i]];
            if (nb == 0) continue;
            if (from == gb::kNotSelected || (from + nb) * gb::kColumns > cnt.table.n)
                return fail(SECEDO_E_HIP, "a selected contig has no rows in the counted table");
            SECEDO_TRY(hipMemcpyAsync(moved.p + lay.base[i] * gb::kColumns, cnt.table.p + from * gb::kColumns,
                                      nb * gb::kColumns * 4, hipMemcpyDeviceToDevice, s));
        }
        d_counts = moved.p;
    } else if (n_bins * gb::kColumns > cnt.table.n) {
        return fail(SECEDO_E_HIP, "the counted table is shorter than the bins");
    }
    res->counts.resize(n_bins * gb::kColumns);
    if (n_bins)
        SECEDO_TRY(hipMemcpyAsync(res->counts.data(), d_counts, n_bins * gb::kColumns * 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));

    if (rq.write) {
        TextCounts tc;  // what the text layer did, also where it failed
        const int wrc = write_file(rq, lay, res->names, d_counts, &of, &tc, s);
        g_info.text_bytes += tc.text_bytes, g_info.compressed_bytes += tc.compressed_bytes;
        g_info.members += tc.members, g_info.format_ms += tc.format_ms, g_info.deflate_ms += tc.deflate_ms;
        g_info.download_ms += tc.download_ms, g_info.write_ms += tc.write_ms;
        SECEDO_CALL(wrc);
    }
    g_result = std::move(res);
    return SECEDO_OK;
}

}  // namespace

extern "C" {

int secedo_variant_genome_bins(const char *fasta, uint32_t bin_size, const char *const *names, const uint64_t *lengths,
                               uint32_t n_names, const char *out_path, int output, int overwrite,
                               secedo_variant_genome_bins_info *info) {
    if (!info || !fasta) return fail(SECEDO_E_INVALID_ARG, "null argument");
    g_info = secedo_variant_genome_bins_info{};
    g_result.reset();
    const int rc = genome_bins(fasta, bin_size, names, lengths, n_names, out_path, output, overwrite);
    *info = g_info;
    return rc;
}

int secedo_variant_genome_bins_fetch(char *names, uint64_t *name_off, uint64_t *contig_lengths, uint32_t *bin_contig,
                                     uint32_t *bin_start, uint32_t *bin_end, uint32_t *counts) {
    if (!g_result) return fail(SECEDO_E_STATE, "no genome_bins result: call secedo_variant_genome_bins first");
    const Result &r = *g_result;
    uint64_t at = 0;
    for (size_t i = 0; i < r.names.size(); ++i) {
        if (name_off) name_off[i] = at;
        if (names) std::memcpy(names + at, r.names[i].data(), r.names[i].size());
        at += r.names[i].size();
    }
    if (name_off) name_off[r.names.size()] = at;
    if (contig_lengths) std::copy(r.lengths.begin(), r.lengths.end(), contig_lengths);
    if (bin_contig) std::copy(r.bin_contig.begin(), r.bin_contig.end(), bin_contig);
    if (bin_start) std::copy(r.bin_start.begin(), r.bin_start.end(), bin_start);
    if (bin_end) std::copy(r.bin_end.begin(), r.bin_end.end(), bin_end);
    if (counts) std::copy(r.counts.begin(), r.counts.end(), counts);
    return SECEDO_OK;
}

int secedo_variant_genome_bins_stats(secedo_variant_genome_bins_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = g_info;
    return SECEDO_OK;
}

}  // extern "C"
