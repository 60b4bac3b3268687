// fasta_device.cpp -- the device route of the reference genome (include/secedo_variant.h): the FASTA text, or the
// compressed members of a BGZF file, uploaded range by range; inflated (bgzf_kernels.hip), parsed into codes and a
// header table and gathered per locus in HBM (fasta_kernels.hip). The host keeps what is serial and small: the header
// table of at most 2 n_chr + 1 contigs and their assignment to chromosomes (fasta_lines.hpp).
//
// Two streams. The caller's stream runs the passes of range r; a second one uploads (and inflates) range r + 1 into
// the other of two text buffers meanwhile. The only host synchronisation per range is the read-back of its header
// table (and, for BGZF, of its members' status words).
//
// A piece of a contig is gathered into the loci of its chromosome and of every chromosome after it: a FASTA with fewer
// contigs than the pileup has chromosomes leaves the last contig in place for the rest (variant_calling.cpp:161-163),
// and which contig is the last is known only at the end of the file. Pieces run in file order on one stream, so a
// later chromosome's own contig overwrites what an earlier one left there; where it is shorter, the loci it does not
// reach lie at or past that chromosome's end and the final pass zeroes them.
#include "fasta_stage.hpp"

#include <algorithm>
#include <cstring>

namespace secedo {
namespace fasta_host {

int device_genotypes(const Source &src, bool diploid, const uint32_t *d_chr_locus_off, const uint32_t *chr_locus_off,
                     uint32_t n_chr, const uint32_t *d_locus_pos, uint32_t n_loci, uint8_t *d_locus_ref,
                     uint32_t *chr_locus_end, hipStream_t s) {
    secedo_variant_fasta_info &st = info();
    st.route = SECEDO_FASTA_DEVICE;
    if (n_chr > (1u << 30)) return fail(SECEDO_E_LIMIT, "more than 2^30 chromosomes");
    for (uint32_t c = 0; c < n_chr; ++c)
        if (chr_locus_off[c] > chr_locus_off[c + 1]) return fail(SECEDO_E_INVALID_ARG, "chr_locus_off must not decrease");
    const bool members = src.kind == SECEDO_FASTA_KIND_BGZF;
    Stager stager(src, members);
    SECEDO_CALL(stager.init());
    const std::vector<Range> &ranges = stager.ranges;
    st.ranges = ranges.size();

    const uint32_t needed = 2 * n_chr + 1, cap = needed + 2, max_len = stager.max_len();
    const uint32_t chunks = std::max<uint32_t>(F::num_chunks(max_len), 1);
    Buf b_tf, b_tf_in, b_cnt, b_cnt_before, b_codes, b_table, b_scan, b_mat, b_pat, b_len, b_hap, b_end;
    F::RangeWork w{};
    w.cap = cap;
    w.scan_bytes = F::scan_workspace(max_len);
    SECEDO_TRY(b_tf.alloc(size_t(chunks) * sizeof(F::Transfer)));
    SECEDO_TRY(b_tf_in.alloc(size_t(chunks) * sizeof(F::Transfer)));
    SECEDO_TRY(b_cnt.alloc(size_t(chunks) * 8));
    SECEDO_TRY(b_cnt_before.alloc(size_t(chunks) * 8));
    SECEDO_TRY(b_codes.alloc(max_len));
    SECEDO_TRY(b_table.alloc(F::table_bytes(cap)));
    SECEDO_TRY(b_scan.alloc(w.scan_bytes));
    SECEDO_TRY(b_mat.alloc(n_loci));
    SECEDO_TRY(b_pat.alloc(n_loci));
    SECEDO_TRY(b_len.alloc(size_t(n_chr) * 8));
    SECEDO_TRY(b_hap.alloc(n_chr));
    SECEDO_TRY(b_end.alloc(size_t(n_chr) * 4));
    w.tf = b_tf.as<F::Transfer>(), w.tf_in = b_tf_in.as<F::Transfer>();
    w.cnt = b_cnt.as<uint64_t>(), w.cnt_before = b_cnt_before.as<uint64_t>();
    w.codes = b_codes.p, w.totals = b_table.as<F::RangeTotals>(), w.scan_tmp = b_scan.p;
    if (n_loci) {
        SECEDO_TRY(hipMemsetAsync(b_mat.p, 0, n_loci, s));
        SECEDO_TRY(hipMemsetAsync(b_pat.p, 0, n_loci, s));
    }
    Events<10> ev;  // per parity k of a range: [4k, 4k + 1] its passes, [4k + 2, 4k + 3] its gathers; [8, 9] the final pass
    SECEDO_CALL(ev.create());

    F::Table table(diploid, needed);
    std::vector<uint8_t> h_table(F::table_bytes(cap));
    std::vector<uint32_t> h_status;
    std::vector<F::Table::Piece> pieces;
    uint32_t state = F::kLine0;
    uint64_t bad_k = UINT64_MAX;
    uint32_t bad_status = 0;
    float ms = 0;
    int timed = -1;  // the parity of the range whose events are recorded and not yet read: read after the next wait
    auto read_timed = [&]() -> int {
        if (timed < 0) return SECEDO_OK;
        for (int pair = 0; pair < 2; ++pair) {  // the host's waits between the passes and the gathers are not counted
            SECEDO_TRY(hipEventElapsedTime(&ms, ev.e[4 * timed + 2 * pair], ev.e[4 * timed + 2 * pair + 1]));
            st.parse_gather_ms += ms;
        }
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
            SECEDO_TRY(hipEventElapsedTime(&ms, stager.ev.e[4 + 2 * k], stager.ev.e[5 + 2 * k]));
            st.inflate_ms += ms;
            note_bad(h_status, x, &bad_k, &bad_status);
        }
        const bool parse = bad_k == UINT64_MAX;
        if (parse) {
            SECEDO_TRY(hipEventRecord(ev.e[4 * k], s));
            SECEDO_TRY(F::parse_range(stager.text[k].p, x.len, state, w, s));
            SECEDO_TRY(hipEventRecord(ev.e[4 * k + 1], s));
            SECEDO_TRY(hipMemcpyAsync(h_table.data(), b_table.p, h_table.size(), hipMemcpyDeviceToHost, s));
        }
        SECEDO_TRY(hipEventRecord(stager.ev.e[2 + k], s));
        // the next range's upload (and inflate) beside this range's passes
        if (r + 1 < ranges.size()) SECEDO_CALL(stager.stage(r + 1, r >= 1));
        if (!parse) continue;
        SECEDO_TRY(hipStreamSynchronize(s));
        SECEDO_CALL(read_timed());
        F::RangeTotals totals;
        std::memcpy(&totals, h_table.data(), sizeof totals);
        if (totals.seq > x.len || totals.headers > x.len || totals.state >= F::kStates)
            return fail(SECEDO_E_HIP, "the FASTA passes returned totals beyond their range");
        table.range(totals, reinterpret_cast<const F::HeaderSlot *>(h_table.data() + sizeof totals), x.len, &pieces);
        state = totals.state;
        st.text_bytes += x.len;
        SECEDO_TRY(hipEventRecord(ev.e[4 * k + 2], s));
        for (const F::Table::Piece &p : pieces) {
            if (p.role.chr >= n_chr || uint64_t(p.code_off) + p.count > totals.seq) continue;
            SECEDO_TRY(F::gather(b_codes.p, p.code_off, p.count, p.q0, d_locus_pos, chr_locus_off[p.role.chr], n_loci,
                                 p.role.slot ? b_pat.p : b_mat.p, s));
        }
        SECEDO_TRY(hipEventRecord(ev.e[4 * k + 3], s));
        timed = k;
    }
    SECEDO_TRY(hipStreamSynchronize(stager.up.s));
    SECEDO_TRY(hipStreamSynchronize(s));
    SECEDO_CALL(read_timed());
    if (bad_k != UINT64_MAX) return bad_member(src.path, bad_k, bm::status_text(bad_status));

    table.finish();
    st.contigs = table.headers();
    std::vector<uint64_t> len;
    std::vector<uint8_t> hap;
    std::vector<uint32_t> source;
    const std::string err = F::resolve(table.assign.chroms, table.contigs, n_chr, &len, &hap, &source);
    if (!err.empty()) return fail(SECEDO_E_INVALID_ARG, err);
    for (uint32_t c = 0; c < n_chr && c < table.assign.chroms.size(); ++c)
        st.contigs_used += table.assign.chroms[c].pat >= 0 ? 2 : 1;
    if (n_chr) {
        SECEDO_TRY(hipEventRecord(ev.e[8], s));
        SECEDO_TRY(hipMemcpyAsync(b_len.p, len.data(), size_t(n_chr) * 8, hipMemcpyHostToDevice, s));
        SECEDO_TRY(hipMemcpyAsync(b_hap.p, hap.data(), n_chr, hipMemcpyHostToDevice, s));
        SECEDO_TRY(F::finish(d_chr_locus_off, n_chr, d_locus_pos, n_loci, b_len.as<uint64_t>(), b_hap.p, b_mat.p, b_pat.p,
                             d_locus_ref, b_end.as<uint32_t>(), s));
        SECEDO_TRY(hipEventRecord(ev.e[9], s));
        SECEDO_TRY(hipMemcpyAsync(chr_locus_end, b_end.p, size_t(n_chr) * 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        SECEDO_TRY(hipEventElapsedTime(&ms, ev.e[8], ev.e[9]));
        st.parse_gather_ms += ms;
    }
    return SECEDO_OK;
}

int download_bgzf_text(Source *src, hipStream_t s) {
    secedo_variant_fasta_info &st = info();
    Stager stager(*src, true);
    SECEDO_CALL(stager.init());
    const std::vector<Range> &ranges = stager.ranges;
    src->inflated.resize(src->members_text);
    std::vector<uint32_t> h_status;
    uint64_t bad_k = UINT64_MAX, at = 0;
    uint32_t bad_status = 0;
    float ms = 0;
    if (!ranges.empty()) SECEDO_CALL(stager.stage(0, false));
    for (size_t r = 0; r < ranges.size(); ++r) {
        const int k = int(r & 1);
        const Range &x = ranges[r];
        SECEDO_TRY(hipStreamWaitEvent(s, stager.ev.e[k], 0));
        h_status.resize(x.b - x.a);
        SECEDO_TRY(hipMemcpyAsync(h_status.data(), stager.status[k].p, h_status.size() * 4, hipMemcpyDeviceToHost, s));
        if (x.len) SECEDO_TRY(hipMemcpyAsync(src->inflated.data() + at, stager.text[k].p, x.len, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipEventRecord(stager.ev.e[2 + k], s));
        if (r + 1 < ranges.size()) SECEDO_CALL(stager.stage(r + 1, r >= 1));
        SECEDO_TRY(hipStreamSynchronize(s));
        SECEDO_TRY(hipEventElapsedTime(&ms, stager.ev.e[4 + 2 * k], stager.ev.e[5 + 2 * k]));
        st.inflate_ms += ms;
        note_bad(h_status, x, &bad_k, &bad_status);
        at += x.len;
    }
    SECEDO_TRY(hipStreamSynchronize(stager.up.s));
    if (bad_k != UINT64_MAX) return bad_member(src->path, bad_k, bm::status_text(bad_status));
    src->has_text = true;
    return SECEDO_OK;
}

}  // namespace fasta_host
}  // namespace secedo
