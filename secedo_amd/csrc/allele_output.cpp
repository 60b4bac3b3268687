// allele_output.cpp -- see allele_output.hpp. One formatter, on the GPU, for both outputs: under PLAIN a range's text
// is downloaded and appended to the files, under BGZF it goes through vcf::deflate_device and only compressed bytes
// come down (every range but the last loses the EOF member deflate_device closes a file with).
#include "allele_output.hpp"

#include "bgzf_deflate_kernels.hpp"
#include "bgzf_encoder.hpp"
#include "host_util.hpp"
#include "vcf_output.hpp"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace secedo {
namespace allele {

using namespace secedo::host;

namespace {

std::atomic<int> g_selection{-1};
thread_local secedo_variant_allele_info g_info;
std::mutex g_names_mutex;
std::vector<std::string> g_names;

constexpr uint64_t kDefaultBatchBytes = 256ull << 20;
constexpr uint64_t kMaxBatchBytes = 1ull << 30;  // keeps a range's items and threads well inside 2^31

std::vector<std::string> cell_names() {
    std::lock_guard<std::mutex> lock(g_names_mutex);
    return g_names;
}

// What the passes leave in HBM, and the few numbers the host needs of it.
struct Counted {
    Buf site_locus, site_mask, deep_off, keys_sorted, counts, pair_off, pairs;
    uint32_t n_sites = 0;
    uint64_t n_pairs = 0;
    Totals totals{};
    bool fits = true;  // false: more sites or pairs than the caller's capacity; the pairs were not written
};

// Site pass, count pass and, where the counts fit the capacities, write pass.
int run_counts(const Pileup &p, const secedo_variant_record *d_records, uint32_t n_records, const uint8_t *d_locus_ref,
               int selection, uint64_t site_capacity, uint64_t pair_capacity, Counted *c, hipStream_t s) {
    Clock::time_point t0 = Clock::now();
    Events<6> ev;
    SECEDO_CALL(ev.create());
    float ms = 0, part = 0;
    Buf b_flag, b_mask, b_index, b_scan, b_deep_len, b_keys, b_sort, b_totals, b_pair_len;
    const size_t site_scan = site_scan_workspace(n_records);
    SECEDO_TRY(b_flag.alloc(((size_t)n_records + 1) * 4));
    SECEDO_TRY(b_mask.alloc((size_t)n_records + 1));
    SECEDO_TRY(b_index.alloc(((size_t)n_records + 1) * 4));
    SECEDO_TRY(b_scan.alloc(site_scan));
    SECEDO_TRY(hipEventRecord(ev.e[0], s));
    SECEDO_TRY(site_flags(d_records, n_records, d_locus_ref, selection, b_flag.as<uint32_t>(), b_mask.as<uint8_t>(),
                          b_index.as<uint32_t>(), b_scan.p, site_scan, s));
    SECEDO_TRY(hipEventRecord(ev.e[1], s));
    SECEDO_TRY(hipMemcpyAsync(&c->n_sites, b_index.as<uint32_t>() + n_records, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    SECEDO_TRY(hipEventElapsedTime(&part, ev.e[0], ev.e[1]));
    ms += part;
    const uint32_t n_sites = c->n_sites;

    const size_t pair_scan = pair_scan_workspace(n_sites);
    SECEDO_TRY(b_scan.alloc(pair_scan));
    SECEDO_TRY(c->site_locus.alloc((size_t)n_sites * 4));
    SECEDO_TRY(c->site_mask.alloc(n_sites));
    SECEDO_TRY(b_deep_len.alloc(((size_t)n_sites + 1) * 8));
    SECEDO_TRY(c->deep_off.alloc(((size_t)n_sites + 1) * 8));
    SECEDO_TRY(c->counts.alloc((size_t)n_sites * sizeof(SiteCounts)));
    SECEDO_TRY(b_totals.alloc(sizeof(Totals)));
    SECEDO_TRY(b_pair_len.alloc(((size_t)n_sites + 1) * 8));
    SECEDO_TRY(c->pair_off.alloc(((size_t)n_sites + 1) * 8));
    SECEDO_TRY(hipEventRecord(ev.e[2], s));
    SECEDO_TRY(site_compact(d_records, n_records, b_flag.as<uint32_t>(), b_mask.as<uint8_t>(), b_index.as<uint32_t>(), p,
                            n_sites, c->site_locus.as<uint32_t>(), c->site_mask.as<uint8_t>(),
                            b_deep_len.as<uint64_t>(), c->deep_off.as<uint64_t>(), b_scan.p, pair_scan, s));
    uint64_t n_deep = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_deep, c->deep_off.as<uint64_t>() + n_sites, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (n_deep > 0x7FFFFFFFull)
        return fail(SECEDO_E_LIMIT, "allele counts: the loci of more than 128 entries hold " + std::to_string(n_deep) +
                                        " entries, more than the 2^31 - 1 one call sorts");
    if (n_deep) {
        const size_t sort_bytes = deep_sort_workspace(n_deep);
        SECEDO_TRY(b_keys.alloc(n_deep * 8));
        SECEDO_TRY(c->keys_sorted.alloc(n_deep * 8));
        SECEDO_TRY(b_sort.alloc(sort_bytes));
        SECEDO_TRY(deep_sort(p, c->site_locus.as<uint32_t>(), c->site_mask.as<uint8_t>(), n_sites,
                             c->deep_off.as<uint64_t>(), n_deep, b_keys.as<uint64_t>(), c->keys_sorted.as<uint64_t>(),
                             b_sort.p, sort_bytes, s));
    }
    const Sites sites{c->site_locus.as<uint32_t>(), c->site_mask.as<uint8_t>(), n_sites, c->deep_off.as<uint64_t>(),
                      c->keys_sorted.as<uint64_t>()};
    SECEDO_TRY(count_pairs(p, sites, c->counts.as<SiteCounts>(), b_totals.as<Totals>(), b_pair_len.as<uint64_t>(),
                           c->pair_off.as<uint64_t>(), b_scan.p, pair_scan, s));
    SECEDO_TRY(hipEventRecord(ev.e[3], s));
    SECEDO_TRY(hipMemcpyAsync(&c->n_pairs, c->pair_off.as<uint64_t>() + n_sites, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(&c->totals, b_totals.p, sizeof(Totals), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    SECEDO_TRY(hipEventElapsedTime(&part, ev.e[2], ev.e[3]));
    ms += part;
    if (c->totals.error) return fail(SECEDO_E_INVALID_ARG, "a group id of the pileup is >= the number of cells");
    c->fits = n_sites <= site_capacity && c->n_pairs <= pair_capacity;
    if (c->fits) {
        SECEDO_TRY(c->pairs.alloc((size_t)c->n_pairs * sizeof(secedo_allele_pair)));
        SECEDO_TRY(hipEventRecord(ev.e[4], s));
        SECEDO_TRY(write_pairs(p, sites, c->pair_off.as<uint64_t>(), c->n_pairs, c->pairs.as<secedo_allele_pair>(), s));
        SECEDO_TRY(hipEventRecord(ev.e[5], s));
        SECEDO_TRY(hipStreamSynchronize(s));
        SECEDO_TRY(hipEventElapsedTime(&part, ev.e[4], ev.e[5]));
        ms += part;
    }
    g_info.selection = (uint32_t)selection;
    g_info.sites = n_sites;
    g_info.deep_sites = c->totals.deep_sites;
    g_info.entries_read = c->totals.entries;
    g_info.pairs = c->n_pairs;
    g_info.nnz_ad = c->totals.nnz_ad;
    g_info.nnz_dp = c->totals.nnz_dp;
    g_info.nnz_oth = c->totals.nnz_oth;
    g_info.count_kernel_ms = ms;
    g_info.count_ms = ms_since(t0);
    return SECEDO_OK;
}

struct OutFile {
    FILE *f = nullptr;
    std::string path;
    ~OutFile() {
        if (f) fclose(f);
    }
    int open(const std::filesystem::path &p) {
        path = p.string();
        f = fopen(path.c_str(), "wb");
        return f ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, "cannot write " + path);
    }
    int append(const void *data, size_t n) {
        if (n && fwrite(data, 1, n, f) != n) return fail(SECEDO_E_INVALID_ARG, "cannot write " + path);
        return SECEDO_OK;
    }
    int close() {
        const bool ok = fclose(f) == 0;
        f = nullptr;
        return ok ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, "cannot write " + path);
    }
};

std::string mtx_header(uint64_t n_sites, uint64_t n_cells, uint64_t nnz) {
    return "%%MatrixMarket matrix coordinate integer general\n%\n" + std::to_string(n_sites) + "\t" +
           std::to_string(n_cells) + "\t" + std::to_string(nnz) + "\n";
}

}  // namespace

int get_selection() {
    const int sel = g_selection.load();
    if (sel >= 0) return sel;
    const char *e = std::getenv("SECEDO_ALLELE_COUNTS");
    if (!e || !*e || std::strcmp(e, "none") == 0) return SECEDO_ALLELE_NONE;
    if (std::strcmp(e, "all") == 0) return SECEDO_ALLELE_ALL;
    if (std::strcmp(e, "cluster") == 0) return SECEDO_ALLELE_CLUSTER;
    return fail(SECEDO_E_INVALID_ARG, std::string("SECEDO_ALLELE_COUNTS=") + e + ": expected none, all or cluster");
}

int selection_kind(int *selection) {
    const int sel = get_selection();
    if (sel < 0) return sel;
    *selection = sel;
    return SECEDO_OK;
}

secedo_variant_allele_info &info() { return g_info; }

int check_cell_names(uint32_t n_cells) {
    std::lock_guard<std::mutex> lock(g_names_mutex);
    if (!g_names.empty() && g_names.size() != n_cells)
        return fail(SECEDO_E_INVALID_ARG, std::to_string(g_names.size()) + " cell names for " + std::to_string(n_cells) +
                                              " cells");
    return SECEDO_OK;
}

int write_outputs(const std::filesystem::path &out_dir, int selection, bool bgzf, const Pileup &pileup,
                  const secedo_variant_record *d_records, uint32_t n_records, const uint8_t *d_locus_ref,
                  const uint32_t *d_chr_locus_off, uint32_t n_chr, const uint32_t *d_locus_pos, hipStream_t s) {
    g_info = secedo_variant_allele_info{};
    g_info.output = bgzf ? SECEDO_VCF_BGZF : SECEDO_VCF_PLAIN;
    const uint32_t n_cells = pileup.n_cells;
    SECEDO_CALL(check_cell_names(n_cells));
    Counted c;
    SECEDO_CALL(run_counts(pileup, d_records, n_records, d_locus_ref, selection, UINT64_MAX, UINT64_MAX, &c, s));
    Clock::time_point t0 = Clock::now();
    const std::filesystem::path dir = out_dir / "allele_counts";
    std::error_code ec;
    std::filesystem::create_directories(dir, ec);
    if (ec) return fail(SECEDO_E_INVALID_ARG, "cannot create " + dir.string() + ": " + ec.message());
    {
        std::vector<std::string> names = cell_names();
        std::string text;
        for (uint32_t i = 0; i < n_cells; ++i) text += (names.empty() ? "cell_" + std::to_string(i) : names[i]) + "\n";
        OutFile f;
        SECEDO_CALL(f.open(dir / "cellSNP.samples.tsv"));
        SECEDO_CALL(f.append(text.data(), text.size()));
        SECEDO_CALL(f.close());
    }
    const char *const stem[kFiles] = {"cellSNP.tag.AD.mtx", "cellSNP.tag.DP.mtx", "cellSNP.tag.OTH.mtx", "cellSNP.base.vcf"};
    OutFile files[kFiles];
    for (uint32_t f = 0; f < kFiles; ++f) SECEDO_CALL(files[f].open(dir / (std::string(stem[f]) + (bgzf ? ".gz" : ""))));
    const std::string hdr[kFiles] = {mtx_header(c.n_sites, n_cells, c.totals.nnz_ad),
                                     mtx_header(c.n_sites, n_cells, c.totals.nnz_dp),
                                     mtx_header(c.n_sites, n_cells, c.totals.nnz_oth),
                                     "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"};
    std::string all_hdr;
    for (const std::string &h : hdr) all_hdr += h;
    Buf b_hdr;
    SECEDO_TRY(b_hdr.alloc(all_hdr.size()));
    SECEDO_TRY(hipMemcpyAsync(b_hdr.p, all_hdr.data(), all_hdr.size(), hipMemcpyHostToDevice, s));
    // a range: as many sites as keep the text's upper bound within the batch, one at the least
    std::vector<uint64_t> pair_off((size_t)c.n_sites + 1, 0);
    SECEDO_TRY(hipMemcpyAsync(pair_off.data(), c.pair_off.p, pair_off.size() * 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    g_info.write_ms += ms_lap(t0);
    const uint64_t batch = std::min(env_u64("SECEDO_ALLELE_BATCH_BYTES", kDefaultBatchBytes), kMaxBatchBytes);
    const auto bound = [&](uint32_t s0, uint32_t s1) {
        return (pair_off[s1] - pair_off[s0]) * 3 * kMaxMtxLine + uint64_t(s1 - s0) * kMaxVcfLine;
    };
    Buf b_len, b_off, b_scan, b_file_off, b_text;
    SECEDO_TRY(b_file_off.alloc((kFiles + 1) * 8));
    std::vector<uint8_t> down, packed;
    std::vector<uint64_t> packed_off;
    uint32_t s0 = 0;
    do {
        uint32_t s1 = s0 < c.n_sites ? s0 + 1 : s0;
        while (s1 < c.n_sites && bound(s0, s1 + 1) <= batch) ++s1;
        const bool first = s0 == 0, last = s1 == c.n_sites;
        FormatIn in{c.pairs.as<secedo_allele_pair>(), c.counts.as<SiteCounts>(), c.site_locus.as<uint32_t>(),
                    c.site_mask.as<uint8_t>(), d_chr_locus_off, n_chr, d_locus_pos, s0, s1, pair_off[s0], pair_off[s1],
                    {0, 0, 0, 0}};
        if (in.p1 - in.p0 > 0x3FFFFFFFull)
            return fail(SECEDO_E_LIMIT, "allele counts: one site with more than 2^30 cells");
        for (uint32_t f = 0; first && f < kFiles; ++f) in.hdr_len[f] = (uint32_t)hdr[f].size();
        const uint64_t items = format_items(in);
        const size_t scan_bytes = format_scan_workspace(items);
        SECEDO_TRY(b_len.grow(items * 8, 0, s));
        SECEDO_TRY(b_off.grow(items * 8, 0, s));
        SECEDO_TRY(b_scan.grow(scan_bytes, 0, s));
        SECEDO_TRY(format_measure(in, b_len.as<uint64_t>(), b_off.as<uint64_t>(), b_file_off.as<uint64_t>(), b_scan.p,
                                  scan_bytes, s));
        std::vector<uint64_t> file_off(kFiles + 1);
        SECEDO_TRY(hipMemcpyAsync(file_off.data(), b_file_off.p, (kFiles + 1) * 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        const uint64_t total = file_off[kFiles];
        SECEDO_TRY(b_text.grow(total + 2 * bgzf::kDeflateInSlack, 0, s));
        uint8_t *d_text = b_text.as<uint8_t>() + bgzf::kDeflateInSlack;
        SECEDO_TRY(format_write(in, b_off.as<uint64_t>(), b_hdr.as<uint8_t>(), d_text, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        g_info.text_bytes += total;
        g_info.ranges += 1;
        g_info.format_ms += ms_lap(t0);
        if (bgzf) {
            bgzf::EncoderCounts counts;
            SECEDO_CALL(vcf::deflate_device(d_text, file_off, &packed, &packed_off, s, nullptr, &counts));
            g_info.deflate_ms += counts.deflate_ms;
            g_info.download_ms += counts.download_ms;
            (void)ms_lap(t0);
            for (uint32_t f = 0; f < kFiles; ++f) {  // the EOF member closes the file, not the range
                const uint64_t n = packed_off[f + 1] - packed_off[f] - (last ? 0 : bgzf::kEofBytes);
                SECEDO_CALL(files[f].append(packed.data() + packed_off[f], n));
                g_info.compressed_bytes += n;
            }
        } else {
            down.resize(total);
            if (total) SECEDO_TRY(hipMemcpyAsync(down.data(), d_text, total, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            g_info.download_ms += ms_lap(t0);
            for (uint32_t f = 0; f < kFiles; ++f)
                SECEDO_CALL(files[f].append(down.data() + file_off[f], file_off[f + 1] - file_off[f]));
        }
        g_info.write_ms += ms_lap(t0);
        s0 = s1;
    } while (s0 < c.n_sites);
    for (OutFile &f : files) SECEDO_CALL(f.close());
    g_info.write_ms += ms_lap(t0);
    return SECEDO_OK;
}

}  // namespace allele
}  // namespace secedo

using namespace secedo::host;
namespace A = secedo::allele;

extern "C" {

int secedo_variant_set_allele_counts(int selection) {
    if (selection != SECEDO_ALLELE_NONE && selection != SECEDO_ALLELE_ALL && selection != SECEDO_ALLELE_CLUSTER)
        return fail(SECEDO_E_INVALID_ARG, "selection must be SECEDO_ALLELE_NONE, SECEDO_ALLELE_ALL or SECEDO_ALLELE_CLUSTER");
    A::g_selection.store(selection);
    return SECEDO_OK;
}

int secedo_variant_get_allele_counts(void) { return A::get_selection(); }

int secedo_variant_set_cell_names(const char *const *names, uint32_t n) {
    if (n && !names) return fail(SECEDO_E_INVALID_ARG, "null argument");
    std::vector<std::string> v(n);
    for (uint32_t i = 0; i < n; ++i) {
        v[i] = names[i] ? names[i] : "";
        if (v[i].empty() || v[i].find_first_of("\t\n\r") != std::string::npos)
            return fail(SECEDO_E_INVALID_ARG, "cell name " + std::to_string(i) + " is empty or holds a tab or a line break");
    }
    std::lock_guard<std::mutex> lock(A::g_names_mutex);
    A::g_names = std::move(v);
    return SECEDO_OK;
}

int secedo_variant_set_cell_names_file(const char *path) {
    if (!path) return fail(SECEDO_E_INVALID_ARG, "null argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(SECEDO_E_INVALID_ARG, std::string("cannot read ") + path);
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
    std::vector<std::string> v;
    for (size_t b = 0; b < text.size();) {
        size_t e = text.find('\n', b);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(b, e - b);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line.find('\t') != std::string::npos)
            return fail(SECEDO_E_INVALID_ARG, std::string(path) + ": line " + std::to_string(v.size() + 1) +
                                                  " is empty or holds a tab");
        v.push_back(std::move(line));
        b = e + 1;
    }
    std::lock_guard<std::mutex> lock(A::g_names_mutex);
    A::g_names = std::move(v);
    return SECEDO_OK;
}

static int check_selection(int selection) {
    if (selection != SECEDO_ALLELE_ALL && selection != SECEDO_ALLELE_CLUSTER)
        return fail(SECEDO_E_INVALID_ARG, "selection must be SECEDO_ALLELE_ALL or SECEDO_ALLELE_CLUSTER");
    return SECEDO_OK;
}

static int check_records(const secedo_variant_record *records, uint32_t n_records, uint32_t n_loci) {
    if (n_records && !records) return fail(SECEDO_E_INVALID_ARG, "null argument");
    for (uint32_t k = 0; k < n_records; ++k) {
        if (records[k].locus >= n_loci) return fail(SECEDO_E_INVALID_ARG, "a record's locus is >= n_loci");
        if (k && records[k].locus < records[k - 1].locus) return fail(SECEDO_E_INVALID_ARG, "records must ascend in locus");
    }
    return SECEDO_OK;
}

int secedo_variant_allele_masks(const secedo_variant_record *records, uint32_t n_records, const uint8_t *locus_ref,
                                uint32_t n_loci, int selection, uint32_t *site_locus, uint8_t *ref_mask,
                                uint8_t *alt_mask, uint32_t capacity, uint32_t *n_sites) {
    if (!n_sites || (n_records && !locus_ref)) return fail(SECEDO_E_INVALID_ARG, "null argument");
    SECEDO_CALL(check_selection(selection));
    SECEDO_CALL(check_records(records, n_records, n_loci));
    for (int pass = 0; pass < 2; ++pass) {  // count, then fill
        uint32_t n = 0;
        for (uint32_t r = 0; r < n_records;) {
            const uint32_t l = records[r].locus;
            uint32_t g = 0;
            bool cluster = false;
            for (; r < n_records && records[r].locus == l; ++r) {
                g |= A::genotype_bits(records[r].genotype);
                cluster = cluster || records[r].kind == SECEDO_VARIANT_CLUSTER;
            }
            if (selection != SECEDO_ALLELE_ALL && !cluster) continue;
            if (pass) {
                const uint32_t m = A::site_masks(locus_ref[l], g);
                site_locus[n] = l;
                ref_mask[n] = uint8_t(m & 15);
                alt_mask[n] = uint8_t(m >> 4);
            }
            ++n;
        }
        *n_sites = n;
        if (n > capacity) return fail(SECEDO_E_LIMIT, std::to_string(n) + " sites, capacity " + std::to_string(capacity));
        if (n && (!site_locus || !ref_mask || !alt_mask)) return fail(SECEDO_E_INVALID_ARG, "null argument");
    }
    return SECEDO_OK;
}

int secedo_variant_allele_counts_device(int device_id, const uint64_t *d_locus_entry_off, const uint16_t *d_id_base16,
                                        const uint32_t *d_id_base32, uint32_t n_loci,
                                        const secedo_variant_record *records, uint32_t n_records,
                                        const uint8_t *d_locus_ref, uint32_t n_cells, int selection,
                                        uint32_t *site_locus, uint8_t *ref_mask, uint8_t *alt_mask,
                                        uint32_t *site_totals, uint32_t site_capacity, uint32_t *n_sites,
                                        secedo_allele_pair *pairs, uint64_t pair_capacity, uint64_t *n_pairs,
                                        void *stream) {
    if (!n_sites || !n_pairs || !d_locus_entry_off || (n_records && !d_locus_ref) || (!!d_id_base16 == !!d_id_base32))
        return fail(SECEDO_E_INVALID_ARG, "invalid argument (exactly one of id_base16 / id_base32)");
    SECEDO_CALL(check_selection(selection));
    SECEDO_CALL(check_records(records, n_records, n_loci));
    SECEDO_CALL(set_device(device_id));
    hipStream_t s = static_cast<hipStream_t>(stream);
    A::g_info = secedo_variant_allele_info{};
    Buf b_rec;
    SECEDO_TRY(b_rec.alloc((size_t)n_records * sizeof(secedo_variant_record)));
    if (n_records)
        SECEDO_TRY(hipMemcpyAsync(b_rec.p, records, (size_t)n_records * sizeof(secedo_variant_record), hipMemcpyHostToDevice, s));
    const A::Pileup p{d_locus_entry_off, d_id_base16, d_id_base32, n_cells};
    A::Counted c;
    SECEDO_CALL(A::run_counts(p, b_rec.as<secedo_variant_record>(), n_records, d_locus_ref, selection, site_capacity,
                              pair_capacity, &c, s));
    *n_sites = c.n_sites;
    *n_pairs = c.n_pairs;
    if (!c.fits)
        return fail(SECEDO_E_LIMIT, std::to_string(c.n_sites) + " sites, capacity " + std::to_string(site_capacity) + "; " +
                                        std::to_string(c.n_pairs) + " pairs, capacity " + std::to_string(pair_capacity));
    if ((c.n_sites && (!site_locus || !ref_mask || !alt_mask || !site_totals)) || (c.n_pairs && !pairs))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    Clock::time_point t0 = Clock::now();
    std::vector<uint8_t> mask(c.n_sites);
    std::vector<A::SiteCounts> counts(c.n_sites);
    if (c.n_sites) {
        SECEDO_TRY(hipMemcpyAsync(site_locus, c.site_locus.p, (size_t)c.n_sites * 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(mask.data(), c.site_mask.p, c.n_sites, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(counts.data(), c.counts.p, (size_t)c.n_sites * sizeof(A::SiteCounts), hipMemcpyDeviceToHost, s));
    }
    if (c.n_pairs)
        SECEDO_TRY(hipMemcpyAsync(pairs, c.pairs.p, (size_t)c.n_pairs * sizeof(secedo_allele_pair), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < c.n_sites; ++i) {
        ref_mask[i] = mask[i] & 15;
        alt_mask[i] = mask[i] >> 4;
        site_totals[3 * i] = counts[i].ad;
        site_totals[3 * i + 1] = counts[i].rd;
        site_totals[3 * i + 2] = counts[i].oth;
    }
    A::g_info.download_ms = ms_since(t0);
    return SECEDO_OK;
}

int secedo_variant_allele_stats(secedo_variant_allele_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = A::info();
    return SECEDO_OK;
}

}  // extern "C"
