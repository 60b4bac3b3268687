// variant_api.cpp -- host side of include/secedo_variant.h: the reference genome (FASTA + Varsim map), the
// per-locus gather of the reference genotype, the constant tables and the launches of variant_kernels.hip for the
// reference's variant_calling() (variant_calling.cpp:81-461). The files it leaves are vcf_output.cpp's.
//
// The FASTA is memory-mapped (a compressed one inflated, fasta_source.cpp) and read through a small restatement of
// the std::ifstream calls the reference makes (getline, peek, get, putback), so that its quirks carry over: a contig
// header directly after another is read as sequence, a FASTA with fewer contigs than the pileup has chromosomes
// leaves the last contig in place (:161-163), and a missing paternal contig reads as empty. That is the host route;
// the device route of the same results is fasta_device.cpp.
#include "secedo_variant.h"
#include "secedo_simmat.h"
#include "allele_output.hpp"
#include "fasta_source.hpp"
#include "host_util.hpp"
#include "bgzf_deflate_kernels.hpp"
#include "variant_kernels.hpp"
#include "tabix_host.hpp"
#include "vcf_output.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace {

using secedo::variant::Logs;
using namespace secedo::host;
using namespace secedo::fasta_host;

// CharToInt (util/util.hpp:17-22): A/a 0, C/c 1, G/g 2, T/t/U/u 3, anything else 5
uint8_t char_to_int(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 5;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The reference genome

// A text it does not own (the mapped file, or what was inflated from it) with the std::istream calls
// get_next_chromosome makes. `fail` is the stream's failbit: once set, every call fails, as the reference's stream
// does.
struct Fasta {
    const char *p = nullptr;
    size_t n = 0, pos = 0;
    bool fail = false;
    uint64_t headers = 0;  // header lines read

    Fasta(const uint8_t *text, size_t bytes) : p(reinterpret_cast<const char *>(text)), n(bytes) {}
    bool getline(std::string_view *line) {
        if (fail || pos >= n) {
            fail = true;
            return false;
        }
        const char *nl = static_cast<const char *>(memchr(p + pos, '\n', n - pos));
        const size_t end = nl ? static_cast<size_t>(nl - p) : n;
        *line = std::string_view(p + pos, end - pos);
        pos = nl ? end + 1 : n;
        return true;
    }
    int peek() const { return (fail || pos >= n) ? EOF : static_cast<unsigned char>(p[pos]); }
    int get() {
        if (fail || pos >= n) {
            fail = true;
            return EOF;
        }
        return static_cast<unsigned char>(p[pos++]);
    }
    void putback() {
        if (!fail && pos > 0) --pos;
    }
};

struct ChrMap {
    uint32_t start_pos;
    uint32_t len;
    char tr;
    uint8_t chromosome_id;
};

struct MapEntry {
    std::string name;
    ChrMap m;
};

// split(s, '\t') of util.cpp: std::getline segments, so a trailing delimiter adds no empty field
std::vector<std::string> split(const std::string &s, char c) {
    std::vector<std::string> out;
    size_t b = 0;
    while (b < s.size()) {
        size_t e = s.find(c, b);
        if (e == std::string::npos) e = s.size();
        out.emplace_back(s, b, e - b);
        b = e + 1;
    }
    return out;
}

bool parse_ulong(const std::string &s, unsigned long *v) {  // std::stoul, which throws where this fails
    const char *b = s.c_str();
    char *end;
    errno = 0;
    *v = strtoul(b, &end, 10);
    return end != b && errno == 0;
}

// chromosome_to_id (util.cpp:143-160)
bool chromosome_to_id(const std::string &chromosome, uint8_t *id) {
    char *p;
    const uint32_t converted = static_cast<uint32_t>(strtol(chromosome.c_str(), &p, 10));
    if (*p) {
        if (chromosome != "X" && chromosome != "Y") return false;
        *id = chromosome == "X" ? 22 : 23;
        return true;
    }
    if (converted > 22) return false;
    *id = static_cast<uint8_t>(converted - 1);
    return true;
}

// read_map (:81-115), entries in file order
int read_map(const char *map_file, std::vector<MapEntry> *out) {
    out->clear();
    if (!map_file || !*map_file) return SECEDO_OK;
    FILE *f = fopen(map_file, "rb");
    if (!f) return fail(SECEDO_E_INVALID_ARG, std::string("Map file: ") + map_file + " does not exist.");
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
    size_t b = 0;
    while (b < text.size()) {
        size_t e = text.find('\n', b);
        if (e == std::string::npos) e = text.size();
        const std::string line = text.substr(b, e - b);
        b = e + 1;
        if (line.empty() || line[0] == '#') continue;
        const std::vector<std::string> cols = split(line, '\t');
        if (cols.size() != 8)
            return fail(SECEDO_E_INVALID_ARG, std::string("Invalid map file: ") + map_file + ". Has " +
                                                      std::to_string(cols.size()) + " columns, expected 8.");
        // the chromosome-name guard of :102 (c < '1' && c > '9' && ...) is never true: no line is skipped there
        if (cols[6] == "SEQ") continue;
        unsigned long start, len;
        if (!parse_ulong(cols[2], &start) || !parse_ulong(cols[0], &len))
            return fail(SECEDO_E_INVALID_ARG, std::string("Invalid map file: ") + map_file + ". Bad line: " + line);
        MapEntry m;
        m.name = cols[1];
        m.m.start_pos = static_cast<uint32_t>(start) - 1;
        m.m.len = static_cast<uint32_t>(len);
        m.m.tr = cols[6] == "INS" ? 'I' : 'D';
        if (!chromosome_to_id(cols[3], &m.m.chromosome_id))
            return fail(SECEDO_E_INVALID_ARG, "Invalid chromosome: " + cols[3] + ". Must be 1..22, X, Y");
        out->push_back(std::move(m));
    }
    return SECEDO_OK;
}

// apply_map (:117-141). A start position past the contig's end, where the reference reads out of bounds, is
// an error.
int apply_map(const std::vector<ChrMap> &map, const std::vector<uint8_t> &chr_data, std::vector<uint8_t> *out) {
    uint64_t i = 0;
    out->clear();
    out->reserve(chr_data.size());
    for (const ChrMap &m : map) {
        if (i < m.start_pos) {
            if (m.start_pos > chr_data.size())
                return fail(SECEDO_E_INVALID_ARG, "map entry at " + std::to_string(m.start_pos) +
                                                          " lies past the contig's end (" +
                                                          std::to_string(chr_data.size()) + ")");
            out->insert(out->end(), chr_data.begin() + i, chr_data.begin() + m.start_pos);
            i = m.start_pos;
        }
        if (m.tr == 'D') out->insert(out->end(), m.len, 5);
        else i += m.len;
    }
    if (i < chr_data.size()) out->insert(out->end(), chr_data.begin() + i, chr_data.end());
    return SECEDO_OK;
}

using Map = std::unordered_map<std::string, std::vector<ChrMap>>;

Map group_map(const std::vector<MapEntry> &entries) {
    Map m;
    for (const MapEntry &e : entries) m[e.name].push_back(e.m);
    return m;
}

// read_contig (:143-153)
void read_contig(Fasta &f, std::vector<uint8_t> *chr_data) {
    std::string_view line;
    while (f.getline(&line)) {
        const size_t at = chr_data->size();
        chr_data->resize(at + line.size());
        uint8_t *d = chr_data->data() + at;
        for (size_t k = 0; k < line.size(); ++k) d[k] = char_to_int(line[k]);
        if (f.peek() == '>') break;
    }
}

// check_is_diploid (:281-286): the first whitespace-delimited word contains "maternal"
bool check_is_diploid(const Fasta &f) {
    size_t b = 0;
    while (b < f.n && isspace(static_cast<unsigned char>(f.p[b]))) ++b;
    size_t e = b;
    while (e < f.n && !isspace(static_cast<unsigned char>(f.p[e]))) ++e;
    return std::string_view(f.p + b, e - b).find("maternal") != std::string_view::npos;
}

// get_next_chromosome (:155-224)
int get_next_chromosome(Fasta &f, const Map &map, bool is_diploid, std::vector<uint8_t> *chr_data,
                        std::vector<uint8_t> *tmp1, std::vector<uint8_t> *tmp2) {
    std::string_view header;
    if (!f.getline(&header)) return SECEDO_OK;  // fewer contigs: the previous one stays
    ++f.headers;
    if (header.empty()) return fail(SECEDO_E_INVALID_ARG, "reference genome: empty line where a contig header is expected");
    const char chromosome = header.size() > 1 ? header[1] : '\0';
    std::string chr_name(header.substr(1));
    tmp1->clear();
    read_contig(f, tmp1);
    auto it = map.find(chr_name);
    if (it != map.end()) SECEDO_CALL(apply_map(it->second, *tmp1, chr_data));
    else std::swap(*tmp1, *chr_data);

    const int ch1 = f.get();
    const int ch2 = f.peek();
    if (ch1 != EOF) f.putback();
    if (!is_diploid || (chromosome == 'X' && ch2 == 'Y') || chromosome == 'Y') {
        for (uint8_t &x : *chr_data) x |= static_cast<uint8_t>(x << 3);
        return SECEDO_OK;
    }
    std::string_view second;
    const bool has_second = f.getline(&second);
    f.headers += has_second;
    if (has_second && !second.empty()) chr_name.assign(second.substr(1));  // else the line is unchanged
    tmp1->clear();
    read_contig(f, tmp1);
    it = map.find(chr_name);
    if (it != map.end()) SECEDO_CALL(apply_map(it->second, *tmp1, tmp2));
    else std::swap(*tmp1, *tmp2);
    if (chr_data->size() != tmp2->size())
        return fail(SECEDO_E_INVALID_ARG, "Invalid reference genome. Maternal and paternal chromosome sizes don't "
                                          "match (" + std::to_string(chr_data->size()) + " vs " +
                                          std::to_string(tmp2->size()) + ")");
    for (size_t i = 0; i < chr_data->size(); ++i) (*chr_data)[i] = static_cast<uint8_t>(((*chr_data)[i] << 3) | (*tmp2)[i]);
    return SECEDO_OK;
}

// The file opened for a host function: both compressed kinds inflated with zlib.
int open_text(const char *path, Source *src) {
    SECEDO_CALL(open_source(path, src));
    if (!src->has_text) SECEDO_CALL(inflate_bgzf_host(src));
    return SECEDO_OK;
}

// The host half of variant_calling before the locus loop: locus_ref and chr_locus_end (see the header).
int reference_genotypes(const Source &src, const char *map_file, const uint32_t *chr_locus_off, uint32_t n_chr,
                        const uint32_t *locus_pos, uint8_t *locus_ref, uint32_t *chr_locus_end, double *fasta_ms) {
    Clock::time_point t0 = Clock::now();
    Fasta f(src.text(), src.text_bytes());
    std::vector<MapEntry> entries;
    SECEDO_CALL(read_map(map_file, &entries));
    const Map map = group_map(entries);
    const bool diploid = check_is_diploid(f);
    std::vector<uint8_t> chr, tmp1, tmp2;
    double parse = 0;
    for (uint32_t c = 0; c < n_chr; ++c) {
        Clock::time_point t1 = Clock::now();
        SECEDO_CALL(get_next_chromosome(f, map, diploid, &chr, &tmp1, &tmp2));
        parse += ms_lap(t1);
        const uint32_t b = chr_locus_off[c], e = chr_locus_off[c + 1];
        uint32_t l = b;
        for (; l < e; ++l) {
            const uint32_t p = locus_pos[l] - 1;  // uint32: position 0 wraps and ends the chromosome
            if (p >= chr.size()) break;
            locus_ref[l] = chr[p];
        }
        chr_locus_end[c] = l;
        for (; l < e; ++l) locus_ref[l] = 0;
    }
    if (fasta_ms) *fasta_ms = parse + (n_chr == 0 ? ms_lap(t0) : 0.0);
    secedo_variant_fasta_info &st = info();
    st.route = SECEDO_FASTA_HOST;
    st.text_bytes = f.pos;
    st.contigs = st.contigs_used = f.headers;
    return SECEDO_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Device side

// The reference genotypes of a pileup resident in HBM, by the route the file and the setting ask for.
struct RefArgs {
    const uint32_t *d_chr_locus_off, *chr_locus_off;  // device and host copies
    uint32_t n_chr;
    const uint32_t *d_locus_pos, *locus_pos;  // either may be null: the missing copy is made when the route needs it
    uint32_t n_loci;
    uint8_t *d_locus_ref;  // out, HBM
    uint8_t *locus_ref;    // out, host; may be null
    uint32_t *chr_locus_end;
};

// fasta_ms / gather_ms as secedo_variant_times has them: on the device route the whole is fasta_ms. On the host route
// with a.locus_ref given, its upload is left in flight on s.
int reference_any(const char *fasta, const char *map_file, const RefArgs &a, double *fasta_ms, double *gather_ms,
                  hipStream_t s) {
    Clock::time_point t0 = Clock::now();
    Source src;
    SECEDO_CALL(open_source(fasta, &src));
    bool device = false;
    SECEDO_CALL(fasta_route(&device));
    device = device || src.kind == SECEDO_FASTA_KIND_BGZF;
    if (device && map_file && *map_file) {  // the Varsim map is the host route's alone
        device = false;
        if (!src.has_text) SECEDO_CALL(download_bgzf_text(&src, s));
        info().fell_back_for_map = 1;
    }
    if (!device) {
        std::vector<uint32_t> pos;
        std::vector<uint8_t> ref;
        const uint32_t *locus_pos = a.locus_pos;
        if (!locus_pos) {
            pos.resize(a.n_loci);
            if (a.n_loci) SECEDO_TRY(hipMemcpyAsync(pos.data(), a.d_locus_pos, (size_t)a.n_loci * 4, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            locus_pos = pos.data();
        }
        uint8_t *locus_ref = a.locus_ref;
        if (!locus_ref) {
            ref.resize(a.n_loci);
            locus_ref = ref.data();
        }
        SECEDO_CALL(reference_genotypes(src, map_file, a.chr_locus_off, a.n_chr, locus_pos, locus_ref, a.chr_locus_end,
                                        fasta_ms));
        *gather_ms = ms_since(t0) - *fasta_ms;
        if (a.n_loci) SECEDO_TRY(hipMemcpyAsync(a.d_locus_ref, locus_ref, a.n_loci, hipMemcpyHostToDevice, s));
        if (!a.locus_ref) SECEDO_TRY(hipStreamSynchronize(s));
        return SECEDO_OK;
    }
    Buf b_pos;
    const uint32_t *d_locus_pos = a.d_locus_pos;
    if (!d_locus_pos) {
        SECEDO_TRY(b_pos.alloc((size_t)a.n_loci * 4));
        if (a.n_loci) SECEDO_TRY(hipMemcpyAsync(b_pos.p, a.locus_pos, (size_t)a.n_loci * 4, hipMemcpyHostToDevice, s));
        d_locus_pos = b_pos.as<uint32_t>();
    }
    bool diploid = false;
    if (src.has_text) diploid = first_word_has_maternal(src.text(), src.text_bytes());
    else SECEDO_CALL(bgzf_is_diploid(src, &diploid));
    SECEDO_CALL(device_genotypes(src, diploid, a.d_chr_locus_off, a.chr_locus_off, a.n_chr, d_locus_pos, a.n_loci,
                                 a.d_locus_ref, a.chr_locus_end, s));
    if (a.locus_ref && a.n_loci)
        SECEDO_TRY(hipMemcpyAsync(a.locus_ref, a.d_locus_ref, a.n_loci, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    *fasta_ms = ms_since(t0);
    *gather_ms = 0;
    return SECEDO_OK;
}

Logs host_logs(double hetero_prior, double theta) {
    return Logs{std::log(theta / 3), std::log(1 - theta), std::log(0.5 - theta / 3), std::log(hetero_prior)};
}

// likely_homozygous' threshold, std::round(cov * theta + std::sqrt(cov * theta * (1 - theta))), for every u16 cov
std::vector<double> threshold_table(double theta) {
    std::vector<double> t(secedo::variant::kThresholds);
    for (uint32_t cov = 0; cov < t.size(); ++cov) t[cov] = std::round(cov * theta + std::sqrt(cov * theta * (1 - theta)));
    return t;
}

// Global atomics by default: on the whole-pileup bench the LDS copy (64 KiB per workgroup, two workgroups per CU)
// took 25.1 ms against 20.0 ms, on C3 1.22 ms against 1.21 ms.
constexpr bool kLdsDefault = false;

struct Calls {
    std::vector<secedo_variant_record> records;
    Buf d_records;  // the records in HBM, for a caller that asked to keep them there
    uint32_t total = 0;
    double kernel_ms = 0;
};

// Both passes on a resident pileup; records downloaded when they fit `capacity`, or left in out->d_records and not
// downloaded when keep_on_device.
int run_calls(const uint32_t *d_chr_locus_off, uint32_t n_chr, const uint64_t *d_locus_entry_off,
              const uint16_t *d_id_base16, const uint32_t *d_id_base32, uint32_t n_loci, const uint16_t *d_clusters,
              uint32_t n_groups, const uint8_t *d_locus_ref, const uint32_t *chr_locus_end, double hetero_prior,
              double theta, uint32_t capacity, uint32_t *d_mismatch, uint32_t *d_loci, Calls *out, hipStream_t s,
              bool keep_on_device = false) {
    namespace V = secedo::variant;
    const uint32_t ranges = V::num_ranges(n_loci);
    const std::vector<double> thr = threshold_table(theta);
    const size_t scan_bytes = V::scan_workspace(n_loci);
    Buf b_thr, b_end, b_cnt, b_off, b_flag, b_err, b_scan;
    Buf &b_rec = out->d_records;
    SECEDO_TRY(b_thr.alloc(thr.size() * sizeof(double)));
    SECEDO_TRY(b_end.alloc((size_t)n_chr * 4));
    SECEDO_TRY(b_cnt.alloc(((size_t)ranges + 1) * 4));
    SECEDO_TRY(b_off.alloc(((size_t)ranges + 1) * 4));
    SECEDO_TRY(b_flag.alloc(n_loci));
    SECEDO_TRY(b_err.alloc(4));
    SECEDO_TRY(b_scan.alloc(scan_bytes));
    SECEDO_TRY(hipMemcpyAsync(b_thr.p, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_chr) SECEDO_TRY(hipMemcpyAsync(b_end.p, chr_locus_end, (size_t)n_chr * 4, hipMemcpyHostToDevice, s));

    V::CallsIn in{d_chr_locus_off, b_end.as<uint32_t>(), n_chr, d_locus_entry_off, d_id_base16, d_id_base32, n_loci,
                  d_clusters, n_groups, d_locus_ref, b_thr.as<double>(), host_logs(hetero_prior, theta)};
    hipEvent_t e0, e1, e2, e3;
    SECEDO_TRY(hipEventCreate(&e0));
    SECEDO_TRY(hipEventCreate(&e1));
    SECEDO_TRY(hipEventCreate(&e2));
    SECEDO_TRY(hipEventCreate(&e3));
    struct Ev {
        hipEvent_t *e[4];
        ~Ev() { for (hipEvent_t *x : e) (void)hipEventDestroy(*x); }
    } ev{{&e0, &e1, &e2, &e3}};
    // the counted-entry counters: LDS-privatised or global atomics (env SECEDO_VARIANT_COUNTERS=lds|global; the
    // default is the faster on the measured workloads, see DESIGN)
    const char *mode = getenv("SECEDO_VARIANT_COUNTERS");
    const bool lds = mode ? strcmp(mode, "global") != 0 : kLdsDefault;
    int dev = 0, cus = 0;
    SECEDO_TRY(hipGetDevice(&dev));
    SECEDO_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint32_t max_blocks = static_cast<uint32_t>(std::max(cus, 1)) * (lds ? 2u : 8u);
    SECEDO_TRY(hipEventRecord(e0, s));
    SECEDO_TRY(V::count_calls(in, d_mismatch, d_loci, b_cnt.as<uint32_t>(), b_off.as<uint32_t>(), b_flag.as<uint8_t>(),
                          b_err.as<uint32_t>(), b_scan.p, scan_bytes, lds, max_blocks, s));
    SECEDO_TRY(hipEventRecord(e1, s));
    uint32_t head[2] = {0, 0};
    SECEDO_TRY(hipMemcpyAsync(&head[0], b_off.as<uint32_t>() + ranges, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(&head[1], b_err.p, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (head[1]) return fail(SECEDO_E_INVALID_ARG, "a group id of the pileup is >= the length of clusters");
    out->total = head[0];
    float k1 = 0, k2 = 0;
    SECEDO_TRY(hipEventElapsedTime(&k1, e0, e1));
    out->kernel_ms = k1;
    if (out->total > capacity) return SECEDO_OK;
    SECEDO_TRY(b_rec.alloc((size_t)out->total * sizeof(secedo_variant_record)));
    SECEDO_TRY(hipEventRecord(e2, s));
    SECEDO_TRY(V::write_calls(in, b_off.as<uint32_t>(), b_flag.as<uint8_t>(), b_rec.as<secedo_variant_record>(), s));
    SECEDO_TRY(hipEventRecord(e3, s));
    if (!keep_on_device) out->records.resize(out->total);
    if (out->total && !keep_on_device)
        SECEDO_TRY(hipMemcpyAsync(out->records.data(), b_rec.p, (size_t)out->total * sizeof(secedo_variant_record),
                              hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    SECEDO_TRY(hipEventElapsedTime(&k2, e2, e3));
    out->kernel_ms += k2;
    return SECEDO_OK;
}

// A reference genome that the reference refuses (unequal maternal and paternal contigs: its process ends there, after
// the preambles are written) leaves nothing behind here: out_dir is removed again if this call created it. remove()
// takes an empty directory only. Every other failure leaves out_dir as it is.
struct OutDirGuard {
    const char *dir = nullptr;
    bool created = false, refused = false;
    int done(int rc) {
        if (rc != SECEDO_OK && created && refused && dir) {
            std::error_code ec;
            std::filesystem::remove(dir, ec);
        }
        return rc;
    }
};

// variant_calling on a resident pileup with the host copies of its chromosome offsets and positions (the positions
// also in HBM where the caller has them there: d_locus_pos, else null).
int calling(int device_id, const uint32_t *d_chr_locus_off, const uint32_t *chr_locus_off, uint32_t n_chr,
            const uint32_t *locus_pos, const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
            const uint16_t *d_id_base16,
            const uint32_t *d_id_base32, uint32_t n_loci, const uint16_t *clusters, uint32_t n,
            const char *reference_genome, const char *map_file, double hetero_prior, double theta,
            const char *out_dir, secedo_variant_times *times, hipStream_t s, double pre_device_ms,
            OutDirGuard *out_guard) {
    secedo_variant_times t{};
    Clock::time_point t0 = Clock::now();
    int output = SECEDO_VCF_PLAIN;
    SECEDO_CALL(secedo::vcf::output_kind(&output));
    const bool bgzf = output == SECEDO_VCF_BGZF;  // the text is then made in HBM: locus_ref stays there too
    int index = SECEDO_VCF_INDEX_NONE;
    SECEDO_CALL(secedo::tabix_host::index_kind(&index));
    secedo::tabix_host::info() = secedo_variant_tabix_info{};
    if (index == SECEDO_VCF_INDEX_TBI && !bgzf)
        return fail(SECEDO_E_INVALID_ARG, "vcf_index tbi indexes the compressed output only: add --vcf_output bgzf "
                                          "(SECEDO_VCF=bgzf, secedo_variant_set_vcf_output)");
    int allele = SECEDO_ALLELE_NONE;
    SECEDO_CALL(secedo::allele::selection_kind(&allele));
    secedo::allele::info() = secedo_variant_allele_info{};
    if (allele != SECEDO_ALLELE_NONE) SECEDO_CALL(secedo::allele::check_cell_names(n));
    std::vector<uint8_t> locus_ref(bgzf ? 0 : n_loci);
    std::vector<uint32_t> chr_end(n_chr);
    Buf b_ref, b_cl, b_mm, b_loci, b_pos;
    SECEDO_TRY(b_ref.alloc(n_loci));
    const RefArgs ref{d_chr_locus_off, chr_locus_off, n_chr, d_locus_pos, locus_pos, n_loci, b_ref.as<uint8_t>(),
                      bgzf ? nullptr : locus_ref.data(), chr_end.data()};
    if (int rc = reference_any(reference_genome, map_file, ref, &t.fasta_ms, &t.gather_ms, s)) {
        out_guard->refused = true;
        return rc;
    }
    (void)ms_lap(t0);
    const uint32_t num_clusters = static_cast<uint32_t>(*std::max_element(clusters, clusters + n)) + 1;

    SECEDO_TRY(b_cl.alloc((size_t)n * 2));
    SECEDO_TRY(b_mm.alloc((size_t)n * 4));
    SECEDO_TRY(b_loci.alloc((size_t)n * 4));
    SECEDO_TRY(hipMemcpyAsync(b_cl.p, clusters, (size_t)n * 2, hipMemcpyHostToDevice, s));
    Calls calls;
    SECEDO_CALL(run_calls(d_chr_locus_off, n_chr, d_locus_entry_off, d_id_base16, d_id_base32, n_loci, b_cl.as<uint16_t>(),
                      n, b_ref.as<uint8_t>(), chr_end.data(), hetero_prior, theta, UINT32_MAX, b_mm.as<uint32_t>(),
                      b_loci.as<uint32_t>(), &calls, s, bgzf));
    std::vector<uint32_t> mismatch(n), loci(n);
    SECEDO_TRY(hipMemcpyAsync(mismatch.data(), b_mm.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(loci.data(), b_loci.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    t.device_ms = ms_lap(t0) + pre_device_ms;
    t.kernel_ms = calls.kernel_ms;
    if (bgzf) {
        if (!d_locus_pos) {  // a host pileup: the formatter reads the positions in HBM
            SECEDO_TRY(b_pos.alloc((size_t)n_loci * 4));
            if (n_loci) SECEDO_TRY(hipMemcpyAsync(b_pos.p, locus_pos, (size_t)n_loci * 4, hipMemcpyHostToDevice, s));
            d_locus_pos = b_pos.as<uint32_t>();
        }
        SECEDO_CALL(secedo::vcf::write_outputs_bgzf(out_dir, reference_genome, num_clusters,
                                                    calls.d_records.as<secedo_variant_record>(), calls.total,
                                                    d_chr_locus_off, n_chr, d_locus_pos, b_ref.as<uint8_t>(), mismatch,
                                                    loci, s));
    } else {
        SECEDO_CALL(secedo::vcf::write_outputs(out_dir, reference_genome, num_clusters, calls.records, chr_locus_off,
                                               n_chr, locus_pos, locus_ref.data(), mismatch, loci));
    }
    t.write_ms = ms_lap(t0);
    if (times) *times = t;
    if (allele != SECEDO_ALLELE_NONE) {  // its own stage, timed by secedo_variant_allele_stats
        if (!d_locus_pos) {  // a host pileup under the plain output: the formatter reads the positions in HBM
            SECEDO_TRY(b_pos.alloc((size_t)n_loci * 4));
            if (n_loci) SECEDO_TRY(hipMemcpyAsync(b_pos.p, locus_pos, (size_t)n_loci * 4, hipMemcpyHostToDevice, s));
            d_locus_pos = b_pos.as<uint32_t>();
        }
        const secedo::allele::Pileup pileup{d_locus_entry_off, d_id_base16, d_id_base32, n};
        SECEDO_CALL(secedo::allele::write_outputs(out_dir, allele, bgzf, pileup,
                                                  calls.d_records.as<secedo_variant_record>(), calls.total,
                                                  b_ref.as<uint8_t>(), d_chr_locus_off, n_chr, d_locus_pos, s));
    }
    return SECEDO_OK;
}

// The steps before the reference's locus loop (:330-337): nothing for no cells; out_dir is created before the
// reference genome is checked. More than 24 chromosomes are refused before anything is made: the reference names the
// 23rd X and the 24th Y and asserts on a line for any later one (id_to_chromosome, util.cpp:162-170).
int begin_calling(uint32_t n, uint32_t n_chr, const char *reference_genome, const char *out_dir, bool *done,
                  OutDirGuard *out_guard) {
    *done = n == 0;
    if (*done) return SECEDO_OK;
    if (n_chr > 24)
        return fail(SECEDO_E_INVALID_ARG, "more than 24 chromosomes (" + std::to_string(n_chr) +
                                          "): the VCF lines name them 1..22, X, Y");
    int allele = SECEDO_ALLELE_NONE;  // an unknown SECEDO_ALLELE_COUNTS is refused before anything is made
    SECEDO_CALL(secedo::allele::selection_kind(&allele));
    if (!out_dir || !reference_genome) return fail(SECEDO_E_INVALID_ARG, "null path");
    std::error_code ec;
    out_guard->dir = out_dir;
    out_guard->created = std::filesystem::create_directories(out_dir, ec);
    if (ec) return fail(SECEDO_E_INVALID_ARG, std::string("cannot create ") + out_dir + ": " + ec.message());
    if (!std::filesystem::exists(reference_genome))
        return fail(SECEDO_E_INVALID_ARG, std::string("Reference genome ") + reference_genome + " does not exist");
    return SECEDO_OK;
}

}  // namespace

extern "C" {

const char *secedo_variant_last_error(void) { return g_error.c_str(); }

int secedo_variant_reference_genotypes(const char *fasta, const char *map_file, const uint32_t *chr_locus_off,
                                       uint32_t n_chr, const uint32_t *locus_pos, uint32_t n_loci,
                                       uint8_t *locus_ref, uint32_t *chr_locus_end, double *fasta_ms) {
    if (!chr_locus_off || (n_chr && !chr_locus_end) || (n_loci && (!locus_pos || !locus_ref)))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (chr_locus_off[0] != 0 || chr_locus_off[n_chr] != n_loci)
        return fail(SECEDO_E_INVALID_ARG, "chr_locus_off must run from 0 to n_loci");
    Source src;
    SECEDO_CALL(open_text(fasta, &src));
    return reference_genotypes(src, map_file, chr_locus_off, n_chr, locus_pos, locus_ref, chr_locus_end, fasta_ms);
}

int secedo_variant_set_fasta_route(int route) {
    if (route != SECEDO_FASTA_HOST && route != SECEDO_FASTA_DEVICE)
        return fail(SECEDO_E_INVALID_ARG, "route must be SECEDO_FASTA_HOST or SECEDO_FASTA_DEVICE");
    set_route(route);
    return SECEDO_OK;
}

int secedo_variant_get_fasta_route(void) { return get_route(); }

int secedo_variant_fasta_stats(secedo_variant_fasta_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = info();
    return SECEDO_OK;
}

int secedo_variant_reference_genotypes_device(int device_id, const char *fasta, const char *map_file,
                                              const uint32_t *d_chr_locus_off, const uint32_t *chr_locus_off,
                                              uint32_t n_chr, const uint32_t *d_locus_pos, uint32_t n_loci,
                                              uint8_t *d_locus_ref, uint32_t *chr_locus_end,
                                              secedo_variant_times *times, void *stream) {
    if (!chr_locus_off || !d_chr_locus_off || (n_chr && !chr_locus_end) || (n_loci && (!d_locus_pos || !d_locus_ref)))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (chr_locus_off[0] != 0 || chr_locus_off[n_chr] != n_loci)
        return fail(SECEDO_E_INVALID_ARG, "chr_locus_off must run from 0 to n_loci");
    SECEDO_CALL(set_device(device_id));
    secedo_variant_times t{};
    const RefArgs ref{d_chr_locus_off, chr_locus_off, n_chr, d_locus_pos, nullptr, n_loci, d_locus_ref, nullptr, chr_locus_end};
    SECEDO_CALL(reference_any(fasta, map_file, ref, &t.fasta_ms, &t.gather_ms, static_cast<hipStream_t>(stream)));
    if (times) *times = t;
    return SECEDO_OK;
}

int secedo_variant_is_diploid(const char *fasta) {
    Source src;
    SECEDO_CALL(open_text(fasta, &src));
    return first_word_has_maternal(src.text(), src.text_bytes()) ? 1 : 0;
}

int secedo_variant_read_chromosome(const char *fasta, const char *map_file, uint32_t index, uint8_t *out,
                                   uint64_t capacity, uint64_t *length) {
    Source src;
    SECEDO_CALL(open_text(fasta, &src));
    Fasta f(src.text(), src.text_bytes());
    std::vector<MapEntry> entries;
    SECEDO_CALL(read_map(map_file, &entries));
    const Map map = group_map(entries);
    const bool diploid = check_is_diploid(f);
    std::vector<uint8_t> chr, tmp1, tmp2;
    for (uint32_t c = 0; c <= index; ++c) SECEDO_CALL(get_next_chromosome(f, map, diploid, &chr, &tmp1, &tmp2));
    *length = chr.size();
    if (chr.size() > capacity) return fail(SECEDO_E_LIMIT, "contig longer than capacity");
    if (!chr.empty()) memcpy(out, chr.data(), chr.size());
    return SECEDO_OK;
}

int secedo_variant_read_map(const char *map_file, char *names, uint32_t name_len, uint32_t *start_pos,
                            uint32_t *len, char *tr, uint8_t *chromosome_id, uint32_t capacity,
                            uint32_t *n_entries) {
    std::vector<MapEntry> entries;
    SECEDO_CALL(read_map(map_file, &entries));
    *n_entries = static_cast<uint32_t>(entries.size());
    if (entries.size() > capacity) return fail(SECEDO_E_LIMIT, "more map entries than capacity");
    for (size_t i = 0; i < entries.size(); ++i) {
        if (name_len) {
            const size_t k = std::min<size_t>(entries[i].name.size(), name_len - 1);
            memcpy(names + i * name_len, entries[i].name.data(), k);
            names[i * name_len + k] = '\0';
        }
        start_pos[i] = entries[i].m.start_pos;
        len[i] = entries[i].m.len;
        tr[i] = entries[i].m.tr;
        chromosome_id[i] = entries[i].m.chromosome_id;
    }
    return SECEDO_OK;
}

int secedo_variant_apply_map(const uint32_t *start_pos, const uint32_t *len, const char *tr, uint32_t n_map,
                             const uint8_t *chr_data, uint64_t n, uint8_t *out, uint64_t capacity,
                             uint64_t *out_len) {
    std::vector<ChrMap> map(n_map);
    for (uint32_t i = 0; i < n_map; ++i) map[i] = ChrMap{start_pos[i], len[i], tr[i], 0};
    std::vector<uint8_t> in(chr_data, chr_data + n), res;
    SECEDO_CALL(apply_map(map, in, &res));
    *out_len = res.size();
    if (res.size() > capacity) return fail(SECEDO_E_LIMIT, "result longer than capacity");
    if (!res.empty()) memcpy(out, res.data(), res.size());
    return SECEDO_OK;
}

int secedo_variant_calls_device(int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                                const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                                const uint16_t *d_id_base16, const uint32_t *d_id_base32, uint32_t n_loci,
                                uint64_t n_entries, const uint16_t *d_clusters, uint32_t n_clusters_entries,
                                const uint8_t *d_locus_ref, const uint32_t *chr_locus_end, double hetero_prior,
                                double theta, secedo_variant_record *records, uint32_t capacity,
                                uint32_t *n_records, uint32_t *d_mismatch, uint32_t *d_loci, double *kernel_ms,
                                void *stream) {
    (void)d_locus_pos;
    (void)n_entries;
    SECEDO_CALL(set_device(device_id));
    if (!n_records || (!!d_id_base16 == !!d_id_base32) || (capacity && !records))
        return fail(SECEDO_E_INVALID_ARG, "invalid argument (exactly one of id_base16 / id_base32)");
    Calls calls;
    SECEDO_CALL(run_calls(d_chr_locus_off, n_chr, d_locus_entry_off, d_id_base16, d_id_base32, n_loci, d_clusters,
                      n_clusters_entries, d_locus_ref, chr_locus_end, hetero_prior, theta, capacity, d_mismatch,
                      d_loci, &calls, static_cast<hipStream_t>(stream)));
    *n_records = calls.total;
    if (kernel_ms) *kernel_ms = calls.kernel_ms;
    if (calls.total > capacity)
        return fail(SECEDO_E_LIMIT, std::to_string(calls.total) + " records, capacity " + std::to_string(capacity));
    if (calls.total) memcpy(records, calls.records.data(), calls.records.size() * sizeof(secedo_variant_record));
    return SECEDO_OK;
}

int secedo_variant_genotypes_device(int device_id, const uint16_t *counts, uint32_t n,
                                    int likely_homozygous_total, double hetero_prior, double theta,
                                    uint8_t *homozygous, uint8_t *genotype) {
    SECEDO_CALL(set_device(device_id));
    if (n == 0) return SECEDO_OK;
    const std::vector<double> thr = threshold_table(theta);
    Buf b_c, b_t, b_h, b_g;
    SECEDO_TRY(b_c.alloc((size_t)n * 8));
    SECEDO_TRY(b_t.alloc(thr.size() * sizeof(double)));
    SECEDO_TRY(b_h.alloc(n));
    SECEDO_TRY(b_g.alloc(n));
    SECEDO_TRY(hipMemcpy(b_c.p, counts, (size_t)n * 8, hipMemcpyHostToDevice));
    SECEDO_TRY(hipMemcpy(b_t.p, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice));
    SECEDO_TRY(secedo::variant::genotypes(b_c.as<uint16_t>(), n, likely_homozygous_total, b_t.as<double>(),
                                      host_logs(hetero_prior, theta), b_h.as<uint8_t>(), b_g.as<uint8_t>(), 0));
    SECEDO_TRY(hipMemcpy(homozygous, b_h.p, n, hipMemcpyDeviceToHost));
    SECEDO_TRY(hipMemcpy(genotype, b_g.p, n, hipMemcpyDeviceToHost));
    return SECEDO_OK;
}

int secedo_variant_set_vcf_output(int output) {
    if (output != SECEDO_VCF_PLAIN && output != SECEDO_VCF_BGZF)
        return fail(SECEDO_E_INVALID_ARG, "output must be SECEDO_VCF_PLAIN or SECEDO_VCF_BGZF");
    secedo::vcf::set_output(output);
    return SECEDO_OK;
}

int secedo_variant_get_vcf_output(void) { return secedo::vcf::get_output(); }

int secedo_variant_vcf_stats(secedo_variant_vcf_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = secedo::vcf::info();
    return SECEDO_OK;
}

}  // extern "C"

namespace {

std::vector<std::string> preamble_strings(const char *preamble, const uint64_t *preamble_off, uint32_t num_clusters) {
    std::vector<std::string> pre(num_clusters);
    if (preamble && preamble_off)
        for (uint32_t i = 0; i < num_clusters; ++i) pre[i].assign(preamble + preamble_off[i], preamble_off[i + 1] - preamble_off[i]);
    return pre;
}

int check_format_args(const secedo_variant_record *records, uint32_t n_records, const uint32_t *chr_locus_off,
                      uint32_t n_chr, const uint32_t *locus_pos, const uint8_t *locus_ref, uint32_t n_loci,
                      uint32_t num_clusters, const uint64_t *file_off) {
    if (!chr_locus_off || !file_off || (n_records && !records) || (n_loci && (!locus_pos || !locus_ref)))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    (void)n_chr;
    for (uint32_t k = 0; k < n_records; ++k) {
        if (records[k].locus >= n_loci) return fail(SECEDO_E_INVALID_ARG, "a record's locus is >= n_loci");
        if (records[k].kind == SECEDO_VARIANT_CLUSTER && records[k].cluster >= num_clusters)
            return fail(SECEDO_E_INVALID_ARG, "a record's cluster is >= num_clusters");
        if (k && records[k].locus < records[k - 1].locus)
            return fail(SECEDO_E_INVALID_ARG, "records must ascend in locus");
    }
    return SECEDO_OK;
}

}  // namespace

extern "C" {

int secedo_variant_format_host(const secedo_variant_record *records, uint32_t n_records,
                               const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                               const uint8_t *locus_ref, uint32_t n_loci, uint32_t num_clusters, const char *preamble,
                               const uint64_t *preamble_off, char *text, uint64_t capacity, uint64_t *file_off) {
    SECEDO_CALL(check_format_args(records, n_records, chr_locus_off, n_chr, locus_pos, locus_ref, n_loci, num_clusters,
                                  file_off));
    std::vector<std::string> vcfs;
    std::string common;
    secedo::vcf::build_texts(preamble_strings(preamble, preamble_off, num_clusters), records, n_records, chr_locus_off,
                             n_chr, locus_pos, locus_ref, &vcfs, &common);
    vcfs.push_back(std::move(common));
    uint64_t at = 0;
    for (uint32_t f = 0; f <= num_clusters; ++f) {
        file_off[f] = at;
        if (text && at + vcfs[f].size() <= capacity) memcpy(text + at, vcfs[f].data(), vcfs[f].size());
        at += vcfs[f].size();
    }
    file_off[num_clusters + 1] = at;
    if (at > capacity) return fail(SECEDO_E_LIMIT, std::to_string(at) + " bytes of text, capacity " + std::to_string(capacity));
    return SECEDO_OK;
}

int secedo_variant_format_device(int device_id, const secedo_variant_record *records, uint32_t n_records,
                                 const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                                 const uint8_t *locus_ref, uint32_t n_loci, uint32_t num_clusters,
                                 const char *preamble, const uint64_t *preamble_off, char *text, uint64_t capacity,
                                 uint64_t *file_off) {
    SECEDO_CALL(check_format_args(records, n_records, chr_locus_off, n_chr, locus_pos, locus_ref, n_loci, num_clusters,
                                  file_off));
    SECEDO_CALL(set_device(device_id));
    Buf b_rec, b_chr, b_pos, b_ref;
    SECEDO_TRY(b_rec.alloc((size_t)n_records * sizeof(secedo_variant_record)));
    SECEDO_TRY(b_chr.alloc(((size_t)n_chr + 1) * 4));
    SECEDO_TRY(b_pos.alloc((size_t)n_loci * 4));
    SECEDO_TRY(b_ref.alloc(n_loci));
    if (n_records) SECEDO_TRY(hipMemcpy(b_rec.p, records, (size_t)n_records * sizeof(secedo_variant_record), hipMemcpyHostToDevice));
    SECEDO_TRY(hipMemcpy(b_chr.p, chr_locus_off, ((size_t)n_chr + 1) * 4, hipMemcpyHostToDevice));
    if (n_loci) SECEDO_TRY(hipMemcpy(b_pos.p, locus_pos, (size_t)n_loci * 4, hipMemcpyHostToDevice));
    if (n_loci) SECEDO_TRY(hipMemcpy(b_ref.p, locus_ref, n_loci, hipMemcpyHostToDevice));
    secedo::vcf::DeviceText dt;
    SECEDO_CALL(secedo::vcf::format_device(preamble_strings(preamble, preamble_off, num_clusters),
                                           b_rec.as<secedo_variant_record>(), n_records, b_chr.as<uint32_t>(), n_chr,
                                           b_pos.as<uint32_t>(), b_ref.as<uint8_t>(), &dt, nullptr));
    for (uint32_t f = 0; f <= num_clusters + 1; ++f) file_off[f] = dt.file_off[f];
    const uint64_t total = dt.file_off.back();
    if (total > capacity) return fail(SECEDO_E_LIMIT, std::to_string(total) + " bytes of text, capacity " + std::to_string(capacity));
    if (total) SECEDO_TRY(hipMemcpy(text, dt.text(), total, hipMemcpyDeviceToHost));
    return SECEDO_OK;
}

int secedo_variant_bgzf_deflate(int device_id, const uint8_t *data, const uint64_t *data_off, uint32_t n_files,
                                uint8_t *out, uint64_t capacity, uint64_t *out_off, void *stream) {
    if (!data_off || !out_off || (data_off[n_files] && !data)) return fail(SECEDO_E_INVALID_ARG, "null argument");
    for (uint32_t f = 0; f < n_files; ++f)
        if (data_off[f] > data_off[f + 1]) return fail(SECEDO_E_INVALID_ARG, "data_off must not decrease");
    SECEDO_CALL(set_device(device_id));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t b = data_off[0], total = data_off[n_files] - b;
    Buf b_text;
    SECEDO_TRY(b_text.alloc(total + 2 * secedo::bgzf::kDeflateInSlack));
    uint8_t *d_text = b_text.as<uint8_t>() + secedo::bgzf::kDeflateInSlack;
    if (total) SECEDO_TRY(hipMemcpyAsync(d_text, data + b, total, hipMemcpyHostToDevice, s));
    std::vector<uint64_t> file_off(data_off, data_off + n_files + 1);
    for (uint64_t &v : file_off) v -= b;
    secedo::vcf::info() = secedo_variant_vcf_info{};
    secedo::vcf::info().output = SECEDO_VCF_BGZF;
    secedo::vcf::info().files = n_files;
    secedo::vcf::info().text_bytes = total;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    SECEDO_CALL(secedo::vcf::deflate_device(d_text, file_off, &bytes, &off, s));
    for (uint32_t f = 0; f <= n_files; ++f) out_off[f] = off[f];
    if (bytes.size() > capacity)
        return fail(SECEDO_E_LIMIT, std::to_string(bytes.size()) + " bytes of output, capacity " + std::to_string(capacity));
    if (!bytes.empty()) memcpy(out, bytes.data(), bytes.size());
    return SECEDO_OK;
}

static int calling_host(OutDirGuard *out_guard, int device_id, const uint32_t *chr_locus_off, uint32_t n_chr,
                        const uint32_t *locus_pos, const uint64_t *locus_entry_off, const uint16_t *id_base16,
                        const uint32_t *id_base32, const uint16_t *clusters, uint32_t n,
                        const char *reference_genome, const char *map_file, double hetero_prior, double theta,
                        const char *out_dir, secedo_variant_times *times) {
    bool done;
    SECEDO_CALL(begin_calling(n, n_chr, reference_genome, out_dir, &done, out_guard));
    if (done) return SECEDO_OK;
    if (!chr_locus_off || !clusters || (!!id_base16 == !!id_base32 && chr_locus_off[n_chr] > 0))
        return fail(SECEDO_E_INVALID_ARG, "invalid argument (exactly one of id_base16 / id_base32)");
    SECEDO_CALL(set_device(device_id));
    Clock::time_point t0 = Clock::now();
    const uint32_t n_loci = chr_locus_off[n_chr];
    const uint64_t n_entries = locus_entry_off[n_loci];
    const size_t idb_bytes = (size_t)n_entries * (id_base16 ? 2 : 4);
    StreamGuard guard;
    SECEDO_TRY(hipStreamCreateWithFlags(&guard.s, hipStreamNonBlocking));
    const hipStream_t s = guard.s;
    Buf b_chr, b_off, b_idb;
    SECEDO_TRY(b_chr.alloc(((size_t)n_chr + 1) * 4));
    SECEDO_TRY(b_off.alloc(((size_t)n_loci + 1) * 8));
    SECEDO_TRY(b_idb.alloc(idb_bytes));
    SECEDO_TRY(hipMemcpyAsync(b_chr.p, chr_locus_off, ((size_t)n_chr + 1) * 4, hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(b_off.p, locus_entry_off, ((size_t)n_loci + 1) * 8, hipMemcpyHostToDevice, s));
    if (idb_bytes)
        SECEDO_TRY(hipMemcpyAsync(b_idb.p, id_base16 ? (const void *)id_base16 : (const void *)id_base32, idb_bytes,
                              hipMemcpyHostToDevice, s));
    const double upload_ms = ms_lap(t0);
    return calling(device_id, b_chr.as<uint32_t>(), chr_locus_off, n_chr, locus_pos, nullptr, b_off.as<uint64_t>(),
                   id_base16 ? b_idb.as<uint16_t>() : nullptr, id_base16 ? nullptr : b_idb.as<uint32_t>(), n_loci,
                   clusters, n, reference_genome, map_file, hetero_prior, theta, out_dir, times, s, upload_ms, out_guard);
}

int secedo_variant_calling(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr,
                           const uint32_t *locus_pos, const uint64_t *locus_entry_off, const uint16_t *id_base16,
                           const uint32_t *id_base32, const uint16_t *clusters, uint32_t n,
                           const char *reference_genome, const char *map_file, double hetero_prior, double theta,
                           const char *out_dir, secedo_variant_times *times) {
    OutDirGuard out_guard;
    return out_guard.done(calling_host(&out_guard, device_id, chr_locus_off, n_chr, locus_pos, locus_entry_off,
                                       id_base16, id_base32, clusters, n, reference_genome, map_file, hetero_prior,
                                       theta, out_dir, times));
}

static int calling_resident(OutDirGuard *out_guard, int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                            const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                            const uint16_t *d_id_base16, const uint32_t *d_id_base32, uint32_t n_loci,
                            const uint16_t *clusters, uint32_t n, const char *reference_genome, const char *map_file,
                            double hetero_prior, double theta, const char *out_dir, secedo_variant_times *times,
                            void *stream) {
    bool done;
    SECEDO_CALL(begin_calling(n, n_chr, reference_genome, out_dir, &done, out_guard));
    if (done) return SECEDO_OK;
    if (!clusters || (!!d_id_base16 == !!d_id_base32 && n_loci > 0))
        return fail(SECEDO_E_INVALID_ARG, "invalid argument (exactly one of id_base16 / id_base32)");
    SECEDO_CALL(set_device(device_id));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Clock::time_point t0 = Clock::now();
    std::vector<uint32_t> chr_off((size_t)n_chr + 1), pos(n_loci);
    SECEDO_TRY(hipMemcpyAsync(chr_off.data(), d_chr_locus_off, ((size_t)n_chr + 1) * 4, hipMemcpyDeviceToHost, s));
    if (n_loci) SECEDO_TRY(hipMemcpyAsync(pos.data(), d_locus_pos, (size_t)n_loci * 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (chr_off[0] != 0 || chr_off[n_chr] != n_loci)
        return fail(SECEDO_E_INVALID_ARG, "chr_locus_off must run from 0 to n_loci");
    const double download_ms = ms_lap(t0);
    return calling(device_id, d_chr_locus_off, chr_off.data(), n_chr, pos.data(), d_locus_pos, d_locus_entry_off, d_id_base16,
                   d_id_base32, n_loci, clusters, n, reference_genome, map_file, hetero_prior, theta, out_dir, times,
                   s, download_ms, out_guard);
}

int secedo_variant_calling_device(int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                                  const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                                  const uint16_t *d_id_base16, const uint32_t *d_id_base32, uint32_t n_loci,
                                  uint64_t n_entries, const uint16_t *clusters, uint32_t n,
                                  const char *reference_genome, const char *map_file, double hetero_prior,
                                  double theta, const char *out_dir, secedo_variant_times *times, void *stream) {
    (void)n_entries;
    OutDirGuard out_guard;
    return out_guard.done(calling_resident(&out_guard, device_id, d_chr_locus_off, n_chr, d_locus_pos,
                                           d_locus_entry_off, d_id_base16, d_id_base32, n_loci, clusters, n,
                                           reference_genome, map_file, hetero_prior, theta, out_dir, times, stream));
}

}  // extern "C"
