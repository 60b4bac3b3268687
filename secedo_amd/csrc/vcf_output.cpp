// vcf_output.cpp -- see vcf_output.hpp. The text functions are the reference's write_vcf_preamble, write_vcf_line and
// get_differing_bases restated on the host; put_record and its helpers in variant_kernels.hip restate them once more
// for the device, and tests/test_gpu_vcf_output.py holds the two against each other.
#include "vcf_output.hpp"

#include "bgzf_encoder.hpp"
#include "host_util.hpp"
#include "tabix_host.hpp"
#include "tabix_kernels.hpp"
#include "variant_kernels.hpp"

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

namespace secedo {
namespace vcf {

using namespace secedo::host;

namespace {

std::atomic<int> g_output{-1};
thread_local secedo_variant_vcf_info g_info;

constexpr char kIntToChar[6] = {'A', 'C', 'G', 'T', 'N', 'N'};

std::string id_to_chromosome(uint32_t chr_id) {
    if (chr_id < 22) return std::to_string(chr_id + 1);
    return chr_id == 22 ? "X" : "Y";
}

const char *const kInfoFormat = "\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t";

bool is_homozygous(uint32_t g) { return (g & 7) == (g >> 3); }

void append_counts(std::string &o, const uint16_t c[4]) {
    for (int j = 0; j < 4; ++j) {
        o += std::to_string(c[j]);
        o += ' ';
    }
    o += '\n';
}

void append_head(std::string &o, const std::string &chr, uint32_t pos, char ref, const std::string &alt) {
    o += chr;
    o += '\t';
    o += std::to_string(pos);
    o += "\t.\t";
    o += ref;
    o += '\t';
    o += alt;
    o += kInfoFormat;
}

// write_vcf_line (:288-321) for a record the device already found to be written; get_differing_bases (:247-279)
void append_vcf_line(std::string &o, const std::string &chr, uint32_t pos, uint32_t ref, uint32_t g,
                     const uint16_t c[4]) {
    if (is_homozygous(ref)) {
        std::string alt(1, kIntToChar[g & 7]);
        const char *gt = "1/1";
        if (!is_homozygous(g)) {
            alt += kIntToChar[g >> 3];
            gt = "0/1";
        }
        append_head(o, chr, pos, kIntToChar[ref & 7], alt);
        o += gt;
        o += '\t';
        append_counts(o, c);
        return;
    }
    char r1 = kIntToChar[ref & 7], r2 = kIntToChar[ref >> 3];
    if (r1 > r2) std::swap(r1, r2);
    char g1 = kIntToChar[g & 7], g2 = kIntToChar[g >> 3];
    if (g1 > g2) std::swap(g1, g2);
    std::pair<char, char> pairs[2];
    int n = 0;
    if (g1 == r1 && g2 == r2) n = 0;
    else if (g1 == r1) pairs[n++] = {r2, g2};
    else if (g2 == r2) pairs[n++] = {r1, g1};
    else {
        pairs[n++] = {r1, g1};
        pairs[n++] = {r2, g2};
    }
    for (int k = 0; k < n; ++k) {
        append_head(o, chr, pos, pairs[k].first, std::string(1, pairs[k].second));
        o += "1/1\t";
        append_counts(o, c);
    }
}

int write_bytes(const std::filesystem::path &path, const void *data, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return fail(SECEDO_E_INVALID_ARG, "cannot write " + path.string());
    const size_t w = n == 0 ? 0 : fwrite(data, 1, n, f);
    const bool closed = fclose(f) == 0;
    const bool ok = w == n && closed;
    return ok ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, "cannot write " + path.string());
}

int write_file(const std::filesystem::path &path, const std::string &text) {
    return write_bytes(path, text.data(), text.size());
}

// write_vcf_preamble (:226-241)
std::string preamble(const std::string &reference, uint32_t cluster) {
    std::time_t now = std::chrono::system_clock::to_time_t(std::chrono::system_clock::now());
    std::string o = "##fileformat=VCFv4.2\n##fileDate=";
    o += std::ctime(&now);
    o += "##source=SVC (Somatic Variant Caller)\n##reference=" + reference + "\n##cluster=" +
         std::to_string(cluster) + "\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tcluster-" +
         std::to_string(cluster) + "\n";
    return o;
}

// `variant` and `scores`, the same on both routes
int write_variant_and_scores(const std::filesystem::path &out_dir, const std::vector<uint32_t> &mismatch,
                             const std::vector<uint32_t> &loci) {
    SECEDO_CALL(write_file(out_dir / "variant", ""));
    // write_vec(scores): default ostream formatting (%g, 6 digits); 0.0 / 0 prints as -nan on x86-64
    std::string scores;
    char buf[64];
    for (size_t i = 0; i < loci.size(); ++i) {
        if (i) scores += ',';
        if (loci[i] == 0) {
            scores += "-nan";
        } else {
            snprintf(buf, sizeof buf, "%g", static_cast<double>(mismatch[i]) / loci[i]);
            scores += buf;
        }
    }
    scores += '\n';
    return write_file(out_dir / "scores", scores);
}

}  // namespace

void set_output(int kind) { g_output.store(kind); }

int get_output() {
    const int kind = g_output.load();
    if (kind >= 0) return kind;
    const char *e = std::getenv("SECEDO_VCF");
    if (!e || !*e || std::strcmp(e, "plain") == 0) return SECEDO_VCF_PLAIN;
    if (std::strcmp(e, "bgzf") == 0) return SECEDO_VCF_BGZF;
    return fail(SECEDO_E_INVALID_ARG, std::string("SECEDO_VCF=") + e + ": expected plain or bgzf");
}

int output_kind(int *kind) {
    const int k = get_output();
    if (k < 0) return k;
    *kind = k;
    return SECEDO_OK;
}

secedo_variant_vcf_info &info() { return g_info; }

std::vector<std::string> preambles(const std::string &reference, uint32_t num_clusters) {
    std::vector<std::string> out(num_clusters);
    for (uint32_t i = 0; i < num_clusters; ++i) out[i] = preamble(reference, i);
    return out;
}

void build_texts(const std::vector<std::string> &pre, const secedo_variant_record *records, size_t n_records,
                 const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos, const uint8_t *locus_ref,
                 std::vector<std::string> *out, std::string *common_out) {
    std::vector<std::string> &vcfs = *out;
    std::string &common = *common_out;
    vcfs = pre;
    common.clear();
    uint32_t chr = 0;
    std::string chr_name = id_to_chromosome(0);
    for (size_t k = 0; k < n_records; ++k) {
        const secedo_variant_record &r = records[k];
        while (chr + 1 < n_chr && r.locus >= chr_locus_off[chr + 1]) chr_name = id_to_chromosome(++chr);
        const uint32_t pos = locus_pos[r.locus], ref = locus_ref[r.locus];
        if (r.kind == SECEDO_VARIANT_POOLED) {  // :395-406
            const uint32_t new_base = r.genotype & 7;
            const uint32_t ref_base = (ref & 7) == new_base ? (ref >> 3) & 7 : ref & 7;
            append_head(common, chr_name, pos, kIntToChar[ref_base], std::string(1, kIntToChar[new_base]));
            common += "1/1\t";
            append_counts(common, r.counts);
        } else if (r.kind == SECEDO_VARIANT_COMMON) {
            append_vcf_line(common, chr_name, pos, ref, r.genotype, r.counts);
        } else {
            append_vcf_line(vcfs[r.cluster], chr_name, pos, ref, r.genotype, r.counts);
        }
    }
}

int write_outputs(const std::filesystem::path &out_dir, const std::string &reference, uint32_t num_clusters,
                  const std::vector<secedo_variant_record> &records, const uint32_t *chr_locus_off, uint32_t n_chr,
                  const uint32_t *locus_pos, const uint8_t *locus_ref, const std::vector<uint32_t> &mismatch,
                  const std::vector<uint32_t> &loci) {
    g_info = secedo_variant_vcf_info{};
    g_info.output = SECEDO_VCF_PLAIN;
    Clock::time_point t0 = Clock::now();
    std::vector<std::string> vcfs;
    std::string common;
    build_texts(preambles(reference, num_clusters), records.data(), records.size(), chr_locus_off, n_chr, locus_pos,
                locus_ref, &vcfs, &common);
    g_info.files = uint64_t(num_clusters) + 1;
    g_info.text_bytes = common.size();
    for (const std::string &v : vcfs) g_info.text_bytes += v.size();
    for (uint32_t i = 0; i < num_clusters; ++i)
        SECEDO_CALL(write_file(out_dir / ("cluster_" + std::to_string(i) + ".vcf"), vcfs[i]));
    SECEDO_CALL(write_file(out_dir / "common.vcf", common));
    SECEDO_CALL(write_variant_and_scores(out_dir, mismatch, loci));
    g_info.write_ms = ms_since(t0);
    return SECEDO_OK;
}

DeviceText::~DeviceText() {
    if (alloc) (void)hipFree(alloc);
}
const uint8_t *DeviceText::text() const { return alloc + bgzf::kDeflateInSlack; }

int format_device(const std::vector<std::string> &pre, const secedo_variant_record *d_records, uint32_t n_records,
                  const uint32_t *d_chr_locus_off, uint32_t n_chr, const uint32_t *d_locus_pos,
                  const uint8_t *d_locus_ref, DeviceText *out, hipStream_t s) {
    namespace V = secedo::variant;
    const uint32_t num_clusters = static_cast<uint32_t>(pre.size()), n_files = num_clusters + 1;
    std::string all;
    std::vector<uint64_t> pre_off(size_t(n_files) + 1);
    for (uint32_t f = 0; f < num_clusters; ++f) {
        pre_off[f] = all.size();
        all += pre[f];
    }
    pre_off[num_clusters] = pre_off[n_files] = all.size();  // common has no preamble
    Buf b_pre, b_pre_off, b_work, b_file_off;
    SECEDO_TRY(b_pre.alloc(all.size()));
    SECEDO_TRY(b_pre_off.alloc(pre_off.size() * 8));
    SECEDO_TRY(b_file_off.alloc(pre_off.size() * 8));
    const size_t work_bytes = V::format_workspace(n_records);
    SECEDO_TRY(b_work.alloc(work_bytes));
    if (!all.empty()) SECEDO_TRY(hipMemcpyAsync(b_pre.p, all.data(), all.size(), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(b_pre_off.p, pre_off.data(), pre_off.size() * 8, hipMemcpyHostToDevice, s));
    const V::FormatIn in{d_records,   n_records,    d_chr_locus_off,        n_chr,
                         d_locus_pos, d_locus_ref,  num_clusters,           b_pre.as<uint8_t>(),
                         b_pre_off.as<uint64_t>()};
    SECEDO_TRY(V::format_measure(in, b_work.p, work_bytes, b_file_off.as<uint64_t>(), s));
    out->file_off.assign(pre_off.size(), 0);
    SECEDO_TRY(hipMemcpyAsync(out->file_off.data(), b_file_off.p, pre_off.size() * 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));  // the uploads' sources and the offsets are the host's again
    const uint64_t total = out->file_off[n_files];
    if (out->alloc) (void)hipFree(out->alloc);
    out->alloc = nullptr;
    SECEDO_TRY(hipMalloc(&out->alloc, total + 2 * bgzf::kDeflateInSlack));
    SECEDO_TRY(V::format_write(in, b_work.p, work_bytes, b_file_off.as<uint64_t>(), out->alloc + bgzf::kDeflateInSlack, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    return SECEDO_OK;
}

int deflate_device(const uint8_t *d_text, const std::vector<uint64_t> &file_off, std::vector<uint8_t> *out,
                   std::vector<uint64_t> *out_off, hipStream_t s, MemberTable *table, bgzf::EncoderCounts *counts) {
    using namespace secedo::bgzf;
    const size_t n_files = file_off.size() - 1;
    std::vector<DeflateDesc> desc;  // every member of every file, in file order
    for (size_t f = 0; f < n_files; ++f) member_cuts(file_off[f], file_off[f + 1], &desc);
    out->clear();
    out_off->assign(n_files + 1, 0);
    if (table) *table = MemberTable{{}, std::vector<size_t>(n_files + 1, 0)};
    uint64_t end = 0;  // bytes of output laid out so far
    size_t file = 0;   // the file the next member belongs to
    std::vector<uint64_t> eof_at;
    // with the text before `pos` laid out, the files that end there: room for their EOF member, the next file's start
    const auto close_files = [&](uint64_t pos) {
        while (file < n_files && pos == file_off[file + 1]) {
            if (table) {
                table->m.push_back(bamindexbuild::Member{end - (*out_off)[file], file_off[file + 1] - file_off[file], 0});
                table->first[file + 1] = table->m.size();
            }
            eof_at.push_back(end);
            end += kEofBytes;
            (*out_off)[++file] = end;
        }
    };
    close_files(file_off[0]);
    Encoder enc(16384, true);  // 1 GiB of slots; the kernel's time is a field of the statistics
    SECEDO_CALL(enc.run(d_text, desc, s, [&](size_t b0, uint32_t n, const uint32_t *bytes, uint64_t *at) {
        // where each member goes: behind the one before, EOF members in between
        const uint64_t first = end;
        for (uint32_t k = 0; k < n; ++k) {
            const DeflateDesc &d = desc[b0 + k];
            if (table) table->m.push_back(bamindexbuild::Member{end - (*out_off)[file], d.in_off - file_off[file], d.n});
            at[k] = end - first;
            end += bytes[k];
            close_files(d.in_off + d.n);
        }
        out->resize(end);
        return enc.fetch(end - first, out, first);
    }));
    // the EOF members, over what came down in their place; files without text had no slice to make their room
    Clock::time_point t0 = Clock::now();
    out->resize(end);
    const auto eof = eof_member();
    for (const uint64_t e : eof_at) std::copy(eof.begin(), eof.end(), out->begin() + e);
    enc.counts.download_ms += ms_since(t0);
    if (counts) { *counts = enc.counts; return SECEDO_OK; }
    g_info.blocks += enc.counts.members;
    g_info.stored_blocks += enc.counts.stored_members;
    g_info.deflate_kernel_ms += enc.counts.kernel_ms;
    g_info.deflate_ms += enc.counts.deflate_ms;
    g_info.download_ms += enc.counts.download_ms;
    g_info.compressed_bytes += end;
    return SECEDO_OK;
}

int write_outputs_bgzf(const std::filesystem::path &out_dir, const std::string &reference, uint32_t num_clusters,
                       const secedo_variant_record *d_records, uint32_t n_records, const uint32_t *d_chr_locus_off,
                       uint32_t n_chr, const uint32_t *d_locus_pos, const uint8_t *d_locus_ref,
                       const std::vector<uint32_t> &mismatch, const std::vector<uint32_t> &loci, hipStream_t s) {
    g_info = secedo_variant_vcf_info{};
    g_info.output = SECEDO_VCF_BGZF;
    Clock::time_point t0 = Clock::now();
    DeviceText text;
    SECEDO_CALL(format_device(preambles(reference, num_clusters), d_records, n_records, d_chr_locus_off, n_chr,
                              d_locus_pos, d_locus_ref, &text, s));
    g_info.files = uint64_t(num_clusters) + 1;
    g_info.text_bytes = text.file_off.back();
    g_info.format_ms = ms_lap(t0);
    int index = SECEDO_VCF_INDEX_NONE;
    SECEDO_CALL(tabix_host::index_kind(&index));
    const bool tbi = index == SECEDO_VCF_INDEX_TBI;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    MemberTable table;
    SECEDO_CALL(deflate_device(text.text(), text.file_off, &bytes, &off, s, tbi ? &table : nullptr));
    (void)ms_lap(t0);
    std::vector<std::string> names(size_t(num_clusters) + 1);
    for (uint32_t i = 0; i <= num_clusters; ++i) {
        names[i] = i < num_clusters ? "cluster_" + std::to_string(i) + ".vcf.gz" : "common.vcf.gz";
        SECEDO_CALL(write_bytes(out_dir / names[i], bytes.data() + off[i], off[i + 1] - off[i]));
    }
    SECEDO_CALL(write_variant_and_scores(out_dir, mismatch, loci));
    g_info.write_ms = ms_lap(t0);
    if (!tbi) return SECEDO_OK;
    // the indexes: the line pass over the text where the formatter left it, the members as the encoder laid them out
    static_assert(tabix::kTextSlack <= bgzf::kDeflateInSlack, "the line pass reads within the encoder's slack");
    std::vector<tabix_host::IndexedFile> files(names.size());
    std::vector<std::string> paths(names.size());
    for (size_t i = 0; i < names.size(); ++i) {
        files[i].label = (out_dir / names[i]).string();
        files[i].members.assign(table.m.begin() + table.first[i], table.m.begin() + table.first[i + 1]);
        files[i].file_bytes = off[i + 1] - off[i];
        paths[i] = files[i].label + ".tbi";
    }
    std::vector<std::vector<uint8_t>> raw;
    size_t n_good = 0;
    SECEDO_CALL(tabix_host::build_raw(text.text(), text.file_off, files, &raw, &n_good, s));
    return tabix_host::compress_and_write(raw, n_good, paths, s);
}

}  // namespace vcf
}  // namespace secedo
