// tabix_api.cpp -- see tabix_host.hpp. The line pass of tabix_kernels.hip driven range by range, its heads, windows and
// name changes fed to one tabix_build.hpp builder per file; the index bodies through the BGZF encoder; and the
// stand-alone route, which uploads the compressed bytes of files that exist and inflates them in HBM first.
#include "tabix_host.hpp"

#include "bgzf_encoder.hpp"  // kDeflateInSlack, EncoderCounts
#include "bgzf_kernels.hpp"
#include "bgzf_members.hpp"  // the member list of a file that is read, its descriptors and its error words
#include "host_util.hpp"
#include "tabix_build.hpp"
#include "tabix_kernels.hpp"
#include "vcf_output.hpp"

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace secedo {
namespace tabix_host {

using namespace secedo::host;
namespace T = secedo::tabix;
namespace bm = secedo::bgzf_members;

namespace {

std::atomic<int> g_index{-1};
thread_local secedo_variant_tabix_info g_info;

// text bytes per range of the line pass (tabix_kernels.hpp)
uint64_t budget_bytes() {
    return std::min(std::max(env_u64("SECEDO_TABIX_BATCH_BYTES", T::kDefaultBudget), T::kMinBudget), T::kMaxRange);
}

// windows a range may emit (tabix_kernels.hpp)
uint64_t max_range_windows() {
    return std::min(env_u64("SECEDO_TABIX_MAX_WINDOWS", T::kMaxRangeWindows), T::kMaxRangeWindows);
}

// the file that holds text byte x: the last one that begins at or before it
uint32_t file_of(const std::vector<uint64_t> &file_off, uint64_t x) {
    return uint32_t(std::upper_bound(file_off.begin(), file_off.end(), x) - file_off.begin() - 1);
}

const char *what_of(uint32_t code) {
    switch (code) {
        case T::kErrColumns: return "fewer than two columns";
        case T::kErrPos: return "POS is not a decimal number";
        case T::kErrEnd: return "the line ends past 2^29: a .tbi index cannot hold it";
        default: return "POS is lower than that of the data line before it: the file is not sorted";
    }
}

int write_renamed(const std::string &path, const uint8_t *bytes, size_t n) {
    const std::string tmp = path + ".tmp." + std::to_string((long long)getpid());
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) return fail(SECEDO_E_INVALID_ARG, "cannot write " + path);
    const bool ok = (n == 0 || std::fwrite(bytes, 1, n, f) == n);
    if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), path.c_str()) != 0) {
        std::remove(tmp.c_str());
        return fail(SECEDO_E_INVALID_ARG, "cannot write " + path);
    }
    return SECEDO_OK;
}

// Where the range that begins at line start `a` ends: a + budget cut back to the last line start (a file's first byte,
// or the byte behind a '\n'); stretched while there is none.
int cut_range(const uint8_t *d_text, const std::vector<uint64_t> &file_off, uint64_t a, uint64_t budget, Buf &b_end,
              uint64_t *end, hipStream_t s) {
    const uint64_t total = file_off.back();
    for (uint64_t want = budget;; want = std::min(want * 2, T::kMaxRange)) {
        const uint64_t b = std::min(total, a + want);
        if (b == total) {
            if (b - a > T::kMaxRange) break;
            *end = b;
            return SECEDO_OK;
        }
        const uint64_t at_file = *(std::upper_bound(file_off.begin(), file_off.end(), b) - 1);  // file_off[0] = 0 <= b
        // the search starts on a 16-byte boundary at or before a: a '\n' it finds in front of a gives a cut <= a
        const uint64_t pad = (reinterpret_cast<uintptr_t>(d_text) + a) & 15;
        unsigned long long nl = 0;
        SECEDO_TRY(secedo::bam::bgzf_last_newline(d_text + a - pad, b - a + pad, b_end.as<unsigned long long>(), s));
        SECEDO_TRY(hipMemcpyAsync(&nl, b_end.p, 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        const uint64_t cut = std::max<uint64_t>(at_file, nl ? a - pad + nl : 0);
        if (cut > a) {
            *end = cut;
            return SECEDO_OK;
        }
        if (want >= T::kMaxRange) break;
    }
    return fail(SECEDO_E_LIMIT, "a line of more than 2^30 bytes");
}

// One device allocation carved into 256-byte aligned pieces. It only grows, so a call that walks many ranges allocates
// for the largest and releases once.
struct Arena {
    Buf buf;
    std::vector<size_t> at;
    hipError_t reserve(std::initializer_list<size_t> bytes, hipStream_t s) {
        at.clear();
        size_t total = 0;
        for (const size_t b : bytes) {
            at.push_back(total);
            total += (b + 255) / 256 * 256;
        }
        return buf.grow(total, 0, s);
    }
    template <class U>
    U *piece(size_t k) const {
        return reinterpret_cast<U *>(buf.p + at[k]);
    }
};

struct Found {  // the lowest error of a range
    bool any = false;
    uint32_t file = 0;
    uint64_t line = 0;  // 1-based, in the file
    std::string what;
    void take(uint32_t f, uint64_t l, const std::string &w) {
        if (any && (file < f || (file == f && line <= l))) return;
        any = true, file = f, line = l, what = w;
    }
};

}  // namespace

void set_index(int kind) { g_index.store(kind); }

int get_index() {
    const int kind = g_index.load();
    if (kind >= 0) return kind;
    const char *e = std::getenv("SECEDO_VCF_INDEX");
    if (!e || !*e || std::strcmp(e, "none") == 0) return SECEDO_VCF_INDEX_NONE;
    if (std::strcmp(e, "tbi") == 0) return SECEDO_VCF_INDEX_TBI;
    return fail(SECEDO_E_INVALID_ARG, std::string("SECEDO_VCF_INDEX=") + e + ": expected none or tbi");
}

int index_kind(int *kind) {
    const int k = get_index();
    if (k < 0) return k;
    *kind = k;
    return SECEDO_OK;
}

secedo_variant_tabix_info &info() { return g_info; }

int build_raw(const uint8_t *d_text, const std::vector<uint64_t> &file_off, const std::vector<IndexedFile> &files,
              std::vector<std::vector<uint8_t>> *raw, size_t *n_good, hipStream_t s) {
    const size_t n_files = files.size();
    raw->assign(n_files, std::vector<uint8_t>());
    *n_good = n_files;
    if (n_files >= (1u << 31)) return fail(SECEDO_E_LIMIT, "more than 2^31 files to index");
    const uint64_t total = file_off.back(), budget = budget_bytes();
    Clock::time_point t0 = Clock::now();
    Buf b_off, b_end;
    SECEDO_TRY(b_off.alloc((n_files + 1) * 8));
    SECEDO_TRY(b_end.alloc(8));
    SECEDO_TRY(hipMemcpyAsync(b_off.p, file_off.data(), (n_files + 1) * 8, hipMemcpyHostToDevice, s));
    const T::Text text{d_text, b_off.as<uint64_t>(), uint32_t(n_files)};
    std::vector<tabixbuild::Builder> builders(n_files);
    std::vector<uint64_t> lines(n_files, 0), data(n_files, 0);  // of the ranges so far
    T::Carry carry{};
    Found bad;
    const auto voff = [&](uint32_t f, uint64_t lin) {
        return bamindexbuild::voffset(files[f].members, file_off[f + 1] - file_off[f], files[f].file_bytes, lin);
    };
    const auto inconsistent = [&](uint32_t f, const std::string &why) {
        return fail(SECEDO_E_STATE, files[f].label + ": the device line pass returned inconsistent results (" + why + ")");
    };

    // The device memory of all ranges, one allocation per stage (each is sized by what the stage before read back): it
    // grows to what the largest range needs and is released once, with the call.
    Arena by_chunk, by_line, emitted, named;
    const uint64_t max_windows = max_range_windows();
    for (uint64_t a = 0; a < total && !bad.any;) {
        uint64_t b = 0;
        SECEDO_CALL(cut_range(d_text, file_off, a, budget, b_end, &b, s));
        const T::Range r{a, uint32_t(b - a), file_of(file_off, a), file_of(file_off, b - 1)};
        const uint32_t chunks = T::range_chunks(text, r), n_f = r.f_hi - r.f_lo + 1;
        T::Work w{};
        w.scan_bytes = T::scan_workspace(chunks, 0);
        SECEDO_TRY(by_chunk.reserve({(size_t(chunks) / 2 + 1) * 4, (size_t(chunks) + 1) * 8, (size_t(chunks) + 1) * 8,
                                     size_t(n_f) * 4, size_t(n_f) * 4, 8, sizeof(T::Tail), w.scan_bytes}, s));
        w.file_bits = by_chunk.piece<uint32_t>(0), w.chunk_cnt = by_chunk.piece<uint64_t>(1);
        w.chunk_scan = by_chunk.piece<uint64_t>(2);
        w.first_line = by_chunk.piece<uint32_t>(3), w.first_data = by_chunk.piece<uint32_t>(4);
        w.err = by_chunk.piece<uint64_t>(5), w.tail = by_chunk.piece<T::Tail>(6);
        w.scan_tmp = by_chunk.piece<void>(7);
        SECEDO_TRY(T::mark_lines(text, r, w, s));
        uint64_t counts = 0;
        SECEDO_TRY(hipMemcpyAsync(&counts, w.chunk_scan + chunks, 8, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        const uint32_t n_lines = uint32_t(counts), n_data = uint32_t(counts >> 32);
        if (n_data > n_lines || n_lines > r.n) return inconsistent(r.f_lo, "more lines than bytes");

        // per data line: 4-byte arrays, 8-byte arrays (the window counts and their sum, one element longer, behind them),
        // and the 4-byte arrays the scans read one element past
        const size_t n1 = size_t(n_data) + 1;
        w.scan_bytes = T::scan_workspace(chunks, n_data);
        SECEDO_TRY(by_line.reserve({7 * size_t(n_data) * 4, (3 * size_t(n_data) + 2 * n1) * 8, 4 * n1 * 4, w.scan_bytes}, s));
        uint32_t *u32 = by_line.piece<uint32_t>(0), *u32p = by_line.piece<uint32_t>(2);
        uint64_t *u64 = by_line.piece<uint64_t>(1);
        w.start = u32, w.line = u32 + n_data, w.file = u32 + 2 * size_t(n_data), w.name_len = u32 + 3 * size_t(n_data);
        w.beg = u32 + 4 * size_t(n_data), w.end = u32 + 5 * size_t(n_data), w.bin = u32 + 6 * size_t(n_data);
        w.pos = u64, w.key = u64 + n_data, w.key_max = u64 + 2 * size_t(n_data);
        w.change = u32p, w.seg_ex = u32p + n1, w.head = u32p + 2 * n1, w.head_scan = u32p + 3 * n1;
        w.n_win = u64 + 3 * size_t(n_data), w.n_win_scan = w.n_win + n1;
        w.scan_tmp = by_line.piece<void>(3);
        SECEDO_TRY(T::index_lines(text, r, carry, n_data, w, s));
        T::Tail tail;
        std::vector<uint32_t> first_line(n_f), first_data(n_f);
        SECEDO_TRY(hipMemcpyAsync(&tail, w.tail, sizeof tail, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(first_line.data(), w.first_line, size_t(n_f) * 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(first_data.data(), w.first_data, size_t(n_f) * 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        if (tail.n_heads > n_data || tail.n_changes > n_data || tail.n_changes > tail.n_heads ||
            tail.n_wins > uint64_t(n_data) * bamindexbuild::kMaxWindows)
            return inconsistent(r.f_lo, "more heads than lines");
        // before anything is emitted: the window buffer is sized by this total
        if (tail.n_wins > max_windows)
            return fail(SECEDO_E_LIMIT, files[r.f_lo].label + ": the lines of one range of the text touch " +
                                            std::to_string(tail.n_wins) + " index windows, more than " +
                                            std::to_string(max_windows) + ": too many names with lines that span a chromosome");

        std::vector<T::Head> heads(tail.n_heads);
        std::vector<T::Win> wins(tail.n_wins);
        std::vector<T::Change> changes(tail.n_changes);
        std::vector<uint8_t> names;
        std::vector<uint64_t> name_at(changes.size() + 1, 0);
        if (n_data) {
            SECEDO_TRY(emitted.reserve({heads.size() * sizeof(T::Head), wins.size() * sizeof(T::Win),
                                        changes.size() * sizeof(T::Change)}, s));
            T::Head *d_heads = emitted.piece<T::Head>(0);
            T::Win *d_wins = emitted.piece<T::Win>(1);
            T::Change *d_changes = emitted.piece<T::Change>(2);
            SECEDO_TRY(T::emit(text, r, n_data, w, d_heads, d_wins, d_changes, s));
            SECEDO_TRY(hipMemcpyAsync(heads.data(), d_heads, heads.size() * sizeof(T::Head), hipMemcpyDeviceToHost, s));
            if (!wins.empty())
                SECEDO_TRY(hipMemcpyAsync(wins.data(), d_wins, wins.size() * sizeof(T::Win), hipMemcpyDeviceToHost, s));
            if (!changes.empty())
                SECEDO_TRY(hipMemcpyAsync(changes.data(), d_changes, changes.size() * sizeof(T::Change),
                                          hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            // the names of the change points: gathered into one buffer and downloaded
            std::vector<uint64_t> at(changes.size());
            std::vector<uint32_t> len(changes.size());
            for (size_t k = 0; k < changes.size(); ++k) {
                const T::Change &c = changes[k];
                if (c.file < r.f_lo || c.file > r.f_hi || c.name_at < a || c.name_at + c.name_len > b)
                    return inconsistent(r.f_lo, "a name outside the range");
                at[k] = c.name_at, len[k] = c.name_len;
                name_at[k + 1] = name_at[k] + c.name_len;
            }
            names.resize(name_at.back());
            if (!changes.empty()) {
                SECEDO_TRY(named.reserve({at.size() * 8, at.size() * 8, len.size() * 4, names.size()}, s));
                uint64_t *d_at = named.piece<uint64_t>(0), *d_out_at = named.piece<uint64_t>(1);
                uint32_t *d_len = named.piece<uint32_t>(2);
                uint8_t *d_names = named.piece<uint8_t>(3);
                SECEDO_TRY(hipMemcpyAsync(d_at, at.data(), at.size() * 8, hipMemcpyHostToDevice, s));
                SECEDO_TRY(hipMemcpyAsync(d_len, len.data(), len.size() * 4, hipMemcpyHostToDevice, s));
                SECEDO_TRY(hipMemcpyAsync(d_out_at, name_at.data(), at.size() * 8, hipMemcpyHostToDevice, s));
                SECEDO_TRY(T::gather_names(text, d_at, d_len, d_out_at, uint32_t(at.size()), d_names, s));
                if (!names.empty())
                    SECEDO_TRY(hipMemcpyAsync(names.data(), d_names, names.size(), hipMemcpyDeviceToHost, s));
                SECEDO_TRY(hipStreamSynchronize(s));
            }
        }
        g_info.pass_ms += ms_lap(t0);

        // ---- the host builder
        // lines and data lines of file f in front of this range: only the range's first file can have any
        const auto before = [&](const std::vector<uint64_t> &count, uint32_t f) { return f == r.f_lo ? count[f] : 0; };
        if (tail.err != T::kNoErr) {
            if (tail.err_file < r.f_lo || tail.err_file > r.f_hi) return inconsistent(r.f_lo, "an error outside the range");
            bad.take(tail.err_file, before(lines, tail.err_file) + tail.err_line + 1, what_of(uint32_t(tail.err & 0xFF)));
        }
        // segment -> the name's number in its file
        std::vector<uint32_t> name_of(changes.size() + 1, 0);
        if (carry.valid) name_of[0] = builders[carry.file].n_names() - 1;
        for (size_t k = 0; k < changes.size(); ++k) {
            const T::Change &c = changes[k];
            const std::string name(reinterpret_cast<const char *>(names.data()) + name_at[k], c.name_len);
            name_of[k + 1] = builders[c.file].n_names();
            const std::string why = builders[c.file].add_name(name);
            if (!why.empty()) {
                bad.take(c.file, before(lines, c.file) + c.line + 1, why + " (" + name + " comes back)");
                break;
            }
        }
        for (const T::Head &h : heads) {
            if (h.file < r.f_lo || h.file > r.f_hi || h.seg >= name_of.size()) return inconsistent(r.f_lo, "a head outside the range");
            if (bad.any && h.file >= bad.file) break;
            if (h.seg == 0 && (!carry.valid || carry.file != h.file)) return inconsistent(h.file, "a head without a name");
            const std::string why = builders[h.file].add_head(name_of[h.seg], h.bin, voff(h.file, h.off),
                                                              before(data, h.file) + h.ord);
            if (!why.empty()) return inconsistent(h.file, why);
        }
        for (const T::Win &x : wins) {
            if (x.file < r.f_lo || x.file > r.f_hi || x.seg >= name_of.size()) return inconsistent(r.f_lo, "a window outside the range");
            if (bad.any && x.file >= bad.file) break;
            if (x.seg == 0 && (!carry.valid || carry.file != x.file)) return inconsistent(x.file, "a window without a name");
            const std::string why = builders[x.file].add_window(name_of[x.seg], x.w, voff(x.file, x.off));
            if (!why.empty()) return inconsistent(x.file, why);
        }
        for (uint32_t k = 0; k < n_f; ++k) {
            lines[r.f_lo + k] += (k + 1 < n_f ? first_line[k + 1] : n_lines) - first_line[k];
            data[r.f_lo + k] += (k + 1 < n_f ? first_data[k + 1] : n_data) - first_data[k];
        }
        carry = tail.carry;
        g_info.ranges += 1;
        g_info.build_ms += ms_lap(t0);
        a = b;
    }

    const size_t n_done = bad.any ? bad.file : n_files;
    for (size_t f = 0; f < n_done; ++f) {
        tabixbuild::Stats st;
        const std::string why = builders[f].finish(voff(uint32_t(f), file_off[f + 1] - file_off[f]), data[f], &(*raw)[f], &st);
        if (!why.empty()) return inconsistent(uint32_t(f), why);
        g_info.files += 1;
        g_info.lines += lines[f];
        g_info.data_lines += data[f];
        g_info.names += st.names;
        g_info.bins += st.bins;
        g_info.chunks += st.chunks;
        g_info.windows += st.windows;
        g_info.index_bytes += (*raw)[f].size();
    }
    g_info.build_ms += ms_lap(t0);
    if (bad.any) {
        *n_good = bad.file;
        return fail(SECEDO_E_INVALID_ARG, files[bad.file].label + ": line " + std::to_string(bad.line) + ": " + bad.what);
    }
    return SECEDO_OK;
}

int compress_and_write(const std::vector<std::vector<uint8_t>> &raw, size_t n, const std::vector<std::string> &paths,
                       hipStream_t s) {
    if (!n) return SECEDO_OK;
    Clock::time_point t0 = Clock::now();
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t k = 0; k < n; ++k) off[k + 1] = off[k] + raw[k].size();
    std::vector<uint8_t> all(off[n]);
    for (size_t k = 0; k < n; ++k) std::copy(raw[k].begin(), raw[k].end(), all.begin() + off[k]);
    Buf b_text;
    constexpr uint32_t kSlack = secedo::bgzf::kDeflateInSlack;  // what the encoder reads around its input
    SECEDO_TRY(b_text.alloc(all.size() + 2 * kSlack));
    SECEDO_TRY(hipMemcpyAsync(b_text.p + kSlack, all.data(), all.size(), hipMemcpyHostToDevice, s));
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> out_off;
    secedo::bgzf::EncoderCounts counts;  // the encoder's counts of the index bodies: not the VCF files' statistics
    SECEDO_CALL(secedo::vcf::deflate_device(b_text.p + kSlack, off, &bytes, &out_off, s, nullptr, &counts));
    g_info.deflate_ms += ms_lap(t0);
    for (size_t k = 0; k < n; ++k) {
        SECEDO_CALL(write_renamed(paths[k], bytes.data() + out_off[k], out_off[k + 1] - out_off[k]));
        g_info.compressed_bytes += out_off[k + 1] - out_off[k];
    }
    g_info.write_ms += ms_lap(t0);
    return SECEDO_OK;
}

namespace {

// ---- the stand-alone route

struct Opened {
    std::string path;
    std::vector<uint8_t> bytes;
    IndexedFile file;  // its members as bgzf_members.hpp lists them: the payloads for the inflate are among them
    uint64_t text_bytes = 0;
};

int open_vcf_gz(const std::string &path, int overwrite, Opened *o) {
    o->path = path;
    o->file.label = path;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return fail(SECEDO_E_INVALID_ARG, "Could not open " + path);
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) o->bytes.insert(o->bytes.end(), buf, buf + got);
    const bool ok = !std::ferror(f);
    std::fclose(f);
    if (!ok) return fail(SECEDO_E_INVALID_ARG, "Could not read " + path);
    const std::vector<uint8_t> &b = o->bytes;
    if (b.size() < 2 || b[0] != 31 || b[1] != 139)
        return fail(SECEDO_E_INVALID_ARG, path + ": not a bgzip-compressed file; compress it with bgzip");
    uint32_t len = 0, isize = 0, xlen = 0;
    if (bm::member_header(b.data(), b.size(), 0, &len, &isize, &xlen) == bm::kNoMember)
        return fail(SECEDO_E_INVALID_ARG, path + ": a gzip file that is not BGZF; decompress it and compress it with "
                                                 "bgzip");
    if (!overwrite && access((path + ".tbi").c_str(), F_OK) == 0)
        return fail(SECEDO_E_INVALID_ARG, path + ": the index " + path + ".tbi exists; pass overwrite to replace it");
    const std::string why = bm::list_members(b.data(), b.size(), &o->file.members, &o->text_bytes);
    if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, path + ": " + why);
    o->file.file_bytes = b.size();
    return SECEDO_OK;
}

// text bytes per batch of files; a larger file is a batch of its own, its text whole in HBM
constexpr uint64_t kBatchText = 1ull << 30;

int run_batch(std::vector<Opened> &batch, hipStream_t s) {
    if (batch.empty()) return SECEDO_OK;
    using secedo::bam::BgzfDesc;
    using secedo::bam::kBgzfInSlack;  // around the whole batch: every file goes up from its first byte to its last
    Clock::time_point t0 = Clock::now();
    std::vector<uint64_t> file_off(batch.size() + 1, 0), in_off(batch.size() + 1, 0);
    std::vector<BgzfDesc> desc;
    std::vector<IndexedFile> files;
    for (size_t f = 0; f < batch.size(); ++f) {
        const Opened &o = batch[f];
        file_off[f + 1] = file_off[f] + o.text_bytes;
        in_off[f + 1] = in_off[f] + o.bytes.size();
        desc.resize(desc.size() + o.file.members.size());
        bm::fill_desc(o.file.members, 0, o.file.members.size(), 0, in_off[f], file_off[f],
                      desc.data() + desc.size() - o.file.members.size());
        files.push_back(o.file);
    }
    if (desc.size() >= (1u << 31)) return fail(SECEDO_E_LIMIT, "more than 2^31 BGZF blocks in a batch");
    Buf b_in, b_desc, b_status, b_text;
    SECEDO_TRY(b_in.alloc(in_off.back() + 2 * kBgzfInSlack));
    SECEDO_TRY(b_desc.alloc(desc.size() * sizeof(BgzfDesc)));
    SECEDO_TRY(b_status.alloc(desc.size() * 4));
    SECEDO_TRY(b_text.alloc(file_off.back() + 2 * T::kTextSlack));
    for (size_t f = 0; f < batch.size(); ++f)
        SECEDO_TRY(hipMemcpyAsync(b_in.p + kBgzfInSlack + in_off[f], batch[f].bytes.data(), batch[f].bytes.size(),
                                  hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(b_desc.p, desc.data(), desc.size() * sizeof(BgzfDesc), hipMemcpyHostToDevice, s));
    SECEDO_TRY(secedo::bam::bgzf_inflate(b_in.p + kBgzfInSlack, b_desc.as<BgzfDesc>(), uint32_t(desc.size()),
                                         b_text.p + T::kTextSlack, b_status.as<uint32_t>(), s));
    std::vector<uint32_t> status(desc.size());
    SECEDO_TRY(hipMemcpyAsync(status.data(), b_status.p, status.size() * 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    b_in.reset();
    g_info.pass_ms += ms_lap(t0);
    // a bad member: the files in front of it are indexed, its own error is the call's
    size_t n_ok = batch.size();
    std::string bad;
    size_t k = bm::first_bad(status.data(), status.size());  // of the batch, then of its file
    if (k < status.size()) {
        const uint32_t what = status[k];
        size_t f = 0;
        while (k >= batch[f].file.members.size()) k -= batch[f++].file.members.size();
        n_ok = f;
        bad = batch[f].path + ": " + bm::block_where(k) + ": " + bm::status_text(what);
    }
    files.resize(n_ok);
    file_off.resize(n_ok + 1);
    std::vector<std::vector<uint8_t>> raw;
    size_t n_good = 0;
    const int rc = build_raw(b_text.p + T::kTextSlack, file_off, files, &raw, &n_good, s);
    const std::string msg = g_error;
    if (rc != SECEDO_OK && rc != SECEDO_E_INVALID_ARG) return rc;
    std::vector<std::string> paths;
    for (size_t f = 0; f < n_good; ++f) paths.push_back(batch[f].path + ".tbi");
    SECEDO_CALL(compress_and_write(raw, n_good, paths, s));
    batch.clear();
    if (rc != SECEDO_OK) return fail(rc, msg);
    return bad.empty() ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, bad);
}

int tabix_build(const char *const *paths, uint32_t n, int overwrite, hipStream_t s) {
    std::vector<Opened> batch;
    uint64_t text = 0;
    for (uint32_t f = 0; f < n; ++f) {
        if (!paths[f]) return fail(SECEDO_E_INVALID_ARG, "null file name");
        Opened o;
        const int rc = open_vcf_gz(paths[f], overwrite, &o);
        if (rc != SECEDO_OK) {  // the files in front of it come first
            const std::string msg = g_error;
            SECEDO_CALL(run_batch(batch, s));
            return fail(rc, msg);
        }
        if (!batch.empty() && text + o.text_bytes > kBatchText) {
            SECEDO_CALL(run_batch(batch, s));
            text = 0;
        }
        text += o.text_bytes;
        batch.push_back(std::move(o));
    }
    return run_batch(batch, s);
}

}  // namespace
}  // namespace tabix_host
}  // namespace secedo

extern "C" {

int secedo_variant_set_vcf_index(int index) {
    if (index != SECEDO_VCF_INDEX_NONE && index != SECEDO_VCF_INDEX_TBI)
        return secedo::host::fail(SECEDO_E_INVALID_ARG, "index must be SECEDO_VCF_INDEX_NONE or SECEDO_VCF_INDEX_TBI");
    secedo::tabix_host::set_index(index);
    return SECEDO_OK;
}

int secedo_variant_get_vcf_index(void) { return secedo::tabix_host::get_index(); }

int secedo_variant_tabix_stats(secedo_variant_tabix_info *out) {
    if (!out) return secedo::host::fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = secedo::tabix_host::info();
    return SECEDO_OK;
}

int secedo_variant_tabix_build(int device_id, const char *const *paths, uint32_t n, int overwrite, void *stream) {
    secedo::tabix_host::info() = secedo_variant_tabix_info{};
    if (!paths && n) return secedo::host::fail(SECEDO_E_INVALID_ARG, "null argument");
    SECEDO_CALL(secedo::host::set_device(device_id));
    return secedo::tabix_host::tabix_build(paths, n, overwrite, static_cast<hipStream_t>(stream));
}

}  // extern "C"
