// bam_host.cpp -- host side of include/secedo_bam.h: BGZF inflate, BAM header and record walk, the global record
// order, the launches of bam_kernels.hip and the .bin / .map / .txt files of the reference's pileup_bams()
// (pileup.cpp:235-348).
//
// Each file is memory-mapped; its BGZF blocks (BSIZE from the BC extra field) are inflated with zlib raw inflate
// in a pool of at most 16 threads, CRC32 and ISIZE checked. Files are inflated in batches of about 512 MiB of
// inflated data; of each file only the byte run of the requested chromosomes' records is kept. No .bai is needed:
// the run is found by walking block_size, so with or without an index the result is the same.
#include "secedo_bam.h"
#include "secedo_simmat.h"
#include "bam_kernels.hpp"

#include <hip/hip_runtime.h>
#include <zlib.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace {

using namespace secedo::bam;

thread_local std::string g_error;

int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

#define BAM_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(SECEDO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define BAM_CALL(expr)                    \
    do {                                  \
        int rc_ = (expr);                 \
        if (rc_ != SECEDO_OK) return rc_; \
    } while (0)

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

constexpr uint32_t kMaxThreads = 16;
constexpr uint64_t kBatchBytes = 512ull << 20;

inline uint32_t rd32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint16_t rd16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }

template <class F>
void parallel_for(uint32_t threads, uint64_t n, F f) {
    threads = std::max<uint32_t>(1, std::min<uint64_t>(std::min(threads, kMaxThreads), n));
    std::atomic<uint64_t> next{0};
    auto work = [&] {
        for (uint64_t i; (i = next.fetch_add(1)) < n;) f(i);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
}

struct Mapped {
    const uint8_t *p = nullptr;
    size_t n = 0;
    ~Mapped() {
        if (p && n) munmap(const_cast<uint8_t *>(p), n);
    }
};

int map_file(const std::string &path, Mapped *m) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return fail(SECEDO_E_INVALID_ARG, "Could not open " + path);
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(fd);
        return fail(SECEDO_E_INVALID_ARG, "Could not stat " + path);
    }
    m->n = size_t(st.st_size);
    if (m->n) {
        void *p = mmap(nullptr, m->n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) {
            close(fd);
            return fail(SECEDO_E_INVALID_ARG, "Could not map " + path);
        }
        m->p = static_cast<const uint8_t *>(p);
    }
    close(fd);
    return SECEDO_OK;
}

struct Block {
    const uint8_t *cdata;
    uint32_t clen, crc, isize;
    uint64_t out;  // offset in the file's inflated buffer
};

// BGZF block list of one mapped file
int list_blocks(const std::string &path, const Mapped &m, std::vector<Block> *blocks, uint64_t *total) {
    uint64_t off = 0, out = 0;
    while (off < m.n) {
        const uint8_t *b = m.p + off;
        if (m.n - off < 18 || b[0] != 31 || b[1] != 139 || b[2] != 8 || !(b[3] & 4))
            return fail(SECEDO_E_INVALID_ARG, path + ": not a BGZF block at byte " + std::to_string(off));
        const uint32_t xlen = rd16(b + 10);
        uint32_t bsize = UINT32_MAX;
        for (uint32_t x = 12; x + 4 <= 12 + xlen && 12 + xlen <= m.n - off;) {
            const uint32_t slen = rd16(b + x + 2);
            if (b[x] == 'B' && b[x + 1] == 'C' && slen == 2) bsize = rd16(b + x + 4);
            x += 4 + slen;
        }
        if (bsize == UINT32_MAX || uint64_t(bsize) + 1 > m.n - off || bsize + 1 < 12 + xlen + 8)
            return fail(SECEDO_E_INVALID_ARG, path + ": bad BGZF block size at byte " + std::to_string(off));
        const uint32_t len = bsize + 1;
        Block blk{b + 12 + xlen, len - xlen - 20, rd32(b + len - 8), rd32(b + len - 4), out};
        if (blk.isize > 65536) return fail(SECEDO_E_INVALID_ARG, path + ": BGZF ISIZE above 64 KiB");
        blocks->push_back(blk);
        out += blk.isize;
        off += len;
    }
    *total = out;
    return SECEDO_OK;
}

// 0 on success, else a message
std::string inflate_block(const Block &b, uint8_t *dst) {
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) return "inflateInit2 failed";
    z.next_in = const_cast<Bytef *>(b.cdata);
    z.avail_in = b.clen;
    z.next_out = dst;
    z.avail_out = b.isize;
    const int rc = inflate(&z, Z_FINISH);
    const uint64_t got = z.total_out;
    inflateEnd(&z);
    if (rc != Z_STREAM_END || got != b.isize) return "inflate failed or ISIZE mismatch";
    if (uint32_t(crc32(crc32(0, nullptr, 0), dst, b.isize)) != b.crc) return "CRC32 mismatch";
    return std::string();
}

struct Inflated {
    std::string path;
    std::vector<uint8_t> data;
    uint64_t n_blocks = 0;
};

// inflate a batch of files: all their blocks in one pool
int inflate_files(const std::vector<std::string> &paths, uint32_t threads, std::vector<Inflated> *out) {
    std::vector<Mapped> maps(paths.size());
    std::vector<std::vector<Block>> blocks(paths.size());
    std::vector<std::pair<uint32_t, uint32_t>> tasks;
    out->resize(paths.size());
    for (size_t f = 0; f < paths.size(); ++f) {
        BAM_CALL(map_file(paths[f], &maps[f]));
        uint64_t total = 0;
        BAM_CALL(list_blocks(paths[f], maps[f], &blocks[f], &total));
        (*out)[f].path = paths[f];
        (*out)[f].data.resize(total);
        (*out)[f].n_blocks = blocks[f].size();
        for (uint32_t b = 0; b < blocks[f].size(); ++b) tasks.emplace_back(uint32_t(f), b);
    }
    std::vector<std::string> errs(tasks.size());
    parallel_for(threads, tasks.size(), [&](uint64_t t) {
        const Block &b = blocks[tasks[t].first][tasks[t].second];
        errs[t] = inflate_block(b, (*out)[tasks[t].first].data.data() + b.out);
    });
    for (size_t t = 0; t < tasks.size(); ++t)
        if (!errs[t].empty())
            return fail(SECEDO_E_INVALID_ARG, paths[tasks[t].first] + ": BGZF block " +
                                                  std::to_string(tasks[t].second) + ": " + errs[t]);
    return SECEDO_OK;
}

struct Header {
    uint32_t l_text = 0, n_ref = 0;
    uint64_t first_record = 0;
};

int parse_header(const Inflated &f, Header *h) {
    const std::vector<uint8_t> &d = f.data;
    if (d.size() < 12 || std::memcmp(d.data(), "BAM\1", 4) != 0)
        return fail(SECEDO_E_INVALID_ARG, f.path + ": not a BAM file (magic)");
    h->l_text = rd32(&d[4]);
    uint64_t o = 8 + uint64_t(h->l_text);
    if (o + 4 > d.size()) return fail(SECEDO_E_INVALID_ARG, f.path + ": truncated header");
    h->n_ref = rd32(&d[o]);
    o += 4;
    for (uint32_t r = 0; r < h->n_ref; ++r) {
        if (o + 4 > d.size()) return fail(SECEDO_E_INVALID_ARG, f.path + ": truncated reference list");
        o += 4 + uint64_t(rd32(&d[o]));
        if (o + 4 > d.size()) return fail(SECEDO_E_INVALID_ARG, f.path + ": truncated reference list");
        o += 4;
    }
    h->first_record = o;
    return SECEDO_OK;
}

// One pass over the records: structure and sortedness checked; on_record(index, offset, refID, pos).
template <class F>
int walk_records(const Inflated &f, const Header &h, uint64_t *n_records, F on_record) {
    const std::vector<uint8_t> &d = f.data;
    uint64_t o = h.first_record, idx = 0;
    int64_t prev_ref = -1, prev_pos = 0;
    while (o < d.size()) {
        const std::string where = f.path + ": record " + std::to_string(idx);
        if (d.size() - o < 4 + 32) return fail(SECEDO_E_INVALID_ARG, where + " is truncated");
        const uint32_t bs = rd32(&d[o]);
        const uint8_t *c = &d[o + 4];
        if (bs < 32 || bs > d.size() - o - 4) return fail(SECEDO_E_INVALID_ARG, where + " has a bad block_size");
        const uint64_t need = 32 + uint64_t(c[8]) + 4ull * rd16(c + 12) + (uint64_t(rd32(c + 16)) + 1) / 2 +
                              uint64_t(rd32(c + 16));
        if (need > bs) return fail(SECEDO_E_INVALID_ARG, where + " is longer than its block_size");
        const int32_t ref = int32_t(rd32(c)), pos = int32_t(rd32(c + 4));
        const int64_t key_ref = ref < 0 ? INT64_MAX : ref;
        if (idx > 0 && (key_ref < prev_ref || (key_ref == prev_ref && ref >= 0 && pos < prev_pos)))
            return fail(SECEDO_E_INVALID_ARG, where + ": input is not coordinate-sorted");
        prev_ref = key_ref;
        prev_pos = pos;
        BAM_CALL(on_record(idx, o, ref, pos));
        o += 4 + uint64_t(bs);
        ++idx;
    }
    *n_records = idx;
    return SECEDO_OK;
}

// CIGAR ops and SEQ length agree (BuildCharData's substr would otherwise truncate)
int check_cigar(const uint8_t *rec, const std::string &where) {
    const uint8_t *c = rec + 4;
    const uint32_t l_name = c[8], n_cigar = rd16(c + 12), l_seq = rd32(c + 16);
    uint64_t query = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t v = rd32(c + 32 + l_name + 4 * k), t = v & 15;
        if (t > 8) return fail(SECEDO_E_INVALID_ARG, where + ": invalid CIGAR op code " + std::to_string(t));
        if (t == 0 || t == 1 || t == 4 || t == 7 || t == 8) query += v >> 4;
    }
    if (l_seq > 0 && n_cigar > 0 && query != l_seq)
        return fail(SECEDO_E_INVALID_ARG, where + ": CIGAR and SEQ lengths differ");
    return SECEDO_OK;
}

// the chromosome's records of every file, in the global order
struct ChrInput {
    uint32_t chromosome;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> file_base;          // [n_files] start of each file's run in bytes
    std::vector<std::vector<uint64_t>> roff;  // per file: record offsets (relative to its run)
    std::vector<std::vector<int32_t>> rpos;
    std::vector<std::vector<uint64_t>> ridx;  // record index in the file (messages)
};

int load_inputs(const std::vector<std::string> &files, uint32_t threads, std::vector<ChrInput> *chrs,
                secedo_bam_times *t) {
    const size_t n_files = files.size();
    for (auto &c : *chrs) {
        c.file_base.assign(n_files, 0);
        c.roff.assign(n_files, {});
        c.rpos.assign(n_files, {});
        c.ridx.assign(n_files, {});
    }
    std::vector<std::vector<std::vector<uint8_t>>> runs(chrs->size(), std::vector<std::vector<uint8_t>>(n_files));
    size_t f0 = 0;
    while (f0 < n_files) {
        // a batch of files of at most kBatchBytes on disk (BGZF inflates 3-4x), at least one file
        size_t f1 = f0;
        uint64_t disk = 0;
        while (f1 < n_files && (f1 == f0 || disk < kBatchBytes / 4)) {
            struct stat st;
            disk += stat(files[f1].c_str(), &st) == 0 ? uint64_t(st.st_size) : 0;
            ++f1;
        }
        std::vector<Inflated> inf;
        Clock::time_point t0 = Clock::now();
        BAM_CALL(inflate_files(std::vector<std::string>(files.begin() + f0, files.begin() + f1), threads, &inf));
        if (t) {
            t->inflate_ms += ms_since(t0);
            for (auto &x : inf) t->inflated_bytes += double(x.data.size());
        }
        t0 = Clock::now();
        std::vector<int> rcs(inf.size(), SECEDO_OK);
        std::vector<std::string> errs(inf.size());
        parallel_for(threads, inf.size(), [&](uint64_t k) {
            const size_t f = f0 + k;
            Header h;
            int rc = parse_header(inf[k], &h);
            std::vector<uint64_t> first(chrs->size(), UINT64_MAX), last(chrs->size(), 0);
            std::vector<int> done(chrs->size(), 0);
            uint64_t n = 0;
            if (rc == SECEDO_OK)
                rc = walk_records(inf[k], h, &n, [&](uint64_t idx, uint64_t o, int32_t ref, int32_t pos) {
                    for (size_t c = 0; c < chrs->size(); ++c) {
                        ChrInput &ci = (*chrs)[c];
                        if (done[c]) continue;
                        if (ref < 0 || uint32_t(ref) != ci.chromosome) {
                            if (first[c] != UINT64_MAX) done[c] = 1;  // the reader stops at another RefID
                            continue;
                        }
                        const std::string where = files[f] + ": record " + std::to_string(idx);
                        if (pos < 0) return fail(SECEDO_E_INVALID_ARG, where + " has a negative position");
                        BAM_CALL(check_cigar(&inf[k].data[o], where));
                        if (first[c] == UINT64_MAX) first[c] = o;
                        last[c] = o + 4 + rd32(&inf[k].data[o]);
                        ci.roff[f].push_back(o - first[c]);
                        ci.rpos[f].push_back(pos);
                        ci.ridx[f].push_back(idx);
                    }
                    return SECEDO_OK;
                });
            if (rc == SECEDO_OK)
                for (size_t c = 0; c < chrs->size(); ++c)
                    if (first[c] != UINT64_MAX)
                        runs[c][f].assign(inf[k].data.begin() + first[c], inf[k].data.begin() + last[c]);
            rcs[k] = rc;
            errs[k] = g_error;
        });
        for (size_t k = 0; k < inf.size(); ++k)
            if (rcs[k] != SECEDO_OK) return fail(rcs[k], errs[k]);
        if (t) t->walk_ms += ms_since(t0);
        f0 = f1;
    }
    const Clock::time_point t0 = Clock::now();
    for (size_t c = 0; c < chrs->size(); ++c) {
        ChrInput &ci = (*chrs)[c];
        uint64_t total = 0;
        for (size_t f = 0; f < n_files; ++f) total += runs[c][f].size();
        ci.bytes.reserve(total);
        for (size_t f = 0; f < n_files; ++f) {
            ci.file_base[f] = ci.bytes.size();
            ci.bytes.insert(ci.bytes.end(), runs[c][f].begin(), runs[c][f].end());
            std::vector<uint8_t>().swap(runs[c][f]);
        }
    }
    if (t) t->walk_ms += ms_since(t0);
    return SECEDO_OK;
}

template <class T>
struct Dev {
    T *p = nullptr;
    size_t n = 0;
    Dev() = default;
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
    ~Dev() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        reset();
        n = count;
        return hipMalloc(&p, std::max<size_t>(1, count) * sizeof(T));
    }
    // keep the first `keep` elements, grow to at least `count`
    hipError_t grow(size_t count, size_t keep, hipStream_t s) {
        if (count <= n && p) return hipSuccess;
        size_t cap = std::max<size_t>(count, 2 * n);
        T *q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(1, cap) * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep) e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (p) (void)hipFree(p);
        p = q;
        n = cap;
        return e;
    }
};

struct Result {
    std::vector<uint32_t> chr_locus_off{0};
    Dev<uint32_t> pos, rid;
    Dev<uint64_t> off;
    Dev<uint16_t> idb;
    uint64_t n_loci = 0, n_entries = 0;
    uint32_t num_cells = 1, max_read_length = 0;
};

thread_local Result *g_result = nullptr;

struct ChrOut {
    std::vector<uint8_t> first;  // per ordinal: first occurrence of its name (host files only)
    std::vector<uint32_t> id;
    std::vector<uint64_t> ord_off;  // per ordinal: byte offset in ChrInput::bytes
};

// The device passes of one chromosome, appended to `res`.
int run_chromosome(const ChrInput &ci, const Params &prm, const uint16_t *d_i2g, uint32_t n_groups, bool want_map,
                   hipStream_t s, Result *res, ChrOut *co, secedo_bam_times *t) {
    const size_t n_files = ci.roff.size();
    Clock::time_point t0 = Clock::now();
    // global order: chunk of Position, file, record
    int32_t max_pos = -1, min_pos = INT32_MAX;
    uint64_t n64 = 0;
    for (size_t f = 0; f < n_files; ++f) {
        n64 += ci.rpos[f].size();
        if (!ci.rpos[f].empty()) {
            max_pos = std::max(max_pos, ci.rpos[f].back());
            min_pos = std::min(min_pos, ci.rpos[f].front());
        }
    }
    if (n64 >= (1ull << 32)) return fail(SECEDO_E_LIMIT, "more than 2^32 records in one chromosome");
    const uint32_t n = uint32_t(n64);
    const uint32_t last_chunk = max_pos < 0 ? 0 : uint32_t(max_pos) / kChunk;
    std::vector<uint64_t> ord_off;
    std::vector<uint16_t> ord_file;
    std::vector<uint64_t> ord_idx;
    ord_off.reserve(n);
    ord_file.reserve(n);
    ord_idx.reserve(n);
    {
        std::vector<size_t> cur(n_files, 0);
        for (uint32_t c = 0; c <= last_chunk; ++c)
            for (size_t f = 0; f < n_files; ++f)
                for (size_t &k = cur[f]; k < ci.rpos[f].size() && uint32_t(ci.rpos[f][k]) / kChunk == c; ++k) {
                    ord_off.push_back(ci.file_base[f] + ci.roff[f][k]);
                    ord_file.push_back(uint16_t(f));
                    ord_idx.push_back(ci.ridx[f][k]);
                }
    }
    if (t) t->walk_ms += ms_since(t0);
    t0 = Clock::now();
    Dev<uint8_t> d_bytes;
    Dev<uint64_t> d_off;
    Dev<uint16_t> d_file;
    BAM_TRY(d_bytes.alloc(ci.bytes.size()));
    BAM_TRY(d_off.alloc(n));
    BAM_TRY(d_file.alloc(n));
    if (!ci.bytes.empty())
        BAM_TRY(hipMemcpyAsync(d_bytes.p, ci.bytes.data(), ci.bytes.size(), hipMemcpyHostToDevice, s));
    if (n) {
        BAM_TRY(hipMemcpyAsync(d_off.p, ord_off.data(), n * 8ull, hipMemcpyHostToDevice, s));
        BAM_TRY(hipMemcpyAsync(d_file.p, ord_file.data(), n * 2ull, hipMemcpyHostToDevice, s));
    }
    BAM_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_since(t0);
    t0 = Clock::now();

    const Records rs{d_bytes.p, d_off.p, d_file.p, n};
    Dev<uint64_t> key, key2;
    Dev<uint32_t> val, val2, run, rep, flag, scan, id, span_end;
    Dev<uint8_t> pass;
    Dev<unsigned long long> err;
    BAM_TRY(key.alloc(n));
    BAM_TRY(key2.alloc(n));
    BAM_TRY(val.alloc(n));
    BAM_TRY(val2.alloc(n));
    BAM_TRY(run.alloc(n));
    BAM_TRY(rep.alloc(n));
    BAM_TRY(flag.alloc(n + 1));
    BAM_TRY(scan.alloc(n + 1));
    BAM_TRY(id.alloc(n));
    BAM_TRY(span_end.alloc(n));
    BAM_TRY(pass.alloc(n));
    BAM_TRY(err.alloc(1));
    BAM_TRY(hipMemsetAsync(err.p, 0xFF, 8, s));
    BAM_TRY(decode(rs, prm, key.p, val.p, pass.p, span_end.p, err.p, s));
    unsigned long long h_err = 0;
    BAM_TRY(hipMemcpyAsync(&h_err, err.p, 8, hipMemcpyDeviceToHost, s));
    BAM_TRY(hipStreamSynchronize(s));
    if (h_err != ~0ull) {
        static const char *what[] = {"", "is not paired, not a proper pair or failed QC",
                                     "has a kept base at or past MAX_INSERT_SIZE after its chunk's end",
                                     "walks past the end of its CIGAR", "has a D op over a base",
                                     "reads past its quality string", "has a negative position"};
        const uint32_t o = uint32_t(h_err >> 8), code = uint32_t(h_err & 0xFF);
        return fail(SECEDO_E_INVALID_ARG, "file " + std::to_string(ord_file[o]) + ", record " +
                                              std::to_string(ord_idx[o]) + ": " + (code < 7 ? what[code] : "?"));
    }
    // name numbering
    Dev<uint8_t> tmp;
    size_t tmp_bytes = std::max(sort_pairs_bytes(n), scan_bytes(uint64_t(n) + 1));
    BAM_TRY(tmp.alloc(tmp_bytes));
    uint32_t n_ids = 0;
    if (n) {
        BAM_TRY(sort_pairs(tmp.p, tmp_bytes, key.p, key2.p, val.p, val2.p, n, s));
        BAM_TRY(first_occurrence(rs, key2.p, val2.p, run.p, rep.p, flag.p, tmp.p, tmp_bytes, s));
        BAM_TRY(hipMemsetAsync(flag.p + n, 0, 4, s));
        BAM_TRY(exclusive_sum(tmp.p, tmp_bytes, flag.p, scan.p, uint64_t(n) + 1, s));
        BAM_TRY(assign_ids(rep.p, scan.p, id.p, n, s));
        BAM_TRY(hipMemcpyAsync(&n_ids, scan.p + n, 4, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipStreamSynchronize(s));
    }
    key.reset();
    key2.reset();
    val.reset();
    val2.reset();
    run.reset();
    rep.reset();
    if (want_map) {
        co->first.resize(n);
        co->id.resize(n);
        std::vector<uint32_t> fl(n);
        if (n) {
            BAM_TRY(hipMemcpyAsync(fl.data(), flag.p, n * 4ull, hipMemcpyDeviceToHost, s));
            BAM_TRY(hipMemcpyAsync(co->id.data(), id.p, n * 4ull, hipMemcpyDeviceToHost, s));
            BAM_TRY(hipStreamSynchronize(s));
        }
        for (uint32_t o = 0; o < n; ++o) co->first[o] = uint8_t(fl[o]);
        co->ord_off = ord_off;
    }
    flag.reset();
    scan.reset();

    // windows over [first window start, end of the last chunk)
    const uint64_t locus_base = res->n_loci;
    const uint64_t limit = uint64_t(last_chunk + 1) * kChunk;
    if (n) {
        Dev<uint32_t> cnt, cand, cscan, cpos, ctot, fill, keep, kscan, flags;
        Dev<uint64_t> arr, ascan, carr, ekey, eval, ekey2, eval2, kept, escan;
        const uint32_t W = kWindow;
        BAM_TRY(cnt.alloc(size_t(W) * 4));
        BAM_TRY(cand.alloc(W + 1));
        BAM_TRY(cscan.alloc(W + 1));
        BAM_TRY(arr.alloc(W + 1));
        BAM_TRY(ascan.alloc(W + 1));
        BAM_TRY(flags.alloc(2));
        BAM_TRY(hipMemsetAsync(flags.p, 0, 8, s));
        size_t wtmp_bytes = scan_bytes(uint64_t(W) + 1);
        Dev<uint8_t> wtmp;
        BAM_TRY(wtmp.alloc(wtmp_bytes));
        for (uint64_t w0 = uint64_t(min_pos) / W * W; w0 < limit; w0 += W) {
            const uint32_t w1 = uint32_t(std::min<uint64_t>(w0 + W, limit));
            const uint32_t n_pos = w1 - uint32_t(w0);
            BAM_TRY(hipMemsetAsync(cnt.p, 0, size_t(n_pos) * 16, s));
            BAM_TRY(count(rs, prm, pass.p, span_end.p, uint32_t(w0), w1, cnt.p, s));
            BAM_TRY(select(cnt.p, prm, n_pos, cand.p, arr.p, s));
            BAM_TRY(hipMemsetAsync(cand.p + n_pos, 0, 4, s));
            BAM_TRY(hipMemsetAsync(arr.p + n_pos, 0, 8, s));
            BAM_TRY(exclusive_sum(wtmp.p, wtmp_bytes, cand.p, cscan.p, uint64_t(n_pos) + 1, s));
            BAM_TRY(exclusive_sum64(wtmp.p, wtmp_bytes, arr.p, ascan.p, uint64_t(n_pos) + 1, s));
            uint32_t n_cand = 0;
            uint64_t n_arr = 0;
            BAM_TRY(hipMemcpyAsync(&n_cand, cscan.p + n_pos, 4, hipMemcpyDeviceToHost, s));
            BAM_TRY(hipMemcpyAsync(&n_arr, ascan.p + n_pos, 8, hipMemcpyDeviceToHost, s));
            BAM_TRY(hipStreamSynchronize(s));
            if (n_cand == 0) continue;
            BAM_TRY(cpos.alloc(n_cand));
            BAM_TRY(ctot.alloc(n_cand));
            BAM_TRY(carr.alloc(n_cand));
            BAM_TRY(fill.alloc(n_cand));
            BAM_TRY(compact_candidates(cnt.p, cand.p, cscan.p, ascan.p, uint32_t(w0), n_pos, cpos.p, carr.p,
                                       ctot.p, s));
            BAM_TRY(hipMemsetAsync(fill.p, 0, n_cand * 4ull, s));
            BAM_TRY(ekey.alloc(n_arr));
            BAM_TRY(eval.alloc(n_arr));
            BAM_TRY(ekey2.alloc(n_arr));
            BAM_TRY(eval2.alloc(n_arr));
            BAM_TRY(emit(rs, prm, pass.p, span_end.p, id.p, uint32_t(w0), w1, cand.p, cscan.p, ascan.p, fill.p,
                         ekey.p, eval.p, s));
            int bits = 32;
            while (bits < 64 && (uint64_t(n_cand - 1) >> (bits - 32)) != 0) ++bits;
            const size_t sb = sort_pairs64_bytes(n_arr), cb = scan_bytes(uint64_t(n_cand) + 1);
            Dev<uint8_t> stmp;
            BAM_TRY(stmp.alloc(std::max(sb, cb)));
            BAM_TRY(sort_pairs64(stmp.p, sb, ekey.p, ekey2.p, eval.p, eval2.p, n_arr, bits, s));
            ekey.reset();
            eval.reset();
            ekey2.reset();
            BAM_TRY(keep.alloc(n_cand + 1));
            BAM_TRY(kscan.alloc(n_cand + 1));
            BAM_TRY(kept.alloc(n_cand + 1));
            BAM_TRY(escan.alloc(n_cand + 1));
            BAM_TRY(finalize(eval2.p, carr.p, ctot.p, prm, n_cand, keep.p, kept.p, s));
            BAM_TRY(hipMemsetAsync(keep.p + n_cand, 0, 4, s));
            BAM_TRY(hipMemsetAsync(kept.p + n_cand, 0, 8, s));
            BAM_TRY(exclusive_sum(stmp.p, cb, keep.p, kscan.p, uint64_t(n_cand) + 1, s));
            BAM_TRY(exclusive_sum64(stmp.p, cb, kept.p, escan.p, uint64_t(n_cand) + 1, s));
            uint32_t n_keep = 0;
            uint64_t n_kept = 0;
            BAM_TRY(hipMemcpyAsync(&n_keep, kscan.p + n_cand, 4, hipMemcpyDeviceToHost, s));
            BAM_TRY(hipMemcpyAsync(&n_kept, escan.p + n_cand, 8, hipMemcpyDeviceToHost, s));
            BAM_TRY(hipStreamSynchronize(s));
            if (n_keep) {
                BAM_TRY(res->pos.grow(res->n_loci + n_keep, res->n_loci, s));
                BAM_TRY(res->off.grow(res->n_loci + n_keep + 1, res->n_loci + 1, s));
                BAM_TRY(res->rid.grow(res->n_entries + n_kept, res->n_entries, s));
                BAM_TRY(res->idb.grow(res->n_entries + n_kept, res->n_entries, s));
                BAM_TRY(gather(eval2.p, cpos.p, carr.p, ctot.p, keep.p, kscan.p, escan.p, n_cand, d_i2g, n_groups,
                               res->pos.p + res->n_loci, res->off.p + res->n_loci, res->rid.p + res->n_entries,
                               res->idb.p + res->n_entries, res->n_entries, flags.p, s));
                res->n_loci += n_keep;
                res->n_entries += n_kept;
            }
            eval2.reset();
        }
        uint32_t h_flags[2] = {0, 0};
        BAM_TRY(hipMemcpyAsync(h_flags, flags.p, 8, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipStreamSynchronize(s));
        if (h_flags[0]) return fail(SECEDO_E_INVALID_ARG, "a cell id is too large for the id_to_group mapping");
        if (res->n_loci > locus_base) res->num_cells = std::max(res->num_cells, h_flags[1] + 1);
    }
    // the reader's max_read_length over this chromosome
    const uint64_t n_new = res->n_loci - locus_base;
    if (n_new) {
        Dev<uint32_t> mn, mx, ml;
        BAM_TRY(mn.alloc(n_ids));
        BAM_TRY(mx.alloc(n_ids));
        BAM_TRY(ml.alloc(1));
        BAM_TRY(hipMemsetAsync(mn.p, 0xFF, n_ids * 4ull, s));
        BAM_TRY(hipMemsetAsync(mx.p, 0, n_ids * 4ull, s));
        BAM_TRY(hipMemsetAsync(ml.p, 0, 4, s));
        BAM_TRY(read_stats(res->pos.p + locus_base, res->off.p + locus_base, res->rid.p, uint32_t(n_new), mn.p,
                           mx.p, n_ids, ml.p, s));
        uint32_t h_ml = 0;
        BAM_TRY(hipMemcpyAsync(&h_ml, ml.p, 4, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipStreamSynchronize(s));
        res->max_read_length = std::max(res->max_read_length, h_ml);
    }
    if (t) t->device_ms += ms_since(t0);
    return SECEDO_OK;
}

std::string name_at(const ChrInput &ci, uint64_t off) {
    const uint8_t *c = ci.bytes.data() + off + 4;
    const char *nm = reinterpret_cast<const char *>(c + 32);
    return std::string(nm, strnlen(nm, c[8]));
}

int write_files(const std::string &prefix, bool text, uint32_t chromosome_id, const ChrInput &ci, const ChrOut &co,
                const std::vector<uint32_t> &pos, const std::vector<uint64_t> &off, const std::vector<uint32_t> &rid,
                const std::vector<uint16_t> &idb) {
    FILE *fm = fopen((prefix + ".map").c_str(), "wb");
    if (!fm) return fail(SECEDO_E_INVALID_ARG, "Could not write " + prefix + ".map");
    std::string buf;
    for (size_t o = 0; o < co.first.size(); ++o)
        if (co.first[o]) buf += name_at(ci, co.ord_off[o]) + "\t" + std::to_string(co.id[o]) + "\n";
    fwrite(buf.data(), 1, buf.size(), fm);
    fclose(fm);
    FILE *fb = fopen((prefix + ".bin").c_str(), "wb");
    FILE *ft = fopen((prefix + ".txt").c_str(), "wb");
    if (!fb || !ft) {
        if (fb) fclose(fb);
        if (ft) fclose(ft);
        return fail(SECEDO_E_INVALID_ARG, "Could not write " + prefix + ".bin/.txt");
    }
    std::string bin, txt;
    static const char kIntToChar[4] = {'A', 'C', 'G', 'T'};
    std::vector<std::pair<uint16_t, uint32_t>> e;
    for (size_t l = 0; l < pos.size(); ++l) {
        const uint64_t b = off[l], en = off[l + 1];
        const uint16_t cov = uint16_t(en - b);
        bin.append(reinterpret_cast<const char *>(&pos[l]), 4);
        bin.append(reinterpret_cast<const char *>(&cov), 2);
        bin.append(reinterpret_cast<const char *>(&rid[b]), cov * 4ull);
        bin.append(reinterpret_cast<const char *>(&idb[b]), cov * 2ull);
        if (text) {
            e.clear();
            for (uint64_t k = b; k < en; ++k) e.emplace_back(idb[k], rid[k]);
            std::stable_sort(e.begin(), e.end(), [](const auto &x, const auto &y) { return (x.first >> 2) < (y.first >> 2); });
            txt += std::to_string(chromosome_id + 1) + "\t" + std::to_string(pos[l]) + "\t" + std::to_string(cov) + "\t";
            for (auto &x : e) txt += kIntToChar[x.first & 3];
            txt += '\t';
            for (size_t k = 0; k < e.size(); ++k) txt += (k ? "," : "") + std::to_string(e[k].first >> 2);
            txt += '\t';
            for (size_t k = 0; k < e.size(); ++k) txt += (k ? "," : "") + std::to_string(e[k].second);
            txt += '\n';
        }
        if (bin.size() > (16u << 20)) {
            fwrite(bin.data(), 1, bin.size(), fb);
            bin.clear();
        }
        if (txt.size() > (16u << 20)) {
            fwrite(txt.data(), 1, txt.size(), ft);
            txt.clear();
        }
    }
    fwrite(bin.data(), 1, bin.size(), fb);
    fwrite(txt.data(), 1, txt.size(), ft);
    const bool ok = fclose(fb) == 0;
    return (fclose(ft) == 0 && ok) ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, "Could not write " + prefix);
}

int run(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids, uint32_t n_chr,
        const char *out_pileup, bool text, const Params &base, uint32_t num_threads, const uint16_t *id_to_group,
        uint32_t n_ids, secedo_bam_result_info *info, secedo_bam_times *times) {
    const Clock::time_point t_all = Clock::now();
    secedo_bam_times tl{};
    if (!info || (n_files && !bam_files) || (n_chr && !chromosome_ids))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (n_files > SECEDO_BAM_MAX_FILES)
        return fail(SECEDO_E_LIMIT, "more than 16384 BAM files: cell ids do not fit cell << 2 | base in 16 bits");
    std::vector<std::string> files;
    for (uint32_t f = 0; f < n_files; ++f) {
        if (!bam_files[f]) return fail(SECEDO_E_INVALID_ARG, "null file name");
        files.emplace_back(bam_files[f]);
    }
    delete g_result;
    g_result = new Result();
    Result *res = g_result;
    std::vector<ChrInput> chrs(n_chr);
    for (uint32_t c = 0; c < n_chr; ++c) chrs[c].chromosome = chromosome_ids[c];
    BAM_CALL(load_inputs(files, num_threads ? num_threads : 1, &chrs, &tl));
    hipStream_t s;
    BAM_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } guard{s};
    Dev<uint16_t> d_i2g;
    if (id_to_group) {
        BAM_TRY(d_i2g.alloc(n_ids));
        if (n_ids) BAM_TRY(hipMemcpy(d_i2g.p, id_to_group, n_ids * 2ull, hipMemcpyHostToDevice));
    }
    BAM_TRY(res->off.grow(1, 0, s));
    BAM_TRY(hipMemsetAsync(res->off.p, 0, 8, s));
    for (uint32_t c = 0; c < n_chr; ++c) {
        Params p = base;
        p.chromosome = chromosome_ids[c];
        ChrOut co;
        const uint64_t l0 = res->n_loci, e0 = res->n_entries;
        BAM_CALL(run_chromosome(chrs[c], p, id_to_group ? d_i2g.p : nullptr, n_ids, out_pileup != nullptr, s, res,
                                &co, &tl));
        res->chr_locus_off.push_back(uint32_t(res->n_loci));
        if (out_pileup) {
            const Clock::time_point t0 = Clock::now();
            const uint64_t nl = res->n_loci - l0, ne = res->n_entries - e0;
            std::vector<uint32_t> pos(nl), rid(ne);
            std::vector<uint64_t> off(nl + 1);
            std::vector<uint16_t> idb(ne);
            if (nl) {
                BAM_TRY(hipMemcpy(pos.data(), res->pos.p + l0, nl * 4, hipMemcpyDeviceToHost));
                BAM_TRY(hipMemcpy(off.data(), res->off.p + l0, (nl + 1) * 8, hipMemcpyDeviceToHost));
                BAM_TRY(hipMemcpy(rid.data(), res->rid.p + e0, ne * 4, hipMemcpyDeviceToHost));
                BAM_TRY(hipMemcpy(idb.data(), res->idb.p + e0, ne * 2, hipMemcpyDeviceToHost));
                for (auto &o : off) o -= e0;
            }
            BAM_CALL(write_files(out_pileup, text, chromosome_ids[c], chrs[c], co, pos, off, rid, idb));
            tl.write_ms += ms_since(t0);
        }
        std::vector<uint8_t>().swap(chrs[c].bytes);
    }
    info->n_loci = res->n_loci;
    info->n_entries = res->n_entries;
    info->n_chr = n_chr;
    info->num_cells = res->num_cells;
    info->max_read_length = res->max_read_length;
    info->reserved = 0;
    tl.total_ms = ms_since(t_all);
    if (times) *times = tl;
    return SECEDO_OK;
}

Params make_params(uint32_t max_coverage, uint32_t min_base_quality, uint32_t min_map_quality,
                   uint32_t min_alignment_score, uint16_t min_different) {
    Params p{};
    p.max_coverage = max_coverage;
    p.min_base_quality = min_base_quality;
    p.min_map_quality = min_map_quality;
    p.min_alignment_score = min_alignment_score;
    p.min_different = min_different;
    return p;
}

}  // namespace

extern "C" {

const char *secedo_bam_last_error(void) { return g_error.c_str(); }

int secedo_bam_scan(const char *path, uint32_t num_threads, secedo_bam_scan_info *info, uint64_t *records_per_ref,
                    uint32_t capacity) {
    if (!path || !info) return fail(SECEDO_E_INVALID_ARG, "null argument");
    std::vector<Inflated> inf;
    BAM_CALL(inflate_files({std::string(path)}, num_threads ? num_threads : 1, &inf));
    Header h;
    BAM_CALL(parse_header(inf[0], &h));
    std::vector<uint64_t> per(h.n_ref, 0);
    uint64_t n = 0, unmapped = 0;
    int sorted = 1;
    int rc = walk_records(inf[0], h, &n, [&](uint64_t, uint64_t, int32_t ref, int32_t) {
        if (ref < 0) ++unmapped;
        else if (uint32_t(ref) < h.n_ref) ++per[ref];
        return SECEDO_OK;
    });
    if (rc != SECEDO_OK) {
        if (g_error.find("not coordinate-sorted") == std::string::npos) return rc;
        sorted = 0;  // count again without the order check
        n = 0;
        unmapped = 0;
        std::fill(per.begin(), per.end(), 0);
        const std::vector<uint8_t> &d = inf[0].data;
        for (uint64_t o = h.first_record; o < d.size(); ++n) {
            const uint32_t bs = d.size() - o >= 36 ? rd32(&d[o]) : 0;
            if (bs < 32 || bs > d.size() - o - 4)
                return fail(SECEDO_E_INVALID_ARG, std::string(path) + ": record " + std::to_string(n) + " is truncated");
            const int32_t ref = int32_t(rd32(&d[o + 4]));
            if (ref < 0) ++unmapped;
            else if (uint32_t(ref) < h.n_ref) ++per[ref];
            o += 4 + uint64_t(bs);
        }
    }
    info->n_ref = h.n_ref;
    info->sorted = uint32_t(sorted);
    info->n_records = n;
    info->n_unmapped = unmapped;
    info->n_blocks = inf[0].n_blocks;
    info->inflated_bytes = inf[0].data.size();
    info->l_text = h.l_text;
    info->reserved = 0;
    if (records_per_ref)
        for (uint32_t r = 0; r < std::min(capacity, h.n_ref); ++r) records_per_ref[r] = per[r];
    return SECEDO_OK;
}

int secedo_pileup_bams(const char *const *bam_files, uint32_t n_files, const char *out_pileup, int write_text_file,
                       uint32_t chromosome_id, uint32_t max_coverage, uint32_t min_base_quality,
                       uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                       uint16_t min_different, secedo_bam_result_info *info, secedo_bam_times *times) {
    const Params p = make_params(max_coverage, min_base_quality, min_map_quality, min_alignment_score, min_different);
    return run(bam_files, n_files, &chromosome_id, 1, out_pileup, write_text_file != 0, p, num_threads, nullptr, 0,
               info, times);
}

int secedo_pileup_bams_device(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                              uint32_t n_chr, uint32_t max_coverage, uint32_t min_base_quality,
                              uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                              uint16_t min_different, const uint16_t *id_to_group, uint32_t n_ids,
                              secedo_bam_result_info *info, secedo_bam_times *times) {
    const Params p = make_params(max_coverage, min_base_quality, min_map_quality, min_alignment_score, min_different);
    return run(bam_files, n_files, chromosome_ids, n_chr, nullptr, false, p, num_threads, id_to_group, n_ids, info,
               times);
}

int secedo_bam_fetch(uint32_t *chr_locus_off, uint32_t *locus_pos, uint64_t *locus_entry_off, uint32_t *read_ids,
                     uint16_t *id_base16) {
    const Result *r = g_result;
    if (!r) return fail(SECEDO_E_STATE, "no pileup_bams result on this thread");
    if (chr_locus_off)
        BAM_TRY(hipMemcpy(chr_locus_off, r->chr_locus_off.data(), r->chr_locus_off.size() * 4, hipMemcpyDefault));
    if (locus_pos && r->n_loci) BAM_TRY(hipMemcpy(locus_pos, r->pos.p, r->n_loci * 4, hipMemcpyDefault));
    if (locus_entry_off) BAM_TRY(hipMemcpy(locus_entry_off, r->off.p, (r->n_loci + 1) * 8, hipMemcpyDefault));
    if (read_ids && r->n_entries) BAM_TRY(hipMemcpy(read_ids, r->rid.p, r->n_entries * 4, hipMemcpyDefault));
    if (id_base16 && r->n_entries) BAM_TRY(hipMemcpy(id_base16, r->idb.p, r->n_entries * 2, hipMemcpyDefault));
    return SECEDO_OK;
}

void secedo_bam_release(void) {
    delete g_result;
    g_result = nullptr;
}

}  // extern "C"
