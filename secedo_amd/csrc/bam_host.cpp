// bam_host.cpp -- host side of include/secedo_bam.h: BGZF inflate, BAM header and record walk, the global record
// order, the launches of bam_kernels.hip and the .bin / .map / .txt files of the reference's pileup_bams()
// (pileup.cpp:235-348).
//
// Each file is memory-mapped; its BGZF blocks (BSIZE from the BC extra field) are inflated with zlib raw inflate
// in a pool of at most 16 threads, CRC32 and ISIZE checked. Files are inflated in batches of about 512 MiB of
// inflated data (SECEDO_BAM_BATCH_BYTES overrides it); a file alone in its batch is inflated and walked in ranges
// of BGZF blocks of that size, a record cut at a range's end carried into the next, so one large multiplexed BAM
// never sits inflated in RAM. Of each file only the byte run of the requested chromosomes' records is kept. No .bai
// is needed: the run is found by walking block_size, so with or without an index the result is the same.
//
// Tag mode (secedo_pileup_bams_cells) uploads the chromosome's records in input order and builds the global order
// on the device (bam_kernels.hip rule 3b); secedo_bam_barcodes counts the distinct tag values.
#include "secedo_bam.h"
#include "secedo_simmat.h"
#include "bam_kernels.hpp"
#include "sam_kernels.hpp"

#include <hip/hip_runtime.h>
#include <zlib.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
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

// inflated bytes per batch of files and per block range of one file; SECEDO_BAM_BATCH_BYTES overrides it (tests:
// outputs do not depend on it), read at every call
uint64_t batch_bytes() {
    const char *e = std::getenv("SECEDO_BAM_BATCH_BYTES");
    if (e && *e) {
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v > 0) return v;
    }
    return kBatchBytes;
}

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

constexpr int kNeedMore = 1;  // parse_header / walk_range: the bytes end inside the header or a record

// final: d ends the file, so a cut header is an error; else kNeedMore
int parse_header(const std::string &path, const uint8_t *d, uint64_t n, bool final, Header *h) {
    if ((n >= 4 && std::memcmp(d, "BAM\1", 4) != 0) || (final && n < 12))
        return fail(SECEDO_E_INVALID_ARG, path + ": not a BAM file (magic)");
    if (n < 12) return kNeedMore;
    h->l_text = rd32(d + 4);
    uint64_t o = 8 + uint64_t(h->l_text);
    if (o + 4 > n) return final ? fail(SECEDO_E_INVALID_ARG, path + ": truncated header") : kNeedMore;
    h->n_ref = rd32(d + o);
    o += 4;
    for (uint32_t r = 0; r < h->n_ref; ++r) {
        if (o + 4 > n) return final ? fail(SECEDO_E_INVALID_ARG, path + ": truncated reference list") : kNeedMore;
        o += 4 + uint64_t(rd32(d + o));
        if (o + 4 > n) return final ? fail(SECEDO_E_INVALID_ARG, path + ": truncated reference list") : kNeedMore;
        o += 4;
    }
    h->first_record = o;
    return SECEDO_OK;
}

int parse_header(const Inflated &f, Header *h) {
    return parse_header(f.path, f.data.data(), f.data.size(), true, h);
}

// The record walk of one file, carried across its block ranges.
struct WalkState {
    bool have_header = false;
    Header h;
    uint64_t idx = 0;
    int64_t prev_ref = -1, prev_pos = 0;
};

// Walks the header (first) and the complete records of d[0, n), the file's inflated bytes that follow what earlier
// calls consumed; *used = bytes consumed, the rest starts the next range. final: d ends the file, so a cut record is
// an error. Structure and sortedness checked; on_record(index, record, refID, pos).
template <class F>
int walk_range(const std::string &path, const uint8_t *d, uint64_t n, bool final, WalkState *st, uint64_t *used,
               F on_record) {
    uint64_t o = 0;
    *used = 0;
    if (!st->have_header) {
        const int rc = parse_header(path, d, n, final, &st->h);
        if (rc == kNeedMore) return SECEDO_OK;
        BAM_CALL(rc);
        st->have_header = true;
        o = st->h.first_record;
    }
    for (;; ++st->idx) {
        *used = o;
        if (o >= n) return SECEDO_OK;
        const std::string where = path + ": record " + std::to_string(st->idx);
        if (n - o < 4 + 32) return final ? fail(SECEDO_E_INVALID_ARG, where + " is truncated") : SECEDO_OK;
        const uint32_t bs = rd32(d + o);
        const uint8_t *c = d + o + 4;
        if (bs < 32) return fail(SECEDO_E_INVALID_ARG, where + " has a bad block_size");
        if (bs > n - o - 4) return final ? fail(SECEDO_E_INVALID_ARG, where + " has a bad block_size") : SECEDO_OK;
        const uint64_t need = 32 + uint64_t(c[8]) + 4ull * rd16(c + 12) + (uint64_t(rd32(c + 16)) + 1) / 2 +
                              uint64_t(rd32(c + 16));
        if (need > bs) return fail(SECEDO_E_INVALID_ARG, where + " is longer than its block_size");
        const int32_t ref = int32_t(rd32(c)), pos = int32_t(rd32(c + 4));
        const int64_t key_ref = ref < 0 ? INT64_MAX : ref;
        if (st->idx > 0 && (key_ref < st->prev_ref || (key_ref == st->prev_ref && ref >= 0 && pos < st->prev_pos)))
            return fail(SECEDO_E_INVALID_ARG, where + ": input is not coordinate-sorted");
        st->prev_ref = key_ref;
        st->prev_pos = pos;
        BAM_CALL(on_record(st->idx, d + o, ref, pos));
        o += 4 + uint64_t(bs);
    }
}

// One pass over the records of a whole inflated file.
template <class F>
int walk_records(const Inflated &f, const Header &h, uint64_t *n_records, F on_record) {
    WalkState st;
    st.have_header = true;
    st.h = h;
    uint64_t used = 0;
    BAM_CALL(walk_range(f.path, f.data.data() + h.first_record, f.data.size() - h.first_record, true, &st, &used,
                        on_record));
    *n_records = st.idx;
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

// The value of the first aux field named by the tag, which the device's census found Z-typed (FindTag's walk).
std::string first_z_value(const uint8_t *p, uint64_t len, const char *tag) {
    uint64_t o = 0;
    while (o + 3 <= len) {
        const uint8_t type = p[o + 2];
        o += 3;
        if (p[o - 3] == uint8_t(tag[0]) && p[o - 2] == uint8_t(tag[1])) {
            const uint64_t b = o;
            while (o < len && p[o]) ++o;
            return std::string(reinterpret_cast<const char *>(p + b), o - b);
        }
        uint64_t skip = 0;
        switch (type) {
            case 'A': case 'c': case 'C': skip = 1; break;
            case 's': case 'S': skip = 2; break;
            case 'f': case 'i': case 'I': skip = 4; break;
            case 'Z': case 'H': while (o + skip < len && p[o + skip]) ++skip; ++skip; break;
            case 'B': {
                const uint8_t at = p[o];
                const uint64_t es = (at == 'c' || at == 'C') ? 1 : (at == 's' || at == 'S') ? 2 : 4;
                skip = 5 + uint64_t(rd32(p + o + 1)) * es;
                break;
            }
            default: return std::string();
        }
        o += skip;
    }
    return std::string();
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

// the chromosome's records of every file, in the global order
struct ChrInput {
    uint32_t chromosome;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> file_base;          // [n_files] start of each file's run in bytes
    std::vector<std::vector<uint64_t>> roff;  // per file: record offsets (relative to its run)
    std::vector<std::vector<int32_t>> rpos;
    std::vector<std::vector<uint64_t>> ridx;  // record index in the file (messages)
    std::vector<std::string> paths;            // [n_files] (messages)
    std::vector<uint64_t> line0;               // [n_files] SAM: the line of record 0 (1-based); BAM: 0
};

// where a record is, for messages: "path: record k" (BAM), "file f (path), line l" (SAM)
std::string record_where(const std::string &path, size_t f, uint64_t line0, uint64_t idx) {
    if (!line0) return path + ": record " + std::to_string(idx);
    return "file " + std::to_string(f) + " (" + path + "), line " + std::to_string(line0 + idx);
}

// Per file: its records of each requested chromosome, appended as the walk meets them (one range after another).
struct FileSink {
    const std::string &path;
    size_t f;
    std::vector<ChrInput> &chrs;
    std::vector<std::vector<uint8_t> *> runs;  // [chr] this file's run
    std::vector<int> started, done;
    uint64_t line0 = 0;  // SAM: the line of record 0
    FileSink(const std::string &p, size_t file, std::vector<ChrInput> &c, std::vector<std::vector<std::vector<uint8_t>>> &r)
        : path(p), f(file), chrs(c), runs(c.size()), started(c.size(), 0), done(c.size(), 0) {
        for (size_t k = 0; k < c.size(); ++k) runs[k] = &r[k][file];
    }
    int operator()(uint64_t idx, const uint8_t *rec, int32_t ref, int32_t pos) {
        for (size_t c = 0; c < chrs.size(); ++c) {
            ChrInput &ci = chrs[c];
            if (done[c]) continue;
            if (ref < 0 || uint32_t(ref) != ci.chromosome) {
                if (started[c]) done[c] = 1;  // the reader stops at another RefID
                continue;
            }
            const std::string where = record_where(path, f, line0, idx);
            if (pos < 0) return fail(SECEDO_E_INVALID_ARG, where + " has a negative position");
            BAM_CALL(check_cigar(rec, where));
            started[c] = 1;
            std::vector<uint8_t> &run = *runs[c];
            ci.roff[f].push_back(run.size());
            ci.rpos[f].push_back(pos);
            ci.ridx[f].push_back(idx);
            run.insert(run.end(), rec, rec + 4 + rd32(rec));
        }
        return SECEDO_OK;
    }
};

// One file larger than a batch, inflated and walked in ranges of BGZF blocks of about `batch` inflated bytes; a
// record cut at a range's end is carried to the front of the next range. Host memory: one range plus the runs kept.
int load_file_ranges(const std::string &path, size_t f, uint32_t threads, uint64_t batch, std::vector<ChrInput> *chrs,
                     std::vector<std::vector<std::vector<uint8_t>>> *runs, secedo_bam_times *t) {
    Mapped m;
    BAM_CALL(map_file(path, &m));
    std::vector<Block> blocks;
    uint64_t total = 0;
    BAM_CALL(list_blocks(path, m, &blocks, &total));
    WalkState st;
    FileSink sink(path, f, *chrs, *runs);
    std::vector<uint8_t> buf;
    uint64_t carry = 0;
    size_t b0 = 0;
    do {
        size_t b1 = b0;
        uint64_t bytes = 0;
        while (b1 < blocks.size() && (b1 == b0 || bytes + blocks[b1].isize <= batch)) bytes += blocks[b1++].isize;
        Clock::time_point t0 = Clock::now();
        buf.resize(carry + bytes);
        std::vector<std::string> errs(b1 - b0);
        const uint64_t out0 = b1 > b0 ? blocks[b0].out : 0;
        parallel_for(threads, b1 - b0, [&](uint64_t k) {
            const Block &b = blocks[b0 + k];
            errs[k] = inflate_block(b, buf.data() + carry + (b.out - out0));
        });
        for (size_t k = 0; k < errs.size(); ++k)
            if (!errs[k].empty())
                return fail(SECEDO_E_INVALID_ARG, path + ": BGZF block " + std::to_string(b0 + k) + ": " + errs[k]);
        if (t) {
            t->inflate_ms += ms_since(t0);
            t->inflated_bytes += double(bytes);
        }
        t0 = Clock::now();
        uint64_t used = 0;
        BAM_CALL(walk_range(path, buf.data(), buf.size(), b1 == blocks.size(), &st, &used, sink));
        carry = buf.size() - used;
        if (used) std::memmove(buf.data(), buf.data() + used, carry);
        buf.resize(carry);
        if (t) t->walk_ms += ms_since(t0);
        b0 = b1;
    } while (b0 < blocks.size());
    return SECEDO_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// SAM text input: the header is parsed here, the alignment lines on the device (sam_kernels.hip) into the BAM records
// the walk above collects. The file type comes from its first bytes: BGZF is BAM, plain gzip is refused, anything
// else is SAM.

// *sam = the file is SAM text; plain gzip (no BGZF extra field) is an error
int sniff(const std::string &path, bool *sam) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return fail(SECEDO_E_INVALID_ARG, "Could not open " + path);
    uint8_t b[512];
    const ssize_t n = pread(fd, b, sizeof(b), 0);
    close(fd);
    if (n < 0) return fail(SECEDO_E_INVALID_ARG, "Could not read " + path);
    *sam = !(n >= 2 && b[0] == 31 && b[1] == 139);
    if (*sam) return SECEDO_OK;
    bool bgzf = false;
    if (n >= 12 && b[2] == 8 && (b[3] & 4)) {
        const uint32_t end = std::min<uint32_t>(12 + rd16(b + 10), uint32_t(n));
        for (uint32_t x = 12; x + 4 <= end; x += 4 + rd16(b + x + 2))
            if (b[x] == 'B' && b[x + 1] == 'C') bgzf = true;
    }
    if (!bgzf)
        return fail(SECEDO_E_INVALID_ARG, path + ": a gzip file that is not BGZF; decompress it to SAM or convert "
                                                 "it to BAM (samtools view -b)");
    return SECEDO_OK;
}

struct SamHeader {
    std::vector<std::string> names;  // @SQ SN values by RefID
    uint64_t lines = 0, body = 0;    // header lines, byte offset of the first alignment line
};

// the leading '@' lines: @SQ SN and LN required, SN unique
int parse_sam_header(const std::string &path, size_t f, const Mapped &m, SamHeader *h) {
    std::set<std::string> seen;
    uint64_t o = 0;
    while (o < m.n && m.p[o] == '@') {
        const uint8_t *nl = static_cast<const uint8_t *>(std::memchr(m.p + o, '\n', m.n - o));
        const uint64_t e = nl ? uint64_t(nl - m.p) : m.n;
        ++h->lines;
        const std::string line(reinterpret_cast<const char *>(m.p + o), e - o);
        o = nl ? e + 1 : m.n;
        if (line.compare(0, 3, "@SQ") != 0 || (line.size() > 3 && line[3] != '\t')) continue;
        const std::string where = "file " + std::to_string(f) + " (" + path + "), line " + std::to_string(h->lines);
        std::string sn;
        bool has_sn = false, has_ln = false;
        for (size_t a = 4; a <= line.size();) {
            size_t b = line.find('\t', a);
            if (b == std::string::npos) b = line.size();
            const std::string fld = line.substr(a, b - a);
            if (fld.compare(0, 3, "SN:") == 0 && !has_sn) {
                sn = fld.substr(3);
                has_sn = true;
            } else if (fld.compare(0, 3, "LN:") == 0 && !has_ln) {
                const std::string v = fld.substr(3);
                if (v.empty() || v.size() > 10 || v.find_first_not_of("0123456789") != std::string::npos ||
                    std::stoull(v) < 1 || std::stoull(v) > 2147483647ull)
                    return fail(SECEDO_E_INVALID_ARG, where + ": @SQ LN is not an integer in [1, 2^31 - 1]");
                has_ln = true;
            }
            a = b + 1;
        }
        if (!has_sn || !has_ln) return fail(SECEDO_E_INVALID_ARG, where + ": @SQ without SN or LN");
        if (!seen.insert(sn).second) return fail(SECEDO_E_INVALID_ARG, where + ": @SQ SN:" + sn + " is listed twice");
        h->names.push_back(sn);
    }
    h->body = o;
    return SECEDO_OK;
}

// device buffers of the SAM passes, kept over the ranges and files of one call
struct SamWork {
    hipStream_t s = nullptr;
    Dev<uint8_t> text, out, names, sel, tmp;
    Dev<uint32_t> cnt, scan, start, name_off, name_id;
    Dev<uint64_t> name_hash, size, off;
    Dev<int32_t> ref, pos;
    Dev<unsigned long long> err;
    std::vector<uint8_t> h_text, h_out;
    std::vector<int32_t> h_ref, h_pos;
    ~SamWork() {
        if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
    }
};

const char *sam_what(uint32_t code) {
    static const char *what[kSamCodes] = {
        "",
        "does not have 11 non-empty tab-separated mandatory fields",
        "has a QNAME longer than 254 characters",
        "has a FLAG that is not an integer in [0, 65535]",
        "has an RNAME that no @SQ line names",
        "has a POS that is not an integer in [0, 2^31 - 1]",
        "has a MAPQ that is not an integer in [0, 255]",
        "has a malformed CIGAR",
        "has an RNEXT that is not '*', '=' or an @SQ name",
        "has a PNEXT that is not an integer in [0, 2^31 - 1]",
        "has a TLEN that is not an integer in [-(2^31 - 1), 2^31 - 1]",
        "has a QUAL that is not '*', not as long as SEQ or not in '!'..'~'",
        "has CIGAR and SEQ lengths that differ",
        "has a malformed optional field",
        "is a header line after the first alignment line",
        "is empty",
        "has more than 65535 CIGAR ops",
        "gives a record of 2^31 bytes or more",
    };
    return code < kSamCodes ? what[code] : "?";
}

// One SAM file: header on the host, then ranges of about `batch` bytes ending at a '\n', each uploaded, parsed on the
// device, and its records of the requested chromosomes downloaded into the file's runs (FileSink, as a BAM's walk).
int load_sam_file(const std::string &path, size_t f, uint64_t batch, SamWork *w, std::vector<ChrInput> *chrs,
                  std::vector<std::vector<std::vector<uint8_t>>> *runs, secedo_bam_times *t) {
    Clock::time_point t0 = Clock::now();
    Mapped m;
    BAM_CALL(map_file(path, &m));
    SamHeader h;
    BAM_CALL(parse_sam_header(path, f, m, &h));
    const uint64_t line0 = h.lines + 1;
    for (auto &ci : *chrs) ci.line0[f] = line0;
    if (t) t->inflate_ms += ms_since(t0);
    t0 = Clock::now();
    if (!w->s) BAM_TRY(hipStreamCreateWithFlags(&w->s, hipStreamNonBlocking));
    hipStream_t s = w->s;
    // the @SQ names: packed, hashed and sorted here; the selected RefIDs
    const uint32_t n_ref = uint32_t(h.names.size());
    std::vector<uint8_t> names, sel(std::max<uint32_t>(n_ref, 1), 0);
    std::vector<uint32_t> name_off{0}, name_id(n_ref);
    std::vector<std::pair<uint64_t, uint32_t>> hs(n_ref);
    for (uint32_t r = 0; r < n_ref; ++r) {
        names.insert(names.end(), h.names[r].begin(), h.names[r].end());
        name_off.push_back(uint32_t(names.size()));
        hs[r] = {sam_name_hash(reinterpret_cast<const uint8_t *>(h.names[r].data()), uint32_t(h.names[r].size())),
                 r};
    }
    std::sort(hs.begin(), hs.end());
    std::vector<uint64_t> name_hash(n_ref);
    for (uint32_t r = 0; r < n_ref; ++r) name_hash[r] = hs[r].first, name_id[r] = hs[r].second;
    for (const auto &ci : *chrs)
        if (ci.chromosome < n_ref) sel[ci.chromosome] = 1;
    BAM_TRY(w->names.grow(names.size(), 0, s));
    BAM_TRY(w->name_off.grow(n_ref + 1, 0, s));
    BAM_TRY(w->name_hash.grow(n_ref, 0, s));
    BAM_TRY(w->name_id.grow(n_ref, 0, s));
    BAM_TRY(w->sel.grow(sel.size(), 0, s));
    BAM_TRY(w->err.grow(1, 0, s));
    if (!names.empty()) BAM_TRY(hipMemcpyAsync(w->names.p, names.data(), names.size(), hipMemcpyHostToDevice, s));
    BAM_TRY(hipMemcpyAsync(w->name_off.p, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice, s));
    if (n_ref) {
        BAM_TRY(hipMemcpyAsync(w->name_hash.p, name_hash.data(), n_ref * 8ull, hipMemcpyHostToDevice, s));
        BAM_TRY(hipMemcpyAsync(w->name_id.p, name_id.data(), n_ref * 4ull, hipMemcpyHostToDevice, s));
    }
    BAM_TRY(hipMemcpyAsync(w->sel.p, sel.data(), sel.size(), hipMemcpyHostToDevice, s));
    const SamRefs refs{w->names.p, w->name_off.p, w->name_hash.p, w->name_id.p, w->sel.p, n_ref};
    if (t) t->upload_ms += ms_since(t0);

    FileSink sink(path, f, *chrs, *runs);
    sink.line0 = line0;
    bool have_prev = false;
    int64_t prev_ref = -1, prev_pos = 0;
    uint64_t line_base = 0;  // lines of the body before the range
    for (uint64_t r0 = h.body; r0 < m.n;) {
        uint64_t r1 = std::min<uint64_t>(m.n, r0 + std::max<uint64_t>(batch, 1));
        if (r1 < m.n) {
            const uint8_t *nl = static_cast<const uint8_t *>(std::memchr(m.p + r1 - 1, '\n', m.n - (r1 - 1)));
            r1 = nl ? uint64_t(nl - m.p) + 1 : m.n;
        }
        const uint64_t len = r1 - r0;
        if (len >= (1ull << 32) - 64)
            return fail(SECEDO_E_LIMIT, "file " + std::to_string(f) + " (" + path +
                                            "): a range of SAM lines of 4 GiB or more (a line that long)");
        const bool ends_file = r1 == m.n, trailing = m.p[r1 - 1] == '\n';
        // text read
        t0 = Clock::now();
        w->h_text.assign(m.p + r0, m.p + r1);
        if (t) {
            t->inflate_ms += ms_since(t0);
            t->inflated_bytes += double(len);
        }
        // upload, zero-padded to whole 16-byte vectors plus one
        t0 = Clock::now();
        const uint64_t n16 = (len + 15) / 16, padded = n16 * 16 + 16;
        BAM_TRY(w->text.grow(padded, 0, s));
        BAM_TRY(hipMemcpyAsync(w->text.p, w->h_text.data(), len, hipMemcpyHostToDevice, s));
        BAM_TRY(hipMemsetAsync(w->text.p + len, 0, padded - len, s));
        BAM_TRY(hipStreamSynchronize(s));
        if (t) t->upload_ms += ms_since(t0);
        // device parse
        t0 = Clock::now();
        BAM_TRY(w->cnt.grow(n16 + 1, 0, s));
        BAM_TRY(w->scan.grow(n16 + 1, 0, s));
        size_t tb = scan_bytes(n16 + 1);
        BAM_TRY(w->tmp.grow(tb, 0, s));
        BAM_TRY(sam_newline_count(w->text.p, n16, w->cnt.p, s));
        BAM_TRY(hipMemsetAsync(w->cnt.p + n16, 0, 4, s));
        BAM_TRY(exclusive_sum(w->tmp.p, tb, w->cnt.p, w->scan.p, n16 + 1, s));
        uint32_t n_nl = 0;
        BAM_TRY(hipMemcpyAsync(&n_nl, w->scan.p + n16, 4, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipStreamSynchronize(s));
        const uint32_t n_lines = n_nl + (trailing ? 0 : 1);
        BAM_TRY(w->start.grow(uint64_t(n_lines) + 1, 0, s));
        BAM_TRY(w->size.grow(uint64_t(n_lines) + 1, 0, s));
        BAM_TRY(w->off.grow(uint64_t(n_lines) + 1, 0, s));
        BAM_TRY(w->ref.grow(n_lines, 0, s));
        BAM_TRY(w->pos.grow(n_lines, 0, s));
        BAM_TRY(sam_line_starts(w->text.p, n16, w->scan.p, n_lines, uint32_t(len), !trailing, w->start.p, s));
        BAM_TRY(hipMemsetAsync(w->err.p, 0xFF, 8, s));
        BAM_TRY(sam_size(w->text.p, w->start.p, n_lines, line_base, ends_file, refs, w->size.p, w->ref.p, w->pos.p,
                         w->err.p, s));
        BAM_TRY(hipMemsetAsync(w->size.p + n_lines, 0, 8, s));
        tb = scan_bytes(uint64_t(n_lines) + 1);
        BAM_TRY(w->tmp.grow(tb, 0, s));
        BAM_TRY(exclusive_sum64(w->tmp.p, tb, w->size.p, w->off.p, uint64_t(n_lines) + 1, s));
        uint64_t total = 0;
        unsigned long long err = 0;
        BAM_TRY(hipMemcpyAsync(&total, w->off.p + n_lines, 8, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipMemcpyAsync(&err, w->err.p, 8, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipStreamSynchronize(s));
        // lines below the first bad one are encoded and walked: a structural error there comes first
        const uint32_t limit = err == ~0ull ? n_lines : uint32_t((err >> 8) - line_base);
        BAM_TRY(w->out.grow(total, 0, s));
        BAM_TRY(sam_encode(w->text.p, w->start.p, limit, refs, w->off.p, w->out.p, s));
        w->h_ref.resize(limit);
        w->h_pos.resize(limit);
        w->h_out.resize(total);
        if (limit) {
            BAM_TRY(hipMemcpyAsync(w->h_ref.data(), w->ref.p, limit * 4ull, hipMemcpyDeviceToHost, s));
            BAM_TRY(hipMemcpyAsync(w->h_pos.data(), w->pos.p, limit * 4ull, hipMemcpyDeviceToHost, s));
        }
        if (total) BAM_TRY(hipMemcpyAsync(w->h_out.data(), w->out.p, total, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipStreamSynchronize(s));
        // sortedness over every line, the selected records into the runs
        uint64_t o = 0;
        for (uint32_t k = 0; k < limit; ++k) {
            const int32_t ref = w->h_ref[k], pos = w->h_pos[k];
            if (ref == kSamNoRecord) continue;
            const uint64_t idx = line_base + k;
            const int64_t key_ref = ref < 0 ? INT64_MAX : ref;
            if (have_prev && (key_ref < prev_ref || (key_ref == prev_ref && ref >= 0 && pos < prev_pos)))
                return fail(SECEDO_E_INVALID_ARG,
                            record_where(path, f, line0, idx) + ": input is not coordinate-sorted");
            have_prev = true;
            prev_ref = key_ref;
            prev_pos = pos;
            if (ref >= 0 && uint32_t(ref) < n_ref && sel[ref]) {
                const uint8_t *rec = w->h_out.data() + o;
                BAM_CALL(sink(idx, rec, ref, pos));
                o += 4 + uint64_t(rd32(rec));
            }
        }
        if (err != ~0ull) {
            const uint32_t code = uint32_t(err & 0xFF);
            return fail(code == kSamManyOps || code == kSamTooLong ? SECEDO_E_LIMIT : SECEDO_E_INVALID_ARG,
                        record_where(path, f, line0, err >> 8) + " " + sam_what(code));
        }
        if (t) t->walk_ms += ms_since(t0);
        line_base += n_lines;
        r0 = r1;
    }
    return SECEDO_OK;
}

int load_inputs(const std::vector<std::string> &files, uint32_t threads, std::vector<ChrInput> *chrs,
                secedo_bam_times *t) {
    const size_t n_files = files.size();
    const uint64_t batch = batch_bytes();
    for (auto &c : *chrs) {
        c.file_base.assign(n_files, 0);
        c.roff.assign(n_files, {});
        c.rpos.assign(n_files, {});
        c.ridx.assign(n_files, {});
        c.paths = files;
        c.line0.assign(n_files, 0);
    }
    std::vector<char> sam(n_files, 0);
    for (size_t f = 0; f < n_files; ++f) {
        bool is_sam = false;
        BAM_CALL(sniff(files[f], &is_sam));
        sam[f] = is_sam;
    }
    SamWork sam_work;
    std::vector<std::vector<std::vector<uint8_t>>> runs(chrs->size(), std::vector<std::vector<uint8_t>>(n_files));
    size_t f0 = 0;
    while (f0 < n_files) {
        if (sam[f0]) {  // SAM text: parsed on the device in ranges of about `batch` bytes
            BAM_CALL(load_sam_file(files[f0], f0, batch, &sam_work, chrs, &runs, t));
            ++f0;
            continue;
        }
        // a batch of BAM files of at most `batch` bytes on disk (BGZF inflates 3-4x), at least one file
        size_t f1 = f0;
        uint64_t disk = 0;
        while (f1 < n_files && !sam[f1] && (f1 == f0 || disk < batch / 4)) {
            struct stat st;
            disk += stat(files[f1].c_str(), &st) == 0 ? uint64_t(st.st_size) : 0;
            ++f1;
        }
        if (f1 == f0 + 1) {  // one file: walked in block ranges (one range when it inflates to at most `batch`)
            BAM_CALL(load_file_ranges(files[f0], f0, threads, batch, chrs, &runs, t));
            f0 = f1;
            continue;
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
            WalkState st;
            FileSink sink(files[f0 + k], f0 + k, *chrs, runs);
            uint64_t used = 0;
            rcs[k] = walk_range(files[f0 + k], inf[k].data.data(), inf[k].data.size(), true, &st, &used, sink);
            errs[k] = g_error;
            std::vector<uint8_t>().swap(inf[k].data);
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

// The listed barcodes of tag mode on the device: packed values, their hashes sorted, the cell of each.
struct DevCells {
    Dev<uint8_t> bytes;
    Dev<uint32_t> off, cell;
    Dev<uint64_t> hash;
    CellList list{};
};

int upload_cells(const char tag[2], const std::vector<std::string> &values, hipStream_t s, DevCells *dc) {
    const uint32_t n = uint32_t(values.size());
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off{0};
    for (const auto &v : values) {
        bytes.insert(bytes.end(), v.begin(), v.end());
        off.push_back(uint32_t(bytes.size()));
    }
    Dev<uint64_t> h;
    Dev<uint32_t> idx;
    BAM_TRY(dc->bytes.alloc(bytes.size()));
    BAM_TRY(dc->off.alloc(n + 1));
    BAM_TRY(dc->hash.alloc(n));
    BAM_TRY(dc->cell.alloc(n));
    BAM_TRY(h.alloc(n));
    BAM_TRY(idx.alloc(n));
    if (!bytes.empty()) BAM_TRY(hipMemcpyAsync(dc->bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
    BAM_TRY(hipMemcpyAsync(dc->off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    BAM_TRY(list_hash(dc->bytes.p, dc->off.p, n, h.p, idx.p, s));
    const size_t tb = sort_pairs_bytes(n);
    Dev<uint8_t> tmp;
    BAM_TRY(tmp.alloc(tb));
    BAM_TRY(sort_pairs(tmp.p, tb, h.p, dc->hash.p, idx.p, dc->cell.p, n, s));
    BAM_TRY(hipStreamSynchronize(s));
    dc->list = CellList{dc->bytes.p, dc->off.p, dc->hash.p, dc->cell.p, n, uint8_t(tag[0]), uint8_t(tag[1])};
    return SECEDO_OK;
}

// The chromosome's records in input order (file, record): byte offsets in ci.bytes, input file, record index.
void input_order(const ChrInput &ci, std::vector<uint64_t> *off, std::vector<uint32_t> *file,
                 std::vector<uint64_t> *idx) {
    for (size_t f = 0; f < ci.roff.size(); ++f)
        for (size_t k = 0; k < ci.roff[f].size(); ++k) {
            off->push_back(ci.file_base[f] + ci.roff[f][k]);
            if (file) file->push_back(uint32_t(f));
            if (idx) idx->push_back(ci.ridx[f][k]);
        }
}

// Selected (key, input ordinal) pairs of d_key / d_sel (n records), sorted by key: -> *n_sel, d_ks, d_vs.
int compact_and_sort(const Dev<uint64_t> &d_key, Dev<uint32_t> &d_sel, uint32_t n, hipStream_t s, uint32_t *n_sel,
                     Dev<uint64_t> *d_ks, Dev<uint32_t> *d_vs) {
    Dev<uint32_t> scan, vc;
    Dev<uint64_t> kc;
    Dev<uint8_t> tmp;
    size_t tb = scan_bytes(uint64_t(n) + 1);
    BAM_TRY(tmp.alloc(tb));
    BAM_TRY(scan.alloc(n + 1));
    BAM_TRY(hipMemsetAsync(d_sel.p + n, 0, 4, s));
    BAM_TRY(exclusive_sum(tmp.p, tb, d_sel.p, scan.p, uint64_t(n) + 1, s));
    *n_sel = 0;
    BAM_TRY(hipMemcpyAsync(n_sel, scan.p + n, 4, hipMemcpyDeviceToHost, s));
    BAM_TRY(hipStreamSynchronize(s));
    const uint32_t m = *n_sel;
    BAM_TRY(kc.alloc(m));
    BAM_TRY(vc.alloc(m));
    BAM_TRY(d_ks->alloc(m));
    BAM_TRY(d_vs->alloc(m));
    BAM_TRY(compact_keys(d_key.p, d_sel.p, scan.p, n, kc.p, vc.p, s));
    tb = sort_pairs_bytes(m);
    BAM_TRY(tmp.alloc(tb));
    BAM_TRY(sort_pairs(tmp.p, tb, kc.p, d_ks->p, vc.p, d_vs->p, m, s));  // radix sort: stable
    BAM_TRY(hipStreamSynchronize(s));
    return SECEDO_OK;
}

// Where the records of the global order come from, for error messages and the .map.
struct Order {
    uint32_t n = 0, last_chunk = 0;
    int32_t min_pos = INT32_MAX;
    std::vector<uint64_t> ord_off;  // per-file mode: per ordinal byte offset, input file, record index
    std::vector<uint16_t> ord_file;
    std::vector<uint64_t> ord_idx;
    std::vector<uint32_t> in_file;  // tag mode: per input ordinal; d_ord maps an ordinal to its input ordinal
    std::vector<uint64_t> in_idx;
    Dev<uint32_t> d_ord;
};

// Tag mode: the records in input order go up, the device selects the listed cells and sorts them into the global
// order (chunk, cell, Position, file, record) -> d_off / d_cell of the selected records.
int order_by_cell(const ChrInput &ci, const CellList &L, hipStream_t s, Dev<uint8_t> *d_bytes, Dev<uint64_t> *d_off,
                  Dev<uint16_t> *d_cell, Order *ord, secedo_bam_times *t) {
    Clock::time_point t0 = Clock::now();
    std::vector<uint64_t> in_off;
    input_order(ci, &in_off, &ord->in_file, &ord->in_idx);
    if (in_off.size() >= (1ull << 32)) return fail(SECEDO_E_LIMIT, "more than 2^32 records in one chromosome");
    const uint32_t n_in = uint32_t(in_off.size());
    if (t) t->walk_ms += ms_since(t0);
    t0 = Clock::now();
    Dev<uint64_t> d_in_off;
    BAM_TRY(d_bytes->alloc(ci.bytes.size()));
    BAM_TRY(d_in_off.alloc(n_in));
    if (!ci.bytes.empty())
        BAM_TRY(hipMemcpyAsync(d_bytes->p, ci.bytes.data(), ci.bytes.size(), hipMemcpyHostToDevice, s));
    if (n_in) BAM_TRY(hipMemcpyAsync(d_in_off.p, in_off.data(), n_in * 8ull, hipMemcpyHostToDevice, s));
    BAM_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_since(t0);
    t0 = Clock::now();
    Dev<uint64_t> key, ks;
    Dev<uint32_t> sel, vs;
    BAM_TRY(key.alloc(n_in));
    BAM_TRY(sel.alloc(n_in + 1));
    BAM_TRY(cells(d_bytes->p, d_in_off.p, n_in, L, key.p, sel.p, s));
    uint32_t n = 0;
    BAM_CALL(compact_and_sort(key, sel, n_in, s, &n, &ks, &vs));
    key.reset();
    sel.reset();
    BAM_TRY(d_off->alloc(n));
    BAM_TRY(d_cell->alloc(n));
    BAM_TRY(ord->d_ord.alloc(n));
    BAM_TRY(order_records(ks.p, vs.p, d_in_off.p, n, d_off->p, d_cell->p, ord->d_ord.p, s));
    ord->n = n;
    if (n) {
        uint64_t k0 = 0, k1 = 0;
        BAM_TRY(hipMemcpyAsync(&k0, ks.p, 8, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipMemcpyAsync(&k1, ks.p + n - 1, 8, hipMemcpyDeviceToHost, s));
        BAM_TRY(hipStreamSynchronize(s));
        ord->min_pos = int32_t(uint32_t(k0 >> 46) * kChunk);  // the first window starts at or before it
        ord->last_chunk = uint32_t(k1 >> 46);
    }
    BAM_TRY(hipStreamSynchronize(s));
    if (t) t->device_ms += ms_since(t0);
    return SECEDO_OK;
}

// Per-file mode: the global order (chunk of Position, file, record) built on the host, then uploaded.
int order_by_file(const ChrInput &ci, hipStream_t s, Dev<uint8_t> *d_bytes, Dev<uint64_t> *d_off,
                  Dev<uint16_t> *d_file, Order *ord, secedo_bam_times *t) {
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
    std::vector<uint64_t> &ord_off = ord->ord_off;
    std::vector<uint16_t> &ord_file = ord->ord_file;
    std::vector<uint64_t> &ord_idx = ord->ord_idx;
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
    BAM_TRY(d_bytes->alloc(ci.bytes.size()));
    BAM_TRY(d_off->alloc(n));
    BAM_TRY(d_file->alloc(n));
    if (!ci.bytes.empty())
        BAM_TRY(hipMemcpyAsync(d_bytes->p, ci.bytes.data(), ci.bytes.size(), hipMemcpyHostToDevice, s));
    if (n) {
        BAM_TRY(hipMemcpyAsync(d_off->p, ord_off.data(), n * 8ull, hipMemcpyHostToDevice, s));
        BAM_TRY(hipMemcpyAsync(d_file->p, ord_file.data(), n * 2ull, hipMemcpyHostToDevice, s));
    }
    BAM_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_since(t0);
    ord->n = n;
    ord->min_pos = min_pos;
    ord->last_chunk = last_chunk;
    return SECEDO_OK;
}

// The device passes of one chromosome, appended to `res`. cells: tag mode's list, or null for per-file mode.
int run_chromosome(const ChrInput &ci, const Params &prm, const CellList *cells, const uint16_t *d_i2g,
                   uint32_t n_groups, bool want_map, hipStream_t s, Result *res, ChrOut *co, secedo_bam_times *t) {
    Order ord;
    Dev<uint8_t> d_bytes;
    Dev<uint64_t> d_off;
    Dev<uint16_t> d_file;
    if (cells) BAM_CALL(order_by_cell(ci, *cells, s, &d_bytes, &d_off, &d_file, &ord, t));
    else BAM_CALL(order_by_file(ci, s, &d_bytes, &d_off, &d_file, &ord, t));
    const uint32_t n = ord.n, last_chunk = ord.last_chunk;
    const int32_t min_pos = ord.min_pos;
    Clock::time_point t0 = Clock::now();

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
        uint64_t file = 0, idx = 0;
        if (cells) {  // the input file and record of ordinal o
            uint32_t i = 0;
            BAM_TRY(hipMemcpy(&i, ord.d_ord.p + o, 4, hipMemcpyDeviceToHost));
            file = ord.in_file[i];
            idx = ord.in_idx[i];
        } else {
            file = ord.ord_file[o];
            idx = ord.ord_idx[o];
        }
        const std::string where = ci.line0[file] ? record_where(ci.paths[file], file, ci.line0[file], idx)
                                                 : "file " + std::to_string(file) + ", record " + std::to_string(idx);
        return fail(SECEDO_E_INVALID_ARG, where + ": " + (code < 7 ? what[code] : "?"));
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
        if (cells) {
            co->ord_off.resize(n);
            if (n) BAM_TRY(hipMemcpy(co->ord_off.data(), d_off.p, n * 8ull, hipMemcpyDeviceToHost));
        } else {
            co->ord_off = ord.ord_off;
        }
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

// tag: two characters [A-Za-z][A-Za-z0-9] (SAM spec 1.5)
int check_tag(const char *tag) {
    if (!tag) return fail(SECEDO_E_INVALID_ARG, "null tag");
    const auto alpha = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); };
    if (!alpha(tag[0]) || !(alpha(tag[1]) || (tag[1] >= '0' && tag[1] <= '9')))
        return fail(SECEDO_E_INVALID_ARG, "a tag is two characters [A-Za-z][A-Za-z0-9]");
    return SECEDO_OK;
}

// the barcode list of tag mode: non-empty, at most SECEDO_BAM_MAX_FILES, no value twice
int check_cells(const char *tag, const char *const *barcodes, uint32_t n, std::vector<std::string> *values) {
    BAM_CALL(check_tag(tag));
    if (n == 0 || !barcodes) return fail(SECEDO_E_INVALID_ARG, "an empty barcode list");
    if (n > SECEDO_BAM_MAX_FILES)
        return fail(SECEDO_E_LIMIT, "more than 16384 barcodes: cell ids do not fit cell << 2 | base in 16 bits");
    std::set<std::string> seen;
    for (uint32_t c = 0; c < n; ++c) {
        if (!barcodes[c]) return fail(SECEDO_E_INVALID_ARG, "null barcode");
        values->emplace_back(barcodes[c]);
        if (!seen.insert(values->back()).second)
            return fail(SECEDO_E_INVALID_ARG, "barcode " + values->back() + " is listed twice");
    }
    return SECEDO_OK;
}

int check_files(const char *const *bam_files, uint32_t n_files, std::vector<std::string> *files) {
    for (uint32_t f = 0; f < n_files; ++f) {
        if (!bam_files[f]) return fail(SECEDO_E_INVALID_ARG, "null file name");
        files->emplace_back(bam_files[f]);
    }
    return SECEDO_OK;
}

// tag null: per-file mode (cell = file index); else tag mode with the listed barcodes
int run(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids, uint32_t n_chr,
        const char *out_pileup, bool text, const Params &base, uint32_t num_threads, const uint16_t *id_to_group,
        uint32_t n_ids, const char *tag, const char *const *barcodes, uint32_t n_barcodes,
        secedo_bam_result_info *info, secedo_bam_times *times) {
    const Clock::time_point t_all = Clock::now();
    secedo_bam_times tl{};
    if (!info || (n_files && !bam_files) || (n_chr && !chromosome_ids))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    std::vector<std::string> values;
    if (tag) BAM_CALL(check_cells(tag, barcodes, n_barcodes, &values));
    else if (n_files > SECEDO_BAM_MAX_FILES)
        return fail(SECEDO_E_LIMIT, "more than 16384 BAM files: cell ids do not fit cell << 2 | base in 16 bits");
    std::vector<std::string> files;
    BAM_CALL(check_files(bam_files, n_files, &files));
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
    DevCells dc;
    if (tag) BAM_CALL(upload_cells(tag, values, s, &dc));
    BAM_TRY(res->off.grow(1, 0, s));
    BAM_TRY(hipMemsetAsync(res->off.p, 0, 8, s));
    for (uint32_t c = 0; c < n_chr; ++c) {
        Params p = base;
        p.chromosome = chromosome_ids[c];
        ChrOut co;
        const uint64_t l0 = res->n_loci, e0 = res->n_entries;
        BAM_CALL(run_chromosome(chrs[c], p, tag ? &dc.list : nullptr, id_to_group ? d_i2g.p : nullptr, n_ids,
                                out_pileup != nullptr, s, res, &co, &tl));
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

// the distinct tag values over the requested chromosomes, sorted bytewise, and their record counts
struct Barcodes {
    std::vector<std::string> values;
    std::vector<uint64_t> counts;
};

thread_local Barcodes *g_barcodes = nullptr;

// one chromosome's distinct values (device: hash, sort, exact split of equal-hash runs) added to `acc`
int count_values(const ChrInput &ci, const char *tag, hipStream_t s, std::map<std::string, uint64_t> *acc) {
    std::vector<uint64_t> in_off;
    input_order(ci, &in_off, nullptr, nullptr);
    if (in_off.size() >= (1ull << 32)) return fail(SECEDO_E_LIMIT, "more than 2^32 records in one chromosome");
    const uint32_t n_in = uint32_t(in_off.size());
    if (n_in == 0) return SECEDO_OK;
    Dev<uint8_t> d_bytes, tmp;
    Dev<uint64_t> d_in_off, key, ks, voff;
    Dev<uint32_t> sel, vs, run, cnt, vlen;
    BAM_TRY(d_bytes.alloc(ci.bytes.size()));
    BAM_TRY(d_in_off.alloc(n_in));
    BAM_TRY(hipMemcpyAsync(d_bytes.p, ci.bytes.data(), ci.bytes.size(), hipMemcpyHostToDevice, s));
    BAM_TRY(hipMemcpyAsync(d_in_off.p, in_off.data(), n_in * 8ull, hipMemcpyHostToDevice, s));
    BAM_TRY(key.alloc(n_in));
    BAM_TRY(sel.alloc(n_in + 1));
    const uint8_t t0 = uint8_t(tag[0]), t1 = uint8_t(tag[1]);
    BAM_TRY(tag_keys(d_bytes.p, d_in_off.p, n_in, t0, t1, key.p, sel.p, s));
    uint32_t n = 0;
    BAM_CALL(compact_and_sort(key, sel, n_in, s, &n, &ks, &vs));
    if (n == 0) return SECEDO_OK;
    const size_t tb = scan_bytes(n);
    BAM_TRY(tmp.alloc(tb));
    BAM_TRY(run.alloc(n));
    BAM_TRY(cnt.alloc(n));
    BAM_TRY(hipMemsetAsync(cnt.p, 0, n * 4ull, s));
    BAM_TRY(tag_count(d_bytes.p, d_in_off.p, t0, t1, ks.p, vs.p, run.p, n, cnt.p, tmp.p, tb, s));
    std::vector<uint32_t> h_cnt(n), h_val(n);
    BAM_TRY(hipMemcpyAsync(h_cnt.data(), cnt.p, n * 4ull, hipMemcpyDeviceToHost, s));
    BAM_TRY(hipMemcpyAsync(h_val.data(), vs.p, n * 4ull, hipMemcpyDeviceToHost, s));
    BAM_TRY(hipStreamSynchronize(s));
    for (uint32_t j = 0; j < n; ++j) {
        if (!h_cnt[j]) continue;
        // the value of the record that first showed it: the first aux field named by the tag, Z-typed (the device
        // pass found it there)
        const uint8_t *rec = ci.bytes.data() + in_off[h_val[j]];
        const uint32_t bs = rd32(rec);
        const uint8_t *c = rec + 4;
        const uint64_t aux = 32 + uint64_t(c[8]) + 4ull * rd16(c + 12) + (uint64_t(rd32(c + 16)) + 1) / 2 +
                             uint64_t(rd32(c + 16));
        const std::string v = first_z_value(c + aux, bs - aux, tag);
        (*acc)[v] += h_cnt[j];
    }
    return SECEDO_OK;
}

int barcodes(const char *const *bam_files, uint32_t n_files, const char *tag, const uint32_t *chromosome_ids,
             uint32_t n_chr, uint32_t num_threads, uint32_t *n_values, uint64_t *bytes) {
    if (!n_values || !bytes || (n_files && !bam_files) || (n_chr && !chromosome_ids))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    BAM_CALL(check_tag(tag));
    std::vector<std::string> files;
    BAM_CALL(check_files(bam_files, n_files, &files));
    delete g_barcodes;
    g_barcodes = nullptr;
    std::vector<ChrInput> chrs(n_chr);
    for (uint32_t c = 0; c < n_chr; ++c) chrs[c].chromosome = chromosome_ids[c];
    BAM_CALL(load_inputs(files, num_threads ? num_threads : 1, &chrs, nullptr));
    hipStream_t s;
    BAM_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } guard{s};
    std::map<std::string, uint64_t> acc;
    for (uint32_t c = 0; c < n_chr; ++c) {
        BAM_CALL(count_values(chrs[c], tag, s, &acc));
        std::vector<uint8_t>().swap(chrs[c].bytes);
    }
    if (acc.size() > UINT32_MAX) return fail(SECEDO_E_LIMIT, "more than 2^32 distinct values");
    Barcodes *b = new Barcodes();
    uint64_t total = 0;
    for (const auto &kv : acc) {
        b->values.push_back(kv.first);
        b->counts.push_back(kv.second);
        total += kv.first.size();
    }
    g_barcodes = b;
    *n_values = uint32_t(b->values.size());
    *bytes = total;
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
    int rc = walk_records(inf[0], h, &n, [&](uint64_t, const uint8_t *, int32_t ref, int32_t) {
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
               nullptr, nullptr, 0, info, times);
}

int secedo_pileup_bams_device(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                              uint32_t n_chr, uint32_t max_coverage, uint32_t min_base_quality,
                              uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                              uint16_t min_different, const uint16_t *id_to_group, uint32_t n_ids,
                              secedo_bam_result_info *info, secedo_bam_times *times) {
    const Params p = make_params(max_coverage, min_base_quality, min_map_quality, min_alignment_score, min_different);
    return run(bam_files, n_files, chromosome_ids, n_chr, nullptr, false, p, num_threads, id_to_group, n_ids,
               nullptr, nullptr, 0, info, times);
}

int secedo_pileup_bams_cells(const char *const *bam_files, uint32_t n_files, const char *out_pileup,
                             int write_text_file, uint32_t chromosome_id, uint32_t max_coverage,
                             uint32_t min_base_quality, uint32_t min_map_quality, uint32_t min_alignment_score,
                             uint32_t num_threads, uint16_t min_different, const char tag[2],
                             const char *const *barcodes, uint32_t n_barcodes, secedo_bam_result_info *info,
                             secedo_bam_times *times) {
    const Params p = make_params(max_coverage, min_base_quality, min_map_quality, min_alignment_score, min_different);
    if (!tag) return fail(SECEDO_E_INVALID_ARG, "null tag");
    return run(bam_files, n_files, &chromosome_id, 1, out_pileup, write_text_file != 0, p, num_threads, nullptr, 0,
               tag, barcodes, n_barcodes, info, times);
}

int secedo_pileup_bams_cells_device(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                                    uint32_t n_chr, uint32_t max_coverage, uint32_t min_base_quality,
                                    uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                                    uint16_t min_different, const uint16_t *id_to_group, uint32_t n_ids,
                                    const char tag[2], const char *const *barcodes, uint32_t n_barcodes,
                                    secedo_bam_result_info *info, secedo_bam_times *times) {
    const Params p = make_params(max_coverage, min_base_quality, min_map_quality, min_alignment_score, min_different);
    if (!tag) return fail(SECEDO_E_INVALID_ARG, "null tag");
    return run(bam_files, n_files, chromosome_ids, n_chr, nullptr, false, p, num_threads, id_to_group, n_ids, tag,
               barcodes, n_barcodes, info, times);
}

int secedo_bam_barcodes(const char *const *bam_files, uint32_t n_files, const char tag[2],
                        const uint32_t *chromosome_ids, uint32_t n_chr, uint32_t num_threads, uint32_t *n_barcodes,
                        uint64_t *bytes) {
    return barcodes(bam_files, n_files, tag, chromosome_ids, n_chr, num_threads, n_barcodes, bytes);
}

int secedo_bam_barcodes_fetch(char *values, uint64_t *value_off, uint64_t *counts) {
    const Barcodes *b = g_barcodes;
    if (!b) return fail(SECEDO_E_STATE, "no secedo_bam_barcodes result on this thread");
    uint64_t o = 0;
    for (size_t k = 0; k < b->values.size(); ++k) {
        if (values) std::memcpy(values + o, b->values[k].data(), b->values[k].size());
        if (value_off) value_off[k] = o;
        if (counts) counts[k] = b->counts[k];
        o += b->values[k].size();
    }
    if (value_off) value_off[b->values.size()] = o;
    return SECEDO_OK;
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
