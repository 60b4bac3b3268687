// bam_input.cpp -- the input side of include/secedo_bam.h: BGZF inflate, the BAM header and record walk, the SAM
// header and the driver of the device parse (sam_kernels.hip), BGZF-compressed SAM through the device inflate
// (bgzf_kernels.hip), secedo_bgzf_inflate and secedo_bam_scan. Its product is one ChrInput per requested chromosome
// (bam_host.hpp), which bam_pileup.cpp turns into the pileup.
//
// Each file is memory-mapped; its BGZF blocks (BSIZE from the BC extra field) are inflated with zlib raw inflate
// in a pool of at most 16 threads, CRC32 and ISIZE checked. Files are inflated in batches of about 512 MiB of
// inflated data (SECEDO_BAM_BATCH_BYTES overrides it); a file alone in its batch is inflated and walked in ranges
// of BGZF blocks of that size, a record cut at a range's end carried into the next, so one large multiplexed BAM
// never sits inflated in RAM. Of each file only the byte run of the requested chromosomes' records is kept. No .bai
// is needed: the run is found by walking block_size. Where one is asked for (secedo_bam_set_index), bam_index.hpp
// reads it, plan_index below turns it into spans of members, and only those are inflated and walked, on either route;
// with or without an index the result is the same.
// The opt-in device route for BAM (secedo_bam_set_inflate) branches off in load_inputs to bam_device_input.cpp; the
// BGZF listing and the zlib inflate of one block (bgzf_members.hpp) and the header parse below are what the two routes
// share.
#include "bam_host.hpp"
#include "bam_index.hpp"
#include "bam_kernels.hpp"  // the scan wrappers
#include "bgzf_kernels.hpp"
#include "sam_kernels.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <memory>
#include <set>
#include <thread>

// ---- shared with bam_device_input.cpp (declared in bam_host.hpp)
namespace secedo {
namespace bam_host {

namespace {
constexpr uint64_t kBatchBytes = 512ull << 20;
}

uint64_t batch_bytes() { return env_u64("SECEDO_BAM_BATCH_BYTES", kBatchBytes); }

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

int read_block(const std::string &path, const Mapped &m, uint64_t off, Block *blk, uint32_t *len) {
    const std::string why = bm::read_member(m.p, m.n, off, blk, len);
    return why.empty() ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, path + ": " + why);
}

// a file mapped and its BGZF blocks listed; *total = its inflated size
int open_bgzf(const std::string &path, Mapped *m, std::vector<Block> *blocks, uint64_t *total) {
    SECEDO_CALL(map_file(path, m));
    const std::string why = bm::list_members(m->p, m->n, blocks, total);
    return why.empty() ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, path + ": " + why);
}

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

}  // namespace bam_host
}  // namespace secedo

namespace {

using namespace secedo::bam;
using namespace secedo::bam_host;
namespace bamwalk = secedo::bamwalk;

struct InflateJob {
    const std::string *path;
    const uint8_t *file;  // the mapped file
    const Block *block;
    uint64_t index;  // of the block in its file (messages)
    uint8_t *dst;
    bool by_byte = false;  // an indexed file: the ordinal is unknown, the message names the block's byte
};

// the jobs in one pool; the first failed job in list order is the error
int inflate_blocks(const std::vector<InflateJob> &jobs, uint32_t threads) {
    std::vector<std::string> errs(jobs.size());
    parallel_for(threads, jobs.size(), [&](uint64_t k) {
        const InflateJob &j = jobs[k];
        errs[k] = bm::inflate_member_zlib(j.file + j.block->payload(), *j.block, j.dst);
    });
    route().host_blocks += jobs.size();
    for (size_t k = 0; k < jobs.size(); ++k) {
        const InflateJob &j = jobs[k];
        if (!errs[k].empty())
            return bad_block(*j.path, j.by_byte ? bm::block_where_byte(j.block->coff)
                                                : bm::block_where(j.index), errs[k]);
    }
    return SECEDO_OK;
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
    std::vector<InflateJob> jobs;
    out->resize(paths.size());
    for (size_t f = 0; f < paths.size(); ++f) {
        uint64_t total = 0;
        SECEDO_CALL(open_bgzf(paths[f], &maps[f], &blocks[f], &total));
        (*out)[f].path = paths[f];
        (*out)[f].data.resize(total);
        (*out)[f].n_blocks = blocks[f].size();
        for (size_t b = 0; b < blocks[f].size(); ++b)
            jobs.push_back({&paths[f], maps[f].p, &blocks[f][b], b, (*out)[f].data.data() + blocks[f][b].out});
    }
    return inflate_blocks(jobs, threads);
}

// (RefID, Position) of one record after another: coordinate order puts the unmapped (RefID < 0) last
struct SortCheck {
    bool any = false;
    int64_t prev_ref = -1, prev_pos = 0;
    // false: the record sorts before the one before it
    bool check(int32_t ref, int32_t pos) {
        const int64_t key_ref = ref < 0 ? INT64_MAX : ref;
        const bool ok = !any || !(key_ref < prev_ref || (key_ref == prev_ref && ref >= 0 && pos < prev_pos));
        any = true;
        prev_ref = key_ref;
        prev_pos = pos;
        return ok;
    }
};

// The record walk of one file, carried across its block ranges.
struct WalkState {
    bool have_header = false;
    Header h;
    uint64_t idx = 0;
    SortCheck order;
    bool require_sorted = true;  // false (secedo_bam_scan): an unsorted file is walked to its end, `sorted` says so
    bool sorted = true;
    bool span = false;  // the bytes are a span of an indexed file: a chain that breaks means the index does not fit
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
        SECEDO_CALL(rc);
        st->have_header = true;
        o = st->h.first_record;
    }
    for (;; ++st->idx) {
        *used = o;
        if (o >= n) return SECEDO_OK;
        const std::string where = record_where(path, 0, 0, st->idx, Stage::kLoad, st->span);
        const auto defect = [&](uint32_t code) { return fail(SECEDO_E_INVALID_ARG, where + defect_tail(code)); };
        const auto broken = [&](uint32_t code) { return st->span ? chain_break(path, st->idx, code) : defect(code); };
        if (n - o < 4 + 32) return final ? broken(bamwalk::kErrTruncated) : SECEDO_OK;
        const uint32_t bs = rd32(d + o);
        const uint8_t *c = d + o + 4;
        if (bs < 32) return broken(bamwalk::kErrBlockSize);
        if (bs > n - o - 4) return final ? broken(bamwalk::kErrBlockSize) : SECEDO_OK;
        if (rec_aux_off(c) > bs) return defect(bamwalk::kErrLonger);
        const int32_t ref = int32_t(rd32(c)), pos = int32_t(rd32(c + 4));
        if (!st->order.check(ref, pos)) {
            if (st->require_sorted) return defect(bamwalk::kErrUnsorted);
            st->sorted = false;
        }
        SECEDO_CALL(on_record(st->idx, d + o, ref, pos));
        o += 4 + uint64_t(bs);
    }
}

// CIGAR ops and SEQ length agree (BuildCharData's substr would otherwise truncate)
int check_cigar(const uint8_t *rec, const std::string &where) {
    const uint8_t *c = rec + 4;
    const uint32_t l_name = rec_l_name(c), n_cigar = rec_n_cigar(c), l_seq = rec_l_seq(c);
    uint64_t query = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t v = rd32(c + 32 + l_name + 4 * k), t = v & 15;
        if (t > 8) return fail(SECEDO_E_INVALID_ARG, where + defect_tail(bamwalk::kErrCigarOp | t));
        if (t == 0 || t == 1 || t == 4 || t == 7 || t == 8) query += v >> 4;
    }
    if (l_seq > 0 && n_cigar > 0 && query != l_seq)
        return fail(SECEDO_E_INVALID_ARG, where + defect_tail(bamwalk::kErrCigarSeq));
    return SECEDO_OK;
}

// Per file: its records of each requested chromosome, appended as the walk meets them (one range after another).
struct FileSink {
    Inputs &in;
    size_t f;
    std::vector<std::vector<uint8_t> *> runs;  // [chr] this file's run
    std::vector<int> started, done;
    FileSink(Inputs &inputs, size_t file, Runs &r)
        : in(inputs), f(file), runs(inputs.chrs.size()), started(inputs.chrs.size(), 0), done(inputs.chrs.size(), 0) {
        for (size_t k = 0; k < runs.size(); ++k) runs[k] = &r[k][file];
    }
    int operator()(uint64_t idx, const uint8_t *rec, int32_t ref, int32_t pos) {
        for (size_t c = 0; c < in.chrs.size(); ++c) {
            ChrInput &ci = in.chrs[c];
            if (done[c]) continue;
            if (ref < 0 || uint32_t(ref) != ci.chromosome) {
                if (started[c]) done[c] = 1;  // the reader stops at another RefID
                continue;
            }
            const std::string where = record_where(in.paths[f], f, in.line0[f], idx, Stage::kLoad, in.indexed[f] != 0);
            if (pos < 0) return fail(SECEDO_E_INVALID_ARG, where + defect_tail(bamwalk::kErrNegative));
            SECEDO_CALL(check_cigar(rec, where));
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
int load_file_ranges(size_t f, uint32_t threads, uint64_t batch, Inputs *in, Runs *runs, secedo_bam_times *t) {
    const std::string &path = in->paths[f];
    Mapped m;
    std::vector<Block> blocks;
    uint64_t total = 0;
    SECEDO_CALL(open_bgzf(path, &m, &blocks, &total));
    WalkState st;
    FileSink sink(*in, f, *runs);
    std::vector<uint8_t> buf;
    std::vector<InflateJob> jobs;
    uint64_t carry = 0;
    size_t b0 = 0;
    do {
        const size_t b1 = bm::next_range(blocks, b0, batch);
        const uint64_t bytes = bm::range_bytes(blocks, b0, b1);
        Clock::time_point t0 = Clock::now();
        buf.resize(carry + bytes);
        jobs.clear();
        for (size_t b = b0; b < b1; ++b)
            jobs.push_back({&path, m.p, &blocks[b], b, buf.data() + carry + (blocks[b].out - blocks[b0].out)});
        SECEDO_CALL(inflate_blocks(jobs, threads));
        if (t) {
            t->inflate_ms += ms_since(t0);
            t->inflated_bytes += double(bytes);
        }
        t0 = Clock::now();
        uint64_t used = 0;
        SECEDO_CALL(walk_range(path, buf.data(), buf.size(), b1 == blocks.size(), &st, &used, sink));
        carry = buf.size() - used;
        if (used) std::memmove(buf.data(), buf.data() + used, carry);
        buf.resize(carry);
        if (t) t->walk_ms += ms_since(t0);
        b0 = b1;
    } while (b0 < blocks.size());
    return SECEDO_OK;
}

// One indexed file: only the members of its spans are inflated, through the pool, in ranges of about `batch` inflated
// bytes as above; a span is entered at its first record and walked to its limit. The sortedness check and the runs
// carry across the spans of the file.
int load_file_spans(size_t f, const IndexPlan &plan, uint32_t threads, uint64_t batch, Inputs *in, Runs *runs,
                    secedo_bam_times *t) {
    const std::string &path = in->paths[f];
    WalkState st;
    st.have_header = true;
    st.h = plan.h;
    st.span = true;
    FileSink sink(*in, f, *runs);
    std::vector<uint8_t> buf;
    std::vector<InflateJob> jobs;
    for (const Span &sp : plan.spans) {
        const std::vector<Block> &blocks = sp.blocks;
        std::vector<uint64_t> got(sp.chrs.size(), 0);
        std::vector<char> start_ok(sp.chrs.size(), 0);
        index_info().spans += 1;
        index_info().members += blocks.size();
        uint64_t carry = 0;
        buf.clear();
        for (size_t b0 = 0; b0 < blocks.size();) {
            const size_t b1 = bm::next_range(blocks, b0, batch);
            const uint64_t bytes = bm::range_bytes(blocks, b0, b1);
            const bool final = b1 == blocks.size();
            Clock::time_point t0 = Clock::now();
            buf.resize(carry + bytes);
            jobs.clear();
            for (size_t b = b0; b < b1; ++b)
                jobs.push_back({&path, plan.m.p, &blocks[b], b, buf.data() + carry + (blocks[b].out - blocks[b0].out),
                                true});
            SECEDO_CALL(inflate_blocks(jobs, threads));
            if (t) {
                t->inflate_ms += ms_since(t0);
                t->inflated_bytes += double(bytes);
            }
            t0 = Clock::now();
            const uint64_t lin0 = blocks[b0].out - carry;  // the span offset of buf[0]
            const uint64_t n = final ? sp.limit - lin0 : buf.size();
            const uint64_t o0 = b0 == 0 ? sp.entry : 0;
            if (b0 == 0 && o0 + 8 <= n && rd32(buf.data() + o0 + 4) != sp.chrs[0].chromosome)
                return check_span_chr(path, sp.chrs[0], false, 0);
            const uint8_t *d = buf.data() + o0;
            const auto on_record = [&](uint64_t idx, const uint8_t *rec, int32_t ref, int32_t pos) {
                const uint64_t lin = lin0 + o0 + uint64_t(rec - d);
                for (size_t c = 0; c < sp.chrs.size(); ++c) {
                    const SpanChr &sc = sp.chrs[c];
                    if (lin == sc.beg) start_ok[c] = ref >= 0 && uint32_t(ref) == sc.chromosome;
                    if (sc.beg <= lin && lin < sc.end) ++got[c];
                }
                return sink(idx, rec, ref, pos);
            };
            uint64_t used = 0;
            SECEDO_CALL(walk_range(path, d, n - o0, final, &st, &used, on_record));
            used += o0;
            if (final) {
                for (size_t c = 0; c < sp.chrs.size(); ++c)
                    SECEDO_CALL(check_span_chr(path, sp.chrs[c], start_ok[c] != 0, got[c]));
                if (sp.limit + 8 <= sp.bytes && rd32(buf.data() + n + 4) == sp.chrs.back().chromosome)
                    return span_tail_mismatch(path, sp.chrs.back());
            }
            carry = buf.size() - used;
            if (used) std::memmove(buf.data(), buf.data() + used, carry);
            buf.resize(carry);
            if (t) t->walk_ms += ms_since(t0);
            b0 = b1;
        }
    }
    return SECEDO_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// SAM text input: the header is parsed here, the alignment lines on the device (sam_kernels.hip) into the BAM records
// the walk above collects. The file type comes from its content, never its name: plain gzip is refused; BGZF whose
// first non-empty member starts with "BAM\1" is BAM, other BGZF is compressed SAM; anything else is SAM.

enum Kind : char { kBam = 0, kSam = 1, kSamGz = 2 };

// BGZF: the first member with ISIZE > 0 inflated here decides between BAM and SAM text. A file with no such member,
// or one that does not inflate, stays with the BAM route, which reports it.
int sniff_bgzf(const std::string &path, Kind *kind) {
    *kind = kBam;
    Mapped m;
    SECEDO_CALL(map_file(path, &m));
    for (uint64_t off = 0; off < m.n;) {
        Block blk;
        uint32_t len = 0;
        if (read_block(path, m, off, &blk, &len) != SECEDO_OK) return SECEDO_OK;
        if (blk.isize) {
            std::vector<uint8_t> d(blk.isize);
            if (bm::inflate_member_zlib(m.p + blk.payload(), blk, d.data()).empty() &&
                !(d.size() >= 4 && std::memcmp(d.data(), "BAM\1", 4) == 0))
                *kind = kSamGz;
            return SECEDO_OK;
        }
        off += len;
    }
    return SECEDO_OK;
}

// *kind = what the file is; plain gzip (no BGZF extra field) is an error
int sniff(const std::string &path, Kind *kind) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return fail(SECEDO_E_INVALID_ARG, "Could not open " + path);
    uint8_t b[512];
    const ssize_t n = pread(fd, b, sizeof(b), 0);
    close(fd);
    if (n < 0) return fail(SECEDO_E_INVALID_ARG, "Could not read " + path);
    *kind = kSam;
    if (!(n >= 2 && b[0] == 31 && b[1] == 139)) return SECEDO_OK;
    bool bgzf = false;
    if (n >= 12 && b[2] == 8 && (b[3] & 4)) {
        const uint32_t end = std::min<uint32_t>(12 + rd16(b + 10), uint32_t(n));
        for (uint32_t x = 12; x + 4 <= end; x += 4 + rd16(b + x + 2))
            if (b[x] == 'B' && b[x + 1] == 'C') bgzf = true;
    }
    if (!bgzf)
        return fail(SECEDO_E_INVALID_ARG, path + ": a gzip file that is not BGZF; decompress it to SAM or convert "
                                                 "it to BAM (samtools view -b)");
    return sniff_bgzf(path, kind);
}

struct SamHeader {
    std::vector<std::string> names;  // @SQ SN values by RefID
    uint64_t lines = 0, body = 0;    // header lines, byte offset of the first alignment line
};

// the leading '@' lines: @SQ SN and LN required, SN unique
int parse_sam_header(const std::string &path, size_t f, const uint8_t *p, uint64_t n, SamHeader *h) {
    std::set<std::string> seen;
    uint64_t o = 0;
    while (o < n && p[o] == '@') {
        const uint8_t *nl = static_cast<const uint8_t *>(std::memchr(p + o, '\n', n - o));
        const uint64_t e = nl ? uint64_t(nl - p) : n;
        ++h->lines;
        const std::string line(reinterpret_cast<const char *>(p + o), e - o);
        o = nl ? e + 1 : n;
        if (line.compare(0, 3, "@SQ") != 0 || (line.size() > 3 && line[3] != '\t')) continue;
        const std::string where = record_where(path, f, h->lines, 0);  // the header line itself
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

// device buffers of the BGZF inflate, kept over the ranges and files of one call
struct GzWork {
    Dev<uint8_t> in;
    Dev<BgzfDesc> desc;
    Dev<uint32_t> status;
    std::vector<BgzfDesc> h_desc;
    std::vector<uint32_t> h_status;
};

// Blocks [b0, b1) of a mapped BGZF file inflated on the device: block b lands at d_out + out_base + (its inflated
// offset - that of b0). The compressed bytes go up as they lie in the file, in one copy; ISIZE and CRC32 are checked
// on the device, and the first block in file order that fails is the error, in the words of the host inflate.
int inflate_range_device(const std::string &path, const Mapped &m, const std::vector<Block> &blocks, size_t b0,
                         size_t b1, GzWork *g, uint8_t *d_out, uint64_t out_base, hipStream_t s,
                         secedo_bam_times *t) {
    if (b0 >= b1) return SECEDO_OK;
    Clock::time_point t0 = Clock::now();
    const bm::PayloadSpan sp = bm::payload_span(blocks, b0, b1, m.n);
    const uint64_t n_blocks = b1 - b0;
    if (n_blocks > UINT32_MAX) return fail(SECEDO_E_LIMIT, path + ": too many BGZF blocks in one range");
    g->h_desc.resize(n_blocks);
    bm::fill_desc(blocks, b0, b1, sp.lo, 0, out_base, g->h_desc.data());
    SECEDO_TRY(g->in.grow(sp.needed, 0, s));
    SECEDO_TRY(g->desc.grow(n_blocks, 0, s));
    SECEDO_TRY(g->status.grow(n_blocks, 0, s));
    SECEDO_TRY(hipMemcpyAsync(g->in.p, m.p + sp.lo, size_t(sp.hi - sp.lo), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(g->desc.p, g->h_desc.data(), n_blocks * sizeof(BgzfDesc), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_lap(t0);
    SECEDO_TRY(bgzf_inflate(g->in.p, g->desc.p, uint32_t(n_blocks), d_out, g->status.p, s));
    g->h_status.resize(n_blocks);
    SECEDO_TRY(hipMemcpyAsync(g->h_status.data(), g->status.p, n_blocks * 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) t->inflate_ms += ms_lap(t0);
    route().device_blocks += n_blocks;
    route().uploaded_bytes += sp.hi - sp.lo;
    route().batches += 1;
    const size_t bad = bm::first_bad(g->h_status.data(), n_blocks);
    if (bad < n_blocks)
        return bad_block(path, bm::block_where(b0 + bad), bm::status_text(g->h_status[bad]));
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
    GzWork gz;           // BGZF SAM: the device inflate in front of the parse
    Dev<uint8_t> carry;  // and the cut tail of a range on its way to the front of the next
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

// The @SQ names on the device: packed, hashed and sorted here; *sel marks the requested RefIDs.
int upload_sam_refs(const SamHeader &h, const std::vector<ChrInput> &chrs, SamWork *w, std::vector<uint8_t> *sel,
                    SamRefs *refs) {
    hipStream_t s = w->s;
    const uint32_t n_ref = uint32_t(h.names.size());
    std::vector<uint8_t> names;
    sel->assign(std::max<uint32_t>(n_ref, 1), 0);
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
    for (const auto &ci : chrs)
        if (ci.chromosome < n_ref) (*sel)[ci.chromosome] = 1;
    SECEDO_TRY(w->names.grow(names.size(), 0, s));
    SECEDO_TRY(w->name_off.grow(n_ref + 1, 0, s));
    SECEDO_TRY(w->name_hash.grow(n_ref, 0, s));
    SECEDO_TRY(w->name_id.grow(n_ref, 0, s));
    SECEDO_TRY(w->sel.grow(sel->size(), 0, s));
    SECEDO_TRY(w->err.grow(1, 0, s));
    if (!names.empty()) SECEDO_TRY(hipMemcpyAsync(w->names.p, names.data(), names.size(), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(w->name_off.p, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice, s));
    if (n_ref) {
        SECEDO_TRY(hipMemcpyAsync(w->name_hash.p, name_hash.data(), n_ref * 8ull, hipMemcpyHostToDevice, s));
        SECEDO_TRY(hipMemcpyAsync(w->name_id.p, name_id.data(), n_ref * 4ull, hipMemcpyHostToDevice, s));
    }
    SECEDO_TRY(hipMemcpyAsync(w->sel.p, sel->data(), sel->size(), hipMemcpyHostToDevice, s));
    *refs = SamRefs{w->names.p, w->name_off.p, w->name_hash.p, w->name_id.p, w->sel.p, n_ref};
    return SECEDO_OK;
}

// one range of SAM lines as the device parse sees it and leaves it
struct SamRange {
    uint64_t len = 0;        // bytes of text, uploaded to w->text and zero-padded to n16 + 1 vectors of 16
    uint64_t n16 = 0;
    uint64_t line_base = 0;  // lines of the body before the range
    bool ends_file = false, trailing = false;  // the range ends the file; its last byte is '\n'
    // out: the lines, those below the first bad one (parsed into w->h_ref / h_pos / h_out), the lowest error
    uint32_t n_lines = 0, limit = 0;
    unsigned long long err = ~0ull;
};

// The device parse of one uploaded range: line starts, the size of each line's record, the records themselves; RefID
// and Position of each line and the records of the selected chromosomes come back to the host.
int parse_sam_range(SamWork *w, const SamRefs &refs, SamRange *r) {
    hipStream_t s = w->s;
    const uint64_t n16 = r->n16;
    SECEDO_TRY(w->cnt.grow(n16 + 1, 0, s));
    SECEDO_TRY(w->scan.grow(n16 + 1, 0, s));
    size_t tb = scan_bytes(n16 + 1);
    SECEDO_TRY(w->tmp.grow(tb, 0, s));
    SECEDO_TRY(sam_newline_count(w->text.p, n16, w->cnt.p, s));
    SECEDO_TRY(hipMemsetAsync(w->cnt.p + n16, 0, 4, s));
    SECEDO_TRY(exclusive_sum(w->tmp.p, tb, w->cnt.p, w->scan.p, n16 + 1, s));
    uint32_t n_nl = 0;
    SECEDO_TRY(hipMemcpyAsync(&n_nl, w->scan.p + n16, 4, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    const uint32_t n_lines = n_nl + (r->trailing ? 0 : 1);
    SECEDO_TRY(w->start.grow(uint64_t(n_lines) + 1, 0, s));
    SECEDO_TRY(w->size.grow(uint64_t(n_lines) + 1, 0, s));
    SECEDO_TRY(w->off.grow(uint64_t(n_lines) + 1, 0, s));
    SECEDO_TRY(w->ref.grow(n_lines, 0, s));
    SECEDO_TRY(w->pos.grow(n_lines, 0, s));
    SECEDO_TRY(sam_line_starts(w->text.p, n16, w->scan.p, n_lines, uint32_t(r->len), !r->trailing, w->start.p, s));
    SECEDO_TRY(hipMemsetAsync(w->err.p, 0xFF, 8, s));
    SECEDO_TRY(sam_size(w->text.p, w->start.p, n_lines, r->line_base, r->ends_file, refs, w->size.p, w->ref.p,
                        w->pos.p, w->err.p, s));
    SECEDO_TRY(hipMemsetAsync(w->size.p + n_lines, 0, 8, s));
    tb = scan_bytes(uint64_t(n_lines) + 1);
    SECEDO_TRY(w->tmp.grow(tb, 0, s));
    SECEDO_TRY(exclusive_sum64(w->tmp.p, tb, w->size.p, w->off.p, uint64_t(n_lines) + 1, s));
    uint64_t total = 0;
    unsigned long long err = 0;
    SECEDO_TRY(hipMemcpyAsync(&total, w->off.p + n_lines, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipMemcpyAsync(&err, w->err.p, 8, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    // lines below the first bad one are encoded and walked: a structural error there comes first
    const uint32_t limit = err == ~0ull ? n_lines : uint32_t((err >> 8) - r->line_base);
    SECEDO_TRY(w->out.grow(total, 0, s));
    SECEDO_TRY(sam_encode(w->text.p, w->start.p, limit, refs, w->off.p, w->out.p, s));
    w->h_ref.resize(limit);
    w->h_pos.resize(limit);
    w->h_out.resize(total);
    if (limit) {
        SECEDO_TRY(hipMemcpyAsync(w->h_ref.data(), w->ref.p, limit * 4ull, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipMemcpyAsync(w->h_pos.data(), w->pos.p, limit * 4ull, hipMemcpyDeviceToHost, s));
    }
    if (total) SECEDO_TRY(hipMemcpyAsync(w->h_out.data(), w->out.p, total, hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    r->n_lines = n_lines;
    r->limit = limit;
    r->err = err;
    return SECEDO_OK;
}

// The host pass over a parsed range: sortedness over every line, the selected records into the runs, then the
// range's parse error if it has one.
int collect_sam_range(const SamWork &w, const SamRange &r, const std::vector<uint8_t> &sel, SortCheck *order,
                      FileSink *sink) {
    const std::string &path = sink->in.paths[sink->f];
    const uint64_t line0 = sink->in.line0[sink->f];
    uint64_t o = 0;
    for (uint32_t k = 0; k < r.limit; ++k) {
        const int32_t ref = w.h_ref[k], pos = w.h_pos[k];
        if (ref == kSamNoRecord) continue;
        const uint64_t idx = r.line_base + k;
        if (!order->check(ref, pos))
            return fail(SECEDO_E_INVALID_ARG,
                        record_where(path, sink->f, line0, idx) + defect_tail(bamwalk::kErrUnsorted));
        if (ref >= 0 && size_t(ref) < sel.size() && sel[ref]) {
            const uint8_t *rec = w.h_out.data() + o;
            SECEDO_CALL((*sink)(idx, rec, ref, pos));
            o += 4 + uint64_t(rd32(rec));
        }
    }
    if (r.err != ~0ull) {
        const uint32_t code = uint32_t(r.err & 0xFF);
        return fail(code == kSamManyOps || code == kSamTooLong ? SECEDO_E_LIMIT : SECEDO_E_INVALID_ARG,
                    record_where(path, sink->f, line0, r.err >> 8) + " " + sam_what(code));
    }
    return SECEDO_OK;
}

// One SAM file: header on the host, then ranges of about `batch` bytes ending at a '\n', each uploaded, parsed on the
// device, and its records of the requested chromosomes downloaded into the file's runs (FileSink, as a BAM's walk).
int load_sam_file(size_t f, uint64_t batch, SamWork *w, Inputs *in, Runs *runs, secedo_bam_times *t) {
    const std::string &path = in->paths[f];
    Clock::time_point t0 = Clock::now();
    Mapped m;
    SECEDO_CALL(map_file(path, &m));
    SamHeader h;
    SECEDO_CALL(parse_sam_header(path, f, m.p, m.n, &h));
    in->line0[f] = h.lines + 1;
    if (t) t->inflate_ms += ms_since(t0);
    t0 = Clock::now();
    if (!w->s) SECEDO_TRY(hipStreamCreateWithFlags(&w->s, hipStreamNonBlocking));
    hipStream_t s = w->s;
    std::vector<uint8_t> sel;
    SamRefs refs{};
    SECEDO_CALL(upload_sam_refs(h, in->chrs, w, &sel, &refs));
    if (t) t->upload_ms += ms_since(t0);

    FileSink sink(*in, f, *runs);
    SortCheck order;
    SamRange r;
    for (uint64_t r0 = h.body; r0 < m.n;) {
        uint64_t r1 = std::min<uint64_t>(m.n, r0 + std::max<uint64_t>(batch, 1));
        if (r1 < m.n) {
            const uint8_t *nl = static_cast<const uint8_t *>(std::memchr(m.p + r1 - 1, '\n', m.n - (r1 - 1)));
            r1 = nl ? uint64_t(nl - m.p) + 1 : m.n;
        }
        r.len = r1 - r0;
        if (r.len >= (1ull << 32) - 64)
            return fail(SECEDO_E_LIMIT, "file " + std::to_string(f) + " (" + path +
                                            "): a range of SAM lines of 4 GiB or more (a line that long)");
        r.ends_file = r1 == m.n;
        r.trailing = m.p[r1 - 1] == '\n';
        // text read
        t0 = Clock::now();
        w->h_text.assign(m.p + r0, m.p + r1);
        if (t) {
            t->inflate_ms += ms_since(t0);
            t->inflated_bytes += double(r.len);
        }
        // upload, zero-padded to whole 16-byte vectors plus one
        t0 = Clock::now();
        r.n16 = (r.len + 15) / 16;
        const uint64_t padded = r.n16 * 16 + 16;
        SECEDO_TRY(w->text.grow(padded, 0, s));
        SECEDO_TRY(hipMemcpyAsync(w->text.p, w->h_text.data(), r.len, hipMemcpyHostToDevice, s));
        SECEDO_TRY(hipMemsetAsync(w->text.p + r.len, 0, padded - r.len, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        if (t) t->upload_ms += ms_since(t0);
        // device parse, then the host pass
        t0 = Clock::now();
        SECEDO_CALL(parse_sam_range(w, refs, &r));
        SECEDO_CALL(collect_sam_range(*w, r, sel, &order, &sink));
        if (t) t->walk_ms += ms_since(t0);
        r.line_base += r.n_lines;
        r0 = r1;
    }
    return SECEDO_OK;
}

// The header of a BGZF SAM file: its leading blocks inflated on the host until a line starts with something else than
// '@', or the file ends -> head (what those blocks hold, body bytes behind the header included), *hb = blocks inflated.
int inflate_sam_head(const std::string &path, const Mapped &m, const std::vector<Block> &blocks,
                     std::vector<uint8_t> *head_out, size_t *hb_out) {
    std::vector<uint8_t> &head = *head_out;
    size_t &hb = *hb_out;
    hb = 0;
    for (uint64_t o = 0;;) {  // o: a line start, every line before it an '@' line
        const uint8_t *nl = nullptr;
        if (o < head.size()) {
            if (head[o] != '@') break;
            nl = static_cast<const uint8_t *>(std::memchr(head.data() + o, '\n', head.size() - o));
        }
        if (nl) {
            o = uint64_t(nl - head.data()) + 1;
            continue;
        }
        if (hb == blocks.size()) break;
        const size_t at = head.size();
        head.resize(at + blocks[hb].isize);
        const std::string err = bm::inflate_member_zlib(m.p + blocks[hb].payload(), blocks[hb], head.data() + at);
        if (!err.empty()) return bad_block(path, bm::block_where(hb), err);
        ++hb;
    }
    return SECEDO_OK;
}

// One BGZF-compressed SAM file: what load_sam_file gives on its inflated text. The host lists the blocks and inflates
// the leading ones with zlib until the '@' lines end; every block after those is inflated on the device, in ranges of
// about `batch` inflated bytes, into the text buffer behind the carry (the bytes after the last '\n' of the range
// before). [0, last '\n'] of each range goes to the parse; the inflated text never reaches the host.
int load_samgz_file(size_t f, uint64_t batch, SamWork *w, Inputs *in, Runs *runs, secedo_bam_times *t) {
    const std::string &path = in->paths[f];
    Clock::time_point t0 = Clock::now();
    Mapped m;
    std::vector<Block> blocks;
    uint64_t total = 0;
    SECEDO_CALL(open_bgzf(path, &m, &blocks, &total));
    std::vector<uint8_t> head;
    size_t hb = 0;
    SECEDO_CALL(inflate_sam_head(path, m, blocks, &head, &hb));
    route().host_blocks += hb;
    SamHeader h;
    SECEDO_CALL(parse_sam_header(path, f, head.data(), head.size(), &h));
    in->line0[f] = h.lines + 1;
    if (t) {
        t->inflate_ms += ms_since(t0);
        t->inflated_bytes += double(head.size());
    }
    t0 = Clock::now();
    if (!w->s) SECEDO_TRY(hipStreamCreateWithFlags(&w->s, hipStreamNonBlocking));
    hipStream_t s = w->s;
    std::vector<uint8_t> sel;
    SamRefs refs{};
    SECEDO_CALL(upload_sam_refs(h, in->chrs, w, &sel, &refs));
    // what the header's blocks hold of the body is the first carry
    uint64_t carry = head.size() - h.body;
    SECEDO_TRY(w->text.grow(carry + 32, 0, s));
    if (carry) SECEDO_TRY(hipMemcpyAsync(w->text.p, head.data() + h.body, carry, hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    if (t) t->upload_ms += ms_since(t0);

    FileSink sink(*in, f, *runs);
    SortCheck order;
    SamRange r;
    for (size_t b0 = hb;;) {
        const size_t b1 = bm::next_range(blocks, b0, batch, total);  // a tail of only empty blocks goes with it
        const uint64_t bytes = bm::range_bytes(blocks, b0, b1);
        const bool ends = b1 == blocks.size();
        const uint64_t len = carry + bytes;
        if (len >= (1ull << 32) - 64)
            return fail(SECEDO_E_LIMIT, "file " + std::to_string(f) + " (" + path +
                                            "): a range of SAM lines of 4 GiB or more (a line that long)");
        const uint64_t padded = (len + 15) / 16 * 16 + 16;
        SECEDO_TRY(w->text.grow(padded, carry, s));
        SECEDO_CALL(inflate_range_device(path, m, blocks, b0, b1, &w->gz, w->text.p, carry, s, t));
        if (t) t->inflated_bytes += double(bytes);
        b0 = b1;
        t0 = Clock::now();
        unsigned long long last = 0;  // one past the last '\n'
        if (len) {
            SECEDO_TRY(w->err.grow(1, 0, s));
            SECEDO_TRY(bgzf_last_newline(w->text.p, len, w->err.p, s));
            SECEDO_TRY(hipMemcpyAsync(&last, w->err.p, 8, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
        }
        const uint64_t cut = ends ? len : last;  // the range handed on; the rest is carried
        carry = len - cut;
        if (cut) {
            if (carry) {
                SECEDO_TRY(w->carry.grow(carry, 0, s));
                SECEDO_TRY(hipMemcpyAsync(w->carry.p, w->text.p + cut, carry, hipMemcpyDeviceToDevice, s));
            }
            r.len = cut;
            r.n16 = (cut + 15) / 16;
            r.ends_file = ends;
            r.trailing = last == cut;
            // zero-padded to whole 16-byte vectors plus one, as an uploaded range is
            SECEDO_TRY(hipMemsetAsync(w->text.p + cut, 0, r.n16 * 16 + 16 - cut, s));
            SECEDO_CALL(parse_sam_range(w, refs, &r));
            SECEDO_CALL(collect_sam_range(*w, r, sel, &order, &sink));
            r.line_base += r.n_lines;
            if (carry) SECEDO_TRY(hipMemcpyAsync(w->text.p, w->carry.p, carry, hipMemcpyDeviceToDevice, s));
        }
        if (t) t->walk_ms += ms_since(t0);
        if (ends) break;
    }
    return SECEDO_OK;
}

// the inflated bytes of the last secedo_bgzf_inflate on this thread
struct InflatedFile {
    Dev<uint8_t> data;
    uint64_t n = 0;
};
thread_local InflatedFile *g_inflated = nullptr;

}  // namespace

namespace secedo {
namespace bam_host {

secedo_bam_route_info &route() {
    static thread_local secedo_bam_route_info r{};
    return r;
}

int require_bam(const std::string &path, const std::string &what) {
    Kind kind = kBam;
    SECEDO_CALL(sniff(path, &kind));
    if (kind != kBam)
        return fail(SECEDO_E_INVALID_ARG, path + ": " + (kind == kSam ? "a SAM file" : "a BGZF-compressed SAM file") +
                                              " " + what + "; convert it to BAM (samtools view -b)");
    return SECEDO_OK;
}

namespace {
std::atomic<int> g_inflate_mode{-1};  // -1: not set by secedo_bam_set_inflate, the environment decides
}

namespace {
std::atomic<int> g_index_mode{-1};  // -1: not set by secedo_bam_set_index, the environment decides
}

int index_mode(int *mode) {
    int m = g_index_mode.load();
    if (m < 0) {
        const char *e = std::getenv("SECEDO_BAM_INDEX");
        if (!e || !*e || std::strcmp(e, "off") == 0) m = SECEDO_BAM_INDEX_OFF;
        else if (std::strcmp(e, "auto") == 0) m = SECEDO_BAM_INDEX_AUTO;
        else if (std::strcmp(e, "require") == 0) m = SECEDO_BAM_INDEX_REQUIRE;
        else return fail(SECEDO_E_INVALID_ARG, std::string("SECEDO_BAM_INDEX=") + e + ": expected off, auto or require");
    }
    *mode = m;
    return SECEDO_OK;
}

secedo_bam_index_info &index_info() {
    static thread_local secedo_bam_index_info r{};
    return r;
}

int index_mismatch(const std::string &path, const std::string &why) {
    return fail(SECEDO_E_INVALID_ARG,
                path + ": index does not match the file (" + why + "); re-index it or use --index off");
}

int check_span_chr(const std::string &path, const SpanChr &c, bool start_ok, uint64_t got_count) {
    const std::string ref = "reference " + std::to_string(c.chromosome);
    if (!start_ok) return index_mismatch(path, "no record of " + ref + " starts where the index says its records start");
    if (c.count != bamindex::kNoCount && c.count != got_count)
        return index_mismatch(path, ref + " has " + std::to_string(got_count) +
                                        " records between its start and end, the index counts " +
                                        std::to_string(c.count));
    return SECEDO_OK;
}

int span_tail_mismatch(const std::string &path, const SpanChr &c) {
    return index_mismatch(path, "the record at the end of reference " + std::to_string(c.chromosome) +
                                    " still has its RefID");
}

namespace {

// the index beside a BAM, parsed and checked against it: empty, or why it cannot be used (*found: a file was there)
std::string read_index(const std::string &path, const Mapped &m, uint32_t n_ref, std::vector<bamindex::RefRange> *refs,
                       bool *found) {
    *found = false;
    const std::string name = bamindex::find(path);
    if (name.empty()) return "no index file " + path + ".bai";
    *found = true;
    std::vector<uint8_t> bytes;
    if (!bamindex::read_file(name, &bytes)) return "could not read " + name;
    std::string why = bamindex::parse(bytes.data(), bytes.size(), refs);
    if (why.empty()) why = bamindex::check(*refs, n_ref, m.p, m.n);
    return why.empty() ? why : name + ": " + why;
}

// the header's members of a mapped BAM inflated and the header parsed; bytes (may be null): what was inflated
int read_header(const std::string &path, IndexPlan *plan, std::vector<uint8_t> *bytes = nullptr) {
    std::vector<uint8_t> head;
    uint64_t off = 0;
    for (;;) {
        const int rc = parse_header(path, head.data(), head.size(), off >= plan->m.n, &plan->h);
        if (rc == SECEDO_OK) break;
        if (rc != kNeedMore) return rc;
        Block blk;
        uint32_t len = 0;
        SECEDO_CALL(read_block(path, plan->m, off, &blk, &len));
        blk.out = head.size();
        head.resize(head.size() + blk.isize);
        const std::string err = bm::inflate_member_zlib(plan->m.p + blk.payload(), blk, head.data() + blk.out);
        if (!err.empty()) return bad_block(path, bm::block_where(plan->head.size()), err);
        plan->head.push_back(blk);
        off += len;
    }
    if (bytes) bytes->swap(head);
    return SECEDO_OK;
}

}  // namespace

int plan_index(const std::string &path, const std::vector<uint32_t> &chromosomes, int mode, IndexPlan *plan) {
    const auto full = [&](const std::string &why, bool rejected) {
        if (mode == SECEDO_BAM_INDEX_REQUIRE) return fail(SECEDO_E_INVALID_ARG, path + ": no usable index: " + why);
        index_info().files_full += 1;
        index_info().rejected += rejected ? 1 : 0;
        *plan = IndexPlan();
        return int(SECEDO_OK);
    };
    // a file whose header does not parse: AUTO reads it in full, which reports it in the words of the full read;
    // REQUIRE says that no index can be used and why
    if (map_file(path, &plan->m) != SECEDO_OK || read_header(path, plan) != SECEDO_OK) {
        const std::string why = g_error;
        return full(why, false);
    }
    std::vector<bamindex::RefRange> refs;
    bool found = false;
    const std::string why = read_index(path, plan->m, plan->h.n_ref, &refs, &found);
    if (!why.empty()) return full(why, found);

    // the requested chromosomes that have records, each once, in file order
    struct Want {
        uint32_t chromosome;
        bamindex::RefRange r;
    };
    std::vector<Want> want;
    for (const uint32_t c : chromosomes) {
        if (c >= refs.size() || refs[c].empty() || refs[c].beg == refs[c].end) continue;
        if (std::none_of(want.begin(), want.end(), [&](const Want &w) { return w.chromosome == c; }))
            want.push_back(Want{c, refs[c]});
    }
    std::sort(want.begin(), want.end(), [](const Want &a, const Want &b) { return a.r.beg < b.r.beg; });
    const Mapped &m = plan->m;
    for (size_t a = 0; a < want.size();) {
        // spans whose member ranges touch or overlap are one
        uint64_t end_v = want[a].r.end;
        size_t b = a + 1;
        while (b < want.size() && bamindex::coffset(want[b].r.beg) <= bamindex::coffset(end_v))
            end_v = std::max(end_v, want[b++].r.end);
        Span sp;
        sp.beg_v = want[a].r.beg;
        const uint64_t end_coff = bamindex::coffset(end_v);
        const std::string lead = "the members from " + bamindex::voffset_str(sp.beg_v) + " do not lead to " +
                                 bamindex::voffset_str(end_v);
        for (uint64_t off = bamindex::coffset(sp.beg_v);;) {
            if (off == end_coff && bamindex::uoffset(end_v) == 0) break;
            if (off > end_coff || off >= m.n) return index_mismatch(path, lead);
            Block blk;
            uint32_t len = 0;
            SECEDO_CALL(read_block(path, m, off, &blk, &len));
            blk.out = sp.bytes;
            sp.bytes += blk.isize;
            sp.blocks.push_back(blk);
            if (off == end_coff) break;
            off += len;
        }
        // a virtual offset as an offset of the span's inflated bytes; its member is one of the span's, or the
        // one behind its last (uoffset 0)
        const auto linear = [&](uint64_t v, uint64_t *lin) {
            const uint64_t coff = bamindex::coffset(v);
            const auto it = std::lower_bound(sp.blocks.begin(), sp.blocks.end(), coff,
                                             [](const Block &x, uint64_t c) { return x.coff < c; });
            if (it != sp.blocks.end() && it->coff == coff) {
                if (bamindex::uoffset(v) > it->isize) return false;
                *lin = it->out + bamindex::uoffset(v);
                return true;
            }
            *lin = sp.bytes;
            return coff == end_coff && bamindex::uoffset(v) == 0;
        };
        for (size_t k = a; k < b; ++k) {
            SpanChr sc{want[k].chromosome, 0, 0, want[k].r.count};
            if (!linear(want[k].r.beg, &sc.beg) || !linear(want[k].r.end, &sc.end) || sc.beg > sc.end)
                return index_mismatch(path, "reference " + std::to_string(sc.chromosome) + " at " +
                                                bamindex::voffset_str(want[k].r.beg) + " .. " +
                                                bamindex::voffset_str(want[k].r.end) +
                                                " is not inside the members of its span");
            sp.limit = std::max(sp.limit, sc.end);
            sp.chrs.push_back(sc);
        }
        sp.entry = sp.chrs[0].beg;
        if (sp.chrs.back().end != sp.limit)  // a reference that ends behind the next one's end: not a sorted file's
            return index_mismatch(path, "the references of the span at " + bamindex::voffset_str(sp.beg_v) + " nest");
        plan->spans.push_back(std::move(sp));
        a = b;
    }
    plan->indexed = true;
    index_info().files_indexed += 1;
    route().host_blocks += plan->head.size();
    return SECEDO_OK;
}

int inflate_route(bool *device) {
    int mode = g_inflate_mode.load();
    if (mode < 0) {
        const char *e = std::getenv("SECEDO_BAM_INFLATE");
        if (!e || !*e || std::strcmp(e, "host") == 0) mode = SECEDO_BAM_INFLATE_HOST;
        else if (std::strcmp(e, "device") == 0) mode = SECEDO_BAM_INFLATE_DEVICE;
        else return fail(SECEDO_E_INVALID_ARG, std::string("SECEDO_BAM_INFLATE=") + e + ": expected host or device");
    }
    *device = mode == SECEDO_BAM_INFLATE_DEVICE;
    return SECEDO_OK;
}

void release_inflated() {
    delete g_inflated;
    g_inflated = nullptr;
}

std::string record_where(const std::string &path, size_t f, uint64_t line0, uint64_t idx, Stage stage, bool indexed) {
    if (line0) return "file " + std::to_string(f) + " (" + path + "), line " + std::to_string(line0 + idx);
    const std::string record = (indexed ? "indexed record " : "record ") + std::to_string(idx);
    if (stage == Stage::kLoad) return path + ": " + record;
    return "file " + std::to_string(f) + ", " + record;
}

int load_inputs(const std::vector<std::string> &files, const uint32_t *chromosome_ids, uint32_t n_chr,
                uint32_t threads, Inputs *in, secedo_bam_times *t) {
    const size_t n_files = files.size();
    const uint64_t batch = batch_bytes();
    route() = secedo_bam_route_info{};
    bool device = false;
    SECEDO_CALL(inflate_route(&device));
    std::unique_ptr<BamDevWork, void (*)(BamDevWork *)> dev_work(device ? new_bam_dev_work() : nullptr,
                                                                 delete_bam_dev_work);
    int imode = SECEDO_BAM_INDEX_OFF;
    SECEDO_CALL(index_mode(&imode));
    index_info() = secedo_bam_index_info{};
    in->paths = files;
    in->line0.assign(n_files, 0);
    in->indexed.assign(n_files, 0);
    in->chrs.resize(n_chr);
    for (uint32_t c = 0; c < n_chr; ++c) {
        ChrInput &ci = in->chrs[c];
        ci.chromosome = chromosome_ids[c];
        ci.file_base.assign(n_files, 0);
        ci.roff.assign(n_files, {});
        ci.rpos.assign(n_files, {});
        ci.ridx.assign(n_files, {});
    }
    std::vector<char> sam(n_files, kBam);  // the Kind of each file
    for (size_t f = 0; f < n_files; ++f) {
        Kind kind = kBam;
        SECEDO_CALL(sniff(files[f], &kind));
        sam[f] = kind;
    }
    // the index of every BAM, where one is asked for: which members of it are read
    std::vector<IndexPlan> plans(imode == SECEDO_BAM_INDEX_OFF ? 0 : n_files);
    for (size_t f = 0; f < plans.size(); ++f) {
        if (sam[f]) continue;
        SECEDO_CALL(plan_index(files[f], std::vector<uint32_t>(chromosome_ids, chromosome_ids + n_chr), imode,
                               &plans[f]));
        in->indexed[f] = plans[f].indexed;
    }
    SamWork sam_work;
    Runs runs(n_chr, std::vector<std::vector<uint8_t>>(n_files));
    size_t f0 = 0;
    while (f0 < n_files) {
        if (sam[f0]) {  // SAM text: parsed on the device in ranges of about `batch` bytes
            if (sam[f0] == kSamGz) SECEDO_CALL(load_samgz_file(f0, batch, &sam_work, in, &runs, t));
            else SECEDO_CALL(load_sam_file(f0, batch, &sam_work, in, &runs, t));
            ++f0;
            continue;
        }
        // a batch of BAM files of at most `batch` bytes on disk (BGZF inflates 3-4x), at least one file
        size_t f1 = f0;
        uint64_t disk = 0;
        if (!device && in->indexed[f0]) {  // through its index: only its spans' members
            SECEDO_CALL(load_file_spans(f0, plans[f0], threads, batch, in, &runs, t));
            plans[f0] = IndexPlan();
            ++f0;
            continue;
        }
        while (f1 < n_files && !sam[f1] && (f1 == f0 || disk < batch / 4) && (device || !in->indexed[f1])) {
            struct stat st;
            disk += stat(files[f1].c_str(), &st) == 0 ? uint64_t(st.st_size) : 0;
            ++f1;
        }
        if (device) {  // the opt-in route: device inflate, device walk (bam_device_input.cpp)
            SECEDO_CALL(load_bams_device(f0, f1, threads, batch, dev_work.get(), in, &runs, t,
                                         plans.empty() ? nullptr : &plans));
            f0 = f1;
            continue;
        }
        if (f1 == f0 + 1) {  // one file: walked in block ranges (one range when it inflates to at most `batch`)
            SECEDO_CALL(load_file_ranges(f0, threads, batch, in, &runs, t));
            f0 = f1;
            continue;
        }
        std::vector<Inflated> inf;
        Clock::time_point t0 = Clock::now();
        SECEDO_CALL(inflate_files(std::vector<std::string>(files.begin() + f0, files.begin() + f1), threads, &inf));
        if (t) {
            t->inflate_ms += ms_since(t0);
            for (auto &x : inf) t->inflated_bytes += double(x.data.size());
        }
        t0 = Clock::now();
        // g_error is per thread: each worker's message comes back to this one
        std::vector<int> rcs(inf.size(), SECEDO_OK);
        std::vector<std::string> errs(inf.size());
        parallel_for(threads, inf.size(), [&](uint64_t k) {
            WalkState st;
            FileSink sink(*in, f0 + k, runs);
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
    for (size_t c = 0; c < in->chrs.size(); ++c) {
        ChrInput &ci = in->chrs[c];
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

int read_file_header(const std::string &path, FileHeader *h) {
    Kind kind = kBam;
    SECEDO_CALL(sniff(path, &kind));
    h->sam = kind != kBam;
    if (kind == kBam) {
        IndexPlan plan;
        std::vector<uint8_t> head;
        SECEDO_CALL(map_file(path, &plan.m));
        SECEDO_CALL(read_header(path, &plan, &head));
        h->text.assign(reinterpret_cast<const char *>(head.data()) + 8, plan.h.l_text);
        h->n_ref = plan.h.n_ref;
        h->ref_list.assign(head.begin() + 8 + plan.h.l_text + 4, head.begin() + plan.h.first_record);
        return SECEDO_OK;
    }
    // SAM text: the leading '@' lines; of a BGZF SAM file its members are inflated until they end
    Mapped m;
    std::vector<uint8_t> head;
    const uint8_t *p = nullptr;
    uint64_t n = 0;
    if (kind == kSam) {
        SECEDO_CALL(map_file(path, &m));
        p = m.p, n = m.n;
    } else {
        std::vector<Block> blocks;
        uint64_t total = 0;
        SECEDO_CALL(open_bgzf(path, &m, &blocks, &total));
        size_t hb = 0;
        SECEDO_CALL(inflate_sam_head(path, m, blocks, &head, &hb));
        p = head.data(), n = head.size();
    }
    uint64_t o = 0;
    while (o < n && p[o] == '@') {
        const uint8_t *nl = static_cast<const uint8_t *>(std::memchr(p + o, '\n', n - o));
        o = nl ? uint64_t(nl - p) + 1 : n;
    }
    h->text.assign(reinterpret_cast<const char *>(p), o);
    return SECEDO_OK;
}

}  // namespace bam_host
}  // namespace secedo

extern "C" int secedo_bam_scan(const char *path, uint32_t num_threads, secedo_bam_scan_info *info,
                               uint64_t *records_per_ref, uint32_t capacity) {
    if (!path || !info) return fail(SECEDO_E_INVALID_ARG, "null argument");
    route() = secedo_bam_route_info{};
    std::vector<Inflated> inf;
    SECEDO_CALL(inflate_files({std::string(path)}, num_threads ? num_threads : 1, &inf));
    const std::vector<uint8_t> &d = inf[0].data;
    WalkState st;
    st.require_sorted = false;  // counted to the end either way; st.sorted says which it was
    SECEDO_CALL(parse_header(inf[0].path, d.data(), d.size(), true, &st.h));
    st.have_header = true;
    const Header &h = st.h;
    std::vector<uint64_t> per(h.n_ref, 0);
    uint64_t unmapped = 0, used = 0;
    const auto count = [&](uint64_t, const uint8_t *, int32_t ref, int32_t) {
        if (ref < 0) ++unmapped;
        else if (uint32_t(ref) < h.n_ref) ++per[ref];
        return SECEDO_OK;
    };
    SECEDO_CALL(walk_range(inf[0].path, d.data() + h.first_record, d.size() - h.first_record, true, &st, &used, count));
    info->n_ref = h.n_ref;
    info->sorted = st.sorted ? 1 : 0;
    info->n_records = st.idx;
    info->n_unmapped = unmapped;
    info->n_blocks = inf[0].n_blocks;
    info->inflated_bytes = d.size();
    info->l_text = h.l_text;
    info->reserved = 0;
    if (records_per_ref)
        for (uint32_t r = 0; r < std::min(capacity, h.n_ref); ++r) records_per_ref[r] = per[r];
    return SECEDO_OK;
}

extern "C" int secedo_bam_set_inflate(int mode) {
    if (mode != SECEDO_BAM_INFLATE_HOST && mode != SECEDO_BAM_INFLATE_DEVICE)
        return fail(SECEDO_E_INVALID_ARG, "secedo_bam_set_inflate: mode " + std::to_string(mode) +
                                              " is neither SECEDO_BAM_INFLATE_HOST nor SECEDO_BAM_INFLATE_DEVICE");
    secedo::bam_host::g_inflate_mode.store(mode);
    return SECEDO_OK;
}

extern "C" int secedo_bam_get_inflate(int *mode) {
    if (!mode) return fail(SECEDO_E_INVALID_ARG, "null argument");
    bool device = false;
    SECEDO_CALL(inflate_route(&device));
    *mode = device ? SECEDO_BAM_INFLATE_DEVICE : SECEDO_BAM_INFLATE_HOST;
    return SECEDO_OK;
}

extern "C" int secedo_bam_set_index(int mode) {
    if (mode != SECEDO_BAM_INDEX_OFF && mode != SECEDO_BAM_INDEX_AUTO && mode != SECEDO_BAM_INDEX_REQUIRE)
        return fail(SECEDO_E_INVALID_ARG, "secedo_bam_set_index: mode " + std::to_string(mode) +
                                              " is none of SECEDO_BAM_INDEX_OFF, _AUTO and _REQUIRE");
    secedo::bam_host::g_index_mode.store(mode);
    return SECEDO_OK;
}

extern "C" int secedo_bam_get_index(int *mode) {
    if (!mode) return fail(SECEDO_E_INVALID_ARG, "null argument");
    return index_mode(mode);
}

extern "C" int secedo_bam_index_stats(secedo_bam_index_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = index_info();
    return SECEDO_OK;
}

extern "C" int secedo_bam_index_ranges(const char *bam_path, uint32_t *n_ref, uint64_t *beg, uint64_t *end,
                                       uint64_t *count, uint32_t capacity) {
    if (!bam_path || !n_ref) return fail(SECEDO_E_INVALID_ARG, "null argument");
    const std::string path(bam_path);
    IndexPlan plan;
    SECEDO_CALL(map_file(path, &plan.m));
    SECEDO_CALL(read_header(path, &plan));
    std::vector<secedo::bamindex::RefRange> refs;
    bool found = false;
    const std::string why = read_index(path, plan.m, plan.h.n_ref, &refs, &found);
    if (!why.empty()) return fail(SECEDO_E_INVALID_ARG, path + ": no usable index: " + why);
    *n_ref = uint32_t(refs.size());
    for (uint32_t r = 0; r < std::min<uint64_t>(capacity, refs.size()); ++r) {
        if (beg) beg[r] = refs[r].beg;
        if (end) end[r] = refs[r].end;
        if (count) count[r] = refs[r].count;
    }
    return SECEDO_OK;
}

extern "C" int secedo_bam_route_stats(secedo_bam_route_info *out) {
    if (!out) return fail(SECEDO_E_INVALID_ARG, "null argument");
    *out = route();
    return SECEDO_OK;
}

extern "C" int secedo_bgzf_inflate(const char *path, uint64_t *bytes) {
    if (!path || !bytes) return fail(SECEDO_E_INVALID_ARG, "null argument");
    secedo::bam_host::release_inflated();
    Mapped m;
    std::vector<Block> blocks;
    uint64_t total = 0;
    SECEDO_CALL(open_bgzf(path, &m, &blocks, &total));
    std::unique_ptr<InflatedFile> res(new InflatedFile);
    StreamGuard sg;
    SECEDO_TRY(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    SECEDO_TRY(res->data.alloc(total));
    res->n = total;
    GzWork g;
    const uint64_t batch = batch_bytes();
    for (size_t b0 = 0; b0 < blocks.size();) {
        const size_t b1 = bm::next_range(blocks, b0, batch);
        SECEDO_CALL(inflate_range_device(path, m, blocks, b0, b1, &g, res->data.p, blocks[b0].out, sg.s, nullptr));
        b0 = b1;
    }
    *bytes = total;
    g_inflated = res.release();
    return SECEDO_OK;
}

extern "C" int secedo_bgzf_inflate_fetch(uint8_t *dst) {
    const InflatedFile *r = g_inflated;
    if (!r) return fail(SECEDO_E_STATE, "no secedo_bgzf_inflate result on this thread");
    if (dst && r->n) SECEDO_TRY(hipMemcpy(dst, r->data.p, r->n, hipMemcpyDefault));
    return SECEDO_OK;
}
