// pileup_load.cpp -- host side of include/secedo_pileup.h: the reference's binary pileup files straight into HBM.
//
// Per file (in slot order): bounded reads into pinned staging, a walk over the 6-byte record headers that finds the
// chunk's complete records (a record cut by the end of the staging moves to the front of the next chunk), one
// upload of the bytes and the record starts, and the device passes of pileup_device.hip. The read and walk of chunk
// k + 1 overlap the upload and decode of chunk k; one small read-back per chunk (its totals) carries the locus and
// entry bases and the position max-scan into the next. The end of a file follows secedo_pileup_read: fewer than 6
// bytes left end it silently, a record whose payload is cut is "truncated binary pileup record" unless the position
// list ended the file before it, and a kept cell id past id_to_group reports the first one in file order.
#include "secedo_pileup.h"
#include "secedo_simmat.h"
#include "host_util.hpp"
#include "pileup_device.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace secedo::pileup;
using namespace secedo::host;

// buffers that grow chunk after chunk (the result keeps its prefix): by half, from 1024 elements
template <class T>
using Grown = Dev<T, 150, 1024>;

constexpr uint64_t kDefaultStaging = 64ull << 20;
constexpr uint64_t kMaxStaging = 1ull << 30;
constexpr uint64_t kMaxRecord = 6 + 6 * 65535ull;  // the longest record: coverage 65535

inline uint16_t rd16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }

struct Result {
    std::vector<uint32_t> chr_locus_off{0};
    Grown<uint32_t> pos, rid;
    Grown<uint64_t> off;
    Grown<uint16_t> idb;
    uint64_t n_loci = 0, n_entries = 0;
};

thread_local Result *g_result = nullptr;

// Pinned staging, kept across calls of a thread: two byte buffers and two record-start lists. Never freed at
// thread exit (the HIP runtime may be gone by then); a new size replaces it.
struct Staging {
    uint64_t cap = 0;
    uint8_t *buf[2] = {nullptr, nullptr};
    uint32_t *rec[2] = {nullptr, nullptr};
    void release() {
        for (int i = 0; i < 2; ++i) {
            if (buf[i]) (void)hipHostFree(buf[i]);
            if (rec[i]) (void)hipHostFree(rec[i]);
            buf[i] = nullptr;
            rec[i] = nullptr;
        }
        cap = 0;
    }
    hipError_t ensure(uint64_t bytes) {
        if (cap == bytes) return hipSuccess;
        release();
        for (int i = 0; i < 2; ++i) {
            hipError_t e = hipHostMalloc((void **)&buf[i], bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc((void **)&rec[i], (bytes / 6 + 1) * 4, hipHostMallocDefault);
            if (e != hipSuccess) {
                release();
                return e;
            }
        }
        cap = bytes;
        return hipSuccess;
    }
};

thread_local Staging g_staging;

// One host chunk: bytes [0, have) of which [0, complete) are whole records starting at rec[0..n).
struct HostChunk {
    uint8_t *buf;
    uint32_t *rec;
    uint64_t have = 0, complete = 0, upper_entries = 0;
    uint32_t n = 0;
};

struct Reader {
    FILE *f = nullptr;
    bool eof = false;
    uint64_t staging = 0, cap = 0;
    uint32_t max_coverage = 0;
    double read_ms = 0, walk_ms = 0;
    ~Reader() {
        if (f) std::fclose(f);
    }
    void walk(HostChunk &c) {
        const Clock::time_point t0 = Clock::now();
        uint64_t o = 0;
        c.n = 0;
        c.upper_entries = 0;
        while (o + 6 <= c.have) {
            const uint32_t cov = rd16(c.buf + o + 4);
            const uint64_t len = 6 + 6ull * cov;
            if (o + len > c.have) break;
            c.rec[c.n++] = (uint32_t)o;
            if (cov <= max_coverage) c.upper_entries += cov;
            o += len;
        }
        c.complete = o;
        walk_ms += ms_since(t0);
    }
    // appends up to `staging` bytes (more while no whole record is in the chunk), then walks it
    void fill(HostChunk &c) {
        bool first = true;
        while (!eof && (first || c.n == 0) && c.have < cap) {
            const Clock::time_point t0 = Clock::now();
            const uint64_t want = std::min<uint64_t>(staging, cap - c.have);
            const size_t got = std::fread(c.buf + c.have, 1, want, f);
            read_ms += ms_since(t0);
            c.have += got;
            if (got < want) eof = true;
            walk(c);
            first = false;
        }
        if (first) walk(c);
    }
};

struct EventGuard {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~EventGuard() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

struct PinnedSmall {
    void *p = nullptr;
    ~PinnedSmall() {
        if (p) (void)hipHostFree(p);
    }
};

struct Ctx {
    hipStream_t s;
    hipEvent_t ev[3];
    Grown<uint16_t> bytes;
    Grown<uint32_t> positions;
    Dev<uint32_t> rec, pos, cov, mval, mscan, keep, lidx;
    Dev<uint64_t> cnt, eoff;
    Dev<uint8_t> tmp;
    uint64_t scratch_n = 0;
    const uint16_t *i2g;
    uint32_t n_ids, max_coverage;
    FileState *d_state;
    ChunkTail *d_tail;
    FileState *h_state;
    ChunkTail *h_tail;
    double upload_ms = 0, device_ms = 0;
};

hipError_t ensure_scratch(Ctx &x, uint64_t n) {
    if (n <= x.scratch_n) return hipSuccess;
    const uint64_t m = std::max<uint64_t>(n, 4096);
    hipError_t e;
    if ((e = x.rec.alloc(m)) != hipSuccess || (e = x.pos.alloc(m)) != hipSuccess || (e = x.cov.alloc(m)) != hipSuccess ||
        (e = x.mval.alloc(m)) != hipSuccess || (e = x.mscan.alloc(m)) != hipSuccess ||
        (e = x.keep.alloc(m)) != hipSuccess || (e = x.lidx.alloc(m)) != hipSuccess ||
        (e = x.cnt.alloc(m)) != hipSuccess || (e = x.eoff.alloc(m)) != hipSuccess ||
        (e = x.tmp.alloc(scan_bytes(m))) != hipSuccess)
        return e;
    x.scratch_n = m;
    return hipSuccess;
}

double elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0;
}

// One file appended to the result; *num_cells and *max_len as secedo_pileup_read reports them.
int load_file(Ctx &x, Result &r, const char *path, const uint32_t *positions, uint64_t n_positions, bool want_len,
              uint64_t staging, uint32_t *num_cells, uint32_t *max_len, double *read_ms, double *walk_ms) {
    Reader rd;
    rd.f = std::fopen(path, "rb");
    if (!rd.f) return fail(SECEDO_E_INVALID_ARG, std::string("File ") + path + " does not exist or is not readable.");
    rd.staging = staging;
    rd.cap = staging + kMaxRecord;
    rd.max_coverage = x.max_coverage;
    SECEDO_TRY(g_staging.ensure(rd.cap));
    const hipStream_t s = x.s;
    SECEDO_TRY(x.positions.grow(std::max<uint64_t>(n_positions, 1), 0, s));
    if (n_positions) SECEDO_TRY(hipMemcpyAsync(x.positions.p, positions, n_positions * 4, hipMemcpyHostToDevice, s));
    FileState init{};
    init.err_key = kNoError;
    *x.h_state = init;
    SECEDO_TRY(hipMemcpyAsync(x.d_state, x.h_state, sizeof(FileState), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));

    const uint64_t l0 = r.n_loci, e0 = r.n_entries;
    uint64_t rec_base = 0;
    uint32_t carry = 0;
    HostChunk chunk[2] = {{g_staging.buf[0], g_staging.rec[0]}, {g_staging.buf[1], g_staging.rec[1]}};
    int cur = 0;
    rd.fill(chunk[cur]);
    while (true) {
        HostChunk &c = chunk[cur];
        const bool launched = c.n > 0;
        if (launched) {
            if (r.n_loci + c.n >= (1ull << 32)) return fail(SECEDO_E_LIMIT, "more than 2^32 - 1 loci");
            SECEDO_TRY(ensure_scratch(x, c.n));
            SECEDO_TRY(r.pos.grow(r.n_loci + c.n, r.n_loci, s));
            SECEDO_TRY(r.off.grow(r.n_loci + c.n + 1, r.n_loci, s));
            SECEDO_TRY(r.rid.grow(r.n_entries + c.upper_entries, r.n_entries, s));
            SECEDO_TRY(r.idb.grow(r.n_entries + c.upper_entries, r.n_entries, s));
            SECEDO_TRY(x.bytes.grow((c.complete + 1) / 2, 0, s));
            SECEDO_TRY(hipEventRecord(x.ev[0], s));
            SECEDO_TRY(hipMemcpyAsync(x.bytes.p, c.buf, c.complete, hipMemcpyHostToDevice, s));
            SECEDO_TRY(hipMemcpyAsync(x.rec.p, c.rec, (size_t)c.n * 4, hipMemcpyHostToDevice, s));
            SECEDO_TRY(hipEventRecord(x.ev[1], s));
            Chunk dc{x.bytes.p, x.rec.p, c.n, rec_base};
            ChunkScratch w{x.pos.p, x.cov.p, x.mval.p, x.mscan.p, x.keep.p, x.lidx.p, x.cnt.p, x.eoff.p, x.tmp.p,
                           (size_t)x.tmp.n};
            SECEDO_TRY(decode_chunk(dc, w, x.max_coverage, x.positions.p, n_positions, carry, r.n_loci, r.n_entries, x.i2g,
                                x.n_ids, r.pos.p, r.off.p, r.rid.p, r.idb.p, x.d_state, x.d_tail, s));
            SECEDO_TRY(hipEventRecord(x.ev[2], s));
            SECEDO_TRY(hipMemcpyAsync(x.h_tail, x.d_tail, sizeof(ChunkTail), hipMemcpyDeviceToHost, s));
        }
        // the next chunk: the cut record first, then new bytes; read and walked while the device works
        HostChunk &nx = chunk[1 - cur];
        nx.have = c.have - c.complete;
        if (nx.have) std::memcpy(nx.buf, c.buf + c.complete, nx.have);
        nx.n = 0;
        rd.fill(nx);
        if (launched) {
            SECEDO_TRY(hipStreamSynchronize(s));
            x.upload_ms += elapsed(x.ev[0], x.ev[1]);
            x.device_ms += elapsed(x.ev[1], x.ev[2]);
            r.n_loci += x.h_tail->loci;
            r.n_entries += x.h_tail->entries;
            carry = x.h_tail->max_pos;
            rec_base += c.n;
        }
        cur = 1 - cur;
        if (chunk[cur].n == 0 && rd.eof) break;
    }
    *read_ms += rd.read_ms;
    *walk_ms += rd.walk_ms;
    SECEDO_TRY(hipMemcpyAsync(x.h_state, x.d_state, sizeof(FileState), hipMemcpyDeviceToHost, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    const FileState st = *x.h_state;
    if (st.err_key != kNoError)
        return fail(SECEDO_E_INVALID_ARG, "Cell id " + std::to_string(st.err_key & 0x3FFFu) +
                                              " is too large for the id_to_group mapping");
    const HostChunk &left = chunk[cur];
    if (left.have >= 6 && !st.stopped) return fail(SECEDO_E_INVALID_ARG, "truncated binary pileup record");
    *num_cells = std::max<uint32_t>(st.max_cell_plus1, 1);
    if (!want_len) {
        *max_len = 1000;
        return SECEDO_OK;
    }
    const uint64_t n_loci = r.n_loci - l0, n_entries = r.n_entries - e0;
    if (n_entries == 0) {
        *max_len = 0;
        return SECEDO_OK;
    }
    // the file's own last offset, so the span passes see off[l0 + n_loci]
    SECEDO_TRY(r.off.grow(r.n_loci + 1, r.n_loci, s));
    uint64_t end = r.n_entries;
    SECEDO_TRY(hipMemcpy(r.off.p + r.n_loci, &end, 8, hipMemcpyHostToDevice));
    SECEDO_TRY(hipEventRecord(x.ev[1], s));
    const uint64_t table = (uint64_t)st.max_rid + 1;
    if (table <= 4 * n_entries + 1024 && table <= 0xFFFFFFFFull) {
        Dev<uint32_t> first, last;
        SECEDO_TRY(first.alloc(table));
        SECEDO_TRY(last.alloc(table));
        SECEDO_TRY(spans_dense(r.pos.p, r.off.p, r.rid.p, l0, (uint32_t)n_loci, first.p, last.p, (uint32_t)table,
                           x.d_state, s));
        SECEDO_TRY(hipEventRecord(x.ev[2], s));
        SECEDO_TRY(hipMemcpyAsync(x.h_state, x.d_state, sizeof(FileState), hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
    } else {
        Dev<uint64_t> keys;
        Dev<uint8_t> tmp;
        SECEDO_TRY(keys.alloc(2 * n_entries));
        const size_t tb = sort_bytes(n_entries);
        SECEDO_TRY(tmp.alloc(tb));
        SECEDO_TRY(spans_sparse(r.pos.p, r.off.p, r.rid.p, l0, (uint32_t)n_loci, e0, n_entries, keys.p, tmp.p, tb,
                            x.d_state, s));
        SECEDO_TRY(hipEventRecord(x.ev[2], s));
        SECEDO_TRY(hipMemcpyAsync(x.h_state, x.d_state, sizeof(FileState), hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
    }
    x.device_ms += elapsed(x.ev[1], x.ev[2]);
    *max_len = x.h_state->max_span;
    return SECEDO_OK;
}

}  // namespace

extern "C" {

const char *secedo_pileup_load_last_error(void) { return g_error.c_str(); }

int secedo_pileup_load_device(const char *const *bin_files, uint32_t n_files, const uint32_t *slot_of_file,
                              uint32_t n_slots, const uint16_t *id_to_group, uint32_t n_ids, uint32_t max_coverage,
                              const uint32_t *const *positions, const uint64_t *n_positions,
                              int compute_max_read_len, uint64_t staging_bytes, secedo_pileup_load_info *info,
                              uint32_t *num_cells, uint32_t *max_read_length, secedo_pileup_load_times *times) {
    const Clock::time_point t_all = Clock::now();
    if (!info || (n_files && (!bin_files || !slot_of_file || !num_cells || !max_read_length)) ||
        (!id_to_group && n_ids))
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    std::vector<int64_t> file_of_slot(n_slots, -1);
    for (uint32_t i = 0; i < n_files; ++i) {
        if (!bin_files[i]) return fail(SECEDO_E_INVALID_ARG, "null file name");
        const uint32_t slot = slot_of_file[i];
        if (slot >= n_slots) return fail(SECEDO_E_INVALID_ARG, "slot " + std::to_string(slot) + " >= n_slots");
        if (file_of_slot[slot] >= 0)
            return fail(SECEDO_E_INVALID_ARG, "two files for slot " + std::to_string(slot));
        file_of_slot[slot] = i;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return fail(SECEDO_E_NO_DEVICE, "no HIP device");
    uint64_t staging = staging_bytes ? std::min(staging_bytes, kMaxStaging) : kDefaultStaging;

    delete g_result;
    g_result = new Result();
    Result &r = *g_result;
    r.chr_locus_off.assign(n_slots + 1, 0);
    StreamGuard sg;
    SECEDO_TRY(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    EventGuard eg;
    for (hipEvent_t &e : eg.e) SECEDO_TRY(hipEventCreate(&e));
    Ctx x{};
    x.s = sg.s;
    std::copy(eg.e, eg.e + 3, x.ev);
    x.n_ids = n_ids;
    x.max_coverage = max_coverage;
    Dev<uint16_t> d_i2g;
    SECEDO_TRY(d_i2g.alloc(n_ids));
    if (n_ids) SECEDO_TRY(hipMemcpy(d_i2g.p, id_to_group, n_ids * 2ull, hipMemcpyHostToDevice));
    x.i2g = d_i2g.p;
    Dev<uint8_t> d_small;
    SECEDO_TRY(d_small.alloc(sizeof(FileState) + sizeof(ChunkTail)));
    x.d_state = reinterpret_cast<FileState *>(d_small.p);
    x.d_tail = reinterpret_cast<ChunkTail *>(d_small.p + sizeof(FileState));
    PinnedSmall h_small;
    SECEDO_TRY(hipHostMalloc(&h_small.p, sizeof(FileState) + sizeof(ChunkTail), hipHostMallocDefault));
    x.h_state = reinterpret_cast<FileState *>(h_small.p);
    x.h_tail = reinterpret_cast<ChunkTail *>(static_cast<uint8_t *>(h_small.p) + sizeof(FileState));

    double read_ms = 0, walk_ms = 0;
    for (uint32_t slot = 0; slot < n_slots; ++slot) {
        const int64_t i = file_of_slot[slot];
        if (i >= 0) {
            const uint32_t *p = positions ? positions[i] : nullptr;
            const uint64_t np = (p && n_positions) ? n_positions[i] : 0;
            SECEDO_CALL(load_file(x, r, bin_files[i], p, np, compute_max_read_len != 0, staging, &num_cells[i],
                              &max_read_length[i], &read_ms, &walk_ms));
        }
        r.chr_locus_off[slot + 1] = (uint32_t)r.n_loci;
    }
    SECEDO_TRY(r.pos.grow(std::max<uint64_t>(r.n_loci, 1), r.n_loci, x.s));
    SECEDO_TRY(r.off.grow(r.n_loci + 1, r.n_loci, x.s));
    SECEDO_TRY(r.rid.grow(std::max<uint64_t>(r.n_entries, 1), r.n_entries, x.s));
    SECEDO_TRY(r.idb.grow(std::max<uint64_t>(r.n_entries, 1), r.n_entries, x.s));
    const uint64_t end = r.n_entries;
    SECEDO_TRY(hipMemcpy(r.off.p + r.n_loci, &end, 8, hipMemcpyHostToDevice));
    info->n_loci = r.n_loci;
    info->n_entries = r.n_entries;
    if (times) {
        times->read_ms = read_ms;
        times->walk_ms = walk_ms;
        times->upload_ms = x.upload_ms;
        times->device_ms = x.device_ms;
        times->total_ms = ms_since(t_all);
    }
    return SECEDO_OK;
}

int secedo_pileup_load_fetch(uint32_t *chr_locus_off, uint32_t *locus_pos, uint64_t *locus_entry_off,
                             uint32_t *read_ids, uint16_t *id_base16) {
    const Result *r = g_result;
    if (!r) return fail(SECEDO_E_STATE, "no pileup load result on this thread");
    if (chr_locus_off)
        SECEDO_TRY(hipMemcpy(chr_locus_off, r->chr_locus_off.data(), r->chr_locus_off.size() * 4, hipMemcpyDefault));
    if (locus_pos && r->n_loci) SECEDO_TRY(hipMemcpy(locus_pos, r->pos.p, r->n_loci * 4, hipMemcpyDefault));
    if (locus_entry_off) SECEDO_TRY(hipMemcpy(locus_entry_off, r->off.p, (r->n_loci + 1) * 8, hipMemcpyDefault));
    if (read_ids && r->n_entries) SECEDO_TRY(hipMemcpy(read_ids, r->rid.p, r->n_entries * 4, hipMemcpyDefault));
    if (id_base16 && r->n_entries) SECEDO_TRY(hipMemcpy(id_base16, r->idb.p, r->n_entries * 2, hipMemcpyDefault));
    return SECEDO_OK;
}

void secedo_pileup_load_release(void) {
    delete g_result;
    g_result = nullptr;
}

}  // extern "C"
