// simmat_one_shot.cpp -- secedo_simmat_compute, the call with the reference's signature, and what it keeps between
// calls: the pool of handles, the pinned staging buffers, the pipelined download of the matrix, the device list
// (secedo_simmat_set_devices, SECEDO_GPUS, SECEDO_DEVICE) and the lanes that drive several devices.
#include "simmat_handle.hpp"

#if defined(__linux__)
#include <sys/mman.h>
#endif

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <functional>
#include <map>
#include <mutex>
#include <thread>

using namespace secedo::host;

namespace secedo { void em_release_cache(); }  // em_device.hip

namespace {

// the pileup comes as the FlatPileupView it is; the rest of what the reference's signature passes
struct OneShotParams {
    uint32_t num_cells, max_fragment_length;
    double mutation_rate, homozygous_rate, seq_error_rate;
    uint32_t num_threads;
    int normalization;
};

// Handles kept for secedo_simmat_compute, one per device, handed out to one caller at a time (a second
// concurrent caller on the same device gets a fresh handle). Deliberately not destroyed at process
// exit: static destructors would run after the HIP runtime is gone; the driver reclaims the memory.
// secedo_simmat_release_cache() frees them on request. SECEDO_ONE_SHOT_CACHE=0 turns the pool off.
std::mutex g_pool_mutex;
std::map<int, secedo_simmat_t *> &g_pool = *new std::map<int, secedo_simmat_t *>();

bool pool_enabled() { return env_enabled("SECEDO_ONE_SHOT_CACHE"); }

// key: the device, or -- for the lanes of a multi-device call -- a number of its own per lane (kLaneKey)
constexpr int kLaneKey = 1 << 16;
int one_shot_acquire(int key, int device, secedo_simmat_t **h) {
    if (pool_enabled()) {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        auto it = g_pool.find(key);
        if (it != g_pool.end() && it->second) {
            *h = it->second;
            it->second = nullptr;
            return SECEDO_OK;
        }
    }
    return secedo_simmat_create(h, device);
}

void one_shot_release(int key, secedo_simmat_t *h, bool ok) {
    if (!h) return;
    if (ok && pool_enabled()) {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        secedo_simmat_t *&slot = g_pool[key];
        if (!slot) {
            slot = h;
            return;
        }
    }
    secedo_simmat_destroy(h);
}

// ---- pinned host memory kept between one-shot calls: the caller's staging (five buffers) and the bounce ring of
// the matrix download
std::mutex g_staging_mutex;
bool g_staging_busy = false;
PinnedBuf g_staging[5];
// page-locked rings of the matrix download: [0] the single-device call's, [1 + k] lane k's of a multi-device call;
// each guarded by its mutex for the duration of a download
struct Bounce {
    PinnedBuf buf;
    std::mutex mutex;
};
Bounce g_bounce[1 + kMaxLanes];

}  // namespace

// d_src (device) -> dst (pageable host memory, typically the fresh pages of the caller's matrix): chunks go
// through a page-locked ring by DMA while `threads` host threads copy the chunk before out of the ring, each
// its own slice -- touching the destination's fresh pages in parallel is what a single-threaded copy into
// pageable memory cannot do (12-20 GB/s for hipMemcpy on the 512 MB of C3).
hipError_t secedo::host::download_pipelined(const void *d_src, void *dst, size_t bytes, unsigned threads, int ring) {
    constexpr size_t kChunk = 32u << 20;
    constexpr int kSlots = 4;
    std::lock_guard<std::mutex> lock(g_bounce[ring].mutex);
    PinnedBuf &bounce = g_bounce[ring].buf;
    hipError_t e = bounce.ensure(kChunk * kSlots);
    if (e != hipSuccess) {  // no pinned memory to be had: the plain copy
        (void)hipGetLastError();
        return hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost);
    }
#if defined(__linux__)
    {   // huge pages for the destination where the kernel grants them on request: 2 MiB faults instead of 4 KiB
        const uintptr_t a = (reinterpret_cast<uintptr_t>(dst) + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
        const uintptr_t b = (reinterpret_cast<uintptr_t>(dst) + bytes) & ~(uintptr_t)((2u << 20) - 1);
        if (b > a) (void)madvise(reinterpret_cast<void *>(a), b - a, MADV_HUGEPAGE);
    }
#endif
    // (one stream: alternating the chunks between two measured SLOWER on the MI355X, 17-23 ms against 14-15 for the
    // 512 MB of C3 -- one stream moves 34-36 GB/s and a second one only gets in its way)
    hipStream_t s = nullptr;
    hipEvent_t ev[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) return e;
    for (int i = 0; i < kSlots && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    const size_t n_chunks = (bytes + kChunk - 1) / kChunk;
    threads = std::max(1u, std::min(threads, 16u));
    auto issue = [&](size_t c) {
        const size_t off = c * kChunk, len = std::min(kChunk, bytes - off);
        hipError_t r = hipMemcpyAsync(static_cast<char *>(bounce.p) + (c % kSlots) * kChunk,
                                      static_cast<const char *>(d_src) + off, len, hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipEventRecord(ev[c % kSlots], s);
        return r;
    };
    // The copying threads live for the whole download (round 4: a team per chunk was 16 x 7 thread starts and joins,
    // a fifth of the 14 ms of a C3 matrix): thread t copies slice t of every chunk as soon as the chunk has landed
    // (`landed`, published by this thread after the chunk's event), and a ring slot is written again only when every
    // thread is done with the chunk that used it (`copied`).
    std::atomic<size_t> landed{0};
    std::atomic<bool> give_up{false};
    std::vector<std::atomic<unsigned>> copied(n_chunks);
    for (auto &c : copied) c.store(0);
    auto copier = [&](unsigned t) {
        for (size_t c = 0; c < n_chunks; ++c) {
            while (landed.load(std::memory_order_acquire) <= c) {
                if (give_up.load(std::memory_order_relaxed)) return;
                std::this_thread::yield();
            }
            const size_t off = c * kChunk, len = std::min(kChunk, bytes - off);
            const char *src = static_cast<const char *>(bounce.p) + (c % kSlots) * kChunk;
            char *out = static_cast<char *>(dst) + off;
            const size_t slice = ((len + threads - 1) / threads + 4095) & ~(size_t)4095;
            const size_t lo = std::min(len, (size_t)t * slice), hi = std::min(len, ((size_t)t + 1) * slice);
            if (hi > lo) std::memcpy(out + lo, src + lo, hi - lo);
            copied[c].fetch_add(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t) pool.emplace_back(copier, t);
    for (size_t c = 0; c < std::min<size_t>(kSlots - 1, n_chunks) && e == hipSuccess; ++c) e = issue(c);
    for (size_t c = 0; c < n_chunks && e == hipSuccess; ++c) {
        if (c + kSlots - 1 < n_chunks) {  // its slot held chunk c - 1
            while (c > 0 && copied[c - 1].load(std::memory_order_acquire) < threads) std::this_thread::yield();
            e = issue(c + kSlots - 1);
        }
        if (e == hipSuccess) e = hipEventSynchronize(ev[c % kSlots]);
        if (e != hipSuccess) break;
        landed.store(c + 1, std::memory_order_release);
    }
    if (e != hipSuccess) give_up.store(true);
    for (auto &th : pool) th.join();
    (void)hipStreamSynchronize(s);
    for (int i = 0; i < kSlots; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    (void)hipStreamDestroy(s);
    return e;
}

// ------------------------------------------------------------------------------------------------
// Several GPUs behind the one-shot call (north_star: "the N x N output is block-partitioned across the 8 GPUs of
// one node"; SURVEY.md 8b set_devices, section 5 SECEDO_GPUS). The reference's caller (spectral_clustering.cpp:
// 354-356) keeps calling computeSimilarityMatrix() with the same signature; ONE process drives N devices, a host
// thread ("lane") per device:
//   1. every lane uploads the flat pileup to its device and packs it there (the packing is replicated, the
//      lanes run side by side: nothing travels between devices before the accumulators exist);
//   2. lane k stores its contiguous range of upper-triangular tiles into its own tile-major int64 accumulator,
//      in kChunks launches with an event behind each;
//   3. every lane pulls the other lanes' tiles into its accumulator chunk by chunk as their events fire
//      (hipMemcpyPeerAsync over xGMI on a copy stream of its own: the all-gather of SURVEY 8e as N x (N - 1)
//      direct copies, which point-to-point links serve better than a ring), so that the exchange of a lane's
//      first chunks runs behind the accumulation of its later ones;
//   4. every lane normalises ITS block of rows from the complete accumulator (the maximum ADD_MIN / SCALE_MAX_1
//      need is taken over all tiles on every device: no scalar exchange) and downloads it straight into its
//      rows of the caller's matrix -- N downloads over N PCIe links instead of one.
// Integer accumulators make the result bit-identical to the single-device call whatever N is; a device may be
// listed more than once (that is how the one-GPU test box runs this code: tests/test_gpu_multi_device.py).
// ------------------------------------------------------------------------------------------------
namespace {

std::mutex g_devices_mutex;
std::vector<int> g_devices;     // secedo_simmat_set_devices; empty: SECEDO_GPUS, else SECEDO_DEVICE, else 0
std::mutex g_multi_mutex;       // one multi-device call at a time (the lanes' rings and pool slots are per lane)

int parse_device_list(const char *text, std::vector<int> *out) {
    out->clear();
    const std::string t(text);
    if (t.find(',') == std::string::npos) {  // a count: devices 0 .. N - 1
        char *end = nullptr;
        const long n = std::strtol(t.c_str(), &end, 10);
        if (end == t.c_str() || *end != '\0' || n < 1 || n > kMaxLanes)
            return fail(SECEDO_E_INVALID_ARG, "SECEDO_GPUS must be a count 1.." + std::to_string(kMaxLanes) + " or a comma-separated list of device ids");
        for (long i = 0; i < n; ++i) out->push_back(static_cast<int>(i));
        return SECEDO_OK;
    }
    size_t pos = 0;
    while (pos <= t.size()) {
        const size_t comma = std::min(t.find(',', pos), t.size());
        const std::string item = t.substr(pos, comma - pos);
        char *end = nullptr;
        const long v = std::strtol(item.c_str(), &end, 10);
        if (item.empty() || *end != '\0' || v < 0) return fail(SECEDO_E_INVALID_ARG, "SECEDO_GPUS: bad device id '" + item + "'");
        out->push_back(static_cast<int>(v));
        pos = comma + 1;
    }
    if (out->empty() || out->size() > static_cast<size_t>(kMaxLanes)) return fail(SECEDO_E_INVALID_ARG, "SECEDO_GPUS: 1.." + std::to_string(kMaxLanes) + " devices");
    return SECEDO_OK;
}

int check_devices(const std::vector<int> &ids) {
    const int n = secedo_simmat_device_count();
    if (n <= 0) return no_device("the similarity-matrix path");
    for (int d : ids)
        if (d < 0 || d >= n) return fail(SECEDO_E_NO_DEVICE, "device id " + std::to_string(d) + " out of range (" + std::to_string(n) + " visible)");
    return SECEDO_OK;
}

// the devices of the one-shot call
int one_shot_devices(std::vector<int> *out) {
    {
        std::lock_guard<std::mutex> lock(g_devices_mutex);
        *out = g_devices;
    }
    if (out->empty()) {
        if (const char *env = std::getenv("SECEDO_GPUS")) SECEDO_CALL(parse_device_list(env, out));
        else out->assign(1, env_int("SECEDO_DEVICE", 0));
    }
    if (out->size() > 1) return check_devices(*out);
    return SECEDO_OK;  // (one device: secedo_simmat_create checks it)
}

class HostBarrier {
public:
    explicit HostBarrier(unsigned n) : n_(n) {}
    void wait() {
        std::unique_lock<std::mutex> lock(m_);
        const unsigned gen = gen_;
        if (++count_ == n_) {
            count_ = 0;
            ++gen_;
            cv_.notify_all();
        } else {
            cv_.wait(lock, [&] { return gen_ != gen; });
        }
    }
private:
    std::mutex m_;
    std::condition_variable cv_;
    unsigned n_, count_ = 0, gen_ = 0;
};

constexpr uint32_t kChunks = 4;

struct Lane {
    uint32_t k = 0;                          // its number
    int device = 0;
    secedo_simmat_t *h = nullptr;
    hipStream_t s = nullptr, sc = nullptr;   // accumulation / exchange + normalisation
    std::vector<hipEvent_t> done;            // behind each chunk of the lane's tiles
    uint32_t lo = 0, hi = 0;                 // its tiles ...
    uint32_t tiles = 0, step = 0;            // ... of so many, in chunks of `step`
    int rc = SECEDO_OK;
    std::string err;
    double t_ms[4] = {0, 0, 0, 0};           // SECEDO_ONE_SHOT_TRACE: when each phase was over
};

// what the lanes of one call share
struct LaneCall {
    const std::vector<int> &devices;
    const secedo::FlatPileupView &pileup;
    const OneShotParams &p;
    double *out;
    std::vector<Lane> lanes;
    HostBarrier barrier;
    std::atomic<bool> failed{false};
    Clock::time_point t0 = Clock::now();
    uint32_t n() const { return static_cast<uint32_t>(lanes.size()); }
    void fail_lane(Lane &me, int rc) {  // (the message is this thread's: keep it for the caller's thread)
        me.rc = rc;
        me.err = g_error;
        failed.store(true);
    }
};

// The first failure of a lane wins, and the lane runs on to both barriers so that no other lane waits forever.
// LANE_HIP always evaluates its expression, LANE_RC only while the lane is well. They expect `call` and `me`.
#define LANE_HIP(expr)                                                                               \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess && me.rc == SECEDO_OK)                                                 \
            call.fail_lane(me, fail(SECEDO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__))); \
    } while (0)
#define LANE_RC(expr)                                  \
    do {                                               \
        if (me.rc == SECEDO_OK) {                      \
            const int rc__ = (expr);                   \
            if (rc__ != SECEDO_OK) call.fail_lane(me, rc__); \
        }                                              \
    } while (0)

// ---- 1 + 2: pack, accumulate the lane's tiles chunk by chunk
void lane_accumulate(LaneCall &call, Lane &me) {
    const uint32_t n = call.n(), k = me.k;
    const OneShotParams &p = call.p;
    LANE_HIP(hipSetDevice(me.device));
    for (uint32_t j = 0; j < n && me.rc == SECEDO_OK; ++j) {
        if (call.devices[j] == me.device) continue;
        const hipError_t e = hipDeviceEnablePeerAccess(call.devices[j], 0);  // direct xGMI copies where the link exists
        if (e != hipSuccess) (void)hipGetLastError();                        // (already enabled / not possible: staged copies)
    }
    LANE_RC(one_shot_acquire(kLaneKey + static_cast<int>(k), me.device, &me.h));
    LANE_HIP(hipStreamCreateWithFlags(&me.s, hipStreamNonBlocking));
    LANE_HIP(hipStreamCreateWithFlags(&me.sc, hipStreamNonBlocking));
    me.done.assign(kChunks, nullptr);
    for (uint32_t c = 0; c < kChunks; ++c) LANE_HIP(hipEventCreateWithFlags(&me.done[c], hipEventDisableTiming));
    LANE_RC(set_pileup_view(me.h, call.pileup));
    LANE_RC(secedo_simmat_prepare(me.h, p.num_cells, p.max_fragment_length, p.num_threads, 0, me.s));
    me.t_ms[0] = ms_since(call.t0);
    if (me.rc == SECEDO_OK) {
        me.tiles = me.h->num_tiles;
        const uint32_t per = (me.tiles + n - 1) / n;
        me.lo = std::min(k * per, me.tiles);
        me.hi = std::min((k + 1) * per, me.tiles);
        me.step = std::max(1u, (per + kChunks - 1) / kChunks);
        LANE_HIP(me.h->own_acc.ensure(std::max<uint64_t>(secedo_simmat_acc_elems(me.h), 1) * sizeof(int64_t)));
    }
    for (uint32_t c = 0; c < kChunks; ++c) {
        const uint32_t a = std::min(me.lo + c * me.step, me.hi), b = std::min(me.lo + (c + 1) * me.step, me.hi);
        // (an empty chunk still goes through accumulate once: it sets up the table and the scale finalize needs)
        if (b > a || c == 0)
            LANE_RC(secedo_simmat_assign(me.h, p.mutation_rate, p.homozygous_rate, p.seq_error_rate, a, b,
                                         me.h->own_acc.as<int64_t>(), me.s));
        if (me.rc == SECEDO_OK) LANE_HIP(hipEventRecord(me.done[c], me.s));
    }
}

// ---- 3: the other lanes' tiles, chunk by chunk as their events fire
void lane_exchange(LaneCall &call, Lane &me) {
    const uint32_t n = call.n();
    if (!call.failed.load()) {
        const size_t b2 = static_cast<size_t>(me.h->pk.block_cells) * me.h->pk.block_cells;
        for (uint32_t d = 1; d < n; ++d) {  // (lane k starts with lane k + 1: the pulls spread over the links)
            const Lane &src = call.lanes[(me.k + d) % n];
            if (src.h->num_tiles != me.tiles || src.h->pk.block_cells != me.h->pk.block_cells) {
                call.fail_lane(me, fail(SECEDO_E_STATE, "the lanes packed the same pileup into different geometries"));
                break;
            }
            for (uint32_t c = 0; c < kChunks; ++c) {
                const uint32_t a = std::min(src.lo + c * me.step, src.hi), b = std::min(src.lo + (c + 1) * me.step, src.hi);
                if (b <= a) continue;
                LANE_HIP(hipStreamWaitEvent(me.sc, src.done[c], 0));
                LANE_HIP(hipMemcpyPeerAsync(me.h->own_acc.as<int64_t>() + a * b2, me.device,
                                            src.h->own_acc.as<int64_t>() + a * b2, src.device, (b - a) * b2 * sizeof(int64_t),
                                            me.sc));
            }
        }
        LANE_HIP(hipStreamWaitEvent(me.sc, me.done[kChunks - 1], 0));  // its own tiles
    }
    me.t_ms[1] = ms_since(call.t0);
}

// ---- 4: this lane's rows, normalised here, downloaded from here
void lane_download(LaneCall &call, Lane &me) {
    const uint32_t n = call.n(), k = me.k, num_cells = call.p.num_cells;
    if (!call.failed.load() && me.rc == SECEDO_OK) {
        const uint32_t row_lo = static_cast<uint32_t>(static_cast<uint64_t>(num_cells) * k / n);
        const uint32_t row_hi = static_cast<uint32_t>(static_cast<uint64_t>(num_cells) * (k + 1) / n);
        const size_t row_bytes = static_cast<size_t>(row_hi - row_lo) * num_cells * sizeof(double);
        if (me.h->scale_log2 != call.lanes[0].h->scale_log2)
            call.fail_lane(me, fail(SECEDO_E_STATE, "the lanes quantised the same pileup at different scales"));
        LANE_HIP(me.h->own_out.ensure(std::max<size_t>(row_bytes, 16)));
        LANE_RC(secedo_simmat_finalize_rows(me.h, call.p.normalization, me.h->own_acc.as<int64_t>(), row_lo, row_hi,
                                            me.h->own_out.as<double>(), me.sc));
        LANE_HIP(hipStreamSynchronize(me.sc));
        me.t_ms[2] = ms_since(call.t0);
        if (me.rc == SECEDO_OK && row_bytes) {
            double *dst = call.out + static_cast<size_t>(row_lo) * num_cells;
            if (row_bytes >= (8u << 20))
                // (copier threads: the lanes share what one lane alone would use -- at least 16 in all: touching the
                // fresh pages of the caller's matrix is what bounds a download, 2 GB/s for one thread)
                LANE_HIP(download_pipelined(me.h->own_out.p, dst, row_bytes,
                                            std::max(1u, std::max(call.p.num_threads, 16u) / n), 1 + static_cast<int>(k)));
            else
                LANE_HIP(hipMemcpy(dst, me.h->own_out.p, row_bytes, hipMemcpyDeviceToHost));
        }
    } else if (me.sc) {
        (void)hipStreamSynchronize(me.sc);
    }
    me.t_ms[3] = ms_since(call.t0);
}

void lane_tear_down(LaneCall &call, Lane &me) {
    if (me.s) (void)hipStreamSynchronize(me.s);
    if (me.h) me.h->uploads.settle();  // (their events were recorded on streams that end here)
    for (hipEvent_t ev : me.done)
        if (ev) (void)hipEventDestroy(ev);
    if (me.s) (void)hipStreamDestroy(me.s);
    if (me.sc) (void)hipStreamDestroy(me.sc);
    one_shot_release(kLaneKey + static_cast<int>(me.k), me.h, me.rc == SECEDO_OK && !call.failed.load());
    me.h = nullptr;
}
#undef LANE_HIP
#undef LANE_RC

void lane_main(LaneCall &call, uint32_t k) {
    Lane &me = call.lanes[k];
    me.k = k;
    me.device = call.devices[k];
    lane_accumulate(call, me);
    call.barrier.wait();  // every lane's events are recorded (a wait on an event not yet recorded would not wait)
    lane_exchange(call, me);
    lane_download(call, me);
    call.barrier.wait();  // nobody reads this lane's accumulator any more
    lane_tear_down(call, me);
}

int compute_on_devices(const std::vector<int> &devices, const secedo::FlatPileupView &pileup, const OneShotParams &p,
                       double *out) {
    std::lock_guard<std::mutex> serial(g_multi_mutex);
    const uint32_t n = static_cast<uint32_t>(devices.size());
    static const bool trace = env_set("SECEDO_ONE_SHOT_TRACE");
    LaneCall call{devices, pileup, p, out, std::vector<Lane>(n), HostBarrier(n)};
    std::vector<std::thread> threads;
    for (uint32_t k = 1; k < n; ++k) threads.emplace_back(lane_main, std::ref(call), k);
    lane_main(call, 0);
    for (std::thread &t : threads) t.join();
    if (trace)
        for (const Lane &lane : call.lanes)
            std::fprintf(stderr, "[one-shot, lane %u on device %d] packed at %.2f ms, exchange issued at %.2f, rows normalised at "
                                 "%.2f, downloaded at %.2f\n", lane.k, lane.device, lane.t_ms[0], lane.t_ms[1], lane.t_ms[2], lane.t_ms[3]);
    for (const Lane &lane : call.lanes)
        if (lane.rc != SECEDO_OK) return fail(lane.rc, lane.err);
    return SECEDO_OK;
}

// The caller of the reference's signature calls this once per sub-cluster of the recursion
// (spectral_clustering.cpp:354-356): the handle with its device arenas, streams and tables is kept
// between calls (two thirds of a first call on C2 is allocation). A failed call drops its handle.
int compute_on_device(int device, const secedo::FlatPileupView &pileup, const OneShotParams &p, double *out) {
    secedo_simmat_t *h = nullptr;
    SECEDO_CALL(one_shot_acquire(device, device, &h));
    struct Guard {
        secedo_simmat_t *h;
        int device;
        bool ok = false;
        ~Guard() { one_shot_release(device, h, ok); }
    } guard{h, device};
    static const bool trace = env_set("SECEDO_ONE_SHOT_TRACE");  // phase times on stderr
    Clock::time_point t = Clock::now();
    SECEDO_CALL(set_pileup_view(h, pileup));
    SECEDO_CALL(secedo_simmat_prepare(h, p.num_cells, p.max_fragment_length, p.num_threads, 0, nullptr));
    const double ms_pack = ms_lap(t);
    SECEDO_TRY(h->own_acc.ensure(secedo_simmat_acc_elems(h) * sizeof(int64_t)));
    const size_t out_bytes = static_cast<size_t>(p.num_cells) * p.num_cells * sizeof(double);
    SECEDO_TRY(h->own_out.ensure(out_bytes));
    SECEDO_CALL(secedo_simmat_assign_finalize(h, p.mutation_rate, p.homozygous_rate, p.seq_error_rate, p.normalization,
                                              h->own_acc.as<int64_t>(), h->own_out.as<double>(), nullptr));
    if (trace) SECEDO_TRY(hipDeviceSynchronize());
    const double ms_matrix = ms_lap(t);
    // (a plain hipMemcpy into the caller's pageable, usually untouched matrix runs at 12-20 GB/s: 25-45 ms for
    // the 512 MB of C3, the longest phase of a one-shot call)
    static const bool plain_copy = env_is("SECEDO_ONE_SHOT_COPY", "plain");
    if (out_bytes >= (8u << 20) && !plain_copy) {
        SECEDO_TRY(hipStreamSynchronize(nullptr));  // the matrix is complete (the download runs on a stream of its own)
        SECEDO_TRY(download_pipelined(h->own_out.p, out, out_bytes, std::max(1u, p.num_threads)));
    } else {
        SECEDO_TRY(hipMemcpy(out, h->own_out.p, out_bytes, hipMemcpyDeviceToHost));
    }
    if (trace)
        std::fprintf(stderr, "[one-shot] upload + packing %.2f ms, matrix %.2f ms, copy to the host %.2f ms\n", ms_pack,
                     ms_matrix, ms_since(t));
    guard.ok = true;
    return SECEDO_OK;
}

}  // namespace

extern "C" {

int secedo_simmat_set_devices(const int *device_ids, uint32_t n_devices) {
    if (n_devices && !device_ids) return fail(SECEDO_E_INVALID_ARG, "device_ids is null");
    if (n_devices > static_cast<uint32_t>(kMaxLanes)) return fail(SECEDO_E_LIMIT, "at most " + std::to_string(kMaxLanes) + " devices");
    std::vector<int> ids(device_ids, device_ids + n_devices);
    if (!ids.empty()) SECEDO_CALL(check_devices(ids));
    std::lock_guard<std::mutex> lock(g_devices_mutex);
    g_devices = std::move(ids);
    return SECEDO_OK;
}

int secedo_simmat_get_devices(int *device_ids, uint32_t capacity) {
    std::vector<int> ids;
    SECEDO_CALL(one_shot_devices(&ids));
    for (uint32_t i = 0; i < capacity && i < ids.size() && device_ids; ++i) device_ids[i] = ids[i];
    return static_cast<int>(ids.size());
}

int secedo_simmat_compute(const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                          const uint64_t *locus_entry_off, const uint32_t *read_ids,
                          const uint16_t *id_base16, const uint32_t *id_base32,
                          const uint32_t *group_id_to_pos, uint32_t n_groups, uint32_t num_cells,
                          uint32_t max_fragment_length, double mutation_rate, double homozygous_rate,
                          double seq_error_rate, uint32_t num_threads, int normalization, double *out) {
    SECEDO_CALL(check_normalization(normalization));
    if (!out) return fail(SECEDO_E_INVALID_ARG, "out is null");
    std::vector<int> devices;
    SECEDO_CALL(one_shot_devices(&devices));
    const secedo::FlatPileupView pileup{chr_locus_off, n_chr, locus_pos, locus_entry_off, read_ids,
                                        id_base16, id_base32, group_id_to_pos, n_groups};
    const OneShotParams p{num_cells, max_fragment_length, mutation_rate, homozygous_rate, seq_error_rate, num_threads,
                          normalization};
    if (devices.size() > 1) return compute_on_devices(devices, pileup, p, out);
    return compute_on_device(devices[0], pileup, p, out);
}

int secedo_simmat_staging_acquire(const uint64_t bytes[5], void *ptrs[5]) {
    if (!bytes || !ptrs) return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (secedo_simmat_device_count() <= 0) return fail(SECEDO_E_NO_DEVICE, "no HIP device is visible");
    std::lock_guard<std::mutex> lock(g_staging_mutex);
    if (g_staging_busy) return fail(SECEDO_E_STATE, "the staging buffers are held by another caller");
    for (int i = 0; i < 5; ++i) {
        const hipError_t e = g_staging[i].ensure(static_cast<size_t>(bytes[i]));
        if (e != hipSuccess) return fail(SECEDO_E_HIP, std::string("hipHostMalloc (staging): ") + hipGetErrorString(e));
        ptrs[i] = g_staging[i].p;
    }
    g_staging_busy = true;
    return SECEDO_OK;
}

void secedo_simmat_staging_release(void) {
    std::lock_guard<std::mutex> lock(g_staging_mutex);
    g_staging_busy = false;
}

void secedo_simmat_release_cache(void) {
    secedo::em_release_cache();
    {
        std::lock_guard<std::mutex> lock(g_staging_mutex);
        if (!g_staging_busy)
            for (PinnedBuf &b : g_staging) b.release();
    }
    for (Bounce &b : g_bounce) {
        std::lock_guard<std::mutex> lock(b.mutex);
        b.buf.release();
    }
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    for (auto &slot : g_pool) {
        if (slot.second) secedo_simmat_destroy(slot.second);
        slot.second = nullptr;
    }
}

}  // extern "C"
