// bgzf_kernels.hip -- BGZF members inflated on gfx950: compressed bytes in HBM -> text in HBM, ISIZE and CRC32 checked
// on the way, nothing of it seen by the host.
//
// One wavefront (a 64-thread workgroup) per member. The symbol decode is serial, so all 64 lanes run it with the same
// values (bgzf_inflate.hpp, shared with the host test); the lanes split what is parallel: the input staging, the table
// fill, the match and stored copies, the CRC and the write-out. Across members the grid is the parallelism.
//
// LDS per workgroup (39.5 KiB, four workgroups per CU, one per SIMD):
//   ring  32 KiB  the last 32 KiB of output, the whole DEFLATE window. Back-references read it, never HBM, so no
//                 store of the wave has to become visible to its own later loads. A finished 16 KiB segment is
//                 checksummed and written out with 16-byte vector stores (head and tail bytes singly) while the other
//                 half of the ring stays the window.
//   win    2 KiB  the payload staged in 16-byte vector loads, 64 lanes x 2, refilled when the bit reader leaves it
//   crc    1 KiB  the byte table; each lane takes 260 bytes of a segment, the pieces are joined by x^(8 len) mod P
//   T    3.6 KiB  code lengths, sorted symbols, counts, the 10-bit and 8-bit primary tables
// A workgroup is one wave, so __syncthreads() costs no barrier wait; it is there as the fence that orders one lane's
// LDS stores before another lane's loads.
#include "bgzf_kernels.hpp"

#include "bgzf_inflate.hpp"

#include <hip/hip_runtime.h>

namespace secedo {
namespace bam {
namespace {

using namespace secedo::bgzf;

constexpr uint32_t kLanes = 64;
constexpr uint32_t kRing = 32768, kRingMask = kRing - 1, kSeg = 16384, kWin = 2048;
static_assert(kCrcChunk * kLanes >= kSeg && kCrcChunk % 4 == 0, "a segment is one CRC chunk per lane");

struct Lds {
    uint8_t ring[kRing];
    uint8_t win[kWin];
    uint32_t crc_tab[256];
    Tables T;
};
static_assert(sizeof(Lds) <= 40960, "four workgroups per CU");

// the payload through a window in LDS; positions q = pos + mis count from the 16-byte aligned address below it
struct DevIn {
    const uint8_t *pa;  // aligned base
    uint8_t *win;
    uint32_t mis, clen, w0, lane;
    bool loaded = false;
    __device__ DevIn(const uint8_t *p, uint32_t n, uint8_t *w, uint32_t l)
        : pa(p - (reinterpret_cast<uintptr_t>(p) & 15)), win(w), mis(uint32_t(reinterpret_cast<uintptr_t>(p) & 15)),
          clen(n), w0(0), lane(l) {}
    __device__ uint32_t size() const { return clen; }
    // the window holds [q, q + 8)
    __device__ void ensure(uint32_t q) {
        if (loaded && q >= w0 && q + 8 <= w0 + kWin) return;
        w0 = q & ~15u;
        loaded = true;
        __syncthreads();
        for (uint32_t v = lane; v < kWin / 16; v += kLanes) {
            const uint32_t off = w0 + 16 * v;
            uint4 x = make_uint4(0, 0, 0, 0);
            if (off < mis + clen) x = *reinterpret_cast<const uint4 *>(pa + off);  // at most 15 bytes past the payload
            reinterpret_cast<uint4 *>(win)[v] = x;
        }
        __syncthreads();
    }
    __device__ uint32_t load32(uint32_t pos) {
        if (pos >= clen) return 0;
        const uint32_t q = pos + mis;
        ensure(q);
        const uint32_t o = q - w0;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(win) + (o >> 2);
        return uint32_t((uint64_t(w[1]) << 32 | w[0]) >> ((o & 3) * 8));
    }
    __device__ uint32_t span(uint32_t pos) {
        ensure(pos + mis);
        return w0 + kWin - (pos + mis);
    }
    __device__ uint8_t byte(uint32_t pos) const { return win[pos + mis - w0]; }
};

struct DevOut {
    uint8_t *ring;
    const uint32_t *crc_tab;
    uint8_t *dst;  // the member's first output byte
    uint32_t lane, flushed = 0, crc = 0;
    __device__ DevOut(uint8_t *r, const uint32_t *t, uint8_t *d, uint32_t l) : ring(r), crc_tab(t), dst(d), lane(l) {}

    __device__ void lane_range(uint32_t, uint32_t *first, uint32_t *step) const {
        *first = lane;
        *step = kLanes;
    }
    __device__ void sync() const { __syncthreads(); }

    // output bytes [b, e) of the ring, at most kSeg of them and b a multiple of kSeg: CRC32, then out to HBM
    __device__ void flush(uint32_t b, uint32_t e) {
        __syncthreads();
        const uint32_t n = e - b;
        const uint32_t c0 = min(n, lane * kCrcChunk), c1 = min(n, (lane + 1) * kCrcChunk);
        uint32_t c = ~0u;
        uint32_t i = c0;
        for (; i + 4 <= c1; i += 4) {
            uint32_t w = *reinterpret_cast<const uint32_t *>(ring + ((b + i) & kRingMask));
            for (int k = 0; k < 4; ++k, w >>= 8) c = crc_tab[(c ^ w) & 0xFF] ^ (c >> 8);
        }
        for (; i < c1; ++i) c = crc_tab[(c ^ ring[(b + i) & kRingMask]) & 0xFF] ^ (c >> 8);
        uint32_t part = c1 > c0 ? crc_mul(crc_x8n(n - c1), ~c) : 0;
        for (int d = 32; d; d >>= 1) part ^= __shfl_xor(part, d, kLanes);
        crc = crc_join(crc, part, n);

        uint8_t *d = dst + b;
        const uint32_t head = min(n, uint32_t(-reinterpret_cast<uintptr_t>(d)) & 15u);
        if (lane < head) d[lane] = ring[(b + lane) & kRingMask];
        const uint32_t nvec = (n - head) / 16;
        const uint32_t *r32 = reinterpret_cast<const uint32_t *>(ring);
        const uint32_t sh = ((b + head) & 3) * 8;
        for (uint32_t v = lane; v < nvec; v += kLanes) {
            const uint32_t r = ((b + head + 16 * v) & kRingMask) >> 2;
            uint32_t w[5];
            for (uint32_t k = 0; k < 5; ++k) w[k] = r32[(r + k) & (kRing / 4 - 1)];
            uint4 x;
            x.x = uint32_t((uint64_t(w[1]) << 32 | w[0]) >> sh);
            x.y = uint32_t((uint64_t(w[2]) << 32 | w[1]) >> sh);
            x.z = uint32_t((uint64_t(w[3]) << 32 | w[2]) >> sh);
            x.w = uint32_t((uint64_t(w[4]) << 32 | w[3]) >> sh);
            *reinterpret_cast<uint4 *>(d + head + 16 * v) = x;
        }
        const uint32_t t0 = head + 16 * nvec;
        if (t0 + lane < n) d[t0 + lane] = ring[(b + t0 + lane) & kRingMask];
        flushed = e;
        __syncthreads();
    }
    // the output has reached `end`
    __device__ void advance(uint32_t end) {
        if (end - flushed >= kSeg) flush(flushed, flushed + kSeg);
    }

    __device__ void put(uint32_t at, uint8_t b) {
        ring[at & kRingMask] = b;
        advance(at + 1);
    }
    // sources lie below `at`, so no lane reads what another writes here; with dist <= 32768 and len <= 258 a slot
    // written in one round of 64 is never the source of a later round
    __device__ void match(uint32_t at, uint32_t dist, uint32_t len) {
        __syncthreads();
        const uint32_t from = at - dist;
        for (uint32_t j = lane; j < len; j += kLanes)
            ring[(at + j) & kRingMask] = ring[(from + (dist >= len ? j : j % dist)) & kRingMask];
        advance(at + len);
    }
    __device__ uint32_t room(uint32_t at) const { return kSeg - (at - flushed); }
    __device__ void copy_in(DevIn &in, uint32_t pos, uint32_t at, uint32_t n) {
        __syncthreads();
        for (uint32_t j = lane; j < n; j += kLanes) ring[(at + j) & kRingMask] = in.byte(pos + j);
        advance(at + n);
    }
};

__global__ __launch_bounds__(kLanes) void k_bgzf_inflate(const uint8_t *__restrict__ in,
                                                         const BgzfDesc *__restrict__ desc, uint32_t n_members,
                                                         uint8_t *__restrict__ out, uint32_t *__restrict__ status) {
    __shared__ __align__(16) Lds L;
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    if (m >= n_members) return;
    for (uint32_t i = lane; i < 256; i += kLanes) L.crc_tab[i] = crc_table_entry(i);
    __syncthreads();
    const BgzfDesc d = desc[m];
    uint32_t st = kOutputFull;
    if (d.isize <= kBgzfMaxIsize) {
        DevIn src(in + d.in_off, d.clen, L.win, lane);
        DevOut dst(L.ring, L.crc_tab, out + d.out_off, lane);
        uint32_t produced = 0;
        st = inflate_member(src, dst, L.T, d.isize, &produced);
        if (st == kOk) {
            if (produced > dst.flushed) dst.flush(dst.flushed, produced);
            if (dst.crc != d.crc) st = kCrcMismatch;
        }
    }
    if (lane == 0) status[m] = st;
}

// the highest '\n' of each 16-byte vector, the maximum over the wave, one atomic per wave that found one
__global__ __launch_bounds__(256) void k_bgzf_last_newline(const uint8_t *__restrict__ text, uint64_t n,
                                                           unsigned long long *__restrict__ end) {
    const uint64_t v = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long best = 0;
    if (v * 16 < n) {
        const uint64_t base = v * 16;
        if (base + 16 <= n) {
            const uint4 x = *reinterpret_cast<const uint4 *>(text + base);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
            for (uint32_t k = 0; k < 16; ++k)
                if (((w[k >> 2] >> ((k & 3) * 8)) & 0xFF) == '\n') best = base + k + 1;
        } else {
            for (uint64_t k = base; k < n; ++k)
                if (text[k] == '\n') best = k + 1;
        }
    }
    for (int d = 32; d; d >>= 1) best = max(best, (unsigned long long)__shfl_xor((unsigned long long)best, d, 64));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(end, best);
}

}  // namespace

hipError_t bgzf_inflate(const uint8_t *d_in, const BgzfDesc *d_desc, uint32_t n_members, uint8_t *d_out,
                        uint32_t *d_status, hipStream_t s) {
    if (!n_members) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(n_members), dim3(kLanes), 0, s, d_in, d_desc, n_members, d_out, d_status);
    return hipGetLastError();
}

hipError_t bgzf_last_newline(const uint8_t *d_text, uint64_t n, unsigned long long *d_end, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_end, 0, 8, s);
    if (e != hipSuccess || !n) return e;
    const uint64_t vecs = (n + 15) / 16;
    hipLaunchKernelGGL(k_bgzf_last_newline, dim3(unsigned((vecs + 255) / 256)), dim3(256), 0, s, d_text, n, d_end);
    return hipGetLastError();
}

}  // namespace bam
}  // namespace secedo
