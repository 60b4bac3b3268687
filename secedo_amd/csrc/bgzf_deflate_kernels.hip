// bgzf_deflate_kernels.hip -- BGZF members made on gfx950: text in HBM -> framed, checksummed DEFLATE members in HBM.
//
// One wavefront (a 64-thread workgroup) per member of at most 0xFF00 text bytes, as the decoder of bgzf_kernels.hip has
// one per member; across members the grid is the parallelism. The wave runs deflate_member of bgzf_deflate.hpp, the
// code the host test runs serially: a strip of 64 positions at a time, one position per lane, for the hash, the
// candidate, the match length, the token's bits, their prefix sum and the OR into place; lane 0 alone walks the greedy
// parse of a strip (the serial part: one dependent LDS read per token).
//
// Where the text lives. Every position reads its own 4 bytes, its candidate's, and then both runs dword by dword; a
// candidate is anywhere in the 32 KiB before, so the reads of one strip scatter over the whole window. Through L2 each
// of them is a gather of 64 addresses at global latency inside a dependent loop; in LDS it is two aligned dword reads
// and a funnel shift. So the member's text is staged once, with 16-byte vector loads, and read from LDS only:
//   text   63.8 KiB  the member, at the misalignment it has in HBM (byte accesses are by dword + shift: a byte read of
//                    LDS costs a dword read, and neighbouring lanes' dwords share a bank row without conflict)
//   Work   10.5 KiB  8 KiB hash table (4096 x u16), the CRC byte table, a strip's per-lane state, 24 staging dwords
// 74.3 KiB per workgroup: two workgroups (two waves) per CU of 160 KiB. That occupancy is the price of the text in LDS;
// a wider hash table would halve it again, which is why the table has 12 bits.
// The compressed bits of a strip are OR-ed into the staging dwords with LDS atomics (OR commutes, so the result does
// not depend on the lanes' order) and leave as whole aligned dwords; only a member's last bytes, its header and its
// trailer are byte stores.
#include "bgzf_deflate_kernels.hpp"

#include "bgzf_deflate.hpp"

#include <hip/hip_runtime.h>

namespace secedo {
namespace bgzf {
namespace {

constexpr uint32_t kLanes = kStrip;
constexpr uint32_t kTextBytes = kCut + 32;  // up to 15 bytes of misalignment in front, a funnel's second dword behind

struct Lds {
    uint8_t text[kTextBytes];
    Work W;
};
static_assert(sizeof(Lds) <= 81920, "two workgroups per CU");
static_assert(kDeflateMemberAt + kMaxMember + kOverrunBytes <= kDeflateSlot, "a slot holds a member and an overrun");
static_assert((kDeflateMemberAt + kHeaderBytes) % 4 == 0 && kDeflateSlot % 4 == 0, "payload dwords are aligned");

struct DevText {
    const uint8_t *lds;
    uint32_t mis;
    __device__ uint32_t load32(uint32_t p) const {
        const uint32_t q = p + mis;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(lds) + (q >> 2);
        return uint32_t((uint64_t(w[1]) << 32 | w[0]) >> ((q & 3) * 8));
    }
    __device__ uint32_t byte(uint32_t p) const { return lds[p + mis]; }
};

struct DevMember {
    uint8_t *member;
    __device__ void word(uint32_t k, uint32_t v) const {
        *reinterpret_cast<uint32_t *>(member + kHeaderBytes + 4 * k) = v;
    }
    __device__ void byte(uint32_t at, uint32_t v) const { member[at] = uint8_t(v); }
};

struct DevLanes {
    uint32_t lane;
    __device__ void lane_range(uint32_t, uint32_t *first, uint32_t *step) const {
        *first = lane;
        *step = kLanes;
    }
    __device__ void sync() const { __syncthreads(); }
    __device__ void fence() const {
        __threadfence();
        __syncthreads();
    }
    __device__ bool leader() const { return lane == 0; }
    __device__ void or32(uint32_t *p, uint32_t v) const { atomicOr(p, v); }
};

__global__ __launch_bounds__(kLanes) void k_bgzf_deflate(const uint8_t *__restrict__ text,
                                                         const DeflateDesc *__restrict__ desc, uint32_t n_members,
                                                         uint8_t *__restrict__ slots, uint32_t *__restrict__ size) {
    __shared__ __align__(16) Lds L;
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    if (m >= n_members) return;
    const DeflateDesc d = desc[m];
    if (d.n == 0 || d.n > kCut) {  // not a member this kernel makes; the host never asks
        if (lane == 0) size[m] = 0;
        return;
    }
    const uint8_t *p = text + d.in_off;
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(p) & 15);
    const uint4 *pa = reinterpret_cast<const uint4 *>(p - mis);
    const uint32_t vecs = (mis + d.n + 15) / 16;  // at most 15 bytes before the text and 15 behind it are read
    for (uint32_t v = lane; v < vecs; v += kLanes) reinterpret_cast<uint4 *>(L.text)[v] = pa[v];
    __syncthreads();
    DevText in{L.text, mis};
    DevMember out{slots + size_t(m) * kDeflateSlot + kDeflateMemberAt};
    DevLanes lanes{lane};
    uint32_t stored = 0;
    const uint32_t bytes = deflate_member(in, d.n, out, L.W, lanes, &stored);
    if (lane == 0) size[m] = bytes | (stored ? kDeflateStoredFlag : 0u);
}

__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ size,
                                                   const uint64_t *__restrict__ at, uint32_t n_members,
                                                   uint8_t *__restrict__ out) {
    const uint32_t m = blockIdx.x;
    if (m >= n_members) return;
    const uint32_t n = size[m] & ~kDeflateStoredFlag;
    const uint8_t *src = slots + size_t(m) * kDeflateSlot + kDeflateMemberAt;
    uint8_t *dst = out + at[m];
    for (uint32_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

}  // namespace

hipError_t bgzf_deflate(const uint8_t *d_text, const DeflateDesc *d_desc, uint32_t n_members, uint8_t *d_slots,
                        uint32_t *d_size, hipStream_t s) {
    if (!n_members) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(n_members), dim3(kLanes), 0, s, d_text, d_desc, n_members, d_slots, d_size);
    return hipGetLastError();
}

hipError_t bgzf_pack(const uint8_t *d_slots, const uint32_t *d_size, const uint64_t *d_at, uint32_t n_members,
                     uint8_t *d_out, hipStream_t s) {
    if (!n_members) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_pack, dim3(n_members), dim3(256), 0, s, d_slots, d_size, d_at, n_members, d_out);
    return hipGetLastError();
}

}  // namespace bgzf
}  // namespace secedo
