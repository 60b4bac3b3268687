// bgzf_deflate_kernels.hpp -- launch wrappers of bgzf_deflate_kernels.hip (gfx950): text in HBM cut into BGZF members,
// each deflated, checksummed and framed there, then packed back to back. See bgzf_deflate_kernels.hip for the layout
// and bgzf_deflate.hpp for the rules that decide the bytes; DeflateDesc is in bgzf_members.hpp, beside its cut rule.
#pragma once

#include "bgzf_members.hpp"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace bgzf {

// bytes the kernel may read beyond a text's ends (whole 16-byte vectors): d_text needs that much room before the first
// text and after the last one, as the payloads of BgzfDesc do
constexpr uint32_t kDeflateInSlack = 16;
// member k is built in d_slots[k * kDeflateSlot, ...) from byte kDeflateMemberAt on (its payload then starts on a
// dword); the slot also takes what a compressed attempt wrote before it was given up for the stored form
constexpr uint32_t kDeflateSlot = 65536, kDeflateMemberAt = 2;
constexpr uint32_t kDeflateStoredFlag = 1u << 31;

// d_size[k] = the member's bytes, | kDeflateStoredFlag when it fell back to a stored block
hipError_t bgzf_deflate(const uint8_t *d_text, const DeflateDesc *d_desc, uint32_t n_members, uint8_t *d_slots,
                        uint32_t *d_size, hipStream_t s);

// member k's bytes from its slot to d_out + d_at[k]
hipError_t bgzf_pack(const uint8_t *d_slots, const uint32_t *d_size, const uint64_t *d_at, uint32_t n_members,
                     uint8_t *d_out, hipStream_t s);

}  // namespace bgzf
}  // namespace secedo
