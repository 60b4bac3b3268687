// bgzf_kernels.hpp -- launch wrappers of bgzf_kernels.hip (gfx950): BGZF members inflated in HBM, CRC32 and ISIZE
// checked there, and the last '\n' of a text range. See bgzf_kernels.hip for the kernel's layout; BgzfDesc and the
// input slack are in bgzf_members.hpp, beside the host code that fills them.
#pragma once

#include "bgzf_members.hpp"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace secedo {
namespace bam {

// d_status[k] = secedo::bgzf::Status of member k (0 = inflated, ISIZE and CRC32 right). Members must not overlap in
// d_out; isize <= kBgzfMaxIsize.
hipError_t bgzf_inflate(const uint8_t *d_in, const BgzfDesc *d_desc, uint32_t n_members, uint8_t *d_out,
                        uint32_t *d_status, hipStream_t s);

// *d_end = 1 + the index of the last '\n' of d_text[0, n), 0 when there is none (d_end is set by the call)
hipError_t bgzf_last_newline(const uint8_t *d_text, uint64_t n, unsigned long long *d_end, hipStream_t s);

}  // namespace bam
}  // namespace secedo
