// text_sink.hpp -- what the kernels that format text share (variant_kernels.hip, allele_kernels.hip): a line goes
// through a sink twice, once to count its bytes and once to store them, so the room a line was given is the room it
// takes. Device code; include from a .hip file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace secedo {
namespace text {

struct CountSink {
    uint32_t n = 0;
    __device__ void put(char) { ++n; }
};
struct ByteSink {
    uint8_t *p;
    __device__ void put(char c) { *p++ = uint8_t(c); }
};

template <class S>
__device__ void put_str(S &s, const char *t) {
    for (; *t; ++t) s.put(*t);
}

// std::to_string of an unsigned: decimal, no padding
template <class S>
__device__ void put_uint(S &s, uint32_t v) {
    uint32_t pow = 1;
    while (v / pow >= 10) pow *= 10;  // v / pow < 10 is reached before pow * 10 could overflow
    for (; pow; pow /= 10) s.put(char('0' + (v / pow) % 10));
}

}  // namespace text
}  // namespace secedo
