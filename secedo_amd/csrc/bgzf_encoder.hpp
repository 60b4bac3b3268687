// bgzf_encoder.hpp -- the host loop around the BGZF encoder's kernels, once for every writer: run() takes
// the members of a text (bgzf_members.hpp: member_cuts) in slices, the writer places each slice's and fetch()es them.
#pragma once

#include "bgzf_deflate.hpp"
#include "bgzf_deflate_kernels.hpp"
#include "host_util.hpp"

#include <functional>

namespace secedo {
namespace bgzf {

// what an encoder did; kernel_ms only where asked for, by events; the stage clocks' boundaries are in bgzf_encoder.cpp
struct EncoderCounts {
    uint64_t members = 0, stored_members = 0;
    double kernel_ms = 0, deflate_ms = 0, download_ms = 0;
};

class __attribute__((visibility("hidden"))) Encoder {
public:
    // A slice: members desc[first, first + n) are deflated, bytes[k] is member first + k's size, checked. The writer
    // fills at[k], the member's offset among the slice's fetched bytes (gaps allowed), and calls fetch() once.
    using Each = std::function<int(size_t first, uint32_t n, const uint32_t *bytes, uint64_t *at)>;
    // At most `slice` members per launch; SECEDO_BGZF_SLICE_MEMBERS, read here, lowers it (for tests: same bytes).
    explicit Encoder(size_t slice, bool time_kernel = false)
        : slice_(std::min<uint64_t>(host::env_u64("SECEDO_BGZF_SLICE_MEMBERS", slice), slice)), timed_(time_kernel) {}
    // The members desc of d_text (kDeflateInSlack readable bytes around it); the buffers are kept for the next run.
    int run(const uint8_t *d_text, const std::vector<DeflateDesc> &desc, hipStream_t s, const Each &each);
    // The slice's members packed at their at[k] into (*out)[at, at + total), grown to that: one pack, one download.
    int fetch(uint64_t total, std::vector<uint8_t> *out, uint64_t at);

    EncoderCounts counts;
    std::vector<uint8_t> bytes;  // a destination for a writer without one of its own, kept like the buffers
private:
    const size_t slice_;
    const bool timed_;
    size_t cap_ = 0;  // members the buffers hold
    host::Buf desc_, slots_, size_, at_, packed_;
    std::vector<uint32_t> h_size_;
    std::vector<uint64_t> h_at_;
    host::Events<2> ev_;
    host::Clock::time_point t0_;
    hipStream_t s_ = nullptr;
    uint32_t n_ = 0;  // members of the slice that waits for its fetch()
};

}  // namespace bgzf
}  // namespace secedo
