// fasta_stage.hpp -- the upload side the drivers of the FASTA device route share (fasta_device.cpp, genome_bins.cpp):
// the text, or the members of a BGZF file, cut into ranges, and the double-buffered stager that uploads (and inflates)
// range r + 1 on a stream of its own while the caller's stream runs the passes of range r. Internal.
#pragma once

#include "fasta_source.hpp"

#include "bgzf_kernels.hpp"
#include "fasta_kernels.hpp"

#include <algorithm>
#include <vector>

namespace secedo {
namespace fasta_host {

namespace F = secedo::fasta;
using secedo::bam::BgzfDesc;

struct Range {
    uint64_t a, b;  // text: bytes [a, b) of it; BGZF: members [a, b)
    uint32_t len;   // its text bytes
};

inline std::vector<Range> cut_ranges(const Source &src, bool from_members) {
    const uint64_t batch = std::min<uint64_t>(batch_bytes(), F::kMaxRange);
    std::vector<Range> r;
    if (!from_members) {
        const uint64_t n = src.text_bytes();
        for (uint64_t a = 0; a < n; a += batch) r.push_back(Range{a, std::min(n, a + batch), uint32_t(std::min(n - a, batch))});
        return r;
    }
    for (size_t k = 0; k < src.members.size();) {
        Range x{k, k, 0};
        do x.len += src.members[x.b++].isize;
        while (x.b < src.members.size() && uint64_t(x.len) + src.members[x.b].isize <= batch);
        r.push_back(x);
        k = x.b;
    }
    return r;
}

// The upload side: range r into text buffer r & 1, on its own stream.
struct Stager {
    const Source &src;
    bool members;
    std::vector<Range> ranges;
    StreamGuard up;
    Buf text[2], in[2], desc[2], status[2];
    std::vector<BgzfDesc> h_desc[2];
    Events<10> ev;  // per slot k: [k] staged, [2 + k] consumed, [4 + 2k, 5 + 2k] its inflate's begin and end

    Stager(const Source &s, bool m) : src(s), members(m), ranges(cut_ranges(s, m)) {}

    int init() {
        SECEDO_TRY(hipStreamCreateWithFlags(&up.s, hipStreamNonBlocking));
        SECEDO_CALL(ev.create());
        uint32_t max_len = 0, max_members = 0;
        uint64_t max_in = 0;
        for (const Range &r : ranges) {
            max_len = std::max(max_len, r.len);
            if (members) {
                max_members = std::max<uint32_t>(max_members, uint32_t(r.b - r.a));
                max_in = std::max(max_in, bm::payload_span(src.members, r.a, r.b, src.file_bytes).needed);
            }
        }
        for (int k = 0; k < 2; ++k) {
            SECEDO_TRY(text[k].alloc(size_t(max_len) + 16));
            if (!members) continue;
            SECEDO_TRY(in[k].alloc(max_in));
            SECEDO_TRY(desc[k].alloc(size_t(max_members) * sizeof(BgzfDesc)));
            SECEDO_TRY(status[k].alloc(size_t(max_members) * 4));
        }
        return SECEDO_OK;
    }
    uint32_t max_len() const {
        uint32_t m = 0;
        for (const Range &r : ranges) m = std::max(m, r.len);
        return m;
    }

    // Issues the upload (and inflate) of range r; `consumed`: the passes of range r - 2 read this slot, wait for them.
    int stage(size_t r, bool consumed) {
        const int k = int(r & 1);
        const Range &x = ranges[r];
        secedo_variant_fasta_info &st = info();
        if (consumed) SECEDO_TRY(hipStreamWaitEvent(up.s, ev.e[2 + k], 0));
        Clock::time_point t0 = Clock::now();
        if (!members) {
            SECEDO_TRY(hipMemcpyAsync(text[k].p, src.text() + x.a, x.len, hipMemcpyHostToDevice, up.s));
            st.uploaded_bytes += x.len;
        } else {
            const bm::PayloadSpan sp = bm::payload_span(src.members, x.a, x.b, src.file_bytes);
            const uint64_t span = sp.hi - sp.lo;
            h_desc[k].resize(x.b - x.a);
            bm::fill_desc(src.members, x.a, x.b, sp.lo, 0, 0, h_desc[k].data());
            SECEDO_TRY(hipMemcpyAsync(in[k].p, src.file + sp.lo, span, hipMemcpyHostToDevice, up.s));
            SECEDO_TRY(hipMemcpyAsync(desc[k].p, h_desc[k].data(), h_desc[k].size() * sizeof(BgzfDesc),
                                      hipMemcpyHostToDevice, up.s));
            st.uploaded_bytes += span;
            SECEDO_TRY(hipEventRecord(ev.e[4 + 2 * k], up.s));
            SECEDO_TRY(secedo::bam::bgzf_inflate(in[k].p, desc[k].as<BgzfDesc>(), uint32_t(x.b - x.a), text[k].p,
                                                 status[k].as<uint32_t>(), up.s));
            SECEDO_TRY(hipEventRecord(ev.e[5 + 2 * k], up.s));
            st.device_members += x.b - x.a;
        }
        st.upload_ms += ms_since(t0);
        SECEDO_TRY(hipEventRecord(ev.e[k], up.s));
        return SECEDO_OK;
    }
};

// the lowest bad member of a range whose status words were read back
inline void note_bad(const std::vector<uint32_t> &status, const Range &x, uint64_t *bad_k, uint32_t *bad_status) {
    const size_t m = bm::first_bad(status.data(), x.b - x.a);
    if (*bad_k != UINT64_MAX || m == x.b - x.a) return;
    *bad_k = x.a + m;
    *bad_status = status[m];
}

}  // namespace fasta_host
}  // namespace secedo
