// text_out.hpp -- the way out for text that kernels format, once for every table writer (bam_depth.cpp,
// genome_bins.cpp): the lines of a file are measured, scanned and stored in ranges (Formatter), each range goes down as
// it is or through the shared BGZF encoder (TextOut), and the bytes are appended to a file of an OutFiles
// (out_files.hpp). Header-only and internal, like host_util.hpp: each library that includes it compiles its own copy
// over its own scan.
#pragma once

#include "bam_depth.hpp"  // Names
#include "bgzf_encoder.hpp"
#include "bgzf_members.hpp"
#include "host_util.hpp"
#include "out_files.hpp"

#include <string>
#include <vector>

namespace secedo {
namespace host __attribute__((visibility("hidden"))) {

// Members deflated per launch at the most: 256 MiB of slots, whatever the text's size.
constexpr size_t kSlice = 4096;
// the text of one range, where the caller's variable does not say
constexpr uint64_t kDefaultBatchBytes = 256ull << 20;
constexpr uint64_t kMaxBatchBytes = 1ull << 30;  // keeps a range's lines and threads well inside 2^31
// bytes of text per range: the value of the caller's variable `env` (for tests: same bytes), clamped
inline uint64_t text_batch_bytes(const char *env) {
    return std::min(env_u64(env, kDefaultBatchBytes), kMaxBatchBytes);
}

// what OutFiles says ("" or why) as a return code
inline int out_error(const std::string &why) {
    return why.empty() ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, why);
}

// What the layer did; the caller adds it to its own info struct, also after a failure.
struct TextCounts {
    uint64_t text_bytes = 0, compressed_bytes = 0, members = 0, ranges = 0;
    double format_ms = 0, deflate_ms = 0, download_ms = 0, write_ms = 0;
};

// One GPU-formatted file, file k of `of`: text on the device goes down as it is, or through the encoder with the
// member cuts of this piece of text.
struct TextOut {
    OutFiles *of;
    size_t k;
    bool gz;  // through the encoder
    bgzf::Encoder *enc;
    hipStream_t s;
    TextCounts *c;
    std::vector<uint8_t> down;
    Dev<uint8_t> stage;

    // d_text: `total` bytes with bgzf::kDeflateInSlack readable bytes around them
    int device(const uint8_t *d_text, uint64_t total) {
        if (total == 0) return SECEDO_OK;
        Clock::time_point t0 = Clock::now();
        c->text_bytes += total;
        if (!gz) {
            down.resize(total);
            SECEDO_TRY(hipMemcpyAsync(down.data(), d_text, total, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            c->download_ms += ms_lap(t0);
            SECEDO_CALL(out_error(of->append(k, down.data(), total)));
            c->write_ms += ms_lap(t0);
            return SECEDO_OK;
        }
        std::vector<bgzf::DeflateDesc> desc;
        bgzf::member_cuts(0, total, &desc);
        const int rc = enc->run(d_text, desc, s, [&](size_t, uint32_t n, const uint32_t *bytes, uint64_t *at) -> int {
            uint64_t end = 0;
            for (uint32_t i = 0; i < n; ++i) {
                at[i] = end;
                end += bytes[i];
            }
            SECEDO_CALL(enc->fetch(end, &enc->bytes, 0));
            Clock::time_point t1 = Clock::now();
            SECEDO_CALL(out_error(of->append(k, enc->bytes.data(), end)));
            c->compressed_bytes += end;
            c->write_ms += ms_since(t1);
            return SECEDO_OK;
        });
        c->members += enc->counts.members;
        c->deflate_ms += enc->counts.deflate_ms;
        c->download_ms += enc->counts.download_ms;
        enc->counts = bgzf::EncoderCounts{};  // taken
        return rc;
    }
    // text made on the host (a header line): the same way out
    int host(const std::string &text) {
        if (!gz) {
            c->text_bytes += text.size();
            return out_error(of->append(k, text.data(), text.size()));
        }
        std::vector<uint8_t> all(bgzf::kDeflateInSlack, 0);
        all.insert(all.end(), text.begin(), text.end());
        all.resize(all.size() + bgzf::kDeflateInSlack, 0);
        SECEDO_TRY(stage.alloc(all.size()));
        SECEDO_TRY(hipMemcpyAsync(stage.p, all.data(), all.size(), hipMemcpyHostToDevice, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        return device(stage.p + bgzf::kDeflateInSlack, text.size());
    }
    int finish() {
        if (!gz) return SECEDO_OK;
        const auto eof = bgzf::eof_member();
        c->compressed_bytes += eof.size();
        return out_error(of->append(k, eof.data(), eof.size()));
    }
};

// The 64-bit exclusive scan of the library this header is compiled into (bam:: or genomebins::, the same signatures).
struct Scan64 {
    size_t (*bytes)(uint64_t n);
    hipError_t (*sum)(void *tmp, size_t bytes, const uint64_t *d_in, uint64_t *d_out, uint64_t n, hipStream_t s);
};

// The lines of items [0, n_items) of one file, in ranges of `per_range` lines of at most `max_line` bytes: measure
// gives a range's line lengths (n + 1 entries, the last 0), their scan says where each line begins, write stores them
// between two kDeflateInSlack pads of zeros, and the text goes to `out`. The buffers are kept from file to file.
struct Formatter {
    Dev<uint64_t> len, off;
    Dev<uint8_t> tmp, text;
    template <class Measure, class Write>
    int run(uint64_t n_items, uint64_t per_range, uint64_t max_line, const Measure &measure, const Write &write,
            const Scan64 &scan, TextOut *out, hipStream_t s) {
        for (uint64_t i0 = 0; i0 < n_items; i0 += per_range) {
            Clock::time_point t0 = Clock::now();
            const uint32_t n = uint32_t(std::min<uint64_t>(per_range, n_items - i0));
            const size_t tb = scan.bytes(uint64_t(n) + 1);
            SECEDO_TRY(len.grow(size_t(n) + 1, 0, s));
            SECEDO_TRY(off.grow(size_t(n) + 1, 0, s));
            SECEDO_TRY(tmp.grow(tb, 0, s));
            SECEDO_TRY(measure(i0, n, len.p));
            SECEDO_TRY(scan.sum(tmp.p, tb, len.p, off.p, uint64_t(n) + 1, s));
            uint64_t total = 0;
            SECEDO_TRY(hipMemcpyAsync(&total, off.p + n, 8, hipMemcpyDeviceToHost, s));
            SECEDO_TRY(hipStreamSynchronize(s));
            if (total > uint64_t(n) * max_line)
                return fail(SECEDO_E_HIP, "the line lengths add up to more than the lines can hold");
            SECEDO_TRY(text.grow(total + 2 * bgzf::kDeflateInSlack, 0, s));
            uint8_t *d_text = text.p + bgzf::kDeflateInSlack;
            SECEDO_TRY(hipMemsetAsync(text.p, 0, bgzf::kDeflateInSlack, s));
            SECEDO_TRY(hipMemsetAsync(d_text + total, 0, bgzf::kDeflateInSlack, s));
            SECEDO_TRY(write(i0, n, off.p, d_text));
            SECEDO_TRY(hipStreamSynchronize(s));
            out->c->format_ms += ms_lap(t0);
            out->c->ranges += 1;
            SECEDO_CALL(out->device(d_text, total));
        }
        return SECEDO_OK;
    }
};

// names one after the other on the device, and the longest one's bytes
struct DevNames {
    Dev<uint8_t> bytes;
    Dev<uint32_t> off;
    uint64_t longest = 0;
    bamdepth::Names view() const { return bamdepth::Names{bytes.p, off.p}; }
};

inline int upload_names(const std::vector<std::string> &names, hipStream_t s, DevNames *dn) {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off{0};
    for (const std::string &n : names) {
        bytes.insert(bytes.end(), n.begin(), n.end());
        off.push_back(uint32_t(bytes.size()));
        dn->longest = std::max<uint64_t>(dn->longest, n.size());
    }
    SECEDO_TRY(dn->bytes.alloc(bytes.size()));
    SECEDO_TRY(dn->off.alloc(off.size()));
    if (!bytes.empty()) SECEDO_TRY(hipMemcpyAsync(dn->bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipMemcpyAsync(dn->off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    SECEDO_TRY(hipStreamSynchronize(s));
    return SECEDO_OK;
}

}  // namespace host
}  // namespace secedo
