// bgzf_encoder.cpp -- see bgzf_encoder.hpp.
#include "bgzf_encoder.hpp"

namespace secedo {
namespace bgzf {

using namespace secedo::host;

int Encoder::run(const uint8_t *d_text, const std::vector<DeflateDesc> &desc, hipStream_t s, const Each &each) {
    if (timed_) SECEDO_CALL(ev_.create());
    if (const size_t members = std::min(slice_, desc.size()); members > cap_) {
        SECEDO_TRY(desc_.alloc(members * sizeof(DeflateDesc)));
        SECEDO_TRY(slots_.alloc(members * size_t(kDeflateSlot)));
        SECEDO_TRY(size_.alloc(members * 4));
        SECEDO_TRY(at_.alloc(members * 8));
        h_size_.resize(members);
        h_at_.resize(cap_ = members);
    }
    s_ = s;
    for (size_t b0 = 0; b0 < desc.size(); b0 += slice_) {
        n_ = uint32_t(std::min(slice_, desc.size() - b0));
        t0_ = Clock::now();
        SECEDO_TRY(hipMemcpyAsync(desc_.p, desc.data() + b0, n_ * sizeof(DeflateDesc), hipMemcpyHostToDevice, s));
        if (timed_) SECEDO_TRY(hipEventRecord(ev_.e[0], s));
        SECEDO_TRY(bgzf_deflate(d_text, desc_.as<DeflateDesc>(), n_, slots_.p, size_.as<uint32_t>(), s));
        if (timed_) SECEDO_TRY(hipEventRecord(ev_.e[1], s));
        SECEDO_TRY(hipMemcpyAsync(h_size_.data(), size_.p, n_ * 4, hipMemcpyDeviceToHost, s));
        SECEDO_TRY(hipStreamSynchronize(s));
        float k_ms = 0;
        if (timed_) SECEDO_TRY(hipEventElapsedTime(&k_ms, ev_.e[0], ev_.e[1]));
        counts.kernel_ms += k_ms;
        for (uint32_t k = 0; k < n_; ++k) {
            counts.stored_members += (h_size_[k] & kDeflateStoredFlag) != 0;
            h_size_[k] &= ~kDeflateStoredFlag;
            if (h_size_[k] < kHeaderBytes + kTrailerBytes || h_size_[k] > kMaxMember)
                return fail(SECEDO_E_STATE, "BGZF encoder: a member of " + std::to_string(h_size_[k]) + " bytes");
        }
        counts.members += n_;
        SECEDO_CALL(each(b0, n_, h_size_.data(), h_at_.data()));
        if (n_) return fail(SECEDO_E_STATE, "BGZF encoder: a slice was not fetched");
    }
    return SECEDO_OK;
}

int Encoder::fetch(uint64_t total, std::vector<uint8_t> *out, uint64_t at) {
    if (!n_) return fail(SECEDO_E_STATE, "BGZF encoder: fetch() without a slice");
    if (packed_.n < total) SECEDO_TRY(packed_.alloc(total));
    SECEDO_TRY(hipMemcpyAsync(at_.p, h_at_.data(), n_ * 8, hipMemcpyHostToDevice, s_));
    SECEDO_TRY(bgzf_pack(slots_.p, size_.as<uint32_t>(), at_.as<uint64_t>(), n_, packed_.p, s_));
    SECEDO_TRY(hipStreamSynchronize(s_));
    counts.deflate_ms += ms_lap(t0_);  // from the descriptors' upload, the writer's layout included
    if (out->size() < at + total) out->resize(at + total);
    SECEDO_TRY(hipMemcpyAsync(out->data() + at, packed_.p, total, hipMemcpyDeviceToHost, s_));
    SECEDO_TRY(hipStreamSynchronize(s_));
    counts.download_ms += ms_lap(t0_);  // the destination's growth and the copy
    n_ = 0;
    return SECEDO_OK;
}

}  // namespace bgzf
}  // namespace secedo
