// sam_kernels_shim.cpp -- TEST INFRASTRUCTURE ONLY: a C ABI over the four launch wrappers of
// secedo_amd/csrc/sam_kernels.hpp, so that tests/test_gpu_sam_kernels.py can call every kernel of the SAM parse on
// its own through ctypes. Linked with build/sam_kernels.o into secedo_amd/csrc/build/libsam_kernels_test.so; not part
// of the product library. No logic lives here: device pointers and a stream in, the hipError_t out as an int.
#include "sam_kernels.hpp"

namespace sb = secedo::bam;

static hipStream_t st(void *stream) { return static_cast<hipStream_t>(stream); }

static sb::SamRefs refs(const uint8_t *bytes, const uint32_t *off, const uint64_t *hash, const uint32_t *id,
                        const uint8_t *sel, uint32_t n) {
    return sb::SamRefs{bytes, off, hash, id, sel, n};
}

extern "C" {

int sam_shim_newline_count(const uint8_t *text, uint64_t n16, uint32_t *cnt, void *stream) {
    return (int)sb::sam_newline_count(text, n16, cnt, st(stream));
}

int sam_shim_line_starts(const uint8_t *text, uint64_t n16, const uint32_t *scan, uint32_t n_lines, uint32_t len,
                         int no_trailing_newline, uint32_t *start, void *stream) {
    return (int)sb::sam_line_starts(text, n16, scan, n_lines, len, no_trailing_newline != 0, start, st(stream));
}

int sam_shim_size(const uint8_t *text, const uint32_t *start, uint32_t n_lines, uint64_t line_base, int ends_file,
                  const uint8_t *ref_bytes, const uint32_t *ref_off, const uint64_t *ref_hash, const uint32_t *ref_idx,
                  const uint8_t *ref_sel, uint32_t n_ref, uint64_t *size, int32_t *ref, int32_t *pos,
                  unsigned long long *err, void *stream) {
    return (int)sb::sam_size(text, start, n_lines, line_base, ends_file != 0,
                             refs(ref_bytes, ref_off, ref_hash, ref_idx, ref_sel, n_ref), size, ref, pos, err,
                             st(stream));
}

int sam_shim_encode(const uint8_t *text, const uint32_t *start, uint32_t n_lines, const uint8_t *ref_bytes,
                    const uint32_t *ref_off, const uint64_t *ref_hash, const uint32_t *ref_idx, const uint8_t *ref_sel,
                    uint32_t n_ref, const uint64_t *off, uint8_t *out, void *stream) {
    return (int)sb::sam_encode(text, start, n_lines, refs(ref_bytes, ref_off, ref_hash, ref_idx, ref_sel, n_ref), off,
                               out, st(stream));
}

}  // extern "C"
