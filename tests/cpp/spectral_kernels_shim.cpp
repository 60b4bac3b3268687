// spectral_kernels_shim.cpp -- TEST INFRASTRUCTURE ONLY: a C ABI over the launch wrappers of
// secedo_amd/csrc/spectral_kernels.hpp, so that tests/test_gpu_spectral_kernels.py can call every kernel of the
// spectral step on its own through ctypes. Linked with build/spectral_kernels.o into
// secedo_amd/csrc/build/libspectral_kernels_test.so; not part of the product library. No logic lives here:
// device pointers and a stream in, the hipError_t out as an int.
#include "spectral_kernels.hpp"

namespace sp = secedo::spectral;

static hipStream_t st(void *stream) { return static_cast<hipStream_t>(stream); }

extern "C" {

uint32_t spectral_shim_product_segments(uint32_t n, uint32_t n_rows) { return sp::product_segments(n, n_rows); }
uint32_t spectral_shim_gram_chunks(uint32_t n) { return sp::gram_chunks(n); }
uint32_t spectral_shim_pad16(uint32_t n) { return sp::pad16(n); }

int spectral_shim_row_sums(const double *A_rows, uint32_t n, uint32_t row_begin, uint32_t n_rows, double *sums,
                           void *stream) {
    return (int)sp::row_sums(A_rows, n, row_begin, n_rows, sums, st(stream));
}

int spectral_shim_scale_from_sums(uint32_t n, const double *sums, double *s, double *root, void *stream) {
    return (int)sp::scale_from_sums(n, sums, s, root, st(stream));
}

int spectral_shim_laplacian(const double *A, const double *s, uint32_t n, double *out, void *stream) {
    return (int)sp::laplacian(A, s, n, out, st(stream));
}

int spectral_shim_init_block(uint32_t n, const double *root, double *X, void *stream) {
    return (int)sp::init_block(n, root, X, st(stream));
}

int spectral_shim_product_partial(const double *A_rows, uint32_t n, uint32_t row_begin, uint32_t n_rows,
                                  const double *s, const double *X, double *Z, double *P, double *Ypart,
                                  double *Y_finished, void *stream) {
    return (int)sp::product_partial(A_rows, n, row_begin, n_rows, s, X, Z, P, Ypart, Y_finished, st(stream));
}

int spectral_shim_product_finish(uint32_t n, const double *s, const double *X, const double *Ysum, double *Y,
                                 void *stream) {
    return (int)sp::product_finish(n, s, X, Ysum, Y, st(stream));
}

int spectral_shim_gram(uint32_t n, const double *Q, uint64_t blk_stride, uint32_t nblk, const double *W, double *Gp,
                       double *G, void *stream) {
    return (int)sp::gram(n, Q, (size_t)blk_stride, nblk, W, Gp, G, st(stream));
}

int spectral_shim_block_combine(uint32_t n, const double *Q, uint64_t blk_stride, uint32_t nblk, const double *M,
                                double alpha, double beta, double *out, void *stream) {
    return (int)sp::block_combine(n, Q, (size_t)blk_stride, nblk, M, alpha, beta, out, st(stream));
}

int spectral_shim_cholesky_drop(const double *G, const double *R_prev, double *Rinv, double *R, uint32_t *alive,
                                void *stream) {
    return (int)sp::cholesky_drop(G, R_prev, Rinv, R, alive, st(stream));
}

int spectral_shim_write_vectors(uint32_t n, const double *Y, uint32_t k, double *out, void *stream) {
    return (int)sp::write_vectors(n, Y, k, out, st(stream));
}

}  // extern "C"
