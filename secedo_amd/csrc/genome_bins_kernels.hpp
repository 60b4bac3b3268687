// genome_bins_kernels.hpp -- launch wrappers of genome_bins_kernels.hip (gfx950): the composition of a range of FASTA
// text, resident in HBM and already scanned by the passes of fasta_kernels.hip, counted into a bins x 6 table, and the
// lines of the output file formatted from that table. See genome_bins.hpp for what decides the numbers and the bytes.
#pragma once

#include "fasta_kernels.hpp"
#include "genome_bins.hpp"

#include <hip/hip_runtime_api.h>

namespace secedo {
namespace genomebins {

// Pass 2 of a range: d_text[0, len) entered in `state`, w.tf_in and w.cnt_before as parse_range left them,
// d_pieces[n_pieces] ascending by code_off. Every sequence byte of a selected piece adds 1 to its class (and to
// kMasked) of its bin in d_table[table_bins][kColumns]; a bin at or past table_bins is left out. Integer atomics only.
hipError_t compose(const uint8_t *d_text, uint32_t len, uint32_t state, const fasta::RangeWork &w,
                   const Piece *d_pieces, uint32_t n_pieces, uint32_t S, uint32_t *d_table, uint64_t table_bins,
                   hipStream_t s);

// temporary storage of exclusive_sum64 over n elements; d_out[i] = the sum of d_in[0, i)
size_t scan_bytes(uint64_t n);
hipError_t exclusive_sum64(void *tmp, size_t bytes, const uint64_t *d_in, uint64_t *d_out, uint64_t n, hipStream_t s);

using Names = bd::Names;  // bam_depth.hpp: names one after the other

// The file's lines, item = global bin: d_base[n + 1] and d_len[n] are the layout's, names those of the selected
// contigs, counts the table in selection order.
struct Rows {
    const uint64_t *base;
    const uint32_t *len;
    uint32_t n, S;
    Names names;
    const uint32_t *counts;
};
// count then store (text_sink.hpp): measure gives d_len[k] for the bins [i0, i0 + n) (n + 1 entries, the last 0),
// write stores bin k's line at d_out + d_off[k] (d_off = the exclusive sum of d_len); the host loop over the ranges
// is text_out.hpp's Formatter, over the scan above
hipError_t lines_measure(const Rows &r, uint64_t i0, uint32_t n, uint64_t *d_len, hipStream_t s);
hipError_t lines_write(const Rows &r, uint64_t i0, uint32_t n, const uint64_t *d_off, uint8_t *d_out, hipStream_t s);

}  // namespace genomebins
}  // namespace secedo
