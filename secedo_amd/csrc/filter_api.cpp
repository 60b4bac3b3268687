// filter_api.cpp -- the locus filter's entry points of include/secedo_simmat.h (SURVEY.md section 8f rank 2;
// reference util/is_significant.cpp): the test of one locus on the host (filter_host.cpp) and the filter of a
// whole pileup on the device (filter_device.hip), from device or from host arrays.
#include "filter_device.hpp"
#include "filter_host.hpp"
#include "simmat_handle.hpp"

#include <map>

using namespace secedo::host;

extern "C" {

int secedo_is_significant(const uint16_t *base_count, double seq_error_rate, uint32_t cell_proportion) {
    if (!base_count) return fail(SECEDO_E_INVALID_ARG, "base_count is null");
    if (cell_proportion > 4) return fail(SECEDO_E_INVALID_ARG, "cell_proportion must be in [0, 4]");
    return secedo::is_significant(base_count, seq_error_rate, cell_proportion);
}

int secedo_filter_device(const uint32_t *d_chr_locus_off, uint32_t n_chr, const uint32_t *d_locus_pos,
                         const uint64_t *d_locus_entry_off, const uint32_t *d_read_ids,
                         const uint16_t *d_id_base16, const uint32_t *d_id_base32, const uint32_t *d_id_to_pos,
                         uint32_t n_groups, uint32_t n_loci, uint64_t n_entries, double seq_error_rate,
                         uint32_t cell_proportion, uint32_t *d_out_chr_locus_off, uint32_t *d_out_locus_pos,
                         uint64_t *d_out_locus_entry_off, uint32_t *d_out_read_ids, void *d_out_id_base,
                         uint64_t *out_n_loci, uint64_t *out_n_entries, double *avg_coverage, void *stream) {
    if (!d_chr_locus_off || !d_locus_entry_off || !d_out_chr_locus_off || !d_out_locus_entry_off || !out_n_loci
        || !out_n_entries || !avg_coverage)
        return fail(SECEDO_E_INVALID_ARG, "null argument");
    if (secedo_simmat_device_count() <= 0) return no_device("the locus filter");
    const secedo::DeviceFlatPileup in = make_device_view(d_chr_locus_off, n_chr, d_locus_pos, d_locus_entry_off,
                                                         d_read_ids, d_id_base16, d_id_base32, d_id_to_pos, n_groups,
                                                         n_loci, n_entries);
    secedo::FilterOut out{d_out_chr_locus_off, d_out_locus_pos, d_out_locus_entry_off, d_out_read_ids, d_out_id_base};
    // scratch kept between calls, one set per device (allocations belong to the device they were made on)
    int device = 0;
    SECEDO_TRY(hipGetDevice(&device));
    static thread_local std::map<int, secedo::FilterWorkspace> workspaces;
    secedo::FilterWorkspace &ws = workspaces[device];
    const std::string err = secedo::filter_device(in, seq_error_rate, cell_proportion,
                                                  static_cast<hipStream_t>(stream), &ws, out, out_n_loci,
                                                  out_n_entries, avg_coverage);
    if (!err.empty()) return fail(err.find("hip") == 0 ? SECEDO_E_HIP : SECEDO_E_INVALID_ARG, err);
    return SECEDO_OK;
}

int secedo_filter(const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                  const uint64_t *locus_entry_off, const uint32_t *read_ids, const uint16_t *id_base16,
                  const uint32_t *id_base32, const uint32_t *id_to_pos, uint32_t n_groups,
                  double seq_error_rate, uint32_t cell_proportion, uint32_t *out_chr_locus_off,
                  uint32_t *out_locus_pos, uint64_t *out_locus_entry_off, uint32_t *out_read_ids,
                  void *out_id_base, uint64_t *out_n_loci, uint64_t *out_n_entries, double *avg_coverage) {
    if (!chr_locus_off || !locus_entry_off) return fail(SECEDO_E_INVALID_ARG, "null offset arrays");
    if ((id_base16 != nullptr) == (id_base32 != nullptr))
        return fail(SECEDO_E_INVALID_ARG, "exactly one of id_base16 / id_base32 must be given");
    if (secedo_simmat_device_count() <= 0) return no_device("the locus filter");
    SECEDO_TRY(hipSetDevice(env_int("SECEDO_DEVICE", 0)));
    const secedo::FlatPileupView v{chr_locus_off, n_chr, locus_pos, locus_entry_off, read_ids,
                                   id_base16, id_base32, id_to_pos, n_groups};
    RawPileupBufs raw;
    secedo::DeviceFlatPileup in;
    SECEDO_TRY(upload_flat_pileup(v, raw, &in));
    const uint32_t L = in.n_loci;
    const uint64_t E = in.n_entries;
    const size_t idw = id_base16 ? 2 : 4;
    DevBuf o_chr, o_pos, o_off, o_rid, o_idb;
    SECEDO_TRY(o_chr.ensure(((size_t)n_chr + 1) * 4));
    SECEDO_TRY(o_pos.ensure((size_t)L * 4));
    SECEDO_TRY(o_off.ensure(((size_t)L + 1) * 8));
    SECEDO_TRY(o_rid.ensure(E * 4));
    SECEDO_TRY(o_idb.ensure(E * idw));
    SECEDO_CALL(secedo_filter_device(in.chr_locus_off, n_chr, in.locus_pos, in.locus_entry_off, in.read_ids,
                                     in.id_base16, in.id_base32, in.group_id_to_pos, n_groups, L, E, seq_error_rate,
                                     cell_proportion, o_chr.as<uint32_t>(), o_pos.as<uint32_t>(), o_off.as<uint64_t>(),
                                     o_rid.as<uint32_t>(), o_idb.p, out_n_loci, out_n_entries, avg_coverage, nullptr));
    SECEDO_TRY(hipMemcpy(out_chr_locus_off, o_chr.p, ((size_t)n_chr + 1) * 4, hipMemcpyDeviceToHost));
    if (*out_n_loci) SECEDO_TRY(hipMemcpy(out_locus_pos, o_pos.p, *out_n_loci * 4, hipMemcpyDeviceToHost));
    SECEDO_TRY(hipMemcpy(out_locus_entry_off, o_off.p, (*out_n_loci + 1) * 8, hipMemcpyDeviceToHost));
    if (*out_n_entries) {
        SECEDO_TRY(hipMemcpy(out_read_ids, o_rid.p, *out_n_entries * 4, hipMemcpyDeviceToHost));
        SECEDO_TRY(hipMemcpy(out_id_base, o_idb.p, *out_n_entries * idw, hipMemcpyDeviceToHost));
    }
    return SECEDO_OK;
}

}  // extern "C"
