/*
 * secedo_pileup.h -- C-ABI of the GPU loader of the reference's binary pileup files (*.bin, the format
 * secedo_pileup_read of secedo_simmat.h parses on the host). Library libsecedo_pileup.so.
 *
 * Each locus of a .bin file is: u32 position, u16 coverage, u32 read_ids[coverage],
 * u16 (cell_id << 2 | base)[coverage]; records are variable-length and only 2-byte aligned.
 *
 * The host reads each file in bounded chunks into pinned staging memory and walks only the 6-byte record
 * headers (the chain of record lengths is serial); the bytes and the record offsets go to HBM. Everything that
 * touches a payload runs on the GPU (secedo_amd/csrc/pileup_device.hip): the coverage test, the position-list
 * rule, the locus and entry offsets, the gather of read ids and cell ids with the id_to_group remap and the
 * cell-id check, the largest cell id and the read-span pass. For every file the result equals
 * secedo_pileup_read on that file bit for bit: positions, offsets, read ids, id_base16, num_cells and
 * max_read_length, and the same error code and message for a truncated record or a cell id past id_to_group.
 * Error codes are those of secedo_simmat.h; secedo_pileup_load_last_error() holds the message.
 */
#ifndef SECEDO_PILEUP_H
#define SECEDO_PILEUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Sizes of the last result (see secedo_pileup_load_fetch). */
typedef struct secedo_pileup_load_info {
    uint64_t n_loci;
    uint64_t n_entries;
} secedo_pileup_load_info;

/* Wall times of one call in ms. read: file reads into staging; walk: record-header walk; upload and device:
 * GPU-timeline time of the host-to-device copies and of the kernels (events); total: the whole call. */
typedef struct secedo_pileup_load_times {
    double read_ms;
    double walk_ms;
    double upload_ms;
    double device_ms;
    double total_ms;
} secedo_pileup_load_times;

const char *secedo_pileup_load_last_error(void);

/* Loads bin_files[i] into chromosome slot slot_of_file[i] (< n_slots, all distinct, else SECEDO_E_INVALID_ARG);
 * slots without a file are empty. Files are processed in slot order; the first failing one ends the call.
 * id_to_group[n_ids] maps cell ids to groups (id_base16 = uint16(group << 2 | base)); only kept entries are
 * checked against n_ids. Records with coverage > max_coverage are skipped. positions[i] (sorted, n_positions[i]
 * values; positions or either pointer may be NULL for none) restricts file i as the host reader's position list
 * does: with M_r the running maximum of the positions of the coverage-passing records up to r and
 * i_r = lower_bound(positions, M_r), record r is kept iff i_r < n and positions[i_r] == pos_r; the first
 * coverage-passing record with i_r == n ends the file. compute_max_read_len: max_read_length[i] = largest
 * u32 difference position(last appearance) - position(first appearance) of one read id over the kept entries
 * in file order (0 without entries), else 1000. num_cells[i] = largest kept raw cell id + 1 (1 without
 * entries). staging_bytes: bytes read per chunk (0 = 64 MiB); a record may straddle chunks. times may be NULL.
 * The result stays on the device until the next call on this thread; get it with secedo_pileup_load_fetch.
 * Synchronous. */
int secedo_pileup_load_device(const char *const *bin_files, uint32_t n_files, const uint32_t *slot_of_file,
                              uint32_t n_slots, const uint16_t *id_to_group, uint32_t n_ids, uint32_t max_coverage,
                              const uint32_t *const *positions, const uint64_t *n_positions,
                              int compute_max_read_len, uint64_t staging_bytes, secedo_pileup_load_info *info,
                              uint32_t *num_cells, uint32_t *max_read_length, secedo_pileup_load_times *times);

/* Copies the last result into host or device buffers (any may be NULL): chr_locus_off[n_slots + 1],
 * locus_pos[n_loci], locus_entry_off[n_loci + 1], read_ids[n_entries], id_base16[n_entries]: the flat layout
 * secedo_simmat_set_pileup_device takes. Synchronous. */
int secedo_pileup_load_fetch(uint32_t *chr_locus_off, uint32_t *locus_pos, uint64_t *locus_entry_off,
                             uint32_t *read_ids, uint16_t *id_base16);

/* Frees the device memory of the last result. */
void secedo_pileup_load_release(void);

#ifdef __cplusplus
}
#endif

#endif /* SECEDO_PILEUP_H */
