/*
 * secedo_variant.h -- C-ABI of the variant calling that follows the clustering: the reference's
 * variant_calling() (variant_calling.cpp:323-461) with its helpers read_map, apply_map, read_contig,
 * get_next_chromosome and check_is_diploid (:81-224, :281-286). Library libsecedo_variant.so.
 *
 * The per-locus work (base counts per cluster, the genotype decisions, the per-cell counters behind the
 * `scores` file) runs on the GPU (secedo_amd/csrc/variant_kernels.hip). The FASTA / map reading, the gather of
 * the reference genotype per locus and the VCF text stay on the host. The pileup is the flat layout of
 * secedo_simmat.h, with id_base16 or id_base32. Error codes are those of secedo_simmat.h;
 * secedo_variant_last_error() holds the message. No CPU fallback for the compute entry points.
 *
 * Genotype codes: maternal << 3 | paternal, bases 0..3 = A, C, G, T and 5 = N (the reference's CharToInt);
 * SECEDO_NO_GENOTYPE = 255.
 */
#ifndef SECEDO_VARIANT_H
#define SECEDO_VARIANT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SECEDO_NO_GENOTYPE 255u

/* What a call record stands for: the line (or lines) the reference writes for it. */
#define SECEDO_VARIANT_POOLED 0  /* pooled-homozygous line to common.vcf (variant_calling.cpp:395-406) */
#define SECEDO_VARIANT_COMMON 1  /* all clusters agree: write_vcf_line to common.vcf (:427-432) */
#define SECEDO_VARIANT_CLUSTER 2 /* write_vcf_line to cluster_<cluster>.vcf (:433-442) */

/* One VCF event. Records come in the reference's write order: locus ascending, then the pooled record, then
 * the common one, then clusters ascending. counts: the pooled base counts (POOLED, COMMON) or the cluster's
 * (CLUSTER), as u16 like the reference's arrays. genotype: the pooled-homozygous genotype (POOLED), cluster
 * 0's genotype (COMMON) or the cluster's genotype (CLUSTER). */
typedef struct secedo_variant_record {
    uint32_t locus;    /* index into the flat pileup */
    uint16_t cluster;  /* CLUSTER records; 0 otherwise */
    uint8_t genotype;
    uint8_t kind;      /* SECEDO_VARIANT_* */
    uint16_t counts[4];
} secedo_variant_record;

/* Per-step wall times of a file-writing call, in ms. */
typedef struct secedo_variant_times {
    double fasta_ms;   /* FASTA + map parse, one contig (pair) per chromosome */
    double gather_ms;  /* reference genotype per locus, chromosome ends, threshold table */
    double device_ms;  /* uploads, both kernel launches, record and counter downloads */
    double write_ms;   /* VCF text, scores */
    double kernel_ms;  /* the two kernel launches alone (device events), included in device_ms */
} secedo_variant_times;

const char *secedo_variant_last_error(void);

/* Host only (no GPU needed). The reference genome of the pileup's loci: chromosome c of the pileup takes the
 * c-th contig (diploid FASTA: contig pair) of `fasta`, as the reference's loop over pos_data does (a FASTA
 * with fewer contigs leaves the last one in place, :161-163); `map_file` ("" or NULL for none) is applied
 * with apply_map. Out: locus_ref[n_loci] = the reference genotype at position - 1 (0 for loci at or after
 * their chromosome's end); chr_locus_end[n_chr] = the index of the first locus of chromosome c with
 * position - 1 >= contig length (uint32 arithmetic: position 0 wraps), or chr_locus_off[c + 1]. Loci from
 * there on are skipped entirely (the reference's `break` at :374-376). fasta_ms (may be NULL) receives the
 * parse time. Returns SECEDO_E_INVALID_ARG where the reference exits: a missing file, a map line without 8
 * columns or with a bad chromosome, maternal / paternal lengths that differ. */
int secedo_variant_reference_genotypes(const char *fasta, const char *map_file, const uint32_t *chr_locus_off,
                                       uint32_t n_chr, const uint32_t *locus_pos, uint32_t n_loci,
                                       uint8_t *locus_ref, uint32_t *chr_locus_end, double *fasta_ms);

/* Host only. check_is_diploid (:281-286): 1 when the first word of the file contains "maternal", 0 when not,
 * a negative SECEDO_E_* when the file cannot be opened. */
int secedo_variant_is_diploid(const char *fasta);

/* Host only. The contig (pair) get_next_chromosome returns at its `index`-th call (0-based): codes into
 * out[capacity]; *length = its length (SECEDO_E_LIMIT when more than capacity). */
int secedo_variant_read_chromosome(const char *fasta, const char *map_file, uint32_t index, uint8_t *out,
                                   uint64_t capacity, uint64_t *length);

/* Host only. read_map (:81-115) flattened: for each entry in file order, the contig name into
 * names[i * name_len] (NUL-terminated, truncated to name_len - 1), start_pos, len, tr ('I' or 'D'), and the
 * reference chromosome id. *n_entries = entries (SECEDO_E_LIMIT when more than capacity). */
int secedo_variant_read_map(const char *map_file, char *names, uint32_t name_len, uint32_t *start_pos,
                            uint32_t *len, char *tr, uint8_t *chromosome_id, uint32_t capacity,
                            uint32_t *n_entries);

/* Host only. apply_map (:117-141) on a single contig: map given as parallel arrays in application order. */
int secedo_variant_apply_map(const uint32_t *start_pos, const uint32_t *len, const char *tr, uint32_t n_map,
                             const uint8_t *chr_data, uint64_t n, uint8_t *out, uint64_t capacity,
                             uint64_t *out_len);

/* The hot path, on a flat pileup resident in HBM. d_clusters[n_clusters_entries] (u16, indexed by GROUP id,
 * variant_calling.cpp:381-386); every group id of the counted loci must be < n_clusters_entries
 * (SECEDO_E_INVALID_ARG otherwise, the reference reads out of bounds). d_locus_ref[n_loci] and host
 * chr_locus_end[n_chr] as secedo_variant_reference_genotypes returns them. Out: records[capacity] (host), in
 * write order, and *n_records = their count (SECEDO_E_LIMIT when more than capacity: the required count in
 * *n_records, nothing written to records); d_mismatch[n] / d_loci[n] (device, n = n_clusters_entries): per
 * group, the mismatches (:445-454) and counted entries behind `scores`. kernel_ms (may be NULL) receives the kernel time.
 * Synchronises `stream`. */
int secedo_variant_calls_device(int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                                const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                                const uint16_t *d_id_base16, const uint32_t *d_id_base32, uint32_t n_loci,
                                uint64_t n_entries, const uint16_t *d_clusters, uint32_t n_clusters_entries,
                                const uint8_t *d_locus_ref, const uint32_t *chr_locus_end, double hetero_prior,
                                double theta, secedo_variant_record *records, uint32_t capacity,
                                uint32_t *n_records, uint32_t *d_mismatch, uint32_t *d_loci, double *kernel_ms,
                                void *stream);

/* Test entry point: likely_homozygous(counts[i], theta) and most_likely_genotype(counts[i], -, -,
 * likely_homozygous_total, hetero_prior, theta) for n host count vectors, as the kernel evaluates them.
 * homozygous[n], genotype[n] host out. */
int secedo_variant_genotypes_device(int device_id, const uint16_t *counts, uint32_t n,
                                    int likely_homozygous_total, double hetero_prior, double theta,
                                    uint8_t *homozygous, uint8_t *genotype);

/* The drop-in: variant_calling(pos_data, clusters, reference_genome, map_file, hetero_prior, theta, out_dir)
 * on a host flat pileup. Writes cluster_<i>.vcf for i = 0..max(clusters), common.vcf, an empty `variant` and
 * `scores` under out_dir (created), as the reference does; n == 0 writes nothing. times may be NULL. */
int secedo_variant_calling(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr,
                           const uint32_t *locus_pos, const uint64_t *locus_entry_off, const uint16_t *id_base16,
                           const uint32_t *id_base32, const uint16_t *clusters, uint32_t n,
                           const char *reference_genome, const char *map_file, double hetero_prior, double theta,
                           const char *out_dir, secedo_variant_times *times);

/* Same on a flat pileup resident in HBM (the layout secedo_divide_cluster_device takes); clusters is host.
 * The chromosome offsets and positions are read back for the host gather. Synchronises `stream`. */
int secedo_variant_calling_device(int device_id, const uint32_t *d_chr_locus_off, uint32_t n_chr,
                                  const uint32_t *d_locus_pos, const uint64_t *d_locus_entry_off,
                                  const uint16_t *d_id_base16, const uint32_t *d_id_base32, uint32_t n_loci,
                                  uint64_t n_entries, const uint16_t *clusters, uint32_t n,
                                  const char *reference_genome, const char *map_file, double hetero_prior,
                                  double theta, const char *out_dir, secedo_variant_times *times, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SECEDO_VARIANT_H */
