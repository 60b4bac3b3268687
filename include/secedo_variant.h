/*
 * secedo_variant.h -- C-ABI of the variant calling that follows the clustering: the reference's
 * variant_calling() (variant_calling.cpp:323-461) with its helpers read_map, apply_map, read_contig,
 * get_next_chromosome and check_is_diploid (:81-224, :281-286). Library libsecedo_variant.so.
 *
 * The per-locus work (base counts per cluster, the genotype decisions, the per-cell counters behind the
 * `scores` file) runs on the GPU (secedo_amd/csrc/variant_kernels.hip). The map reading stays on the host, and so
 * does the VCF text by default (under SECEDO_VCF_BGZF it is formatted and compressed on the GPU, below); the FASTA
 * parse and the gather of the reference genotype per locus run on the host by default and on the GPU on the device
 * route (below). The pileup is the flat layout of
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

/* ---- The reference genome file ------------------------------------------------------------------------------
 *
 * Every entry point that takes a FASTA path accepts three kinds of file, told apart by content, never by name, as
 * secedo_bam.h tells its inputs apart:
 *   TEXT  anything that does not start with the gzip magic 1f 8b
 *   BGZF  gzip members with the BC extra subfield (bgzip, what samtools faidx reads)
 *   GZIP  gzip without it, one member or several; inflated on the host with zlib, then treated as text
 * Every member of a compressed file is inflated and its ISIZE and CRC32 are checked, whichever route reads it. A bad
 * BGZF member is SECEDO_E_INVALID_ARG "<path>: BGZF block <k>: inflate failed or ISIZE mismatch" or "... CRC32
 * mismatch" (the lowest k, ahead of any error of the parse); a truncated or corrupt gzip stream is
 * SECEDO_E_INVALID_ARG naming the path.
 *
 * Two routes compute locus_ref and chr_locus_end. HOST: the parser that restates the reference's stream calls, one
 * thread, then the gather on the host. DEVICE: the text (BGZF: the compressed members, inflated by the decoder of
 * bgzf_kernels.hip) is uploaded in ranges of about SECEDO_FASTA_BATCH_BYTES bytes of text (default 256 MiB, at least
 * 64 or one BGZF member; the results never depend on it), parsed and gathered in HBM (fasta_kernels.hip); neither the
 * text nor the inflated bytes of a BGZF file live on the host. The route is read by secedo_variant_calling,
 * secedo_variant_calling_device and secedo_variant_reference_genotypes_device:
 *   - TEXT and GZIP follow the setting: secedo_variant_set_fasta_route, else the environment SECEDO_FASTA=host|device
 *     (unset or empty: host; any other value is SECEDO_E_INVALID_ARG from every call that reads a FASTA, the
 *     host-only ones included);
 *   - BGZF takes the device route in those three calls whatever the setting;
 *   - a non-empty map_file is not supported on the device route (out of scope, not an error): TEXT and GZIP then take
 *     the host route, a BGZF file is inflated on the GPU, its text downloaded and the host route run on it.
 * The functions documented "host only" below stay host-only for all three kinds: there both compressed kinds are
 * inflated with zlib. The results of the two routes are equal byte for byte, the errors word for word. */
#define SECEDO_FASTA_HOST 0
#define SECEDO_FASTA_DEVICE 1

#define SECEDO_FASTA_KIND_TEXT 0
#define SECEDO_FASTA_KIND_BGZF 1
#define SECEDO_FASTA_KIND_GZIP 2

/* Process-wide. set: SECEDO_E_INVALID_ARG for another value; get: the route set, else the environment's, else HOST
 * (a negative SECEDO_E_* for an unknown value of SECEDO_FASTA). */
int secedo_variant_set_fasta_route(int route);
int secedo_variant_get_fasta_route(void);

/* What the last FASTA-reading call of this thread did. The times are the device route's split (ms); they overlap,
 * since the upload and inflate of one range run beside the passes of the range before. */
typedef struct secedo_variant_fasta_info {
    uint32_t kind;                /* SECEDO_FASTA_KIND_* */
    uint32_t route;               /* SECEDO_FASTA_* the call took */
    uint32_t fell_back_for_map;   /* 1: the device route was due but a map file sent the call to the host route */
    uint32_t reserved;
    uint64_t host_inflated_bytes; /* text bytes zlib produced on the host */
    uint64_t device_members;      /* BGZF members inflated on the GPU */
    uint64_t uploaded_bytes;      /* FASTA bytes sent to the GPU: text, or compressed members */
    uint64_t text_bytes;          /* FASTA text parsed: by the host parser as far as it read, by the device all of it */
    uint64_t ranges;              /* ranges of the device route */
    uint64_t contigs;             /* header lines seen (host route: contigs read) */
    uint64_t contigs_used;        /* contigs that became (half of) a chromosome of the pileup */
    double inflate_ms;            /* device: the inflate kernels (device events) */
    double upload_ms;             /* device: host time inside the uploads */
    double parse_gather_ms;       /* device: the parse passes, the gathers and the final pass (device events) */
} secedo_variant_fasta_info;
int secedo_variant_fasta_stats(secedo_variant_fasta_info *out);

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

/* The same results on the device route (see above), for a pileup resident in HBM: d_chr_locus_off[n_chr + 1] and
 * d_locus_pos[n_loci] in HBM, chr_locus_off the host copy of the offsets (they must run from 0 to n_loci and not
 * decrease); d_locus_ref[n_loci] is written in HBM, chr_locus_end[n_chr] on the host. A TEXT or GZIP file under the
 * HOST setting, or any file with a map, is read on the host route and its locus_ref uploaded (d_locus_pos is then
 * read back). times (may be NULL): fasta_ms = the whole call, gather_ms = 0; the split is in
 * secedo_variant_fasta_stats. Synchronises `stream`. */
int secedo_variant_reference_genotypes_device(int device_id, const char *fasta, const char *map_file,
                                              const uint32_t *d_chr_locus_off, const uint32_t *chr_locus_off,
                                              uint32_t n_chr, const uint32_t *d_locus_pos, uint32_t n_loci,
                                              uint8_t *d_locus_ref, uint32_t *chr_locus_end,
                                              secedo_variant_times *times, void *stream);

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

/* ---- The VCF output ----------------------------------------------------------------------------------------------
 *
 * Two kinds of output, chosen process-wide like the FASTA route: secedo_variant_set_vcf_output, else the environment
 * SECEDO_VCF=plain|bgzf (unset or empty: plain; any other value is SECEDO_E_INVALID_ARG from the file-writing calls).
 *   PLAIN  cluster_<i>.vcf and common.vcf, text built on the host from the downloaded records (the default)
 *   BGZF   cluster_<i>.vcf.gz and common.vcf.gz instead: the same text, formatted in HBM from the records where the
 *          calls left them and deflated there; neither the records nor the text come to the host, only the
 *          compressed bytes. Each file is a sequence of BGZF members of at most 0xFF00 text bytes (18-byte header with
 *          the BC subfield and BSIZE, one raw DEFLATE block with the fixed codes or, where that would not be smaller,
 *          a stored one, CRC32, ISIZE) and ends with the 28-byte EOF member, as bgzip writes them; it inflates to the
 *          bytes PLAIN writes. The preamble is made by the host (##fileDate is the time of the call) and compressed as
 *          the file's first bytes. `variant` and `scores` are the same on both; errors are PLAIN's word for word.
 * Both secedo_variant_calling and secedo_variant_calling_device honour the setting. */
#define SECEDO_VCF_PLAIN 0
#define SECEDO_VCF_BGZF 1

/* Process-wide. set: SECEDO_E_INVALID_ARG for another value; get: the kind set, else the environment's, else PLAIN
 * (a negative SECEDO_E_* for an unknown value of SECEDO_VCF). */
int secedo_variant_set_vcf_output(int output);
int secedo_variant_get_vcf_output(void);

/* What the last file-writing call of this thread (or secedo_variant_bgzf_deflate) did. Times in ms, host wall clock. */
typedef struct secedo_variant_vcf_info {
    uint32_t output;            /* SECEDO_VCF_* the call wrote */
    uint32_t reserved;
    uint64_t files;             /* VCF files: clusters + 1 */
    uint64_t text_bytes;        /* their text */
    uint64_t compressed_bytes;  /* BGZF: the bytes of the .vcf.gz files, EOF members included; PLAIN: 0 */
    uint64_t blocks;            /* BGZF members with text (the EOF members not counted) */
    uint64_t stored_blocks;     /* of those, the ones that fell back to a stored block */
    double format_ms;           /* BGZF: preambles, the formatter's kernels, the download of the file offsets */
    double deflate_ms;          /* BGZF: descriptors up, the encoder and pack kernels, member sizes down */
    double download_ms;         /* BGZF: the compressed bytes down */
    double write_ms;            /* the files (PLAIN: building the text as well) */
    double deflate_kernel_ms;   /* BGZF: the encoder kernel alone (device events), included in deflate_ms */
} secedo_variant_vcf_info;
int secedo_variant_vcf_stats(secedo_variant_vcf_info *out);

/* Test entry points: the VCF text of host records, by the host code of the PLAIN route and by the kernels of the
 * BGZF route. records[n_records] in write order (loci ascending, checked), chr_locus_off[n_chr + 1], locus_pos and
 * locus_ref[n_loci] as the calling functions have them; num_clusters cluster files and common. preamble /
 * preamble_off[num_clusters + 1] (both may be NULL: no preambles): cluster file i starts with bytes
 * [preamble_off[i], preamble_off[i + 1]) of preamble. Out: the files' texts back to back in text[capacity], cluster
 * files in order, then common; file_off[num_clusters + 2] their bounds (SECEDO_E_LIMIT when the text exceeds
 * capacity: file_off is set, text is not). */
int secedo_variant_format_host(const secedo_variant_record *records, uint32_t n_records,
                               const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                               const uint8_t *locus_ref, uint32_t n_loci, uint32_t num_clusters, const char *preamble,
                               const uint64_t *preamble_off, char *text, uint64_t capacity, uint64_t *file_off);
int secedo_variant_format_device(int device_id, const secedo_variant_record *records, uint32_t n_records,
                                 const uint32_t *chr_locus_off, uint32_t n_chr, const uint32_t *locus_pos,
                                 const uint8_t *locus_ref, uint32_t n_loci, uint32_t num_clusters,
                                 const char *preamble, const uint64_t *preamble_off, char *text, uint64_t capacity,
                                 uint64_t *file_off);

/* The BGZF encoder alone, on the GPU: n_files inputs, input f the bytes [data_off[f], data_off[f + 1]) of data (host),
 * all compressed in one launch. Out: the BGZF files back to back in out[capacity], out_off[n_files + 1] their bounds;
 * an empty input gives the EOF member alone. An input of n bytes needs at most n + 31 * ceil(n / 65280) + 28 bytes
 * (SECEDO_E_LIMIT when capacity is less: out_off is set, out is not). Sets secedo_variant_vcf_stats. Synchronises
 * `stream`. */
int secedo_variant_bgzf_deflate(int device_id, const uint8_t *data, const uint64_t *data_off, uint32_t n_files,
                                uint8_t *out, uint64_t capacity, uint64_t *out_off, void *stream);

/* ---- The tabix index (.tbi) of a bgzip-compressed VCF -------------------------------------------------------------
 *
 * A region query (tabix file.vcf.gz 7:1000-2000, bcftools view -r) needs <file>.tbi beside the file. Two routes build
 * it on the GPU with one line pass (tabix_kernels.hip) and one host builder (tabix_build.hpp):
 *   the writer      under SECEDO_VCF_INDEX_TBI the BGZF output also leaves cluster_<i>.vcf.gz.tbi and
 *                   common.vcf.gz.tbi: the line pass runs on the text where the formatter left it, the member table is
 *                   the encoder's, and the index bodies are compressed by one more call of the encoder;
 *   stand-alone     secedo_variant_tabix_build for files that exist: their compressed bytes are uploaded, inflated in
 *                   HBM (ISIZE and CRC32 checked) and indexed; many small files go into one batch.
 * Both give the same bytes for the same file. The setting is process-wide like the output: secedo_variant_set_vcf_index,
 * else the environment SECEDO_VCF_INDEX=none|tbi (unset or empty: none; any other value is SECEDO_E_INVALID_ARG from the
 * file-writing calls). TBI with SECEDO_VCF_PLAIN is SECEDO_E_INVALID_ARG: there is no index of plain text.
 *
 * The index: a data line is one whose first byte is not '#' and that is not empty. Its name is column 1, beg = POS - 1
 * (0 for POS 0), end = beg + the length of REF, or the value of INFO's first END= key where that is a decimal number
 * above beg; end > beg always. Bins and 16 kb windows as in a BAI (bins ascending, a chunk per run of consecutive data
 * lines in one bin, the pseudo-bin 37450 last, the linear index filled backward); names in the order of their first line;
 * small bins are not merged into their parents as newer htslib does, which readers accept alike. A chunk begins at its
 * first line and ends where the next run's first line begins, the last one at the end of the data (the EOF member).
 * A file without data lines has n_ref = 0. Refused with SECEDO_E_INVALID_ARG "<file>: line <n>: ...": a data line with
 * fewer than two columns, a POS that is not a decimal number, an end past 2^29, a POS lower than that of the data line
 * before it under the same name, a name that comes back after another one ("chromosome blocks not continuous"). */
#define SECEDO_VCF_INDEX_NONE 0
#define SECEDO_VCF_INDEX_TBI 1

/* Process-wide. set: SECEDO_E_INVALID_ARG for another value; get: the kind set, else the environment's, else NONE
 * (a negative SECEDO_E_* for an unknown value of SECEDO_VCF_INDEX). */
int secedo_variant_set_vcf_index(int index);
int secedo_variant_get_vcf_index(void);

/* Indexes n bgzip-compressed VCF files: paths[f] gets paths[f] + ".tbi". A file that is plain gzip or not compressed
 * is SECEDO_E_INVALID_ARG, as is an index that exists unless overwrite is non-zero. When a file fails, the files in
 * front of it in `paths` keep their indexes. Sets secedo_variant_tabix_stats. Synchronises `stream`. */
int secedo_variant_tabix_build(int device_id, const char *const *paths, uint32_t n, int overwrite, void *stream);

/* What the last index-writing call of this thread did (the writer under TBI, or secedo_variant_tabix_build); all zero
 * after a call that wrote no index. Times in ms, host wall clock. */
typedef struct secedo_variant_tabix_info {
    uint64_t files;             /* indexes written */
    uint64_t lines;             /* lines of their texts, '#' lines and empty ones included */
    uint64_t data_lines;
    uint64_t names;             /* chromosome names, summed over the files */
    uint64_t bins;              /* written, the pseudo-bins not counted */
    uint64_t chunks;
    uint64_t windows;           /* n_intv summed */
    uint64_t ranges;            /* ranges the line pass walked the texts in */
    uint64_t index_bytes;       /* the indexes before compression */
    uint64_t compressed_bytes;  /* the .tbi files */
    double pass_ms;             /* the line pass: kernels, scans, the downloads of heads, windows and names */
    double build_ms;            /* the host builder */
    double deflate_ms;          /* the index bodies through the encoder */
    double write_ms;            /* the .tbi files */
} secedo_variant_tabix_info;
int secedo_variant_tabix_stats(secedo_variant_tabix_info *out);

/* ---- Per-cell allele counts at the called variants (cell x site matrices) ------------------------------------------
 *
 * Opt-in, process-wide like the VCF output: secedo_variant_set_allele_counts, else the environment
 * SECEDO_ALLELE_COUNTS=none|all|cluster (unset or empty: none; any other value is SECEDO_E_INVALID_ARG from the
 * file-writing calls). With NONE nothing below runs and no file is added.
 *
 * A SITE is a locus with at least one call record (ALL), or with at least one SECEDO_VARIANT_CLUSTER record (CLUSTER);
 * sites are numbered in ascending locus order. Each has two 4-bit base masks (bit b = base b, A,C,G,T = 0..3):
 *   Rf = the bits of {ref & 7, ref >> 3} that are 0..3 (an N adds nothing)
 *   G  = the OR, over all records of the locus whatever their kind, of the bits of {genotype & 7, genotype >> 3}
 *   alt_mask = G & ~Rf, ref_mask = Rf; where that alt_mask is 0 (the calls only lose an allele of a heterozygous
 *   reference: diploid FASTA only) alt_mask = G and ref_mask = Rf & ~G. ref_mask may be 0, alt_mask never is.
 * For site s and group (cell) g, over the entries of the locus with that group id: ad = entries whose base is in
 * alt_mask, rd = those in ref_mask, oth = the rest, dp = ad + rd. A pair (s, g) exists when ad + rd + oth > 0; pairs
 * are ordered by s, then g. The entries of a locus need not be sorted by group, and a group may occur many times.
 *
 * The files, under <out_dir>/allele_counts/ (the layout cellsnp-lite writes and vireo / cardelino read; none of these
 * tools was run against them: the contract is the bytes stated here):
 *   cellSNP.tag.AD.mtx, cellSNP.tag.DP.mtx, cellSNP.tag.OTH.mtx   each exactly
 *       "%%MatrixMarket matrix coordinate integer general\n%\n<n_sites>\t<n_cells>\t<nnz>\n" and then
 *       "<site>\t<cell>\t<value>\n" per pair with value > 0, 1-based, site then cell ascending; n_cells = n
 *   cellSNP.base.vcf   "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", then per site
 *       "CHROM\tPOS\t.\tREF\tALT\t.\tPASS\tAD=<sum ad>;DP=<sum dp>;OTH=<sum oth>\n": CHROM as the VCF writer names it,
 *       REF and ALT the masks' letters in ACGT order joined by ',', REF 'N' for an empty ref_mask. A REF of two
 *       letters (heterozygous reference, diploid FASTA only) is not strict VCF.
 *   cellSNP.samples.tsv   one name per line: cell_<i> (0-based group id), or the names of secedo_variant_set_cell_names
 * Under SECEDO_VCF_BGZF the matrices and the VCF are .mtx.gz / .vcf.gz (BGZF, the same bytes once inflated; only
 * compressed bytes are downloaded); samples.tsv is always plain. The text is formatted on the GPU on both outputs, in
 * ranges of sites of at most SECEDO_ALLELE_BATCH_BYTES bytes of text (default 256 MiB, at least one site; the text
 * never depends on it; under BGZF the member cuts follow the ranges). */
#define SECEDO_ALLELE_NONE 0
#define SECEDO_ALLELE_ALL 1
#define SECEDO_ALLELE_CLUSTER 2

/* Process-wide. set: SECEDO_E_INVALID_ARG for another value; get: the selection set, else the environment's, else NONE
 * (a negative SECEDO_E_* for an unknown value of SECEDO_ALLELE_COUNTS). */
int secedo_variant_set_allele_counts(int selection);
int secedo_variant_get_allele_counts(void);

/* Process-wide: the n lines of cellSNP.samples.tsv (copied); n = 0 returns to cell_<i>. A name that is empty or holds
 * a tab or a line break is SECEDO_E_INVALID_ARG. A count other than the length of `clusters` makes the file-writing
 * calls fail with SECEDO_E_INVALID_ARG while a selection is on. The _file variant reads one name per line. */
int secedo_variant_set_cell_names(const char *const *names, uint32_t n);
int secedo_variant_set_cell_names_file(const char *path);

/* One (site, group) pair. */
typedef struct secedo_allele_pair {
    uint32_t site;   /* 0-based */
    uint32_t group;  /* 0-based */
    uint32_t ad, rd, oth;
} secedo_allele_pair;

/* Host only (no GPU needed). The sites of records[n_records] (locus ascending, each < n_loci: checked) under
 * `selection` (ALL or CLUSTER): site_locus / ref_mask / alt_mask[capacity] and *n_sites (SECEDO_E_LIMIT when more than
 * capacity: the required count in *n_sites, nothing written). */
int secedo_variant_allele_masks(const secedo_variant_record *records, uint32_t n_records, const uint8_t *locus_ref,
                                uint32_t n_loci, int selection, uint32_t *site_locus, uint8_t *ref_mask,
                                uint8_t *alt_mask, uint32_t capacity, uint32_t *n_sites);

/* The counts alone, on a flat pileup resident in HBM: host records as secedo_variant_calls_device returns them,
 * d_locus_ref[n_loci] in HBM. Out (host): the sites as secedo_variant_allele_masks gives them, site_totals
 * [3 * site_capacity] = the sums of ad, rd, oth per site, pairs[pair_capacity] in (site, group) order. SECEDO_E_LIMIT
 * when either capacity is too small: the required counts in *n_sites and *n_pairs, nothing written. A group id >=
 * n_cells is SECEDO_E_INVALID_ARG. Sets secedo_variant_allele_stats. Synchronises `stream`. */
int secedo_variant_allele_counts_device(int device_id, const uint64_t *d_locus_entry_off, const uint16_t *d_id_base16,
                                        const uint32_t *d_id_base32, uint32_t n_loci,
                                        const secedo_variant_record *records, uint32_t n_records,
                                        const uint8_t *d_locus_ref, uint32_t n_cells, int selection,
                                        uint32_t *site_locus, uint8_t *ref_mask, uint8_t *alt_mask,
                                        uint32_t *site_totals, uint32_t site_capacity, uint32_t *n_sites,
                                        secedo_allele_pair *pairs, uint64_t pair_capacity, uint64_t *n_pairs,
                                        void *stream);

/* What the allele counting of the last file-writing call of this thread (or secedo_variant_allele_counts_device) did;
 * all zero after a file-writing call under NONE. Times in ms, host wall clock unless said otherwise. */
typedef struct secedo_variant_allele_info {
    uint32_t selection;         /* SECEDO_ALLELE_* */
    uint32_t output;            /* SECEDO_VCF_* of the files; 0 for the counts alone */
    uint64_t sites;
    uint64_t deep_sites;        /* of those, the sites with more than 128 entries (the sorted route) */
    uint64_t entries_read;      /* pileup entries of the sites */
    uint64_t pairs;
    uint64_t nnz_ad, nnz_dp, nnz_oth;
    uint64_t text_bytes;        /* the four texts */
    uint64_t compressed_bytes;  /* BGZF: the four .gz files; PLAIN: 0 */
    uint64_t ranges;            /* ranges of sites the formatter ran in */
    double count_ms;            /* sites, counts, scans and pairs, with their read-backs */
    double format_ms;           /* the formatter's kernels and the download of the file offsets */
    double deflate_ms;          /* BGZF: the encoder */
    double download_ms;         /* the text (PLAIN) or the compressed bytes (BGZF) down */
    double write_ms;            /* the files */
    double count_kernel_ms;     /* the site, count and write kernels alone (device events), included in count_ms */
} secedo_variant_allele_info;
int secedo_variant_allele_stats(secedo_variant_allele_info *out);

/* ---- Genome composition per bin (GC, N, soft-mask) -----------------------------------------------------------------
 *
 * The companion of secedo_bam_depth (secedo_bam.h): per bin of the reference genome the counts that a copy-number tool
 * regresses depth on (GC) and filters bins by (N, repeats). The FASTA may be plain, gzip or BGZF; it is read through
 * the device route's input layer whatever SECEDO_FASTA says, counted in HBM (genome_bins_kernels.hip), and the rules
 * that decide numbers and bytes are in secedo_amd/csrc/genome_bins.hpp. This is the one statement of the contract.
 *
 * Contigs. Lines and their roles are those of fasta_lines.hpp (step): line 0 is a header, a '>' line directly after a
 * header is sequence. Every header starts a contig; its sequence is the sequence bytes up to the next header. There is
 * no maternal / paternal pairing: a diploid FASTA is more contigs. The name is the header's bytes after its first
 * byte, up to but excluding the first space, tab, '\r' or the line's end. A name may be empty; a name longer than 4096
 * bytes is SECEDO_E_INVALID_ARG. Of two contigs with one name the first is taken, the rest are counted in
 * duplicate_names.
 *
 * Selection. names == NULL: all contigs in file order. Else the n_names listed names in the listed order, matched
 * exactly: there is no chr aliasing, and the error says so. A listed name no contig has, or one listed twice, is
 * SECEDO_E_INVALID_ARG and is named in the message. lengths != NULL (with names): a contig whose sequence length
 * differs from lengths[i] is SECEDO_E_INVALID_ARG "<name>: the genome has <n> bases, expected <m>". An empty file and
 * an empty list are SECEDO_E_INVALID_ARG. A selected contig of more than 2^32 - 1 bases is SECEDO_E_LIMIT.
 *
 * Bins. Selected contig k of length L_k has ceil(L_k / S) bins [bS, min((b + 1)S, L_k)); global bin numbers run in
 * selection order: the layout of secedo_bam_depth. S == 0 is SECEDO_E_INVALID_ARG, more than 2^32 - 1 bins
 * SECEDO_E_LIMIT. A contig of length 0 has no bins.
 *
 * Counted. Six uint32 per bin, from the raw byte of every sequence byte in the bin: a (A a), c (C c), g (G g),
 * t (T t U u), other (every other byte: N, IUPAC codes, a '\r' inside a sequence line, a '>' that the line rule reads
 * as sequence) and masked (bytes 'a'..'z', counted in addition to the byte's class). a + c + g + t + other == end -
 * start always, and only integer sums exist: two runs give identical bytes.
 *
 * File. Only with out_path != NULL: "chrom\tstart\tend\ta\tc\tg\tt\tother\tmasked\n", then per global bin
 * "<name>\t<start>\t<end>\t<a>\t<c>\t<g>\t<t>\t<other>\t<masked>\n", 0-based half-open. SECEDO_GENOME_BINS_BGZF
 * writes <out_path>.gz instead, BGZF that inflates to the same bytes. An existing file is refused unless overwrite;
 * the file is written as <name>.tmp.<pid> and renamed, a failed call leaves nothing behind. The lines are formatted
 * on the GPU in ranges of at most SECEDO_GENOME_BINS_BATCH_BYTES of text (default 256 MiB, at least one line), which
 * never changes a byte of text; under BGZF the member cuts follow the ranges and only compressed bytes come down.
 * The text ranges of the input are SECEDO_FASTA_BATCH_BYTES as on the device route.
 *
 * Not done: mappability tracks (bigWig), normalisation of depth by these counts, .fai random access. */
#define SECEDO_GENOME_BINS_PLAIN 0
#define SECEDO_GENOME_BINS_BGZF 1
#define SECEDO_GENOME_BINS_COLUMNS 6 /* a, c, g, t, other, masked */

typedef struct secedo_variant_genome_bins_info {
    uint32_t kind;              /* SECEDO_FASTA_KIND_* */
    uint32_t output;            /* SECEDO_GENOME_BINS_* */
    uint64_t contigs;           /* header lines of the file */
    uint64_t selected;
    uint64_t duplicate_names;
    uint64_t bins;
    uint64_t bases;             /* sequence bytes of the selected contigs */
    uint64_t name_bytes;        /* the selected names one after the other: what _fetch's `names` must hold */
    uint64_t ranges;            /* ranges of FASTA text */
    uint64_t uploaded_bytes;    /* FASTA bytes sent to the GPU: text, or compressed members */
    uint64_t device_members;    /* BGZF members inflated on the GPU */
    uint64_t fasta_bytes;       /* FASTA text parsed and counted */
    uint64_t text_bytes;        /* the output file's text */
    uint64_t compressed_bytes;  /* BGZF: the bytes of the .gz file, the EOF member included; PLAIN: 0 */
    uint64_t members;           /* BGZF members with text */
    double upload_ms;           /* host time inside the uploads (they run beside the passes of the range before) */
    double parse_ms;            /* the reused scans and the header table (device events) */
    double count_ms;            /* k_compose (device events) */
    double format_ms, deflate_ms, download_ms, write_ms; /* the output file, host clocks as for secedo_bam_depth */
} secedo_variant_genome_bins_info;

/* names, lengths, out_path: NULL for none; info may not be NULL. Runs on the calling thread's device. Synchronous. */
int secedo_variant_genome_bins(const char *fasta, uint32_t bin_size, const char *const *names, const uint64_t *lengths,
                               uint32_t n_names, const char *out_path, int output, int overwrite,
                               secedo_variant_genome_bins_info *info);
/* Copies the last result of this thread into host buffers, any may be NULL: the selected names one after the other in
 * names[name_bytes] with name_off[selected + 1] their bounds, contig_lengths[selected], bin_contig (the position in
 * the selection) / bin_start / bin_end [bins], counts[bins][6]. The result stays until the next call on the thread.
 * SECEDO_E_STATE without a result. */
int secedo_variant_genome_bins_fetch(char *names, uint64_t *name_off, uint64_t *contig_lengths, uint32_t *bin_contig,
                                     uint32_t *bin_start, uint32_t *bin_end, uint32_t *counts);
/* the last secedo_variant_genome_bins call of this thread, a failed one up to its failure */
int secedo_variant_genome_bins_stats(secedo_variant_genome_bins_info *out);

/* The drop-in: variant_calling(pos_data, clusters, reference_genome, map_file, hetero_prior, theta, out_dir)
 * on a host flat pileup. Writes cluster_<i>.vcf for i = 0..max(clusters), common.vcf, an empty `variant` and
 * `scores` under out_dir (created), as the reference does (the .vcf files as .vcf.gz under SECEDO_VCF_BGZF, above);
 * n == 0 writes nothing. times may be NULL. Under SECEDO_ALLELE_ALL / _CLUSTER also out_dir/allele_counts/ (above),
 * after the other files; its time is in secedo_variant_allele_stats, not in `times`.
 * n_chr > 24 is SECEDO_E_INVALID_ARG before anything is made: the lines name the chromosomes 1..22, X, Y, and the
 * reference asserts on a later one. A reference genome or map that is refused (unequal maternal and paternal
 * contigs, where the reference ends its process after writing the preambles) leaves nothing behind: out_dir is
 * removed again if the call created it. */
int secedo_variant_calling(int device_id, const uint32_t *chr_locus_off, uint32_t n_chr,
                           const uint32_t *locus_pos, const uint64_t *locus_entry_off, const uint16_t *id_base16,
                           const uint32_t *id_base32, const uint16_t *clusters, uint32_t n,
                           const char *reference_genome, const char *map_file, double hetero_prior, double theta,
                           const char *out_dir, secedo_variant_times *times);

/* Same on a flat pileup resident in HBM (the layout secedo_divide_cluster_device takes); clusters is host.
 * The chromosome offsets and positions are read back: the positions for the VCF text and, on the host route, for the
 * host gather. On the device route locus_ref is computed in HBM and only downloaded for the VCF text; fasta_ms is
 * then the whole of secedo_variant_reference_genotypes_device and gather_ms 0. Synchronises `stream`. */
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
