/*
 * secedo_bam.h -- C-ABI of the pileup creation from aligned reads: the reference's pileup_bams()
 * (pileup.cpp:49-348, pileup.hpp:29-38). Library libsecedo_bam.so.
 *
 * The host memory-maps each BAM, inflates its BGZF blocks with zlib in a thread pool (CRC32 and ISIZE
 * checked), walks the records and uploads the byte run of the requested chromosome. The per-record decode,
 * the read-name numbering, the per-position base counts, the locus rule and the entry placement run on the
 * GPU (secedo_amd/csrc/bam_kernels.hip, which lists the restated semantics). The outputs equal the
 * reference's run with num_threads = 1: .bin and .map byte for byte, .txt wherever a locus has at most 16
 * entries. Error codes are those of secedo_simmat.h; secedo_bam_last_error() holds the message.
 *
 * Tag mode (secedo_pileup_bams_cells[_device]) reads multiplexed BAMs, one cell per value of a barcode tag (10x's
 * CB:Z): the cell of a record is the index of its Z-typed tag value in the barcode list, records of other values are
 * dropped. Its output equals the per-file call on the per-cell split files (record order Position, input file,
 * record); secedo_bam_barcodes lists the values found. Inflated bytes per file are bounded: a large file is inflated
 * and walked in ranges of BGZF blocks (about 512 MiB inflated; the environment variable SECEDO_BAM_BATCH_BYTES
 * overrides it, outputs do not depend on it).
 *
 * SAM input: every file list may mix BAM, coordinate-sorted SAM text files and BGZF-compressed SAM (what `bgzip`
 * writes, usually named .sam.gz). The type is decided by content, never by name: a plain gzip file (no BGZF extra
 * field) is SECEDO_E_INVALID_ARG ("decompress it to SAM or convert it to BAM"); of a BGZF file the first member
 * with ISIZE > 0 is inflated on the host, and it is BAM if that starts with "BAM\1", else BGZF SAM; anything else
 * is SAM. A SAM file gives exactly what the BAM `samtools view -b` writes from
 * it gives, in every call. The host parses the header (the leading '@' lines; every @SQ needs SN and LN, SN unique;
 * @SQ order = RefID = chromosome_id) and cuts the alignment lines into ranges of about SECEDO_BAM_BATCH_BYTES that
 * end at a '\n'; the GPU (secedo_amd/csrc/sam_kernels.hip, which lists the rules) splits the lines, validates them
 * and encodes the BAM records, following htslib's sam_parse1. Departures and limits:
 *  - an RNAME or RNEXT that no @SQ line names is an error (htslib warns and treats the record as unmapped);
 *  - an '@' line after the first alignment line, and an empty line other than the file's last, are errors;
 *  - a SEQ character that is neither a letter nor '=' gives code 15 (N); htslib reads the digits 0 to 3 as A, C, G, T,
 *    and the SAM specification allows neither;
 *  - f aux values are converted to float32 through double (the leading 18 digits times a power of ten, rounded
 *    twice), which is not the correctly rounded float32 for every text. The pileup reads no f value, but
 *    secedo_bam_split_clusters[_rg] copies them into its output files. What the tests pin (tests/sam_cases.py): texts
 *    of up to 9 significant digits, what "%.9g" and "%g" print, give the correctly rounded float32, exact ties
 *    between two floats included;
 *  - no line-length limit below 4 GiB (a range grows to hold its longest line); more than 65535 CIGAR ops or a
 *    record of 2^31 bytes or more is SECEDO_E_LIMIT;
 *  - a .sam.gz that is plain gzip, standard input and CRAM are not read.
 * BGZF SAM gives exactly what its inflated text gives as a plain SAM file, in every call, error messages (file
 * index, path, 1-based line of the inflated text) included. The host lists the blocks and inflates the leading ones
 * with zlib only until the '@' lines end; all other blocks are uploaded compressed and inflated on the GPU
 * (secedo_amd/csrc/bgzf_kernels.hip: full RFC 1951, ISIZE and CRC32 checked on the device) in ranges of about
 * SECEDO_BAM_BATCH_BYTES inflated bytes, each range's text up to its last '\n' going to the SAM passes and the rest
 * to the front of the next range, device to device; the inflated text never reaches the host. A block that does not
 * inflate is SECEDO_E_INVALID_ARG in the BAM route's words ("<path>: BGZF block <k>: inflate failed or ISIZE
 * mismatch" or "... CRC32 mismatch"), the first such block in file order, ahead of any parse error below it. For
 * BGZF SAM, inflate_ms is the header's host inflate plus the device inflate, upload_ms includes the compressed
 * bytes, and inflated_bytes is the inflated size. BAM files are still inflated on the host by default.
 * Errors in a SAM file name the file index, its path and the 1-based line (record k of a file with h header lines
 * is line h + k + 1): parse errors, the host's structural checks and the device passes' rule-6 errors; of several
 * bad lines the first is reported. For SAM, secedo_bam_times.inflate_ms is the text read and walk_ms includes the
 * device parse. secedo_bam_scan reads BAM only and stays on the host.
 *
 * The device route for BAM (opt-in: secedo_bam_set_inflate(SECEDO_BAM_INFLATE_DEVICE), or SECEDO_BAM_INFLATE=device in
 * the environment): BAM files take the way of BGZF SAM. The host inflates a file's leading members only until its
 * header and reference list are complete; every other member goes up compressed and is inflated on the GPU, many small
 * files to one launch, a large file in ranges of about SECEDO_BAM_BATCH_BYTES. The record walk (block_size chain,
 * structure, sortedness, the first run of each requested chromosome, the CIGAR checks) runs on the GPU too
 * (secedo_amd/csrc/bam_walk_kernels.hip), and only the records of the requested chromosomes come back. For valid input
 * every call returns exactly what the host route returns. A file with one defect gives the host route's code and
 * message. Of several defects the lowest file index is reported; within a file a member that does not inflate
 * ("<path>: BGZF block <k>: ...") comes before any record error in or after that member's bytes, and of record errors
 * the lowest record. The route fills secedo_bam_times as BGZF SAM does: inflate_ms is the header's host inflate plus
 * the device inflate, upload_ms the staging and upload of the compressed bytes, walk_ms the device walk and the
 * read-back of the records.
 *
 * Reading through the .bai index (opt-in: secedo_bam_set_index, or SECEDO_BAM_INDEX=auto|require in the environment;
 * the default is off, and then no index file is opened). The index file is <path>.bai, else <path without .bam>.bai;
 * its modification time is not consulted. Of an indexed BAM only the members of the header and of the requested
 * chromosomes' spans are inflated and walked, on either route: per reference the index gives where its records start
 * and end (bam_index.hpp); spans whose members touch or overlap are read as one; the members of a span are found by
 * following BSIZE from its first, so the file is never listed in full. For a coordinate-sorted BAM with a matching
 * index every call returns exactly what it returns with the index off. AUTO reads a BAM without an index file, or with
 * one that fails the file-level checks (magic, n_ref against the BAM header, and for the start and the end of every
 * reference: coffset below the file size, a BGZF member at it, uoffset within its ISIZE, start <= end), in full; REQUIRE makes that SECEDO_E_INVALID_ARG, naming the
 * BAM and the reason. An index that passes those checks and still does not fit the file is SECEDO_E_INVALID_ARG in
 * both modes ("<bam>: index does not match the file (...); re-index it or use --index off"): the record at a
 * chromosome's start has another RefID, the record chain from a span's start breaks or does not land on its end, the
 * pseudo-bin's count differs from the records between start and end, or the record at the end offset, where the
 * span's last member holds it, still has the chromosome's RefID. The whole-file ordinals of an indexed file are
 * unknown: messages say "indexed record k" (k counts from the first record of the file's first span) and "BGZF
 * block at byte <coffset>". A defect outside every span is not seen. SAM, BGZF SAM and secedo_bam_scan[_device]
 * never use an index.
 *
 * Writing BAM (secedo_bam_split_clusters, below): one coordinate-sorted cluster_<k>.bam per cluster of a clustering,
 * the pseudo-bulk files of the subclones. The inputs are read as for a pileup call, every kind, route and index mode;
 * cell to cluster, the merged order (a stable radix sort), the gather of whole records into per-cluster streams and the
 * BGZF DEFLATE run on the GPU (secedo_amd/csrc/bam_split_kernels.hip, bgzf_deflate_kernels.hip), and only compressed
 * bytes come back. Records are copied byte for byte, or with secedo_bam_split_clusters_rg with an RG tag that names
 * their cell written inside the gather; the bytes of every output are fixed by the rules at the call.
 */
#ifndef SECEDO_BAM_H
#define SECEDO_BAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SECEDO_BAM_MAX_FILES 16384u /* cell_base = cell << 2 | base is a u16 */

/* Header and record summary of one BAM file (host only, no GPU). */
typedef struct secedo_bam_scan_info {
    uint32_t n_ref;          /* entries of the @SQ dictionary */
    uint32_t sorted;         /* 1 if (RefID, Position) never decreases (RefID -1 sorts last) */
    uint64_t n_records;      /* all records, unmapped ones included */
    uint64_t n_unmapped;     /* records with RefID -1 */
    uint64_t n_blocks;       /* BGZF blocks, the empty EOF block included */
    uint64_t inflated_bytes; /* total ISIZE */
    uint32_t l_text;         /* length of the SAM header text */
    uint32_t reserved;
} secedo_bam_scan_info;

/* Per-step wall times of one call, in ms (inflated_bytes in bytes). */
typedef struct secedo_bam_times {
    double inflate_ms;     /* BGZF inflate + CRC32 check, all files */
    double inflated_bytes;
    double walk_ms;        /* header parse, record walk, the chromosome's runs concatenated, global ordering */
    double upload_ms;      /* record bytes and offsets to HBM */
    double device_ms;      /* every launch and read-back of the device passes */
    double write_ms;       /* .bin, .map, .txt */
    double total_ms;
} secedo_bam_times;

/* Sizes of the last result (see secedo_bam_fetch). */
typedef struct secedo_bam_result_info {
    uint64_t n_loci;
    uint64_t n_entries;
    uint32_t n_chr;
    uint32_t num_cells;       /* as secedo_pileup_read reports it on the written .bin (max over chromosomes) */
    uint32_t max_read_length; /* idem: longest span of one read id between its kept loci */
    uint32_t reserved;
} secedo_bam_result_info;

/* What the last pileup, barcode or scan call on this thread did with its BGZF members. */
typedef struct secedo_bam_route_info {
    uint64_t host_blocks;             /* members inflated on the host (device route: the headers' members) */
    uint64_t device_blocks;           /* members inflated on the device */
    uint64_t device_records;          /* BAM records walked on the device */
    uint64_t segments;                /* segments of the device walk */
    uint64_t rewalked_segments;       /* of those, the ones whose guessed start was no record start */
    uint64_t uploaded_bytes;          /* compressed bytes uploaded */
    uint64_t downloaded_record_bytes; /* record bytes of the requested chromosomes downloaded (device route) */
    uint64_t batches;                 /* device inflate launches */
} secedo_bam_route_info;

#define SECEDO_BAM_INFLATE_HOST 0   /* the default: zlib in a host pool, host record walk */
#define SECEDO_BAM_INFLATE_DEVICE 1 /* BAM members inflated and records walked on the GPU */

/* What the last pileup or barcode call on this thread did with the .bai indexes of its BAM files. */
typedef struct secedo_bam_index_info {
    uint64_t files_indexed;   /* BAM files read through their index */
    uint64_t files_full;      /* BAM files read in full under AUTO: no index file, or a rejected one */
    uint64_t rejected;        /* of those, the ones whose index file failed the file-level checks */
    uint64_t spans;           /* spans read (member runs of the requested chromosomes, merged where they touch) */
    uint64_t members;         /* BGZF members of those spans */
    uint64_t members_skipped; /* members known to be skipped; needs the member listing, so 0 for an indexed file */
} secedo_bam_index_info;

#define SECEDO_BAM_INDEX_OFF 0     /* the default: no index file is opened, every member is read */
#define SECEDO_BAM_INDEX_AUTO 1    /* a BAM with a usable .bai is read through it, any other in full */
#define SECEDO_BAM_INDEX_REQUIRE 2 /* a BAM without a usable .bai is SECEDO_E_INVALID_ARG */

/* What the last pileup or barcode call on this thread selected by rules 3c and 3d of secedo_amd/csrc/bam_kernels.hip,
 * summed over its chromosomes. All zero when the read filter and the duplicate removal were off: no pass ran. */
typedef struct secedo_bam_select_info {
    uint64_t records;             /* records that reached the flag filter (tag mode: those of listed barcodes;
                                     secedo_bam_barcodes: those with a Z-typed value); 0 with the filter off */
    uint64_t dropped_require;     /* dropped by (flag & require) != require; tested first, a record is counted once */
    uint64_t dropped_exclude;     /* dropped by (flag & exclude) != 0 */
    uint64_t templates;           /* templates (records of one cell with one name) formed by the duplicate removal */
    uint64_t large_templates;     /* of those, the ones of three or more records: never duplicates */
    uint64_t duplicate_templates; /* templates dropped as duplicates */
    uint64_t duplicate_records;   /* their records */
    uint64_t reserved;
} secedo_bam_select_info;

#define SECEDO_BAM_DUPLICATES_KEEP 0   /* the default */
#define SECEDO_BAM_DUPLICATES_REMOVE 1 /* per cell and chromosome, keep the best template of each 5'-end key */

const char *secedo_bam_last_error(void);

/* Record selection by SAM flag, per process, read at every pileup and barcode call (secedo_bam_index_build and the
 * scans ignore it): a record is used iff (flag & require) == require && (flag & exclude) == 0. A dropped record takes
 * no read id, writes no .map line, passes none of the device checks (so a record that is not a proper pair is no
 * error once it is excluded) and gives no base: the outputs equal those of the same call with the filter off on the
 * files without the dropped records. The host's structural checks still cover every record. Masks above 0xFFFF or
 * sharing a bit are SECEDO_E_INVALID_ARG. Until it is set, the environment variables SECEDO_BAM_REQUIRE_FLAGS and
 * SECEDO_BAM_EXCLUDE_FLAGS (decimal or 0x hex; unset or empty: 0) decide. The default 0, 0 runs no pass. */
int secedo_bam_set_read_filter(uint32_t require, uint32_t exclude);
int secedo_bam_get_read_filter(uint32_t *require, uint32_t *exclude);

/* Duplicate removal among the records the filter kept, per process, read at every pileup call (secedo_bam_barcodes
 * ignores it): SECEDO_BAM_DUPLICATES_KEEP or _REMOVE; until it is set, SECEDO_BAM_DUPLICATES (keep or remove; unset or
 * empty: keep) decides. Per chromosome and cell (file, or barcode in tag mode), the records of one read name form a
 * template; singles with the same unclipped 5' end and strand, and pairs with the same two, are duplicates of each
 * other, and all but the one with the highest sum of base qualities >= 15 (ties: the earliest in the global order) are
 * dropped like filtered records. Templates of three or more records are left alone. Bit-identical between runs. */
int secedo_bam_set_duplicates(int mode);
int secedo_bam_get_duplicates(int *mode);
int secedo_bam_select_stats(secedo_bam_select_info *out);

/* Whether BAM files are read through their .bai index, per process, read at every call. Until it is set, the
 * environment variable SECEDO_BAM_INDEX (off, auto or require; unset or empty: off) decides; any other value of it
 * makes every call that reads BAM, and secedo_bam_get_index, fail with SECEDO_E_INVALID_ARG. */
int secedo_bam_set_index(int mode);
int secedo_bam_get_index(int *mode);
int secedo_bam_index_stats(secedo_bam_index_info *out);

/* Host only, no GPU: what the index beside bam_path (<path>.bai, else <path without .bam>.bai) says of each
 * reference r < min(capacity, *n_ref): the virtual offsets (coffset << 16 | uoffset) where its records start and
 * end, both 0 for a reference without records, and its record count from the pseudo-bin, UINT64_MAX where the index
 * has none. The file-level checks against the BAM are made; a missing or rejected index is SECEDO_E_INVALID_ARG.
 * Any array may be NULL. */
int secedo_bam_index_ranges(const char *bam_path, uint32_t *n_ref, uint64_t *beg, uint64_t *end, uint64_t *count,
                            uint32_t capacity);

/* The route BAM files take, per process, read at every call. Until it is set, the environment variable
 * SECEDO_BAM_INFLATE (host or device; unset or empty: host) decides; any other value of it makes every call that
 * reads BAM, and secedo_bam_get_inflate, fail with SECEDO_E_INVALID_ARG. */
int secedo_bam_set_inflate(int mode);
int secedo_bam_get_inflate(int *mode);
int secedo_bam_route_stats(secedo_bam_route_info *out);

/* secedo_bam_scan with the inflate and the record walk on the GPU: the same info and counts. Needs the GPU. */
int secedo_bam_scan_device(const char *path, uint32_t num_threads, secedo_bam_scan_info *info,
                           uint64_t *records_per_ref, uint32_t capacity);

/* What secedo_bam_index_build wrote, summed over the files whose index was finished. */
typedef struct secedo_bam_build_info {
    uint64_t files;       /* indexes written */
    uint64_t records;     /* records of those files */
    uint64_t chunks;      /* chunks written, the pseudo-bins' two not counted */
    uint64_t bins;        /* bins written, the pseudo-bins not counted */
    uint64_t windows;     /* entries of the linear indexes (n_intv summed) */
    uint64_t index_bytes; /* bytes of the index files */
    uint64_t joined_runs; /* range boundaries of a file across which a run of one (RefID, bin, flag 0x4) went on */
    uint64_t reserved;
} secedo_bam_build_info;

/* Writes a .bai index (SAM spec 5.2) for each of n_files coordinate-sorted BAM files in one pass over them, to
 * out_paths[f], or to <bam>.bai where out_paths or out_paths[f] is NULL. Always the device route, whatever
 * secedo_bam_set_inflate says: the members are inflated and the records walked on the GPU as for
 * secedo_bam_scan_device, many small files to a batch, and an index pass (secedo_amd/csrc/bam_index_kernels.hip) finds
 * there each record's end (pos + the CIGAR's reference length, at least pos + 1), its bin (reg2bin of that, the
 * record's own bin field is not read), the heads of the runs of one (RefID, bin) and the first record over each 16 kb
 * window; only those come back. No index is read. What is written is fixed: bins ascending, a bin's chunks (maximal
 * runs of consecutive records of one bin) in file order, the pseudo-bin 37450 for every reference with records, the
 * linear index up to the last touched window with htslib's backward fill, n_no_coor. Virtual offsets name the first
 * member that holds a byte at or past the inflated offset, the end of the data the EOF member, else the file size.
 * Errors are SECEDO_E_INVALID_ARG and name the file and, where there is one, the record: input that is not
 * coordinate-sorted, a SAM, BGZF SAM or plain-gzip file, a member that does not inflate or a broken record chain (in
 * secedo_bam_scan_device's words), a reference longer than 2^29 or a record that ends past 2^29 (BAI cannot hold it),
 * an output that exists while overwrite is 0. An index is written to a temporary name beside its target and renamed, so
 * a failed file leaves nothing; the files in front of it in the list keep their finished indexes, and *info counts
 * those. Sets secedo_bam_route_stats. Synchronous. num_threads: the staging pool, capped at 16 (0 = 1). */
int secedo_bam_index_build(const char *const *bam_files, uint32_t n_files, const char *const *out_paths, int overwrite,
                           uint32_t num_threads, secedo_bam_build_info *info);

/* What the last secedo_bam_split_clusters call on this thread wrote (all of it, also after a failure: then what it
 * had done by then). */
typedef struct secedo_bam_split_info {
    uint64_t files;            /* input files */
    uint64_t clusters;         /* cluster_<k>.bam files written: max(cell_cluster) + 1 */
    uint64_t cells;
    uint64_t records;          /* records written, over all clusters and chromosomes */
    uint64_t dropped_records;  /* tag mode: records of the requested chromosomes without a listed barcode */
    uint64_t text_bytes;       /* uncompressed bytes of the outputs: headers and records */
    uint64_t compressed_bytes; /* bytes of the outputs, the EOF members included */
    uint64_t members;          /* BGZF members made, the EOF members not counted */
    uint64_t stored_members;   /* of those, the ones that fell back to a stored block */
    double order_ms;           /* keys, compaction, sort, destinations, extents */
    double gather_ms;          /* the gather kernel (stream events) */
    double deflate_ms;         /* descriptors up, encoder and packer */
    double download_ms;        /* compressed bytes to the host */
    double write_ms;           /* appending to the temporary files, closing, renaming */
} secedo_bam_split_info;

/* Writes one coordinate-sorted BAM per cluster of a clustering: <out_dir>/cluster_<k>.bam for every k in
 * 0..max(cell_cluster), holding the records of the cells c with cell_cluster[c] == k (a k no cell has gives a
 * header-only file). The pseudo-bulk files of the subclones `secedo_main` found (its `clustering` file is cell_cluster).
 *
 * Cells: per-file mode (tag NULL): the cell of a record is its file's index, n_cells must equal n_files. Tag mode: the
 * cell is the index of the record's Z-typed tag value in barcodes, as in secedo_pileup_bams_cells; n_cells must equal
 * n_barcodes; records without the tag, with another type or an unlisted value are dropped and counted in
 * info->dropped_records.
 *
 * Which records: of every file what the pileup calls read (the first contiguous run of each requested chromosome;
 * BAM, SAM and BGZF SAM; either route, any index mode, any SECEDO_BAM_BATCH_BYTES, with the pileup calls' codes and
 * messages for defective input), byte for byte as in the input, block_size included. Records with RefID -1 are not
 * written. The read filter, the duplicate removal and the quality, MAPQ and pair rules of the pileup do not apply (a
 * selection of the call's own: secedo_bam_split_clusters_select below).
 * chromosome_ids are RefIDs; they are sorted before use; a duplicate or an id at or past n_ref is SECEDO_E_INVALID_ARG.
 * Order within an output: RefID, Position, input file index, the record's ordinal in its file.
 *
 * All inputs must share one reference list (count, names, lengths, order); else SECEDO_E_INVALID_ARG naming the file,
 * the first file and the reference. Header of every output: "BAM\1", l_text, the text, n_ref and the first file's
 * binary reference list (built from its @SQ lines when it is SAM). The text: "@HD\tVN:1.6\tSO:coordinate"; one
 * "@SQ\tSN:<name>\tLN:<len>" per reference of that list; the distinct @RG lines of all inputs in order of first
 * appearance (files in list order, lines in header order, compared as whole lines; two different lines with one ID
 * are SECEDO_E_INVALID_ARG naming both files); "@PG\tID:secedo_amd.split\tPN:secedo_amd";
 * "@CO\tsecedo_amd cluster <k>: <m> of <n> cells". Every line ends in '\n'; input @PG and @CO lines are not carried.
 *
 * Layout, fixed: with M(x) the members the BGZF encoder of secedo_amd/csrc/bgzf_deflate.hpp gives for bytes x (cut
 * every 0xFF00 bytes from x's start, fixed Huffman or stored by its rule, nothing for empty x), a file is M(header),
 * M(records of the first requested chromosome), ..., M(records of the last), the 28-byte EOF member. A member may cut
 * a record anywhere. Cell to cluster, the merged order, the gather of whole records into per-cluster streams and the
 * DEFLATE run on the GPU (secedo_amd/csrc/bam_split_kernels.hip); only compressed bytes come back.
 *
 * Files are written to a temporary name beside the target (<target>.tmp.<pid>) and renamed when all are complete. An
 * existing target is SECEDO_E_INVALID_ARG unless overwrite. A failed call leaves no temporaries and no new
 * cluster_*.bam. times is filled as the pileup calls fill it (write_ms: the outputs); secedo_bam_route_stats and
 * secedo_bam_index_stats are set as for a pileup call. num_threads: the host inflate pool. Not done: unplaced records,
 * CB tags appended to records (RG tags: secedo_bam_split_clusters_rg below), merged cell groups, .csi, several GPUs.
 * Synchronous. */
int secedo_bam_split_clusters(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                              uint32_t n_chr, const uint16_t *cell_cluster, uint32_t n_cells, const char tag[2],
                              const char *const *barcodes, uint32_t n_barcodes, const char *out_dir, int overwrite,
                              uint32_t num_threads, secedo_bam_split_info *info, secedo_bam_times *times);
int secedo_bam_split_stats(secedo_bam_split_info *out);

/* What the last secedo_bam_split_clusters_rg call on this thread edited (also after a failure: up to it). All zero
 * after a secedo_bam_split_clusters call. */
typedef struct secedo_bam_split_rg_info {
    uint64_t tagged_records;   /* records written with an appended RG */
    uint64_t replaced_records; /* of those, the ones whose own RG field was removed */
    uint64_t unparsed_records; /* of those, the ones whose aux area did not parse: nothing removed */
    uint64_t added_bytes;      /* appended bytes, over all records */
    uint64_t removed_bytes;    /* removed bytes, over all records */
    uint64_t reserved[3];
} secedo_bam_split_rg_info;

/* secedo_bam_split_clusters with the cell of every read named in the files: one read group per cell. Everything of
 * that call's contract holds (which records, their order, the layout M(header) M(chr) ... EOF, temporaries and
 * renames, errors leave no file, the stats) except the three rules below; text_bytes and compressed_bytes count the
 * edited bytes. The outputs are multiplexed BAMs: secedo_pileup_bams_cells with tag "RG" and a cluster's names reads
 * one back cell by cell.
 *
 * 1. Cell names. cell_names NULL: the file's base name without the first of .sam.gz, .bam, .sam that it ends in
 * (per-file mode), the barcode (tag mode). Else n_names must equal n_cells. A name, given or default, is 1 to 254
 * bytes, every byte in 0x21..0x7E, and no two cells share one; else SECEDO_E_INVALID_ARG naming the cell index, or both
 * for a clash. The names are checked before any input is read.
 *
 * 2. Header. The inputs' @RG lines are not carried (the tags that referred to them are removed, and their IDs cannot
 * clash). In their place, between the @SQ lines and @PG, cluster k's file has one "@RG\tID:<name>\tSM:cluster_<k>" per
 * cell of cluster k, in cell order.
 *
 * 3. Records. The aux area of a written record is walked strictly: a field is a two-byte tag, a type byte and a value
 * (A c C: 1 byte; s S: 2; i I f: 4; Z H: up to and including the NUL; B: a subtype byte, a u32 count, count elements of
 * the subtype's size); every field ends within the record and the walk ends exactly at its end. If it does, the first
 * field named RG is removed whole (tag, type and value, whatever the type). If it does not (an unknown type, a field
 * past the end, one or two bytes left), nothing is removed and the record counts in unparsed_records. In both cases
 * 'R' 'G' 'Z' <name of the record's cell> '\0' is appended at the record's end and block_size becomes the new length
 * minus 4; no other byte changes. RGZ inside another field's value means nothing. With tag "RG" the cell is found from
 * the old value as ever, and the field is replaced like any other.
 *
 * The walk, the edited lengths and the gather that assembles the edited records run on the GPU
 * (secedo_amd/csrc/bam_split_kernels.hip: k_split_plan, k_split_gather_rg; the rules in bam_split.hpp). Not done:
 * unplaced records, CB tags, PL / LB fields of the @RG lines, merged cell groups. */
int secedo_bam_split_clusters_rg(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                                 uint32_t n_chr, const uint16_t *cell_cluster, uint32_t n_cells, const char tag[2],
                                 const char *const *barcodes, uint32_t n_barcodes, const char *out_dir, int overwrite,
                                 uint32_t num_threads, secedo_bam_split_info *info, secedo_bam_times *times,
                                 const char *const *cell_names, uint32_t n_names,
                                 secedo_bam_split_rg_info *rg_info);
int secedo_bam_split_rg_stats(secedo_bam_split_rg_info *out);

/* secedo_bam_split_clusters (read_groups 0) or secedo_bam_split_clusters_rg (read_groups != 0; rg_info, cell_names and
 * n_names are ignored when it is 0) with records selected while each record's cell is still known: after the merge two
 * reads of one cluster file with the same ends may come from two cells, and are then no duplicates, so no tool can mark
 * a cluster file. require, exclude and duplicates (SECEDO_BAM_DUPLICATES_KEEP, _REMOVE or _MARK) are this call's own;
 * with 0, 0, _KEEP the call is the plain one: the same bytes, launches and allocations. The process-wide
 * secedo_bam_set_read_filter and secedo_bam_set_duplicates and the environment variables SECEDO_BAM_REQUIRE_FLAGS,
 * SECEDO_BAM_EXCLUDE_FLAGS and SECEDO_BAM_DUPLICATES have no effect on any split call, this one included.
 *
 * Let S be the records the plain call would write: those of the requested chromosomes that have a cell.
 * 1. Filter. A record of S is kept iff (flag & require) == require && (flag & exclude) == 0. Masks above 0xFFFF, or
 *    masks that share a bit, are SECEDO_E_INVALID_ARG, as is an unknown duplicates mode; both are checked before any
 *    input is read. Filtered records are not written and take no part in rule 2.
 * 2. Duplicates. Among what rule 1 kept, per cell and per chromosome, exactly as rule 3d of
 *    secedo_amd/csrc/bam_kernels.hip (secedo_bam_set_duplicates above): a template is the records of one cell with one
 *    read name; singles with the same unclipped 5' end and strand are duplicates of each other, pairs with the same two
 *    ends likewise, a single never of a pair; the template with the highest sum of base qualities >= 15 stays, on a tie
 *    the one holding the record that comes first in the pileup's global order; templates of three or more records are
 *    left alone; mates on another chromosome are not seen. The records chosen are the ones
 *    secedo_pileup_bams(_cells) with duplicate removal on drops for the same input, cells and filter.
 * 3. _REMOVE: the chosen records are not written. Every output equals what the plain call writes on inputs that never
 *    held the records dropped by rules 1 and 2.
 * 4. _MARK: the chosen records are written with bit 0x400 set in their FLAG: byte 19 of the record counting from
 *    block_size, OR 0x04. No other byte of any record changes and no bit is ever cleared: a record that arrives marked
 *    and is not chosen keeps its mark (put 0x400 into exclude to drop incoming marks). Record lengths, order, extents,
 *    member cuts and headers are those of the same call with _KEEP.
 * 5. Unchanged from the plain call: the header text (no new @PG line), the layout M(header) M(chr) ... EOF,
 *    temporaries and renames, and a failed call leaves no file. A cluster whose records were all dropped gives a
 *    header-only file; a chromosome whose records were all dropped contributes no member.
 * 6. With read_groups the RG edit is applied to what rules 1 to 3 kept; a marked record gets both edits (the FLAG lies
 *    in the fixed 36 bytes, in front of any hole).
 *
 * *select_info (secedo_bam_split_select_stats: the last split call of this thread, all zero after a call without
 * selection) has the meanings of secedo_bam_select_info: records reached the filter (0 with it off),
 * duplicate_templates and duplicate_records count what rule 2 chose, marked or removed. secedo_bam_select_stats, the
 * pileup's getter, is not touched. info->dropped_records stays the records without a listed barcode; info->records is
 * what was written. The filter, rule 3d's passes over the sorted records, the compaction and the mark (carried to the
 * gather in the top bit of each record's source offset) run on the GPU: secedo_amd/csrc/bam_split_kernels.hip,
 * bam_kernels.hip. Not done: clearing marks, optical or UMI-aware duplicates, a @PG line for the marking. */
#define SECEDO_BAM_DUPLICATES_MARK 2 /* split calls only; secedo_bam_set_duplicates(2) stays an error */
int secedo_bam_split_clusters_select(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                                     uint32_t n_chr, const uint16_t *cell_cluster, uint32_t n_cells, const char tag[2],
                                     const char *const *barcodes, uint32_t n_barcodes, const char *out_dir,
                                     int overwrite, uint32_t num_threads, secedo_bam_split_info *info,
                                     secedo_bam_times *times, const char *const *cell_names, uint32_t n_names,
                                     secedo_bam_split_rg_info *rg_info, int read_groups, uint32_t require,
                                     uint32_t exclude, int duplicates, secedo_bam_select_info *select_info);
int secedo_bam_split_select_stats(secedo_bam_select_info *out);

/* ---- Per-cell read depth in fixed genomic bins: the bins x cells count matrix that copy-number tools
 * start from (HMMcopy's readCounter, Ginkgo, SCOPE), counted on the GPU from the inputs of the pileup calls (BAM, SAM,
 * bgzipped SAM, per cell or multiplexed by tag, either inflate route, through .bai or not). No outside tool was run
 * against the files; the contract is what follows, byte for byte.
 *
 * Bins. Chromosome id c is @SQ index c. LN_c and the name come from the first input's reference list; all inputs must
 * carry the same list (SECEDO_E_INVALID_ARG in the words of the split calls). With bin_size S >= 1 chromosome c has
 * ceil(LN_c / S) bins and bin b covers [b S, min((b + 1) S, LN_c)). Global bin numbers run over the requested
 * chromosomes in ascending id, whatever order they were given in. S == 0 is SECEDO_E_INVALID_ARG, more than 2^32 - 1
 * bins in total SECEDO_E_LIMIT, each with a reason.
 *
 * Cells. As in secedo_bam_split_clusters: the file index, or with tag / barcodes the index of the record's barcode in
 * the list. Names (depth.samples.tsv, depth.cells.tsv): cell_names (n_names = the cell count), else the barcode, else
 * the file's base name without .bam / .sam / .sam.gz; a name that is empty or holds a tab or a line break is
 * SECEDO_E_INVALID_ARG.
 *
 * Selection, in this order, from this call's arguments only (the process-wide secedo_bam_set_read_filter and
 * secedo_bam_set_duplicates and their environment variables have no effect): 1. the barcode; 2. the flag masks:
 * (flag & require) == require && (flag & exclude) == 0, `require` counted first; 3. duplicates (SECEDO_BAM_DUPLICATES_KEEP
 * or _REMOVE): per cell and chromosome exactly as secedo_bam_split_clusters_select's rule 2; 4. MapQuality >=
 * min_map_quality; 5. range: a record whose Position is < 0 or >= LN_c is dropped and counted as out_of_range.
 *
 * What is counted. SECEDO_BAM_DEPTH_READS: each surviving record adds 1 to the bin of its 0-based Position.
 * SECEDO_BAM_DEPTH_BASES: each surviving record adds, to every bin it touches, the number of reference positions in
 * that bin that an M, = or X op of its CIGAR covers; D, N, P, I, S and H add nothing, D and N advance the position,
 * positions >= LN_c add nothing, and a record without a CIGAR adds nothing but is still a counted record (the mean
 * depth times the width that `mosdepth --by` reports, kept as an integer). Values are uint64 everywhere; only integer
 * sums exist, so no result depends on an execution order and two runs are byte-identical.
 *
 * Files, under <out_dir>/depth/ (created when missing), only with out_dir != NULL; out_dir must be a directory. An
 * existing output is refused unless overwrite; every file is written under <name>.tmp.<pid> and renamed when all are
 * complete, and a failed call leaves nothing behind.
 *   depth.bins.bed      "<name>\t<start>\t<end>\n" per global bin, 0-based half-open
 *   depth.counts.mtx    "%%MatrixMarket matrix coordinate integer general\n%\n<n_bins>\t<n_cells>\t<nnz>\n", then
 *                       "<bin>\t<cell>\t<value>\n" per pair with value > 0, numbers 1-based, ordered by bin and then
 *                       cell ascending (the convention of cellSNP.tag.*.mtx)
 *   depth.samples.tsv   one cell name per line
 *   depth.cells.tsv     "cell\tname\trecords\tcounted\tsum\tnonzero_bins\tmax_value\n", then one line per cell (cell
 *                       0-based): records = the cell's records on the requested chromosomes after step 1, counted =
 *                       those that survived all five steps, sum = the sum of the cell's values, nonzero_bins and
 *                       max_value over the cell's pairs
 *   depth.clusters.tsv  with a clustering only (n_clustering = the cell count, else SECEDO_E_INVALID_ARG):
 *                       "chrom\tstart\tend\tcluster_0\t...\tcluster_<K-1>\n", K = max(clustering) + 1, then one line
 *                       per global bin, empty ones included, with the sum over each cluster's cells; a cluster
 *                       without cells gives a column of zeros
 * With SECEDO_BAM_DEPTH_BGZF the .mtx and the two .tsv with per-bin or per-cell lines are BGZF files .mtx.gz /
 * .tsv.gz that inflate to the same bytes; bins.bed and samples.tsv stay plain. The text is formatted on the GPU in
 * ranges of at most SECEDO_DEPTH_BATCH_BYTES bytes (default 256 MiB, at least one line), which never changes a byte
 * of text; under BGZF the member cuts follow the ranges and only compressed bytes are downloaded.
 *
 * The result (bins, pairs, per-cell table, cluster sums) stays on the host until the next call on this thread or
 * secedo_bam_release; secedo_bam_depth_fetch copies it out. Chromosomes are processed one after the other with a
 * chromosome's records resident: fewer than 2^32 records and at most 2^32 - 1 pieces (a piece is a record in `reads`
 * mode, a (record, touched bin) in `bases` mode) per chromosome, else SECEDO_E_LIMIT. GC, N and soft-mask content of
 * the same bins: secedo_variant_genome_bins (secedo_variant.h), given the names and lengths that
 * secedo_bam_depth_chromosomes returns. Not done: mappability tracks (bigWig), normalisation, segmentation, counting
 * templates instead of records, CG-tag CIGARs. */
#define SECEDO_BAM_DEPTH_READS 0
#define SECEDO_BAM_DEPTH_BASES 1
#define SECEDO_BAM_DEPTH_PLAIN 0
#define SECEDO_BAM_DEPTH_BGZF 1

typedef struct secedo_bam_depth_info {
    uint64_t files, cells, chromosomes, bins, clusters; /* clusters: K, 0 without a clustering */
    uint64_t records, counted;                           /* after step 1; after all five steps */
    uint64_t dropped_barcode, dropped_require, dropped_exclude, dropped_duplicate, dropped_mapq, out_of_range;
    uint64_t pieces, pairs;                              /* sorted (record, bin) pieces; pairs with value > 0 */
    uint64_t text_bytes, compressed_bytes, members, ranges; /* of the GPU-formatted files; compressed: BGZF only */
    double order_ms, count_ms, format_ms, deflate_ms, download_ms, write_ms;
} secedo_bam_depth_info;

/* tag / barcodes: NULL for one cell per file. clustering, cell_names, out_dir: NULL for none. info may not be NULL,
 * times may. Synchronous. */
int secedo_bam_depth(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids, uint32_t n_chr,
                     const char tag[2], const char *const *barcodes, uint32_t n_barcodes, uint32_t bin_size, int mode,
                     uint32_t min_map_quality, uint32_t require, uint32_t exclude, int duplicates,
                     const uint16_t *clustering, uint32_t n_clustering, const char *const *cell_names,
                     uint32_t n_names, const char *out_dir, int output, int overwrite, uint32_t num_threads,
                     secedo_bam_depth_info *info, secedo_bam_times *times);
/* Copies the last result of this thread into host buffers, any may be NULL: bin_chr / bin_start / bin_end [bins] (the
 * chromosome id and the 0-based half-open extent of each global bin), pair_bin / pair_cell / pair_value [pairs]
 * (0-based, in the .mtx order), cell_table [cells][5] (records, counted, sum, nonzero_bins, max_value), cluster_sums
 * [bins][clusters]. SECEDO_E_STATE without a result. */
int secedo_bam_depth_fetch(uint32_t *bin_chr, uint32_t *bin_start, uint32_t *bin_end, uint32_t *pair_bin,
                           uint32_t *pair_cell, uint64_t *pair_value, uint64_t *cell_table, uint64_t *cluster_sums);
/* the last secedo_bam_depth call of this thread, a failed one up to its failure */
int secedo_bam_depth_stats(secedo_bam_depth_info *out);
/* The requested chromosomes of the last depth result of this thread, in ascending id (the order of the bins): their
 * @SQ names one after the other in names[capacity] with name_off[chromosomes + 1] their bounds, and lengths
 * [chromosomes] their LN. Any may be NULL. *name_bytes (may be NULL) = the bytes the names take; names with a capacity
 * below that is SECEDO_E_LIMIT (name_bytes is set, nothing else written). SECEDO_E_STATE without a result. */
int secedo_bam_depth_chromosomes(char *names, uint64_t capacity, uint64_t *name_off, uint32_t *lengths,
                                 uint64_t *name_bytes);

/* Host only. records_per_ref[r] (r < min(capacity, n_ref)) = records with RefID r; may be NULL.
 * num_threads: inflate pool size, capped at 16 (0 = 1). */
int secedo_bam_scan(const char *path, uint32_t num_threads, secedo_bam_scan_info *info, uint64_t *records_per_ref,
                    uint32_t capacity);

/* The reference's pileup_bams() for one chromosome. out_pileup: path prefix of <out>.bin, <out>.map and
 * <out>.txt (the .txt is created empty unless write_text_file, like the reference), or NULL to write nothing.
 * The result stays on the device until the next call on this thread; get it with secedo_bam_fetch.
 * times may be NULL. Synchronous. */
int secedo_pileup_bams(const char *const *bam_files, uint32_t n_files, const char *out_pileup, int write_text_file,
                       uint32_t chromosome_id, uint32_t max_coverage, uint32_t min_base_quality,
                       uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                       uint16_t min_different, secedo_bam_result_info *info, secedo_bam_times *times);

/* Several chromosomes in one pass over the files (each file is inflated once); chromosome c of the result is
 * chromosome_ids[c], its read ids numbered from 0 as in its own pileup_bams() call. id_to_group (host, may be
 * NULL for the identity) maps cell ids to groups as secedo_pileup_read does: id_base16 = group << 2 | base, a
 * cell >= n_ids is SECEDO_E_INVALID_ARG. */
int secedo_pileup_bams_device(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                              uint32_t n_chr, uint32_t max_coverage, uint32_t min_base_quality,
                              uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                              uint16_t min_different, const uint16_t *id_to_group, uint32_t n_ids,
                              secedo_bam_result_info *info, secedo_bam_times *times);

/* Tag mode: bam_files are multiplexed BAMs; the cell of a record is the index in barcodes[0..n_barcodes) of the
 * value of its first aux field named tag (two characters [A-Za-z][A-Za-z0-9]) when that field is Z-typed. Records
 * without it, with another type or an unlisted value take no read id, pass no checks of the device passes and give
 * nothing; the host's structural checks still cover every record of the chromosome. The result equals
 * secedo_pileup_bams / secedo_pileup_bams_device on n_barcodes files C_c holding the records of barcode c in
 * (Position, input file, record) order. Error messages name the input file and its record index. An empty list, a
 * duplicate or a bad tag: SECEDO_E_INVALID_ARG; more than SECEDO_BAM_MAX_FILES barcodes: SECEDO_E_LIMIT. */
int secedo_pileup_bams_cells(const char *const *bam_files, uint32_t n_files, const char *out_pileup,
                             int write_text_file, uint32_t chromosome_id, uint32_t max_coverage,
                             uint32_t min_base_quality, uint32_t min_map_quality, uint32_t min_alignment_score,
                             uint32_t num_threads, uint16_t min_different, const char tag[2],
                             const char *const *barcodes, uint32_t n_barcodes, secedo_bam_result_info *info,
                             secedo_bam_times *times);
int secedo_pileup_bams_cells_device(const char *const *bam_files, uint32_t n_files, const uint32_t *chromosome_ids,
                                    uint32_t n_chr, uint32_t max_coverage, uint32_t min_base_quality,
                                    uint32_t min_map_quality, uint32_t min_alignment_score, uint32_t num_threads,
                                    uint16_t min_different, const uint16_t *id_to_group, uint32_t n_ids,
                                    const char tag[2], const char *const *barcodes, uint32_t n_barcodes,
                                    secedo_bam_result_info *info, secedo_bam_times *times);

/* The distinct Z-typed values of tag (first occurrence per record) over the records of the requested chromosomes,
 * sorted bytewise, with their record counts: *n_barcodes values of *bytes bytes in all. The result stays until the
 * next call on this thread; get it with secedo_bam_barcodes_fetch. Synchronous. */
int secedo_bam_barcodes(const char *const *bam_files, uint32_t n_files, const char tag[2],
                        const uint32_t *chromosome_ids, uint32_t n_chr, uint32_t num_threads, uint32_t *n_barcodes,
                        uint64_t *bytes);
/* Host buffers, any may be NULL: values[bytes] packed without separators, value_off[n_barcodes + 1],
 * counts[n_barcodes]. */
int secedo_bam_barcodes_fetch(char *values, uint64_t *value_off, uint64_t *counts);

/* Copies the last result into host or device buffers (any may be NULL): chr_locus_off[n_chr + 1],
 * locus_pos[n_loci], locus_entry_off[n_loci + 1], read_ids[n_entries], id_base16[n_entries].
 * The flat layout secedo_simmat_set_pileup_device takes. Synchronous. */
int secedo_bam_fetch(uint32_t *chr_locus_off, uint32_t *locus_pos, uint64_t *locus_entry_off, uint32_t *read_ids,
                     uint16_t *id_base16);

/* Frees the device memory of the last result (that of secedo_bgzf_inflate too) and the last secedo_bam_depth result. */
void secedo_bam_release(void);

/* Inflates any BGZF file (BAM, bgzipped SAM, ...) on the GPU, in ranges of about SECEDO_BAM_BATCH_BYTES, ISIZE and
 * CRC32 of every member checked there; *bytes = the inflated size. A bad member is SECEDO_E_INVALID_ARG as above.
 * The bytes stay on the device until the next call on this thread or secedo_bam_release. Synchronous. */
int secedo_bgzf_inflate(const char *path, uint64_t *bytes);
/* Copies them into dst[bytes], host or device memory. Synchronous. */
int secedo_bgzf_inflate_fetch(uint8_t *dst);

#ifdef __cplusplus
}
#endif

#endif /* SECEDO_BAM_H */
