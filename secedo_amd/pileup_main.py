"""``python -m secedo_amd.pileup_main``: the reference's ``pileup`` executable (pileup_main.cpp) on the GPU path.

Flags as in the reference: -i (a BAM, SAM or bgzipped SAM file, or a directory searched recursively for *.bam, or for
*.sam when it holds no BAM, or for *.sam.gz when it holds neither), -o (file prefix),
--chromosomes, --min_base_quality, --min_map_quality, --min_map_score, --max_coverage, --min_different,
--num_threads (here only the size of the host inflate pool, capped at 16). Writes
<o>_<chromosome>.pileup.{bin,map,txt} per chromosome and, for a directory input, the cell map
<o>_<chromosomes>.map. The default chromosome list is the real one (1..22, X, Y).

Multiplexed BAMs (--cell_tag TG, e.g. CB for 10x data): every BAM under -i holds many cells, the cell of a record
being its Z-typed TG value. --cells FILE lists the barcodes (one per line; empty and '#' lines skipped, so a 10x
barcodes.tsv works); without it the cells are every value with at least --min_cell_records records over the requested
chromosomes, sorted bytewise, so that every <o>_<chromosome>.pileup.bin shares one numbering. The cell map
<o>_<chromosomes>.map then holds barcode<TAB>index, for a file input too.

SAM text input (coordinate-sorted, as aligners write it) goes the same way: its lines are parsed on the GPU into the
BAM records the BAM route reads, so a SAM file gives what the BAM `samtools view -b` writes from it would give.
A .sam.gz written by `bgzip` (BGZF) is inflated on the GPU in front of that parse and gives what its text gives; a
.sam.gz written by plain `gzip` is refused. Files are told apart by content, the names only serve the directory search.

--build_index writes, before the run, <bam>.bai for every input BAM that has no index file where --index looks
(<bam>.bai, <bam without .bam>.bai), all of them in one pass on the GPU (``secedo_amd.bam_index_build``), and never
touches an index file that exists; the run then goes on as --index says.

--require_flags / --exclude_flags select records by SAM flag as samtools' -f / -F do (a decimal or 0x hex mask, or a
comma list of samtools' names: PAIRED, PROPER_PAIR, UNMAP, MUNMAP, REVERSE, MREVERSE, READ1, READ2, SECONDARY, QCFAIL,
DUP, SUPPLEMENTARY), and --remove_duplicates drops, per cell, all but the best template of each set with the same
unclipped 5' ends. Dropped records are not checked: with --require_flags 3 --exclude_flags 0xF04 a BAM straight from
the aligner runs without a samtools pass in front. Without --cells, --min_cell_records counts the records that pass
the flag filter.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

DEFAULT_CHROMOSOMES = ",".join([str(c) for c in range(1, 23)] + ["X", "Y"])
MAX_POOL = 16


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m secedo_amd.pileup_main", description=__doc__.splitlines()[0])
    ap.add_argument("-i", required=True, help="Input BAM, SAM or bgzipped SAM (.sam.gz) file, or a directory containing BAM files (or SAM files "
                                       "when it holds no BAM, or .sam.gz files when it holds neither)")
    ap.add_argument("-o", default="./", help="File prefix of the output: <o>_<chromosome>.pileup.bin etc.")
    ap.add_argument("--num_threads", type=int, default=8, help="Host inflate threads (at most 16 are used)")
    ap.add_argument("--chromosomes", default=DEFAULT_CHROMOSOMES, help="Comma-separated chromosomes (1..22, X, Y)")
    ap.add_argument("--log_level", default="info", help="Accepted for compatibility")
    ap.add_argument("--min_base_quality", type=int, default=30)
    ap.add_argument("--min_map_quality", type=int, default=30)
    ap.add_argument("--min_map_score", type=int, default=0)
    ap.add_argument("--max_coverage", type=int, default=100)
    ap.add_argument("--min_different", type=int, default=3)
    ap.add_argument("--cell_tag", default=None, help="Multiplexed input: the aux tag naming a record's cell (e.g. CB)")
    ap.add_argument("--cells", default=None, help="With --cell_tag: file of barcodes, one per line")
    ap.add_argument("--min_cell_records", type=int, default=None,
                    help="With --cell_tag and without --cells: cells are the values with at least this many records "
                         "(default 1)")
    ap.add_argument("--inflate", choices=("host", "device"), default=None,
                    help="Where BAM files are inflated and their records walked: host (zlib pool) or device (GPU); "
                         "the outputs are the same. Default: the environment variable SECEDO_BAM_INFLATE, else host")
    ap.add_argument("--index", choices=("off", "auto", "require"), default=None,
                    help="Read BAM files through their .bai index (<file>.bai, else <file without .bam>.bai): auto "
                         "reads of an indexed BAM only the members that hold the requested chromosome and any other "
                         "BAM in full, require fails for a BAM without a usable index, off opens no index; the outputs "
                         "are the same. Default: the environment variable SECEDO_BAM_INDEX, else off")
    ap.add_argument("--build_index", action="store_true",
                    help="Before the run, write <bam>.bai on the GPU for every input BAM without an index file; an "
                         "existing index file is never touched. The run then proceeds as --index says")
    ap.add_argument("--require_flags", default=None,
                    help="Use only records with all of these SAM flag bits: decimal, 0x hex or samtools' names "
                         "separated by commas (samtools -f). Default: SECEDO_BAM_REQUIRE_FLAGS, else 0")
    ap.add_argument("--exclude_flags", default=None,
                    help="Skip records with any of these SAM flag bits, e.g. SECONDARY,SUPPLEMENTARY,DUP,QCFAIL,UNMAP or "
                         "0xF04 (samtools -F). Default: SECEDO_BAM_EXCLUDE_FLAGS, else 0")
    ap.add_argument("--remove_duplicates", action="store_true", default=None,
                    help="Per cell, keep only the best template among those with the same unclipped 5' ends and "
                         "strands. Default: SECEDO_BAM_DUPLICATES, else keep")
    return ap.parse_args(argv)


MAX_CELLS = 16384


def valid_tag(tag: str) -> bool:
    return len(tag) == 2 and tag[0].isascii() and tag[0].isalpha() and tag[1].isascii() and tag[1].isalnum()


def read_cells(path: str) -> List[str]:
    """Barcodes of a --cells file: the first tab-separated field of each line; empty lines and lines starting
    with '#' are skipped."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            out.append(line.split("\t")[0])
    return out


def check_tag_flags(a: argparse.Namespace) -> None:
    """The tag-mode flags, checked before any BAM is read (and before torch is imported)."""
    if a.cell_tag is None:
        if a.cells is not None or a.min_cell_records is not None:
            raise SystemExit("--cells and --min_cell_records need --cell_tag")
        return
    if not valid_tag(a.cell_tag):
        raise SystemExit("Invalid --cell_tag %r: two characters [A-Za-z][A-Za-z0-9]" % a.cell_tag)
    if a.cells is not None and a.min_cell_records is not None:
        raise SystemExit("--cells and --min_cell_records exclude each other")
    if a.cells is not None and not os.path.isfile(a.cells):
        raise SystemExit("--cells file %s does not exist" % a.cells)
    if a.min_cell_records is not None and a.min_cell_records < 1:
        raise SystemExit("--min_cell_records must be at least 1")


def check_select_flags(a: argparse.Namespace) -> None:
    """--require_flags / --exclude_flags, checked before any BAM is read (and before torch is imported); they are
    replaced by their masks."""
    from .sam_flags import parse_filter

    if a.require_flags is None and a.exclude_flags is None:
        return
    try:
        a.require_flags, a.exclude_flags = parse_filter(a.require_flags, a.exclude_flags)
    except ValueError as e:
        raise SystemExit("Invalid --require_flags / --exclude_flags: %s" % e)


def check_index_flags(a: argparse.Namespace) -> None:
    """--build_index against --index and the input, checked before any BAM is read (and before torch is imported)."""
    if not a.build_index:
        return
    if a.index == "off":
        raise SystemExit("--build_index with --index off: the indexes would not be read; use --index auto or require")
    if not os.path.exists(a.i):
        raise SystemExit("Input %s does not exist" % a.i)


def is_bam(path: str) -> bool:
    """By content, as the library tells: gzip whose first inflated bytes are the BAM magic."""
    import zlib
    try:
        with open(path, "rb") as f:
            head = f.read(1 << 16)
        return head[:2] == b"\x1f\x8b" and zlib.decompressobj(31).decompress(head, 4) == b"BAM\1"
    except (OSError, zlib.error):
        return False


def build_missing_indexes(files: List[str], num_threads: int) -> List[str]:
    """<bam>.bai for every BAM of ``files`` without an index file at either place the reader looks -> those BAMs."""
    from .bam_pileup import bam_index_build, index_file_of

    todo = [f for f in files if is_bam(f) and index_file_of(f) is None]
    if todo:
        info = bam_index_build(todo, num_threads=num_threads)
        print("Indexed %d of %d input files (%d records, %d index bytes)"
              % (info["files"], len(files), info["records"], info["index_bytes"]))
    return todo


def chromosome_to_id(chromosome: str) -> int:
    """1..22 -> 0..21, X -> 22, Y -> 23 (reference util/util.cpp:143-160)."""
    if chromosome == "X":
        return 22
    if chromosome == "Y":
        return 23
    if chromosome.isdigit() and 1 <= int(chromosome) <= 22:
        return int(chromosome) - 1
    raise SystemExit("Invalid chromosome: %s. Must be 1..22, X, Y" % chromosome)


def pool_size(num_threads: int) -> int:
    return max(1, min(int(num_threads), MAX_POOL))


def _find(path: str, ext: str) -> List[str]:
    found = []
    for root, _dirs, names in os.walk(path):
        found.extend(os.path.join(root, n) for n in names if _split(n)[1] == ext)
    return sorted(found)


def _split(name: str):
    """os.path.splitext, with .sam.gz as one extension."""
    if name.endswith(".sam.gz"):
        return name[:-len(".sam.gz")], ".sam.gz"
    return os.path.splitext(name)


def input_files(path: str) -> List[str]:
    """A file as given; a directory's *.bam files, or its *.sam files when it holds no BAM, or its *.sam.gz files
    when it holds neither."""
    if not os.path.isdir(path):
        return [path]
    return _find(path, ".bam") or _find(path, ".sam") or _find(path, ".sam.gz")


def cell_map_lines(files: List[str]) -> List[str]:
    """The cell map: file name without extension, cut at its last '_', then the cell index."""
    out = []
    for i, f in enumerate(files):
        stem = _split(os.path.basename(f))[0]
        cut = stem.rfind("_")
        out.append("%s\t%d\n" % (stem[:cut] if cut >= 0 else stem, i))
    return out


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    check_tag_flags(a)
    check_index_flags(a)
    check_select_flags(a)
    if a.cell_tag is not None and not os.path.exists(a.i):
        raise SystemExit("Input %s does not exist" % a.i)
    files = input_files(a.i)
    if os.path.isdir(a.i) and not files:
        print("No BAM or SAM files found in %s. Done." % a.i)
        return 0
    if os.path.isdir(a.i) and a.cell_tag is None:
        with open(a.o + "_" + a.chromosomes + ".map", "w") as f:
            f.writelines(cell_map_lines(files))
    if os.path.isdir(a.o):
        raise SystemExit("-o <output_dir> must be a file prefix, not a directory")
    chromosomes = a.chromosomes.split(",")
    ids = [chromosome_to_id(c) for c in chromosomes]
    if a.build_index:
        build_missing_indexes(files, pool_size(a.num_threads))
    cells = None
    if a.cell_tag is not None:
        if a.cells is not None:
            cells = read_cells(a.cells)
            if not cells:
                raise SystemExit("--cells file %s lists no barcode" % a.cells)
        else:
            from .bam_pileup import bam_barcodes

            values, counts = bam_barcodes(files, a.cell_tag, ids, pool_size(a.num_threads), inflate=a.inflate,
                                          index=a.index, require_flags=a.require_flags,
                                          exclude_flags=a.exclude_flags)
            n = 1 if a.min_cell_records is None else a.min_cell_records
            cells = [v for v, c in zip(values, counts) if int(c) >= n]
            if not cells:
                raise SystemExit("No %s:Z value has %d or more records" % (a.cell_tag, n))
        if len(cells) > MAX_CELLS:
            raise SystemExit("%d cells: at most %d are supported; pass --cells or a larger --min_cell_records"
                             % (len(cells), MAX_CELLS))
        with open(a.o + "_" + a.chromosomes + ".map", "w") as f:
            f.writelines("%s\t%d\n" % (c, i) for i, c in enumerate(cells))
    from .bam_pileup import bam_select_stats, pileup_bams

    tag_kw = {} if a.cell_tag is None else dict(cell_tag=a.cell_tag, cells=cells)
    tag_kw["inflate"] = a.inflate
    tag_kw["index"] = a.index
    tag_kw.update(require_flags=a.require_flags, exclude_flags=a.exclude_flags, remove_duplicates=a.remove_duplicates)
    for chromosome, cid in zip(chromosomes, ids):
        out = a.o + "_" + chromosome + ".pileup"
        p = pileup_bams(files, out, True, cid, a.max_coverage, a.min_base_quality, a.min_map_quality,
                        a.min_map_score, pool_size(a.num_threads), a.min_different, **tag_kw)
        print("Written %d positions to %s.txt/.bin" % (p.n_loci, out))
        st = bam_select_stats()
        if any(st.values()) and a.log_level.lower() in ("trace", "debug", "info"):
            print("Chromosome %s: %d records filtered by flag (%d dropped by --require_flags, %d by --exclude_flags); "
                  "%d templates, %d of three or more records, %d duplicate templates (%d records) dropped"
                  % (chromosome, st["records"], st["dropped_require"], st["dropped_exclude"], st["templates"],
                     st["large_templates"], st["duplicate_templates"], st["duplicate_records"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
