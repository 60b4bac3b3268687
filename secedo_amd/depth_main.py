"""``python -m secedo_amd.depth_main``: per-cell read depth in fixed genomic bins, counted on the GPU.

The bins x cells count matrix that copy-number tools start from (HMMcopy's readCounter, Ginkgo, SCOPE), and with
--clustering the depth profile of each subclone. ``<o>/depth/`` gets depth.bins.bed (the bins, 0-based half-open),
depth.counts.mtx (Matrix Market, 1-based, by bin and then cell), depth.samples.tsv (the cell names), depth.cells.tsv
(per cell: records, counted, sum, nonzero_bins, max_value) and with --clustering depth.clusters.tsv (per bin the sum
over each cluster's cells); the layout of the files is fixed, see include/secedo_bam.h (``secedo_amd.bin_depth``).

-i is the input of ``pileup_main`` (a BAM, SAM or bgzipped SAM file, or a directory searched for them, in the same
sorted order), so cell i here is cell i there. With --cell_tag TG the inputs are multiplexed and --cells FILE lists the
barcodes, one per line, cell c being line c. --chromosomes, --inflate, --index and --build_index are ``pileup_main``'s.
--mode reads adds 1 per record to the bin of its Position; --mode bases adds, per bin a record touches, the reference
positions its M, = and X ops cover there. A record is selected by its barcode, --require_flags / --exclude_flags,
--duplicates remove (per cell and chromosome, as ``pileup_main --remove_duplicates``), --min_map_quality and its
Position lying inside the chromosome, in this order. --clustering FILE is the comma-separated file ``secedo_main``
writes. --cell_names FILE names the cells, one per line; without it a cell is named by its barcode or its file's base
name. --output bgzf writes the .mtx and the two longer .tsv bgzip-compressed (.gz). Existing outputs are refused unless
--overwrite. --reference_genome genome.fa[.gz] adds depth.gc.tsv: per bin the genome's a, c, g, t, other (N and the
rest) and soft-masked counts, for GC correction and bin filtering; the genome must have the BAM header's chromosome
names and lengths (``secedo_amd.genome_bins``, ``python -m secedo_amd.gc_main``).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

from .pileup_main import (DEFAULT_CHROMOSOMES, MAX_CELLS, build_missing_indexes, check_index_flags, check_select_flags,
                          chromosome_to_id, input_files, pool_size, read_cells, valid_tag)

FILES = ("depth.bins.bed", "depth.samples.tsv", "depth.counts.mtx", "depth.cells.tsv", "depth.clusters.tsv")
GC_FILE = "depth.gc.tsv"  # with --reference_genome
COMPRESSED = FILES[2:] + (GC_FILE,)  # .gz under --output bgzf


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m secedo_amd.depth_main", description=__doc__.splitlines()[0])
    ap.add_argument("-i", required=True, help="Input BAM, SAM or bgzipped SAM file, or a directory of them, as for "
                                              "pileup_main")
    ap.add_argument("-o", default="./", help="Output directory: <o>/depth/depth.*")
    ap.add_argument("--bin_size", type=int, default=500000, help="Bin width in reference positions")
    ap.add_argument("--mode", default="reads", help="reads (1 per record, at its Position) or bases (covered positions)")
    ap.add_argument("--min_map_quality", type=int, default=30, help="Count only records with at least this MapQuality")
    ap.add_argument("--chromosomes", default=DEFAULT_CHROMOSOMES, help="Comma-separated chromosomes (1..22, X, Y)")
    ap.add_argument("--cell_tag", default=None, help="Multiplexed input: the aux tag naming a record's cell (e.g. CB)")
    ap.add_argument("--cells", default=None, help="With --cell_tag: file of barcodes, one per line; cell c is line c")
    ap.add_argument("--require_flags", default=None,
                    help="Count only records with all of these SAM flags (decimal, 0x hex or names, e.g. PROPER_PAIR)")
    ap.add_argument("--exclude_flags", default=None,
                    help="Count no record with any of these SAM flags (e.g. SECONDARY,SUPPLEMENTARY,QCFAIL or 0xF00)")
    ap.add_argument("--duplicates", default="off", help="off or remove: duplicates per cell and chromosome are left out")
    ap.add_argument("--clustering", default=None, help="Comma-separated cluster of each cell, as secedo_main writes: "
                                                       "also write depth.clusters.tsv")
    ap.add_argument("--cell_names", default=None, help="File of cell names, one per line; cell c is line c")
    ap.add_argument("--output", default="plain", help="plain or bgzf (.mtx.gz, .tsv.gz)")
    ap.add_argument("--inflate", choices=("host", "device"), default=None,
                    help="Where BAM files are inflated and their records walked; the outputs are the same")
    ap.add_argument("--index", choices=("off", "auto", "require"), default=None,
                    help="Read BAM files through their .bai index; the outputs are the same")
    ap.add_argument("--build_index", action="store_true",
                    help="Before the run, write <bam>.bai on the GPU for every input BAM without an index file")
    ap.add_argument("--reference_genome", default=None,
                    help="FASTA (plain, gzip or bgzip) of the BAMs' reference: also write depth.gc.tsv[.gz], the "
                         "composition of every bin")
    ap.add_argument("--overwrite", action="store_true", help="Replace existing depth.* files")
    ap.add_argument("--num_threads", type=int, default=8, help="Host inflate threads (at most 16 are used)")
    return ap.parse_args(argv)


def output_paths(out_dir: str, output: str, clustered: bool, genome: bool = False) -> List[str]:
    """The files a run writes under <out_dir>/depth/."""
    names = (FILES if clustered else FILES[:-1]) + ((GC_FILE,) if genome else ())
    return [os.path.join(out_dir, "depth", n + (".gz" if output == "bgzf" and n in COMPRESSED else "")) for n in names]


def read_names(path: str) -> List[str]:
    with open(path) as f:
        names = [line.rstrip("\r\n") for line in f]
    while names and not names[-1]:
        names.pop()
    return names


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    # everything below is checked before any BAM is read and before torch is imported
    if a.bin_size < 1 or a.bin_size > 0xFFFFFFFF:
        raise SystemExit("Invalid --bin_size %d: at least 1, at most 4294967295" % a.bin_size)
    if a.mode not in ("reads", "bases"):
        raise SystemExit("Invalid --mode %r: reads or bases" % a.mode)
    if not 0 <= a.min_map_quality <= 255:
        raise SystemExit("Invalid --min_map_quality %d: 0 to 255" % a.min_map_quality)
    if a.duplicates not in ("off", "remove"):
        raise SystemExit("Invalid --duplicates %r: off or remove" % a.duplicates)
    if a.output not in ("plain", "bgzf"):
        raise SystemExit("Invalid --output %r: plain or bgzf" % a.output)
    check_select_flags(a)
    cells = None
    if a.cell_tag is None:
        if a.cells is not None:
            raise SystemExit("--cells needs --cell_tag")
    else:
        if not valid_tag(a.cell_tag):
            raise SystemExit("Invalid --cell_tag %r: two characters [A-Za-z][A-Za-z0-9]" % a.cell_tag)
        if a.cells is None:
            raise SystemExit("--cell_tag needs --cells: the matrix numbers the cells by their line in that file")
        if not os.path.isfile(a.cells):
            raise SystemExit("--cells file %s does not exist" % a.cells)
        cells = read_cells(a.cells)
        if not cells:
            raise SystemExit("--cells file %s lists no barcode" % a.cells)
        if len(cells) > MAX_CELLS:
            raise SystemExit("%d cells: at most %d are supported" % (len(cells), MAX_CELLS))
    check_index_flags(a)
    if not os.path.exists(a.i):
        raise SystemExit("Input %s does not exist" % a.i)
    files = input_files(a.i)
    if not files:
        raise SystemExit("No BAM or SAM files found in %s" % a.i)
    n_cells = len(files) if cells is None else len(cells)
    clustering = None
    if a.clustering is not None:
        if not os.path.isfile(a.clustering):
            raise SystemExit("--clustering file %s does not exist" % a.clustering)
        from .bam_pileup import read_clustering  # imports no torch

        try:
            clustering = read_clustering(a.clustering)
        except ValueError as e:
            raise SystemExit("--clustering file %s" % e)
        if len(clustering) != n_cells:
            raise SystemExit("--clustering file %s lists %d cells, the input has %d%s"
                             % (a.clustering, len(clustering), n_cells, "" if cells is not None else " (one per file)"))
    names = None
    if a.cell_names is not None:
        if not os.path.isfile(a.cell_names):
            raise SystemExit("--cell_names file %s does not exist" % a.cell_names)
        names = read_names(a.cell_names)
        if len(names) != n_cells:
            raise SystemExit("--cell_names file %s lists %d names, the input has %d cells"
                             % (a.cell_names, len(names), n_cells))
        bad = [c for c, n in enumerate(names) if not n or "\t" in n]
        if bad:
            raise SystemExit("--cell_names file %s: the name of cell %d is empty or holds a tab" % (a.cell_names, bad[0]))
    if a.reference_genome is not None and not os.path.isfile(a.reference_genome):
        raise SystemExit("--reference_genome file %s does not exist" % a.reference_genome)
    if not os.path.isdir(a.o):
        raise SystemExit("-o %s is not a directory" % a.o)
    there = [o for o in output_paths(a.o, a.output, clustering is not None, a.reference_genome is not None)
             if os.path.exists(o)]
    if there and not a.overwrite:
        raise SystemExit("%s exists; pass --overwrite to replace it" % there[0])
    ids = [chromosome_to_id(c) for c in a.chromosomes.split(",")]
    if a.build_index:
        build_missing_indexes(files, pool_size(a.num_threads))
    from .bam_pileup import bin_depth

    tag_kw = {} if a.cell_tag is None else dict(cell_tag=a.cell_tag, cells=cells)
    if a.require_flags is not None:
        tag_kw.update(require_flags=a.require_flags, exclude_flags=a.exclude_flags)
    out = bin_depth(files, a.bin_size, ids, out_dir=a.o, mode=a.mode, min_map_quality=a.min_map_quality,
                    duplicates=a.duplicates, clustering=clustering, cell_names=names, output=a.output,
                    overwrite=a.overwrite, inflate=a.inflate, index=a.index, num_threads=pool_size(a.num_threads),
                    reference_genome=a.reference_genome, **tag_kw)
    st = out["stats"]
    print("Counted %d of %d records of %d cells into %d bins of %d bp on %d chromosomes: %d nonzero pairs, written to %s"
          % (st["counted"], st["records"], st["cells"], st["bins"], a.bin_size, st["chromosomes"], st["pairs"],
             os.path.join(a.o, "depth", "depth.*")))
    print("Dropped: %d without a listed barcode, %d lack a required flag, %d have an excluded one, %d duplicates, "
          "%d below MapQuality %d, %d out of range"
          % (st["dropped_barcode"], st["dropped_require"], st["dropped_exclude"], st["dropped_duplicate"],
             st["dropped_mapq"], a.min_map_quality, st["out_of_range"]))
    if "gc" in out:
        gc = out["gc"].sum(axis=0, dtype="uint64")
        print("Genome composition of the bins: %d A, %d C, %d G, %d T, %d other, %d soft-masked, written to %s"
              % (gc[0], gc[1], gc[2], gc[3], gc[4], gc[5], output_paths(a.o, a.output, False, True)[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
