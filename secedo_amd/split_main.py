"""``python -m secedo_amd.split_main``: one coordinate-sorted BAM per cluster of a clustering, on the GPU.

After ``secedo_main`` has clustered the cells, this puts each subclone's reads back together as a pseudo-bulk BAM:
``<o>/cluster_<k>.bam`` for every k in 0..max(clustering) holds the records of the cells of cluster k on the requested
chromosomes, merged in coordinate order, byte for byte as they are in the input (``secedo_amd.split_clusters``; the
layout of the files is fixed, see include/secedo_bam.h). A cluster number no cell has gives a header-only file.

-i is the input of ``pileup_main`` (a BAM, SAM or bgzipped SAM file, or a directory searched for them, in the same
sorted order), so cell i here is cell i there. --clustering FILE is the comma-separated file ``secedo_main`` writes:
the cluster of each cell. With --cell_tag TG the inputs are multiplexed BAMs and --cells FILE lists the barcodes, one
per line, cell c being line c; records without a listed barcode are dropped. --chromosomes, --inflate, --index and
--build_index are ``pileup_main``'s. --bai also writes ``cluster_<k>.bam.bai``. Existing outputs are refused unless
--overwrite.

--read_groups names each read's cell in the files: every record gets RG:Z:<name of its cell> in place of the RG field it
had, and the header of cluster k one ``@RG ID:<name> SM:cluster_<k>`` line per cell of the cluster, so a somatic caller
takes the files and ``pileup_main --cell_tag RG`` reads them back cell by cell. --cell_names FILE gives the names, one
per line, cell c being line c; without it a cell is named by its file's base name, or by its barcode.

--require_flags / --exclude_flags (decimal, 0x hex or samtools' names, as for ``pileup_main``) write only the records
whose FLAG has all of the first and none of the second. --duplicates mark|remove decides PCR duplicates per cell, as
``pileup_main --remove_duplicates`` does, while each read's cell is still known: in the merged files two reads with the
same ends may come from two cells, and no tool could tell. ``mark`` sets 0x400 in the FLAG of the duplicates and changes
nothing else, ``remove`` leaves them out.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

from .pileup_main import (DEFAULT_CHROMOSOMES, MAX_CELLS, build_missing_indexes, check_index_flags, check_select_flags,
                          chromosome_to_id, input_files, pool_size, read_cells, valid_tag)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m secedo_amd.split_main", description=__doc__.splitlines()[0])
    ap.add_argument("-i", required=True, help="Input BAM, SAM or bgzipped SAM file, or a directory of them, as for "
                                              "pileup_main")
    ap.add_argument("--clustering", required=True, help="Comma-separated cluster of each cell, as secedo_main writes")
    ap.add_argument("-o", default="./", help="Output directory: <o>/cluster_<k>.bam")
    ap.add_argument("--chromosomes", default=DEFAULT_CHROMOSOMES, help="Comma-separated chromosomes (1..22, X, Y)")
    ap.add_argument("--cell_tag", default=None, help="Multiplexed input: the aux tag naming a record's cell (e.g. CB)")
    ap.add_argument("--cells", default=None, help="With --cell_tag: file of barcodes, one per line; cell c is line c")
    ap.add_argument("--inflate", choices=("host", "device"), default=None,
                    help="Where BAM files are inflated and their records walked; the outputs are the same")
    ap.add_argument("--index", choices=("off", "auto", "require"), default=None,
                    help="Read BAM files through their .bai index; the outputs are the same")
    ap.add_argument("--build_index", action="store_true",
                    help="Before the run, write <bam>.bai on the GPU for every input BAM without an index file")
    ap.add_argument("--bai", action="store_true", help="Also write cluster_<k>.bam.bai for every output")
    ap.add_argument("--read_groups", action="store_true",
                    help="Tag every record with RG:Z:<name of its cell> and write one @RG line per cell")
    ap.add_argument("--cell_names", default=None,
                    help="With --read_groups: file of read-group names, one per line; cell c is line c")
    ap.add_argument("--require_flags", default=None,
                    help="Write only records with all of these SAM flags (decimal, 0x hex or names, e.g. PROPER_PAIR)")
    ap.add_argument("--exclude_flags", default=None,
                    help="Write no record with any of these SAM flags (e.g. SECONDARY,SUPPLEMENTARY,QCFAIL or 0xF00)")
    ap.add_argument("--duplicates", default="off",
                    help="off, mark or remove: duplicates per cell and chromosome, marked with FLAG 0x400 or left out")
    ap.add_argument("--overwrite", action="store_true", help="Replace existing cluster_<k>.bam files")
    ap.add_argument("--num_threads", type=int, default=8, help="Host inflate threads (at most 16 are used)")
    return ap.parse_args(argv)


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    # everything below is checked before any BAM is read and before torch is imported
    if a.duplicates not in ("off", "mark", "remove"):
        raise SystemExit("Invalid --duplicates %r: off, mark or remove" % a.duplicates)
    check_select_flags(a)
    if not os.path.isfile(a.clustering):
        raise SystemExit("--clustering file %s does not exist" % a.clustering)
    cells = None
    if a.cell_tag is None:
        if a.cells is not None:
            raise SystemExit("--cells needs --cell_tag")
    else:
        if not valid_tag(a.cell_tag):
            raise SystemExit("Invalid --cell_tag %r: two characters [A-Za-z][A-Za-z0-9]" % a.cell_tag)
        if a.cells is None:
            raise SystemExit("--cell_tag needs --cells: the clustering numbers the cells by their line in that file")
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
    from .bam_pileup import read_clustering  # imports no torch

    try:
        clustering = read_clustering(a.clustering)
    except ValueError as e:
        raise SystemExit("--clustering file %s" % e)
    n_cells = len(files) if cells is None else len(cells)
    if len(clustering) != n_cells:
        raise SystemExit("--clustering file %s lists %d cells, the input has %d%s"
                         % (a.clustering, len(clustering), n_cells, "" if cells is not None else " (one per file)"))
    names = None
    if a.cell_names is not None:
        if not a.read_groups:
            raise SystemExit("--cell_names needs --read_groups")
        if not os.path.isfile(a.cell_names):
            raise SystemExit("--cell_names file %s does not exist" % a.cell_names)
        with open(a.cell_names) as f:
            names = [line.rstrip("\r\n") for line in f]
        while names and not names[-1]:
            names.pop()
        if len(names) != n_cells:
            raise SystemExit("--cell_names file %s lists %d names, the input has %d cells"
                             % (a.cell_names, len(names), n_cells))
    if not os.path.isdir(a.o):
        raise SystemExit("-o %s is not a directory" % a.o)
    outs = [os.path.join(a.o, "cluster_%d.bam" % k) for k in range(max(clustering) + 1)]
    there = [o for o in outs if os.path.exists(o)]
    if there and not a.overwrite:
        raise SystemExit("%s exists; pass --overwrite to replace it" % there[0])
    ids = [chromosome_to_id(c) for c in a.chromosomes.split(",")]
    if a.build_index:
        build_missing_indexes(files, pool_size(a.num_threads))
    from .bam_pileup import split_clusters

    tag_kw = {} if a.cell_tag is None else dict(cell_tag=a.cell_tag, cells=cells)
    if a.read_groups:
        tag_kw.update(read_groups=True, cell_names=names)
    filtered = a.require_flags is not None
    if filtered:
        tag_kw.update(require_flags=a.require_flags, exclude_flags=a.exclude_flags)
    if a.duplicates != "off":
        tag_kw.update(duplicates=a.duplicates)
    st = split_clusters(files, clustering, a.o, ids, inflate=a.inflate, index=a.index, bai=a.bai,
                        overwrite=a.overwrite, num_threads=pool_size(a.num_threads), **tag_kw)
    print("Written %d records of %d cells to %d files %s (%d bytes, %d BGZF members, %d of them stored)%s"
          % (st["records"], st["cells"], st["clusters"], os.path.join(a.o, "cluster_<k>.bam"), st["compressed_bytes"],
             st["members"], st["stored_members"],
             "; %d records without a listed barcode dropped" % st["dropped_records"] if cells is not None else ""))
    if a.read_groups:
        print("Tagged %d records with their cell's read group (%d had an RG field, replaced; %d did not parse, kept whole)"
              % (st["tagged_records"], st["replaced_records"], st["unparsed_records"]))
    if filtered and "filter_records" in st:
        print("Flag filter: %d of %d records dropped (%d lack a required flag, %d have an excluded one)"
              % (st["dropped_require"] + st["dropped_exclude"], st["filter_records"], st["dropped_require"],
                 st["dropped_exclude"]))
    if a.duplicates != "off":
        print("Duplicates: %d records of %d templates %s (%d templates seen, %d of three or more records left alone)"
              % (st["duplicate_records"], st["duplicate_templates"],
                 "marked with FLAG 0x400" if a.duplicates == "mark" else "removed", st["templates"],
                 st["large_templates"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
