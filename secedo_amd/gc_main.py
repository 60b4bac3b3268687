"""``python -m secedo_amd.gc_main``: the composition of a reference genome in fixed bins, counted on the GPU.

What a copy-number tool needs beside the depth matrix of ``depth_main``: per bin the counts of A, C, G, T, of every
other byte (N, IUPAC codes) and of soft-masked (lowercase) bases, for GC correction and for dropping bins that are
mostly N or repeat (HMMcopy's gcCounter). ``<o>/genome.gc.tsv`` gets a header line and one line per bin
``chrom start end a c g t other masked``, tab-separated, 0-based half-open; the layout is fixed, see
include/secedo_variant.h (``secedo_amd.genome_bins``).

-r is a FASTA file, plain, gzip or bgzip-compressed. Every header line starts a contig, named by the header up to its
first space. --contigs lists the contigs to count, in the order of the output, by their exact names (``1`` is not
``chr1``); without it all contigs are counted in file order. --bin_size is the bin width; use ``depth_main``'s to get
its bins. --output bgzf writes genome.gc.tsv.gz, bgzip-compressed. An existing output is refused unless --overwrite.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

FILE = "genome.gc.tsv"


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m secedo_amd.gc_main", description=__doc__.splitlines()[0])
    ap.add_argument("-r", required=True, help="Reference genome: FASTA, plain, gzip or bgzip-compressed")
    ap.add_argument("-o", default="./", help="Output directory: <o>/genome.gc.tsv")
    ap.add_argument("--bin_size", type=int, default=500000, help="Bin width in reference positions")
    ap.add_argument("--contigs", default=None, help="Comma-separated contig names, in output order (default: all)")
    ap.add_argument("--output", default="plain", help="plain or bgzf (.tsv.gz)")
    ap.add_argument("--overwrite", action="store_true", help="Replace an existing genome.gc.tsv")
    return ap.parse_args(argv)


def output_path(out_dir: str, output: str) -> str:
    """The file a run writes."""
    return os.path.join(out_dir, FILE + (".gz" if output == "bgzf" else ""))


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    # everything below is checked before the genome is read and before torch is imported
    if a.bin_size < 1 or a.bin_size > 0xFFFFFFFF:
        raise SystemExit("Invalid --bin_size %d: at least 1, at most 4294967295" % a.bin_size)
    if a.output not in ("plain", "bgzf"):
        raise SystemExit("Invalid --output %r: plain or bgzf" % a.output)
    contigs = None
    if a.contigs is not None:
        contigs = a.contigs.split(",")
        if len(set(contigs)) != len(contigs):
            raise SystemExit("Invalid --contigs %r: a name is listed twice" % a.contigs)
    if not os.path.isfile(a.r):
        raise SystemExit("-r %s does not exist" % a.r)
    if not os.path.isdir(a.o):
        raise SystemExit("-o %s is not a directory" % a.o)
    target = output_path(a.o, a.output)
    if os.path.exists(target) and not a.overwrite:
        raise SystemExit("%s exists; pass --overwrite to replace it" % target)
    from .variant import genome_bins

    out = genome_bins(a.r, a.bin_size, contigs=contigs, out_path=os.path.join(a.o, FILE), output=a.output,
                      overwrite=a.overwrite)
    st, total = out["stats"], out["counts"].sum(axis=0, dtype="uint64")
    acgt = int(total[:4].sum())
    print("Counted %d bases of %d of %d contigs into %d bins of %d bp, written to %s"
          % (st["bases"], st["selected"], st["contigs"], st["bins"], a.bin_size, target))
    print("GC %.4f of %d A, C, G, T; %d other; %d soft-masked; %d contigs with a name seen before were left out"
          % ((int(total[1]) + int(total[2])) / acgt if acgt else 0.0, acgt, total[4], total[5], st["duplicate_names"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
