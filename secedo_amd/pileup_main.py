"""``python -m secedo_amd.pileup_main``: the reference's ``pileup`` executable (pileup_main.cpp) on the GPU path.

Flags as in the reference: -i (a BAM file or a directory searched recursively for *.bam), -o (file prefix),
--chromosomes, --min_base_quality, --min_map_quality, --min_map_score, --max_coverage, --min_different,
--num_threads (here only the size of the host inflate pool, capped at 16). Writes
<o>_<chromosome>.pileup.{bin,map,txt} per chromosome and, for a directory input, the cell map
<o>_<chromosomes>.map. The default chromosome list is the real one (1..22, X, Y).
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
    ap.add_argument("-i", required=True, help="Input BAM file, or a directory containing BAM files")
    ap.add_argument("-o", default="./", help="File prefix of the output: <o>_<chromosome>.pileup.bin etc.")
    ap.add_argument("--num_threads", type=int, default=8, help="Host inflate threads (at most 16 are used)")
    ap.add_argument("--chromosomes", default=DEFAULT_CHROMOSOMES, help="Comma-separated chromosomes (1..22, X, Y)")
    ap.add_argument("--log_level", default="info", help="Accepted for compatibility")
    ap.add_argument("--min_base_quality", type=int, default=30)
    ap.add_argument("--min_map_quality", type=int, default=30)
    ap.add_argument("--min_map_score", type=int, default=0)
    ap.add_argument("--max_coverage", type=int, default=100)
    ap.add_argument("--min_different", type=int, default=3)
    return ap.parse_args(argv)


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


def input_files(path: str) -> List[str]:
    if not os.path.isdir(path):
        return [path]
    found = []
    for root, _dirs, names in os.walk(path):
        found.extend(os.path.join(root, n) for n in names if os.path.splitext(n)[1] == ".bam")
    return sorted(found)


def cell_map_lines(files: List[str]) -> List[str]:
    """The cell map: file name without extension, cut at its last '_', then the cell index."""
    out = []
    for i, f in enumerate(files):
        stem = os.path.splitext(os.path.basename(f))[0]
        cut = stem.rfind("_")
        out.append("%s\t%d\n" % (stem[:cut] if cut >= 0 else stem, i))
    return out


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    files = input_files(a.i)
    if os.path.isdir(a.i):
        if not files:
            print("No BAM files found in %s. Done." % a.i)
            return 0
        with open(a.o + "_" + a.chromosomes + ".map", "w") as f:
            f.writelines(cell_map_lines(files))
    if os.path.isdir(a.o):
        raise SystemExit("-o <output_dir> must be a file prefix, not a directory")
    chromosomes = a.chromosomes.split(",")
    ids = [chromosome_to_id(c) for c in chromosomes]
    from .bam_pileup import pileup_bams

    for chromosome, cid in zip(chromosomes, ids):
        out = a.o + "_" + chromosome + ".pileup"
        p = pileup_bams(files, out, True, cid, a.max_coverage, a.min_base_quality, a.min_map_quality,
                        a.min_map_score, pool_size(a.num_threads), a.min_different)
        print("Written %d positions to %s.txt/.bin" % (p.n_loci, out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
