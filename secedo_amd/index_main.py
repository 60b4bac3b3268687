"""``python -m secedo_amd.index_main``: .bai indexes for BAM files, built on the GPU.

-i names a coordinate-sorted BAM file, or a directory searched recursively for *.bam. All files go through one call of
``secedo_amd.bam_index_build``: their BGZF members are inflated and their records walked on the GPU, many small files to
a batch, and each gets <bam>.bai (SAM spec 5.2, what ``samtools index`` writes up to htslib's bin compression). An
index file that exists is an error unless --overwrite. A file that cannot be indexed ends the run with its error; the
files in front of it keep their indexes. Prints one line per file. ``pileup_main --index auto|require`` reads what this
writes.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

MAX_POOL = 16


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m secedo_amd.index_main", description=__doc__.splitlines()[0])
    ap.add_argument("-i", required=True, help="A BAM file, or a directory whose *.bam files are indexed")
    ap.add_argument("--overwrite", action="store_true", help="Replace index files that exist")
    ap.add_argument("--num_threads", type=int, default=8, help="Host staging threads (at most 16 are used)")
    return ap.parse_args(argv)


def input_files(path: str) -> List[str]:
    if not os.path.isdir(path):
        return [path]
    found = []
    for root, _dirs, names in os.walk(path):
        found.extend(os.path.join(root, n) for n in names if n.endswith(".bam"))
    return sorted(found)


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    if not os.path.exists(a.i):
        raise SystemExit("Input %s does not exist" % a.i)
    if a.num_threads < 1:
        raise SystemExit("--num_threads must be at least 1")
    files = input_files(a.i)
    if not files:
        print("No BAM files found in %s. Done." % a.i)
        return 0
    if not a.overwrite:
        have = [f for f in files if os.path.exists(f + ".bai")]
        if have:
            raise SystemExit("%s.bai exists (%d of %d files have an index); pass --overwrite to replace"
                             % (have[0], len(have), len(files)))
    from . import _lib
    from .bam_pileup import bam_index_build

    try:
        info = bam_index_build(files, overwrite=a.overwrite, num_threads=min(a.num_threads, MAX_POOL))
    except _lib.SecedoError as e:
        sys.stderr.write("%s\n" % e)
        return 1
    for f in files:
        print("%s\t%s.bai\t%d bytes" % (f, f, os.path.getsize(f + ".bai")))
    print("Indexed %d files: %d records, %d bins, %d chunks" % (info["files"], info["records"], info["bins"],
                                                               info["chunks"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
