"""``python -m secedo_amd.tabix_main``: .tbi indexes for bgzip-compressed VCF files, built on the GPU.

-i names a .vcf.gz file, or a directory searched recursively for *.vcf.gz. All files go through one call of
``secedo_amd.tabix_build``: their BGZF members are inflated and their lines walked on the GPU, many small files to a
batch, and each gets <file>.tbi (the tabix index ``tabix -p vcf`` writes, up to htslib's merging of small bins). An
index file that exists is an error unless --overwrite. A file that cannot be indexed ends the run with its error; the
files in front of it keep their indexes. Prints one line per file. The files ``secedo_main --vcf_output bgzf`` wrote
without ``--vcf_index tbi`` get their indexes this way.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m secedo_amd.tabix_main", description=__doc__.splitlines()[0])
    ap.add_argument("-i", required=True, help="A .vcf.gz file, or a directory whose *.vcf.gz files are indexed")
    ap.add_argument("--overwrite", action="store_true", help="Replace index files that exist")
    return ap.parse_args(argv)


def input_files(path: str) -> List[str]:
    if not os.path.isdir(path):
        return [path]
    found = []
    for root, _dirs, names in os.walk(path):
        found.extend(os.path.join(root, n) for n in names if n.endswith(".vcf.gz"))
    return sorted(found)


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    if not os.path.exists(a.i):
        raise SystemExit("Input %s does not exist" % a.i)
    files = input_files(a.i)
    if not files:
        print("No .vcf.gz files found in %s. Done." % a.i)
        return 0
    if not a.overwrite:
        have = [f for f in files if os.path.exists(f + ".tbi")]
        if have:
            raise SystemExit("%s.tbi exists (%d of %d files have an index); pass --overwrite to replace"
                             % (have[0], len(have), len(files)))
    from . import _lib
    from .variant import tabix_build

    try:
        info = tabix_build(files, overwrite=a.overwrite)
    except _lib.SecedoError as e:
        sys.stderr.write("%s\n" % e)
        return 1
    for f in files:
        print("%s\t%s.tbi\t%d bytes" % (f, f, os.path.getsize(f + ".tbi")))
    print("Indexed %d files: %d data lines, %d names, %d bins, %d chunks" % (
        info["files"], info["data_lines"], info["names"], info["bins"], info["chunks"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
