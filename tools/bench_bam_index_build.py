#!/usr/bin/env python3
"""bench_bam_index_build.py -- building .bai indexes on one GPU (secedo_amd.bam_index_build), one JSON line.

The set is tools/bench_pileup_bams.py's (write_set: --cells cell files of --pairs read pairs each, and with
--multiplexed the same records as one BAM). Timed in one session, medians of --repeat runs after one untimed run:
  index_ms        bam_index_build over all cell files in one call (indexes written to <dir>/bai, replaced every run)
  scan_ms         secedo_bam_scan_device over the same files, one call per file: the same inflate and walk with no
                  index work, but a batch per file, since the scan takes one path
  big_index_ms    bam_index_build on the multiplexed BAM alone
  big_scan_ms     secedo_bam_scan_device on it: the same ranges, batch for batch, so the difference is what the index
                  pass, its read-back, the host builder and the file write add
Kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_bam_index_build.py --dir D \
        --repeat 1 --index-only
    python tools/bench_bam_index_build.py --merge LINE.json OUT   # adds ms per kernel group
Run every step under a time limit (timeout -k 10 ...)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(f, repeat):
    out = []
    for k in range(repeat + 1):
        t0 = time.perf_counter()
        f()
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 2)


def merge(line_path, prof_dir):
    line = json.loads(open(line_path).read().strip().splitlines()[-1])
    f = sorted(glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)[-1]
    groups = {}
    for r in csv.DictReader(open(f)):
        name = r["Name"]
        short = name.replace("secedo::bam::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        group = ("index" if "k_index_" in name else "inflate" if "bgzf" in name else
                 "walk" if "secedo::bam" in name else "scans" if "rocprim" in name else None)
        if group is None:
            continue
        g = groups.setdefault(group, dict(ms=0.0, kernels={}))
        ms = float(r["TotalDurationNs"]) / 1e6
        g["ms"] = round(g["ms"] + ms, 3)
        if group != "scans":
            g["kernels"][short] = dict(calls=int(r["Calls"]), ms=round(ms, 3))
    line["kernel_groups"] = groups
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/secedo_bam_bench")
    ap.add_argument("--cells", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--mbp", type=float, default=10.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--multiplexed", action="store_true", help="Also the set as one BAM, indexed and scanned alone")
    ap.add_argument("--index-only", action="store_true", help="Only the index calls (for a rocprofv3 run of its own)")
    ap.add_argument("--merge", nargs=2, metavar=("LINE", "PROF_DIR"))
    a = ap.parse_args()
    if a.merge:
        merge(*a.merge)
        return
    import bench_pileup_bams as bp

    paths, gen_s = bp.write_set(a.dir, a.cells, a.pairs, a.mbp)
    big = None
    if a.multiplexed:
        big, _barcodes, _s = bp.write_multiplexed(a.dir, paths, dict(cells=a.cells, pairs=a.pairs, mbp=a.mbp))
    print("set ready (%.1f s)" % gen_s, file=sys.stderr, flush=True)
    import secedo_amd
    from secedo_amd import bam_pileup

    bai = os.path.join(a.dir, "bai")
    os.makedirs(bai, exist_ok=True)
    outs = [os.path.join(bai, os.path.basename(p) + ".bai") for p in paths]
    info = {}
    line = dict(workload="uniform_index", cells=a.cells, pairs=a.pairs, mbp=a.mbp, threads=a.threads, repeat=a.repeat,
                bam_bytes=sum(os.path.getsize(p) for p in paths))
    line["index_ms"] = timed(lambda: info.update(secedo_amd.bam_index_build(paths, outs, True, a.threads)), a.repeat)
    line["index_info"] = dict(info)
    line["index_route_stats"] = bam_pileup.bam_route_stats()
    if not a.index_only:
        line["scan_ms"] = timed(lambda: [bam_pileup.bam_scan(p, a.threads, device=True) for p in paths], a.repeat)
    if big:
        out = os.path.join(bai, "multiplexed.bam.bai")
        line["big_bam_bytes"] = os.path.getsize(big)
        line["big_index_ms"] = timed(lambda: info.update(secedo_amd.bam_index_build([big], [out], True, a.threads)),
                                     a.repeat)
        line["big_index_info"] = dict(info)
        line["big_route_stats"] = bam_pileup.bam_route_stats()
        if not a.index_only:
            line["big_scan_ms"] = timed(lambda: bam_pileup.bam_scan(big, a.threads, device=True), a.repeat)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
