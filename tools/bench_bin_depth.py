#!/usr/bin/env python3
"""bench_bin_depth.py -- per-cell read depth in genomic bins (secedo_amd.bin_depth) on one GPU, one JSON line.

The set is tests/bam_writer.synthetic_set: --cells cell files of --pairs read pairs per reference on 2 references of
--mbp Mbp, reads spread over the whole reference (a third of them with clips, insertions or deletions in their
CIGAR, MapQ drawn from 0..59), written once into --dir. ``bin_depth`` runs on it for `reads` and `bases` at 500 kb
and 1 kb bins, writing its files (--output plain|bgzf) with a clustering of --clusters clusters; every configuration
runs --repeat times after one untimed run. The line holds per configuration

  stats     depth_stats() of the last run, its stage times (order, count, format, deflate, download, write) as medians
  times     the input layer's secedo_bam_times as medians: inflate, walk, upload, device (= the sum of the stages
            above but write), write, total
  device_share   the new device passes (order + count + format + deflate + download) over total_ms
  input_share    inflate + walk + upload over total_ms: what the passes ride on

so that the share of the call the counting takes stands beside the inflate and walk. --min_map_quality defaults to 0
here, so that every record is counted. Run it under a time limit (timeout -k 10 ...)."""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("order_ms", "count_ms", "format_ms", "deflate_ms", "download_ms", "write_ms")
STEPS = ("inflate_ms", "walk_ms", "upload_ms", "device_ms", "write_ms", "total_ms")


def write_set(d, cells, pairs, mbp):
    """The cell files under d, written once -> (paths, seconds spent writing them now)."""
    from tests import bam_writer as bw

    os.makedirs(d, exist_ok=True)
    stamp = os.path.join(d, "set.json")
    want = dict(cells=cells, pairs=pairs, mbp=mbp)
    paths = [os.path.join(d, "cell_%03d.bam" % c) for c in range(cells)]
    if os.path.exists(stamp) and json.load(open(stamp)) == want and all(os.path.exists(p) for p in paths):
        return paths, 0.0
    t0 = time.time()
    ref_len = int(mbp * 1e6)
    got = bw.synthetic_set(d, n_cells=cells, pairs_per_cell=pairs, n_refs=2, ref_len=ref_len, around=ref_len // 2,
                           span=ref_len // 2 - 1000)
    assert got == paths
    json.dump(want, open(stamp, "w"))
    return paths, time.time() - t0


def run(paths, S, mode, out, repeat, threads, **kw):
    import secedo_amd

    runs, times = [], []
    for k in range(repeat + 1):
        t = {}
        r = secedo_amd.bin_depth(paths, S, [0, 1], out_dir=out, mode=mode, overwrite=True, times=t,
                                 num_threads=threads, **kw)
        if k:
            runs.append(r["stats"])
            times.append(t)
    st = dict(runs[-1])
    for key in STAGES:
        st[key] = round(float(np.median([x[key] for x in runs])), 3)
    tm = {key: round(float(np.median([x[key] for x in times])), 3) for key in STEPS}
    device = sum(st[k] for k in STAGES if k != "write_ms")
    return dict(bin_size=S, mode=mode, stats=st, times=tm, total_ms_runs=[round(float(x["total_ms"]), 2) for x in times],
                device_share=round(device / tm["total_ms"], 4),
                input_share=round((tm["inflate_ms"] + tm["walk_ms"] + tm["upload_ms"]) / tm["total_ms"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/secedo_depth_bench")
    ap.add_argument("--cells", type=int, default=48)
    ap.add_argument("--pairs", type=int, default=1500)
    ap.add_argument("--mbp", type=float, default=2.0)
    ap.add_argument("--clusters", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--min_map_quality", type=int, default=0)
    ap.add_argument("--output", choices=("plain", "bgzf"), default="plain")
    ap.add_argument("--inflate", choices=("host", "device"), default=None)
    a = ap.parse_args()
    paths, gen_s = write_set(a.dir, a.cells, a.pairs, a.mbp)
    print("set ready (%.1f s)" % gen_s, file=sys.stderr, flush=True)
    out = os.path.join(a.dir, "out")
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    line = dict(workload="bin_depth_synthetic_set", cells=a.cells, pairs=a.pairs, mbp=a.mbp, clusters=a.clusters,
                threads=a.threads, repeat=a.repeat, min_map_quality=a.min_map_quality, output=a.output,
                inflate=a.inflate, bam_bytes=sum(os.path.getsize(p) for p in paths), configs=[])
    clustering = [c % a.clusters for c in range(a.cells)]
    for mode in ("reads", "bases"):
        for S in (500_000, 1000):
            line["configs"].append(run(paths, S, mode, out, a.repeat, a.threads, min_map_quality=a.min_map_quality,
                                       clustering=clustering, output=a.output, inflate=a.inflate))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
