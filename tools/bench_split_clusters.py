#!/usr/bin/env python3
"""bench_split_clusters.py -- per-cluster BAM files from a clustering (secedo_amd.split_clusters) on one GPU, one JSON
line.

The set is tools/bench_pileup_bams.py's (tests/bam_writer.uniform_cell_bam: --cells cells x --pairs read pairs of
2 x 100 bp on a --mbp Mbp chromosome, qualities drawn per base), written once into --dir, and the same set as one
multiplexed BAM tagged CB:Z. Cell c goes to cluster c % --clusters. The line holds, for the per-cell call and for the
tag-mode call, split_stats() of the last of --repeat runs after one untimed run (stage times as medians), and from them

  gather_GBps         bytes read + bytes written by the gather kernel per second of gather_ms, beside HBM_MEASURED
  deflate_GBps        uncompressed bytes per second of deflate_ms (descriptors up, encoder, packer)
  stored_share        members that fell back to a stored block
  ratio               compressed_bytes / text_bytes
  zlib1_ratio, zlib6_ratio   zlib at level 1 and 6 over the same 0xFF00-byte pieces of one cluster file's bytes (at
                      most --zlib-mib MiB of them), payload bytes over input bytes, and ours on those pieces

and whether the two calls wrote the same number of records. --read_groups runs the same two calls with
read_groups=True (every record tagged RG:Z:<its cell>): the line then also holds split_rg_stats(), and the
gather's bytes are what the editing gather reads and writes. total_ms_runs lists the call totals of the timed runs, so
that two lines can be compared against their own run-to-run spread. --require_flags, --exclude_flags and --duplicates
off|mark|remove run the calls with records selected on the way: the line then also holds the select
counts, and with "mark" the gather is the marking instantiation. The uniform set has almost no duplicates, so
--dup_rate R plants them: in every cell R x pairs of its pairs are written a second time under another name, and the
multiplexed file is made from those cells. Run it under a time limit (timeout -k 10 ...)."""
import argparse
import gzip
import json
import os
import shutil
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_MEASURED = 6.29e12
STAGES = ("order_ms", "gather_ms", "deflate_ms", "download_ms", "write_ms")
STEPS = ("inflate_ms", "walk_ms", "upload_ms", "device_ms", "write_ms", "total_ms")


def run(files, clustering, out, repeat, threads, **kw):
    import secedo_amd

    runs, times = [], []
    for k in range(repeat + 1):
        t = {}
        st = secedo_amd.split_clusters(files, clustering, out, [0], overwrite=True, num_threads=threads, times=t, **kw)
        if k:
            runs.append(st)
            times.append(t)
    r = dict(runs[-1])
    for key in STAGES:
        r[key] = round(float(np.median([x[key] for x in runs])), 3)
    r["times"] = {key: round(float(np.median([x[key] for x in times])), 2) for key in STEPS}
    r["total_ms_runs"] = [round(float(x["total_ms"]), 2) for x in times]
    record_bytes = r["text_bytes"]  # the headers' few hundred bytes per file included
    # the editing gather reads what it writes less the appended bytes plus the removed ones
    moved = 2 * record_bytes - r.get("added_bytes", 0) + r.get("removed_bytes", 0)
    r["gather_GBps"] = moved / (r["gather_ms"] * 1e-3) / 1e9 if r["gather_ms"] else None
    r["gather_fraction_of_hbm_measured"] = r["gather_GBps"] * 1e9 / HBM_MEASURED if r["gather_ms"] else None
    r["deflate_GBps"] = r["text_bytes"] / (r["deflate_ms"] * 1e-3) / 1e9
    r["stored_share"] = r["stored_members"] / max(r["members"], 1)
    r["ratio"] = r["compressed_bytes"] / max(r["text_bytes"], 1)
    return r


def plant_duplicates(paths, d, rate, seed=9):
    """The cells of write_set with int(rate * pairs) of each cell's pairs written twice, the copy under a name whose
    first character differs, records in coordinate order -> (paths under d, records added in all)."""
    from tests import bam_writer as bw

    os.makedirs(d, exist_ok=True)
    stamp = os.path.join(d, "dup.json")
    want = dict(rate=rate, seed=seed, cells=len(paths))
    out = [os.path.join(d, os.path.basename(p)) for p in paths]
    if os.path.exists(stamp):
        have = json.load(open(stamp))
        if {k: have.get(k) for k in want} == want:
            return out, have["added"]
    rng = np.random.default_rng(seed)
    added = 0
    for p, q in zip(paths, out):
        raw = gzip.decompress(open(p, "rb").read())
        o = 8 + struct.unpack_from("<i", raw, 4)[0] + 4 + 4 + 2 + 4  # one reference named "1"
        rec = np.frombuffer(raw, dtype=np.uint8, offset=o).reshape(-1, 211)  # uniform_cell_bam's fixed size
        names = [r.tobytes() for r in rec[:, 36:53]]
        by_name = {}
        for k, name in enumerate(names):
            by_name.setdefault(name, []).append(k)
        pairs = [v for v in by_name.values() if len(v) == 2]
        take = rng.choice(len(pairs), int(rate * len(pairs)), replace=False)
        copy = rec[[k for t in take for k in pairs[t]]].copy()
        copy[:, 36] = ord("~")  # no name of the set starts with it
        both = np.concatenate([rec, copy])
        pos = both[:, 8:12].copy().view("<i4").ravel()
        both = both[np.argsort(pos, kind="stable")]
        added += len(copy)
        with open(q, "wb") as f:
            f.write(bw.bgzf(raw[:o] + both.tobytes()))
    json.dump(dict(want, added=added), open(stamp, "w"))
    return out, added


def zlib_beside(path, mib):
    """zlib level 1 and 6 and our members over the first pieces of one written file."""
    from tests import bgzf_deflate_cases as dc

    raw = open(path, "rb").read()
    members = dc.split_members(raw)[:-1]
    data, ours = b"", 0
    for member, payload, _crc, isize in members:
        if len(data) + isize > mib << 20:
            break
        piece = gzip.decompress(member)
        data += piece
        ours += len(payload)
    z1, z6 = dc.zlib_sizes(data)
    n = max(len(data), 1)
    return dict(sample_bytes=len(data), ours_payload_ratio=ours / n, zlib1_ratio=z1 / n, zlib6_ratio=z6 / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/secedo_split_bench")
    ap.add_argument("--cells", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--mbp", type=float, default=10.0)
    ap.add_argument("--clusters", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--zlib-mib", type=int, default=16)
    ap.add_argument("--read_groups", action="store_true", help="tag every record with its cell's read group")
    ap.add_argument("--require_flags", default=None, help="write only records with all of these SAM flags")
    ap.add_argument("--exclude_flags", default=None, help="write no record with any of these SAM flags")
    ap.add_argument("--duplicates", choices=("off", "mark", "remove"), default="off")
    ap.add_argument("--dup_rate", type=float, default=0.0, help="plant this share of every cell's pairs a second time")
    a = ap.parse_args()
    import bench_pileup_bams as bp

    paths, gen_s = bp.write_set(a.dir, a.cells, a.pairs, a.mbp)
    mux_dir, planted = a.dir, 0
    if a.dup_rate > 0:
        mux_dir = os.path.join(a.dir, "dup_%g" % a.dup_rate)
        paths, planted = plant_duplicates(paths, mux_dir, a.dup_rate)
    mpath, barcodes, mux_s = bp.write_multiplexed(mux_dir, paths, dict(cells=a.cells, pairs=a.pairs, mbp=a.mbp,
                                                                       dup_rate=a.dup_rate))
    print("set ready (%.1f s, multiplexed %.1f s)" % (gen_s, mux_s), file=sys.stderr, flush=True)
    clustering = [c % a.clusters for c in range(a.cells)]
    outs = []
    for name in ("per_cell", "multiplexed"):
        d = os.path.join(a.dir, "split_" + name)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        outs.append(d)
    line = dict(workload="split_clusters_uniform", cells=a.cells, pairs=a.pairs, mbp=a.mbp, clusters=a.clusters,
                threads=a.threads, records=a.cells * a.pairs * 2 + planted,
                record_bytes=(a.cells * a.pairs * 2 + planted) * 211,
                bam_bytes=sum(os.path.getsize(p) for p in paths), hbm_measured_GBps=HBM_MEASURED / 1e9,
                read_groups=a.read_groups, require_flags=a.require_flags, exclude_flags=a.exclude_flags,
                duplicates=a.duplicates, dup_rate=a.dup_rate, planted_records=planted)
    kw = dict(read_groups=True) if a.read_groups else {}
    if a.require_flags is not None or a.exclude_flags is not None:
        kw.update(require_flags=a.require_flags, exclude_flags=a.exclude_flags)
    if a.duplicates != "off":
        kw.update(duplicates=a.duplicates)
    line["per_cell"] = run(paths, clustering, outs[0], a.repeat, a.threads, **kw)
    line["multiplexed"] = run([mpath], clustering, outs[1], a.repeat, a.threads, cell_tag="CB", cells=barcodes, **kw)
    # the multiplexed records carry the CB:Z tag, so the two calls' files differ; their record counts must not
    line["records_equal"] = line["per_cell"]["records"] == line["multiplexed"]["records"]
    if "duplicate_records" not in line["per_cell"]:  # nothing selected: every input record is written
        line["records_equal"] = line["records_equal"] and line["per_cell"]["records"] == line["records"]
    line["zlib"] = zlib_beside(os.path.join(outs[0], "cluster_0.bam"), a.zlib_mib)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
