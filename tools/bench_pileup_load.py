"""Host reader + upload against the GPU loader of binary pileup files, on the C3 workload.

Writes synth_config("C3") as one .bin file per chromosome (the test writer, cell ids as in the synthetic
pileup), then times, after a warm-up, read_pileup per file + one SimilarityMatrixPlan.upload against
read_pileups_resident, with --compute_read_stats off and on. Checks that the resident pileups are equal and prints
one JSON line with the times (median of --reps) and the loader's read / walk / upload / device split.

    python tools/bench_pileup_load.py [--reps 5] [--dir DIR]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import secedo_amd  # noqa: E402
from secedo_amd.pileup import FlatPileup  # noqa: E402
from secedo_amd.synth import synth_config  # noqa: E402
from tests.pileup_file_writer import write_bin  # noqa: E402


def write_files(directory):
    p = synth_config("C3")
    files = []
    for c in range(p.n_chr):
        a, b = int(p.chr_locus_off[c]), int(p.chr_locus_off[c + 1])
        off = np.asarray(p.locus_entry_off[a:b + 1], dtype=np.uint64)
        e0, e1 = int(off[0]), int(off[-1])
        part = FlatPileup(np.asarray([0, b - a], dtype=np.uint32), p.locus_pos[a:b], off - off[0],
                          p.read_ids[e0:e1], p.id_base[e0:e1])
        path = os.path.join(directory, "c3_%s.pileup.bin" % (c + 1 if c < 22 else "X"))
        write_bin(path, part)
        files.append(path)
    return files, p


def host_load(plan, files, stats):
    i2g = secedo_amd.get_grouping()
    parts, nc, ml = [], 0, 0
    for f in files:
        p, n, m = secedo_amd.read_pileup(f, i2g, None, 100, None, stats)
        parts.append(p)
        nc, ml = max(nc, n), max(ml, m)
    chr_off = np.concatenate([[0], np.cumsum([p.n_loci for p in parts])]).astype(np.uint32)
    base = np.concatenate([[0], np.cumsum([p.n_entries for p in parts])]).astype(np.uint64)
    off = np.concatenate([np.zeros(1, np.uint64)] + [np.asarray(p.locus_entry_off[1:], np.uint64) + b
                                                     for p, b in zip(parts, base)])
    flat = FlatPileup(chr_off, np.concatenate([p.locus_pos for p in parts]), off,
                      np.concatenate([p.read_ids for p in parts]), np.concatenate([p.id_base for p in parts]))
    res = plan.upload(flat, None, 8000)
    return res, nc, ml


def gpu_load(plan, files, stats, times=None):
    return secedo_amd.read_pileups_resident(plan, files, list(range(len(files))), len(files),
                                            secedo_amd.get_grouping(), 100, None, stats, times=times)


def timed(fn, torch, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, statistics.median(ts)


def same(a, b):
    keys = ("chr", "pos", "off", "rid", "idb")
    return all(torch_equal(a[k], b[k]) for k in keys) and a["n_loci"] == b["n_loci"] and \
        a["n_entries"] == b["n_entries"]


def torch_equal(x, y):
    return x.shape == y.shape and bool((x == y).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    import torch
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        files, p = write_files(d)
        size = sum(os.path.getsize(f) for f in files)
        out = dict(workload="C3", files=len(files), bytes=size, loci=p.n_loci, entries=p.n_entries, reps=a.reps)
        with secedo_amd.SimilarityMatrixPlan(0) as plan:
            for stats in (False, True):
                tag = "stats_on" if stats else "stats_off"
                host_load(plan, files, stats)  # warm-up
                gpu_load(plan, files, stats)
                (h_res, h_nc, h_ml), h_ms = timed(lambda: host_load(plan, files, stats), torch, a.reps)
                split = {}
                (g_res, g_nc, g_ml), g_ms = timed(lambda: gpu_load(plan, files, stats, split), torch, a.reps)
                assert same(h_res, g_res) and (h_nc, h_ml) == (g_nc, g_ml), tag
                out[tag] = dict(host_read_upload_ms=round(h_ms, 2), gpu_loader_ms=round(g_ms, 2),
                                speedup=round(h_ms / g_ms, 2), gpu_split_ms={k: round(v, 2) for k, v in split.items()},
                                max_read_length=g_ml)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
