#!/usr/bin/env python3
"""bench_genome_bins.py -- the genome composition per bin (secedo_amd.genome_bins) on one GPU, one JSON line.

The genome is synthetic and seeded: --contigs contigs of --mbases Mbases each at --width columns, uniform A, C, G, T
with runs of lowercase (soft-masked repeats) and runs of N laid over them, written once into --dir as plain text and as
BGZF. ``genome_bins`` runs on each form at 1 kb and 500 kb bins, writing its file; every configuration runs --repeat
times after one untimed run. The line holds per configuration

  stats        genome_bins_stats() of the last run, its stage times as medians: upload_ms (host time inside the
               uploads, which run beside the passes of the range before), parse_ms (the reused scans and the header
               table, device events), count_ms (k_compose, device events), format, deflate, download, write
  call_ms      the whole call, host clock, median and its runs
  compose_gbs  FASTA text bytes / count_ms: what k_compose reads per second (it reads every text byte once, plus 10
               bytes of scan results per 16 bytes of text), to be held against the HBM rate
  parse_gbs    the same for the parse passes over the same text

so that count_ms stands beside parse_ms and upload_ms of the same call. Run it under a time limit (timeout -k 10 ...).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("upload_ms", "parse_ms", "count_ms", "format_ms", "deflate_ms", "download_ms", "write_ms")


def genome_text(contigs, mbases, width, seed):
    rng = np.random.default_rng(seed)
    parts = []
    for c in range(contigs):
        n = int(mbases * 1e6)
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
        for _ in range(max(1, n // 200_000)):  # runs of lowercase of up to 20 kb and of N of up to 50 kb
            a = int(rng.integers(0, n))
            seq[a:a + int(rng.integers(100, 20_000))] |= 0x20
            a = int(rng.integers(0, n))
            seq[a:a + int(rng.integers(10, 50_000))] = ord("N")
        rows = -(-n // width)
        padded = np.full(rows * (width + 1), ord("\n"), np.uint8).reshape(rows, width + 1)
        flat = np.full(rows * width, ord("\n"), np.uint8)
        flat[:n] = seq
        padded[:, :width] = flat.reshape(rows, width)
        body = padded.tobytes()
        if rows * width > n:  # the last line is short: drop its padding, keep its '\n'
            body = body[:len(body) - 1 - (rows * width - n)] + b"\n"
        parts.append(b">chr%d synthetic\n" % (c + 1) + body)
    return b"".join(parts)


def write_genome(d, contigs, mbases, width, seed):
    """The two files under d, written once -> ({form: path}, text bytes, seconds spent writing them now)."""
    from tests import bgzf_writer

    os.makedirs(d, exist_ok=True)
    stamp = os.path.join(d, "genome.json")
    want = dict(contigs=contigs, mbases=mbases, width=width, seed=seed)
    paths = dict(plain=os.path.join(d, "genome.fa"), bgzf=os.path.join(d, "genome.fa.gz"))
    if os.path.exists(stamp) and all(os.path.exists(p) for p in paths.values()):
        have = json.load(open(stamp))
        if {k: have.get(k) for k in want} == want:
            return paths, have["text_bytes"], 0.0
    t0 = time.time()
    text = genome_text(contigs, mbases, width, seed)
    with open(paths["plain"], "wb") as f:
        f.write(text)
    with open(paths["bgzf"], "wb") as f:
        f.write(bgzf_writer.bgzf(text, chunk=0xFF00))
    json.dump(dict(want, text_bytes=len(text)), open(stamp, "w"))
    return paths, len(text), time.time() - t0


def run(path, form, S, out_dir, repeat, output):
    import secedo_amd

    runs, calls = [], []
    for k in range(repeat + 1):
        t0 = time.perf_counter()
        r = secedo_amd.genome_bins(path, S, out_path=os.path.join(out_dir, "genome.gc.tsv"), output=output,
                                   overwrite=True)
        if k:
            calls.append((time.perf_counter() - t0) * 1e3)
            runs.append(r["stats"])
    st = dict(runs[-1])
    for key in STAGES:
        st[key] = round(float(np.median([x[key] for x in runs])), 3)
    gbs = lambda ms: round(st["fasta_bytes"] / (ms * 1e-3) / 1e9, 2) if ms > 0 else None  # noqa: E731
    return dict(form=form, bin_size=S, output=output, stats=st, call_ms=round(float(np.median(calls)), 2),
                call_ms_runs=[round(x, 2) for x in calls], compose_gbs=gbs(st["count_ms"]), parse_gbs=gbs(st["parse_ms"]),
                count_ms_runs=[round(x["count_ms"], 3) for x in runs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/secedo_genome_bins_bench")
    ap.add_argument("--contigs", type=int, default=2)
    ap.add_argument("--mbases", type=float, default=128.0)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--output", choices=("plain", "bgzf"), default="plain")
    a = ap.parse_args()
    paths, text_bytes, gen_s = write_genome(a.dir, a.contigs, a.mbases, a.width, a.seed)
    print("genome ready (%.1f s)" % gen_s, file=sys.stderr, flush=True)
    out = os.path.join(a.dir, "out")
    os.makedirs(out, exist_ok=True)
    line = dict(workload="genome_bins_synthetic_genome", contigs=a.contigs, mbases=a.mbases, width=a.width, seed=a.seed,
                repeat=a.repeat, output=a.output, text_bytes=text_bytes,
                file_bytes={k: os.path.getsize(p) for k, p in paths.items()}, configs=[])
    for form in ("plain", "bgzf"):
        for S in (1000, 500_000):
            line["configs"].append(run(paths[form], form, S, out, a.repeat, a.output))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
