#!/usr/bin/env python3
"""bench_variant_calling.py -- the variant calling (include/secedo_variant.h) on the GPU, one JSON line per
workload:

    C3      the C3 pileup of synth_pileup (8000 cells, 100K loci, 22 chromosomes) with positions renumbered 1, 4,
            7, ... per chromosome so that the FASTA stays small, clusters of a ((A1, A2), B) clone tree
            (labels 2, 3, 4 as divide_cluster numbers them, 1 % of the cells unassigned = 0)
    whole   a whole-pileup-sized synthetic: 24 chromosomes, 10 M loci, coverage 30 (300 M entries), one locus
            every 100 bp (a 1 Gbp diploid FASTA, 60 bases per line), the same clone-tree clusters, 2 % of the
            loci with a planted clone-specific variant
    fasta   the genome and the loci of `whole` without its entries: the reference genotypes alone
            (secedo_variant_reference_genotypes on the host route, ..._device on the device route), with the
            device route's inflate / upload / parse+gather split and GB/s of FASTA text

--fasta_route host|device picks the route of the FASTA parse and gather (default: the library's setting),
--compress none|gzip|bgzf how the synthetic genome is written, --lib PATH another build of libsecedo_variant.so
(an A/B against the parent commit; one without the device entry point runs `fasta` on the host function).
--vcf_output plain|bgzf|both picks the kind of VCF files (default: the library's setting); `both` measures the two on
the same data, one JSON line each, with the bgzf route's format / deflate / download / write split, its compressed
size and the encoder kernel's time. --vcf_index tbi (with the bgzf output) also writes the tabix indexes: the line adds
the index's pass / build / deflate / write split and the time of `tabix_build` on the same .vcf.gz files; `both`
measures the bgzf output without and with the index on the same data.

Each line: the two kernels (device events), the end-to-end call split into FASTA parse / gather / device (uploads,
kernels, downloads) / write, and the achieved bytes/s of the kernels against the HBM peak (8 TB/s spec, 6.3
TB/s measured with a float4 copy). The bytes counted are the compulsory ones: id_base, the entry offsets, one cluster
id and one counter update per entry, the reference genotype and flag per locus. Every workload runs once
untimed first. Run every step under a time limit (timeout -k 10 ...)."""
import argparse
import gzip
import json
import os
import shutil
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from secedo_amd import variant  # noqa: E402
from secedo_amd.pileup import FlatPileup  # noqa: E402

HBM_PEAK = 8.0e12
HBM_MEASURED = 6.29e12


def clone_clusters(n, seed=1):
    rng = np.random.default_rng(seed)
    cl = np.where(np.arange(n) < 0.6 * n, 2, np.where(np.arange(n) < 0.8 * n, 3, 4)).astype(np.uint16)
    cl[rng.random(n) < 0.01] = 0
    return cl


def write_fasta(path, lengths, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for c, n in enumerate(lengths):
            name = str(c + 1) if c < 22 else ("X" if c == 22 else "Y")
            mat = acgt[rng.integers(0, 4, n)]
            pat = mat.copy()
            flip = rng.random(n) < 0.001
            pat[flip] = acgt[rng.integers(0, 4, int(flip.sum()))]
            for tag, seq in (("maternal", mat), ("paternal", pat)):
                f.write((">%s_%s\n" % (name, tag)).encode())
                full = n // 60
                rows = np.concatenate([seq[:full * 60].reshape(full, 60), np.full((full, 1), 10, np.uint8)], axis=1)
                body = np.concatenate([rows.reshape(-1), seq[full * 60:], np.full(1 if n % 60 else 0, 10, np.uint8)])
                f.write(body.tobytes())


def _bgzf_member(piece):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    payload = c.compress(piece) + c.flush()
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(payload) + 25) + payload +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


def compress_file(path, how):
    """The file rewritten in place as plain gzip or as BGZF (64 KiB - 256 members, level 1, 16 threads)."""
    if how == "none":
        return
    with open(path, "rb") as f:
        data = f.read()
    with open(path, "wb") as f:
        if how == "gzip":
            f.write(gzip.compress(data, 1, mtime=0))
            return
        view = memoryview(data)
        with ThreadPoolExecutor(16) as pool:  # zlib releases the interpreter lock
            for m in pool.map(_bgzf_member, (view[o:o + 0xFF00] for o in range(0, len(data), 0xFF00))):
                f.write(m)
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


OPTIONS = dict(fasta_route=None, compress="none", vcf_output=None, vcf_index=None, reps=None)


def compulsory_bytes(p, n_groups, idb_bytes):
    e, l = p.n_entries, p.n_loci
    return e * (idb_bytes + 2 + 4) + (l + 1) * 8 + 2 * l + 2 * n_groups * 4


def run(name, p, clusters, fasta, reps=3):
    reps = OPTIONS["reps"] or reps
    outputs = ["plain", "bgzf"] if OPTIONS["vcf_output"] == "both" else [OPTIONS["vcf_output"]]
    for output in outputs:
        for index in (["none", "tbi"] if OPTIONS["vcf_index"] == "both" and output == "bgzf" else [OPTIONS["vcf_index"]]):
            run_one(name, p, clusters, fasta, reps, output, index)


def run_one(name, p, clusters, fasta, reps, output, index):
    out = tempfile.mkdtemp(prefix="vc_bench_")
    kw = {} if output is None else dict(vcf_output=output)  # a parent build's variant.py has no such keyword
    tbi = index == "tbi" and output == "bgzf"
    if tbi:
        kw["vcf_index"] = "tbi"
    has_vcf = hasattr(variant, "vcf_stats") and hasattr(variant.lib(), "secedo_variant_vcf_stats")
    try:
        route = OPTIONS["fasta_route"]
        variant.variant_calling(p, clusters, fasta, "", 1e-3, 0.01, out, fasta_route=route, **kw)  # warm-up
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            t = variant.variant_calling(p, clusters, fasta, "", 1e-3, 0.01, out, fasta_route=route, **kw)
            t["total_ms"] = (time.perf_counter() - t0) * 1e3
            vs = variant.vcf_stats() if has_vcf else dict(output="plain")
            t.update({"vcf_" + k: float(vs[k]) for k in ("format_ms", "deflate_ms", "download_ms", "write_ms",
                                                         "deflate_kernel_ms") if k in vs})
            fs = (variant.fasta_stats() if hasattr(variant.lib(), "secedo_variant_fasta_stats") else
                  dict(route="host", kind="text", text_bytes=0, inflate_ms=0.0, upload_ms=0.0, parse_gather_ms=0.0))
            t.update(fasta_inflate_ms=fs["inflate_ms"], fasta_upload_ms=fs["upload_ms"],
                     fasta_parse_gather_ms=fs["parse_gather_ms"])
            if tbi:
                ts = variant.tabix_stats()
                t.update({"tbi_" + k: float(ts[k]) for k in ("pass_ms", "build_ms", "deflate_ms", "write_ms")})
            runs.append(t)
        med = {k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0]}
        n_lines = sum(1 for f in os.listdir(out) if f.endswith((".vcf", ".vcf.gz"))
                      for line in (gzip.open if f.endswith(".gz") else open)(os.path.join(out, f), "rb")
                      if line[:1] != b"#")
        vcf = {k: vs[k] for k in ("output", "files", "text_bytes", "compressed_bytes", "blocks", "stored_blocks")
               if k in vs}
        if tbi:  # the index of the same files by the stand-alone route
            vcf["tbi"] = {k: ts[k] for k in ("files", "lines", "data_lines", "names", "bins", "chunks", "windows",
                                             "ranges", "index_bytes", "compressed_bytes")}
            gz = sorted(os.path.join(out, f) for f in os.listdir(out) if f.endswith(".vcf.gz"))
            alone = []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                variant.tabix_build(gz, overwrite=True)
                alone.append((time.perf_counter() - t0) * 1e3)
            med["tabix_build_ms"] = round(float(np.median(alone[1:])), 3)
        med["all_total_ms"] = [round(r["total_ms"], 2) for r in runs]
        recs, _, _, kms = variant.variant_calls(p, clusters, fasta, with_kernel_ms=True)
        modes = {}
        for mode in ("lds", "global"):  # the counted-entry counters: LDS-privatised vs global atomics
            os.environ["SECEDO_VARIANT_COUNTERS"] = mode
            variant.variant_calls(p, clusters, fasta)
            modes[mode] = round(float(np.median([variant.variant_calls(p, clusters, fasta, with_kernel_ms=True)[3]
                                                 for _ in range(reps)])), 3)
        del os.environ["SECEDO_VARIANT_COUNTERS"]
    finally:
        shutil.rmtree(out, ignore_errors=True)
    idb_bytes = 2 if p.n_entries == 0 or int(p.id_base.max()) <= 0xFFFF else 4
    by = compulsory_bytes(p, len(clusters), idb_bytes)
    print(json.dumps(dict(workload=name, cells=len(clusters), loci=p.n_loci, entries=p.n_entries,
                          chromosomes=p.n_chr, fasta_bytes=os.path.getsize(fasta), compress=OPTIONS["compress"],
                          fasta_route=fs["route"], fasta_kind=fs["kind"], fasta_text_bytes=fs["text_bytes"],
                          records=len(recs), vcf=vcf, vcf_index="tbi" if tbi else "none",
                          vcf_lines=n_lines, **med, kernel_ms_calls=round(kms, 3),
                          kernel_ms_lds_counters=modes["lds"], kernel_ms_global_counters=modes["global"], compulsory_bytes=by,
                          achieved_bytes_per_s=by / (med["kernel_ms"] * 1e-3),
                          fraction_of_hbm_peak=by / (med["kernel_ms"] * 1e-3) / HBM_PEAK,
                          fraction_of_hbm_measured=by / (med["kernel_ms"] * 1e-3) / HBM_MEASURED)), flush=True)


def c3(tmp):
    from secedo_amd.synth import synth_config
    p0 = synth_config("C3")
    pos = np.zeros(p0.n_loci, dtype=np.uint32)
    lengths = []
    for c in range(p0.n_chr):
        b, e = int(p0.chr_locus_off[c]), int(p0.chr_locus_off[c + 1])
        pos[b:e] = 1 + 3 * np.arange(e - b, dtype=np.uint32)
        lengths.append(3 * (e - b) + 10)
    p = FlatPileup(p0.chr_locus_off, pos, p0.locus_entry_off, p0.read_ids, p0.id_base)
    fasta = os.path.join(tmp, "c3.fa")
    write_fasta(fasta, lengths, 3)
    n_cells = int(p.id_base.max() >> 2) + 1
    run("C3", p, clone_clusters(max(n_cells, 8000)), fasta)


def whole_genome(tmp, n_loci, n_chr, spacing):
    """The genome of `whole`, written as --compress says -> (path, text bytes, chr_locus_off, locus_pos)."""
    per = n_loci // n_chr
    chr_off = (np.arange(n_chr + 1) * per).astype(np.uint32)
    pos = np.tile(1 + spacing * np.arange(per, dtype=np.uint32), n_chr)
    fasta = os.path.join(tmp, "whole.fa")
    write_fasta(fasta, [spacing * per + 10] * n_chr, 5)
    text_bytes = os.path.getsize(fasta)
    compress_file(fasta, OPTIONS["compress"])
    return fasta, text_bytes, chr_off, pos


def fasta_only(tmp, n_loci=10_000_000, n_chr=24, spacing=100, reps=5):
    """The reference genotypes of `whole`'s loci alone: medians of `reps` calls after one untimed call."""
    fasta, text_bytes, chr_off, pos = whole_genome(tmp, n_loci, n_chr, spacing)
    route = OPTIONS["fasta_route"]
    on_device = hasattr(variant.lib(), "secedo_variant_reference_genotypes_device") and route is not None

    def call():
        t0 = time.perf_counter()
        if on_device:
            with variant._route(route):
                ref, end = variant.reference_genotypes(fasta, chr_off, pos, device=0)
        else:
            ref, end = variant.reference_genotypes(fasta, chr_off, pos)
        ms = (time.perf_counter() - t0) * 1e3
        fs = variant.fasta_stats() if hasattr(variant.lib(), "secedo_variant_fasta_stats") else {}
        return ms, fs, int(ref.astype(np.uint64).sum()), int(end.astype(np.uint64).sum())
    call()
    runs = [call() for _ in range(reps)]
    ms = float(np.median([r[0] for r in runs]))
    fs = runs[-1][1]
    split = {k: round(float(np.median([r[1][k] for r in runs])), 3)
             for k in ("inflate_ms", "upload_ms", "parse_gather_ms") if k in fs}
    print(json.dumps(dict(workload="fasta", loci=len(pos), chromosomes=n_chr, text_bytes=text_bytes,
                          file_bytes=os.path.getsize(fasta), compress=OPTIONS["compress"],
                          entry="device" if on_device else "host function", route=fs.get("route", "host"),
                          kind=fs.get("kind", "text"), ranges=fs.get("ranges", 0), call_ms=round(ms, 3),
                          all_call_ms=[round(r[0], 1) for r in runs], text_gb_per_s=round(text_bytes / ms / 1e6, 3),
                          **split, checksum=[runs[0][2], runs[0][3]])), flush=True)


def whole(tmp, n_loci=10_000_000, n_chr=24, cov=30, n_cells=8000, spacing=100):
    rng = np.random.default_rng(7)
    per = n_loci // n_chr
    n_loci = per * n_chr
    fasta, _, chr_off, pos = whole_genome(tmp, n_loci, n_chr, spacing)
    cl = clone_clusters(n_cells)
    counts = rng.poisson(cov, n_loci).astype(np.uint64)
    off = np.zeros(n_loci + 1, dtype=np.uint64)
    np.cumsum(counts, out=off[1:])
    e = int(off[-1])
    cells = rng.integers(0, n_cells, e, dtype=np.uint32)
    bases = rng.integers(0, 4, n_loci, dtype=np.uint32)  # the locus' base (not the FASTA's: many calls)
    locus_of = np.repeat(np.arange(n_loci, dtype=np.uint32), counts.astype(np.int64))
    b = bases[locus_of]
    planted = rng.random(n_loci) < 0.02
    clone_b = (cl[cells] == 2) & planted[locus_of]
    b = np.where(clone_b, (b + 1) & 3, b)
    err = rng.random(e, dtype=np.float32) < 0.01
    b = np.where(err, rng.integers(0, 4, e, dtype=np.uint32), b)
    idb = (cells << 2) | b.astype(np.uint32)
    del locus_of, b, err, clone_b
    p = FlatPileup(chr_off, pos, off, np.arange(e, dtype=np.uint32), idb)
    run("whole", p, cl, fasta, reps=2)


def main(which):
    tmp = tempfile.mkdtemp(prefix="vc_bench_data_")
    try:
        if "C3" in which:
            c3(tmp)
        if "whole" in which:
            whole(tmp)
        if "fasta" in which:
            fasta_only(tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("workloads", nargs="*", default=["C3", "whole"], help="C3, whole, fasta")
    ap.add_argument("--fasta_route", choices=["host", "device"], default=None)
    ap.add_argument("--compress", choices=["none", "gzip", "bgzf"], default="none")
    ap.add_argument("--vcf_output", choices=["plain", "bgzf", "both"], default=None)
    ap.add_argument("--vcf_index", choices=["none", "tbi", "both"], default=None)
    ap.add_argument("--reps", type=int, default=None, help="timed calls per workload (default: C3 3, whole 2)")
    ap.add_argument("--lib", default=None, help="another libsecedo_variant.so to load (A/B against a parent build)")
    args = ap.parse_args()
    OPTIONS.update(fasta_route=args.fasta_route, compress=args.compress, vcf_output=args.vcf_output,
                   vcf_index=args.vcf_index, reps=args.reps)
    if args.lib:
        variant.LIB_PATH = os.path.abspath(args.lib)
        import torch  # noqa: F401  -- one HIP runtime per process: torch's, loaded first, as variant.lib() does
        other = __import__("ctypes").CDLL(variant.LIB_PATH)
        for name in [n for n in variant.SIGNATURES if not hasattr(other, n)]:
            del variant.SIGNATURES[name]  # a build from before the FASTA device route or the bgzf output
    main(args.workloads)
