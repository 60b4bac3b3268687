#!/usr/bin/env python3
"""bench_pileup_bams.py -- the pileup creation from BAM files (include/secedo_bam.h) on one GPU, one JSON line.

The set is written once into --dir with tests/bam_writer.uniform_cell_bam (numpy-built records, 16 worker
processes): --cells cells x --pairs read pairs of 2 x 100 bp on a --mbp Mbp chromosome, a planted variant every
100 bp carried by the odd cells, so that those loci survive min_different = 3. The line holds the step times of
the file-writing call (host inflate with its GB/s of inflated bytes, record walk, upload, device passes, file
writes, end to end) and of the resident call, medians of --repeat runs after one untimed run.

--multiplexed also writes the same set as one tagged BAM (every record gets CB:Z:C<cell>-1, all cells merged in
position order) and adds the tag-mode call (pileup_bams with cell_tag="CB") beside the per-file call: its step
times, and whether its .bin and .map equal the per-file call's. Its device time includes the front passes (cells,
compaction, sort, order); the rocprofv3 merge below lists them as front_ms.

--sam also writes the set as SAM text (one .sam per cell; with --multiplexed also the tagged set as one .sam, lines
in the multiplexed BAM's order) and times the SAM route beside the BAM route in the same process: its step times
(inflate_ms is the text read, walk_ms includes the device parse), and whether its .bin and .map equal the BAM
route's. --sam-only runs just the SAM calls once each, for a rocprofv3 run of its own; --merge-sam LINE.json OUT then
adds the SAM kernels' times and their text GB/s against HBM peak.
--sam-gz (with --sam) also writes every SAM file as BGZF (<name>.sam.gz, zlib level 6, 65280-byte members) and times
that route: upload_ms then covers the compressed bytes and inflate_ms the device inflate (k_bgzf_inflate), whose
inflate_GBps stands beside the BAM route's host zlib pool on the same kind of bytes.
--device-inflate also runs the BAM calls (the per-file one, and with --multiplexed the tag-mode one) with
inflate="device": the BGZF members inflated and the records walked on the GPU. Both routes are timed in the same run;
the line gets the device route's step times, its route stats (bam_route_stats) and whether its files equal the host
route's.
--require-flags / --exclude-flags / --remove-duplicates run the resident call with the record selection on (the flag
filter's front pass, the duplicate removal's); the line then holds bam_select_stats() of the last call, and
resident_device_ms_runs always lists the timed calls one by one, which gives the run-to-run spread.
Kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_pileup_bams.py --dir D \
        --repeat 1 --resident-only
    python tools/bench_pileup_bams.py --merge LINE.json OUT   # adds per-kernel ms and bytes/s vs HBM peak
Run every step under a time limit (timeout -k 10 ...)."""
import argparse
import csv
import glob
import gzip
import json
import os
import struct
import sys
import time
import zlib
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
HBM_MEASURED = 6.29e12


_GENOME = {}


def _one(args):
    from tests import bam_writer as bw
    path, cell, mbp, pairs, seed = args
    if (mbp, seed) not in _GENOME:  # once per worker process
        rng = np.random.default_rng(seed)
        L = int(mbp * 1_000_000)
        genome = rng.integers(0, 4, L).astype(np.int64)
        mask = np.zeros(L, dtype=bool)
        mask[50::100] = True
        _GENOME[(mbp, seed)] = (genome, (genome + 1) % 4, mask)
    genome, alt, mask = _GENOME[(mbp, seed)]
    return bw.uniform_cell_bam(path, cell, genome, alt, mask, pairs, seed=seed)


def write_set(d, cells, pairs, mbp, seed=7):
    os.makedirs(d, exist_ok=True)
    paths = [os.path.join(d, "cell%05d_x.bam" % c) for c in range(cells)]
    stamp = os.path.join(d, "set.json")
    want = dict(cells=cells, pairs=pairs, mbp=mbp, seed=seed)
    if os.path.exists(stamp) and json.load(open(stamp)) == want:
        return paths, 0.0
    t0 = time.time()
    with Pool(16) as pool:
        pool.map(_one, [(p, c, mbp, pairs, seed) for c, p in enumerate(paths)], chunksize=4)
    json.dump(want, open(stamp, "w"))
    return paths, time.time() - t0


TAG_LEN = 3 + 9  # "CBZ" + "C%05d-1" + NUL


def _bgzf_block(chunk):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cdata = c.compress(chunk) + c.flush()
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(cdata) + 25) + cdata +
            struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))


def write_multiplexed(d, paths, seed_stamp):
    """The cells of write_set as one coordinate-sorted BAM, each record tagged CB:Z:C<cell>-1 -> (path, barcodes)."""
    path = os.path.join(d, "multiplexed.bam")
    barcodes = ["C%05d-1" % c for c in range(len(paths))]
    stamp = os.path.join(d, "multiplexed.json")
    if os.path.exists(stamp) and os.path.exists(path) and json.load(open(stamp)) == seed_stamp:
        return path, barcodes, 0.0
    t0 = time.time()
    parts, header = [], None
    for c, p in enumerate(paths):
        raw = gzip.decompress(open(p, "rb").read())
        l_text = struct.unpack_from("<i", raw, 4)[0]
        o = 8 + l_text + 4 + 4 + 2 + 4  # one reference named "1"
        header = raw[:o]
        rec = np.frombuffer(raw, dtype=np.uint8, offset=o).reshape(-1, 211)  # uniform_cell_bam's fixed size
        out = np.empty((rec.shape[0], 211 + TAG_LEN), dtype=np.uint8)
        out[:, :211] = rec
        out[:, :4] = (rec[:, :4].copy().view("<i4") + TAG_LEN).view(np.uint8)
        out[:, 211:] = np.frombuffer(b"CBZ" + barcodes[c].encode() + b"\0", dtype=np.uint8)
        parts.append(out)
    allr = np.concatenate(parts)
    del parts
    pos = allr[:, 8:12].copy().view("<i4").ravel()
    allr = allr[np.argsort(pos, kind="stable")]
    data = header + allr.tobytes()
    del allr
    chunks = [data[i:i + 0xFF00] for i in range(0, len(data), 0xFF00)]
    with Pool(16) as pool:
        blocks = pool.map(_bgzf_block, chunks, chunksize=64)
    with open(path, "wb") as f:
        for b in blocks:
            f.write(b)
        f.write(_bgzf_block(b""))
    json.dump(seed_stamp, open(stamp, "w"))
    return path, barcodes, time.time() - t0


SEQ_LETTERS = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)


def _sam_cell(args):
    """uniform_cell_bam's records (fixed 211-byte layout, a 17-character name stored without its NUL) as SAM lines
    -> (header text, lines, line offsets, positions). A mate position before the chromosome start (no pass reads
    it) becomes PNEXT 0. tag: appended to every line (the multiplexed set's CB:Z field)"""
    path, tag = args
    raw = gzip.decompress(open(path, "rb").read())
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text]
    rec = np.frombuffer(raw, dtype=np.uint8, offset=8 + l_text + 4 + 4 + 2 + 4).reshape(-1, 211)
    n = rec.shape[0]
    pos = rec[:, 8:12].copy().view("<i4").ravel()
    flag = rec[:, 18:20].copy().view("<u2").ravel()
    npos = rec[:, 28:32].copy().view("<i4").ravel()
    seq = np.empty((n, 100), dtype=np.uint8)
    seq[:, 0::2] = SEQ_LETTERS[rec[:, 57:107] >> 4]
    seq[:, 1::2] = SEQ_LETTERS[rec[:, 57:107] & 15]
    qual = rec[:, 107:207] + 33
    score = rec[:, 210]
    suffix = (b"\t" + tag if tag else b"") + b"\n"
    lines = [b"%s\t%d\t1\t%d\t60\t100M\t=\t%d\t0\t%s\t%s\tAS:i:%d%s" % (
        rec[k, 36:53].tobytes(), flag[k], pos[k] + 1, max(npos[k] + 1, 0), seq[k].tobytes(), qual[k].tobytes(), score[k],
        suffix) for k in range(n)]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lines], out=off[1:])
    return text, b"".join(lines), off, pos


def _sam_file(args):
    bam, sam = args
    text, body, _, _ = _sam_cell((bam, None))
    with open(sam, "wb") as f:
        f.write(text + body)


def write_sam_set(d, paths, seed_stamp, multiplexed):
    """The cells of write_set as SAM files under <d>/sam, and with multiplexed the tagged set as one SAM whose lines
    follow the multiplexed BAM's order -> (sam paths, multiplexed sam path or None, seconds)"""
    sd = os.path.join(d, "sam")
    os.makedirs(sd, exist_ok=True)
    sams = [os.path.join(sd, os.path.basename(p)[:-4] + ".sam") for p in paths]
    mpath = os.path.join(d, "multiplexed.sam") if multiplexed else None
    stamp = os.path.join(sd, "set.json")
    want = dict(seed_stamp, multiplexed=multiplexed)
    if os.path.exists(stamp) and json.load(open(stamp)) == want:
        return sams, mpath, 0.0
    t0 = time.time()
    with Pool(16) as pool:
        pool.map(_sam_file, list(zip(paths, sams)), chunksize=4)
        if multiplexed:
            parts = pool.map(_sam_cell, [(p, b"CB:Z:C%05d-1" % c) for c, p in enumerate(paths)], chunksize=4)
            pos = np.concatenate([x[3] for x in parts])
            cell = np.concatenate([np.full(len(x[3]), c, dtype=np.int64) for c, x in enumerate(parts)])
            k = np.concatenate([np.arange(len(x[3])) for x in parts])
            order = np.argsort(pos, kind="stable")  # the multiplexed BAM's record order
            with open(mpath, "wb") as f:
                f.write(parts[0][0])
                for i in order:
                    c, j = cell[i], k[i]
                    f.write(parts[c][1][parts[c][2][j]:parts[c][2][j + 1]])
            del parts
    json.dump(want, open(stamp, "w"))
    return sams, mpath, time.time() - t0


def merge_sam(line_path, prof_dir):
    """The SAM kernels of a --sam-only rocprofv3 run: ms per call and text GB/s against HBM peak"""
    line = json.loads(open(line_path).read().strip().splitlines()[-1])
    f = sorted(glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)[-1]
    kernels = {}
    for r in csv.DictReader(open(f)):
        if "k_sam_" not in r["Name"]:
            continue
        short = r["Name"].replace("secedo::bam::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        kernels[short] = dict(calls=int(r["Calls"]), ms=round(float(r["TotalDurationNs"]) / 1e6, 3))
    total = sum(k["ms"] for k in kernels.values())
    text = line["sam_text_bytes"] + line.get("sam_multiplexed_text_bytes", 0)
    line["sam_kernels"] = kernels
    line["sam_kernel_ms"] = round(total, 3)
    line["sam_text_GBps"] = text / (total * 1e-3) / 1e9
    line["sam_fraction_of_hbm_peak"] = text / (total * 1e-3) / HBM_PEAK
    print(json.dumps(line))


def merge(line_path, prof_dir):
    line = json.loads(open(line_path).read().strip().splitlines()[-1])
    f = sorted(glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)[-1]
    kernels, total = {}, 0.0
    for r in csv.DictReader(open(f)):
        name = r["Name"]
        if "secedo::bam" not in name and "rocprim" not in name:
            continue
        short = name.replace("secedo::bam::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "rocprim" in name:
            short = "rocprim_" + ("radix_sort" if "radix_sort" in name else "scan" if "scan" in name else "other")
        ms = float(r["TotalDurationNs"]) / 1e6
        k = kernels.setdefault(short, dict(calls=0, ms=0.0))
        k["calls"] += int(r["Calls"])
        k["ms"] = round(k["ms"] + ms, 3)
        total += ms
    calls = kernels["k_decode"]["calls"]  # pileup calls in the profiled run (one decode launch each)
    line["kernels"] = kernels
    front = [k for k in ("k_cells", "k_compact_keys", "k_order") if k in kernels]
    if front:  # tag mode's front passes (their radix sort is inside rocprim_radix_sort)
        line["front_ms"] = round(sum(kernels[k]["ms"] for k in front) / calls, 3)
    sel = [k for k in ("k_flag_test", "k_compact_records", "k_ends", "k_tmpl_rep", "k_tmpl_key", "k_group",
                       "k_dup_mark", "k_fill") if k in kernels]
    if sel:  # the record selection's front passes (their two radix sorts are inside rocprim_radix_sort)
        line["select_front_ms"] = round(sum(kernels[k]["ms"] for k in sel) / calls, 3)
    line["profiled_calls"] = calls
    line["kernel_ms_per_call"] = round(total / calls, 3)
    # compulsory bytes of one call: the uploaded records read by decode, count and emit, the counts written and
    # read per window position (16 B each way), the entries written
    by = 3 * line["record_bytes"] + 32 * line["window_positions"] + 6 * line["entries"]
    line["compulsory_bytes"] = by
    line["achieved_bytes_per_s"] = by / (line["kernel_ms_per_call"] * 1e-3)
    line["fraction_of_hbm_peak"] = line["achieved_bytes_per_s"] / HBM_PEAK
    line["fraction_of_hbm_measured"] = line["achieved_bytes_per_s"] / HBM_MEASURED
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/secedo_bam_bench")
    ap.add_argument("--cells", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--mbp", type=float, default=10.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--resident-only", action="store_true")
    ap.add_argument("--multiplexed", action="store_true", help="Also the tag-mode call on the set as one BAM")
    ap.add_argument("--multiplexed-only", action="store_true",
                    help="Only the tag-mode resident call (for a rocprofv3 run of its own)")
    ap.add_argument("--sam", action="store_true", help="Also the SAM route on the set written as SAM")
    ap.add_argument("--sam-gz", action="store_true",
                    help="With --sam: also the set as BGZF-compressed SAM (.sam.gz), inflated on the GPU")
    ap.add_argument("--sam-only", action="store_true", help="Only the SAM calls, once each (for rocprofv3)")
    ap.add_argument("--device-inflate", action="store_true",
                    help="Also the BAM calls with inflate='device' (BGZF inflate and record walk on the GPU), in the "
                         "same run as the host route: step times, route stats, outputs compared")
    ap.add_argument("--refs", type=int, default=0,
                    help="The indexed shape: every cell file holds its records on each of N chromosomes and one is "
                         "requested (with --index)")
    ap.add_argument("--index", action="store_true",
                    help="With --refs N: the set gets .bai files, and index='off' and index='auto' are timed in the same "
                         "run, on the host route and, with --device-inflate, on the device route")
    ap.add_argument("--require-flags", default=None, help="The resident call with require_flags (e.g. 3)")
    ap.add_argument("--exclude-flags", default=None, help="The resident call with exclude_flags (e.g. 0xF04)")
    ap.add_argument("--remove-duplicates", action="store_true", help="The resident call with remove_duplicates")
    ap.add_argument("--merge", nargs=2, metavar=("LINE", "PROF_DIR"))
    ap.add_argument("--merge-sam", nargs=2, metavar=("LINE", "PROF_DIR"))
    a = ap.parse_args()
    if a.merge:
        merge(*a.merge)
        return
    if a.merge_sam:
        merge_sam(*a.merge_sam)
        return
    if a.refs or a.index:
        if not (a.refs and a.index):
            raise SystemExit("--refs N and --index go together")
        index_shape(a)
        return
    paths, gen_s = write_set(a.dir, a.cells, a.pairs, a.mbp)
    import secedo_amd
    from secedo_amd import bam_pileup

    print("set ready (%.1f s)" % gen_s, file=sys.stderr, flush=True)
    if a.multiplexed or a.multiplexed_only:
        mpath, barcodes, mux_s = write_multiplexed(a.dir, paths, dict(cells=a.cells, pairs=a.pairs, mbp=a.mbp))
        print("multiplexed BAM ready (%.1f s)" % mux_s, file=sys.stderr, flush=True)
    if a.sam or a.sam_only:
        sams, msam, sam_s = write_sam_set(a.dir, paths, dict(cells=a.cells, pairs=a.pairs, mbp=a.mbp),
                                          a.multiplexed)
        print("SAM set ready (%.1f s)" % sam_s, file=sys.stderr, flush=True)
    if a.sam_only:
        t = {}
        p = bam_pileup.pileup_bams(sams, None, False, 0, 100, 30, 30, 0, a.threads, 3, times=t)
        line = dict(workload="uniform_sam", cells=a.cells, sam_text_bytes=t["inflated_bytes"], loci=p.n_loci)
        if msam:
            t = {}
            bam_pileup.pileup_bams([msam], None, False, 0, 100, 30, 30, 0, a.threads, 3, times=t, cell_tag="CB",
                                   cells=barcodes)
            line["sam_multiplexed_text_bytes"] = t["inflated_bytes"]
        print(json.dumps(line), flush=True)
        return
    if a.multiplexed_only:
        with secedo_amd.SimilarityMatrixPlan(0) as plan:
            for k in range(a.repeat + 1):
                t = {}
                res, cells, max_len = bam_pileup.pileup_bams_resident(plan, [mpath], [0], 100, 30, 30, 0, a.threads,
                                                                      3, times=t, cell_tag="CB", cells=barcodes)
        print(json.dumps(dict(workload="uniform_multiplexed", cells=a.cells, pairs=a.pairs, records=a.cells * a.pairs * 2,
                              record_bytes=a.cells * a.pairs * 2 * 211, window_positions=int(a.mbp * 1_000_000),
                              entries=res["n_entries"], total_ms=t["total_ms"], device_ms=t["device_ms"])), flush=True)
        return

    med = lambda xs: float(np.median(xs))
    out = os.path.join(a.dir, "out")
    line = dict(workload="uniform", cells=a.cells, pairs=a.pairs, mbp=a.mbp, threads=a.threads,
                set_write_s=round(gen_s, 1), bam_bytes=sum(os.path.getsize(p) for p in paths))
    if not a.resident_only:
        runs = []
        for k in range(a.repeat + 1):
            t = {}
            p = bam_pileup.pileup_bams(paths, out, True, 0, 100, 30, 30, 0, a.threads, 3, times=t)
            if k:
                runs.append(t)
        for key in ("inflate_ms", "walk_ms", "upload_ms", "device_ms", "write_ms", "total_ms"):
            line[key] = round(med([r[key] for r in runs]), 2)
        line["inflated_bytes"] = runs[0]["inflated_bytes"]
        line["inflate_GBps"] = line["inflated_bytes"] / (line["inflate_ms"] * 1e-3) / 1e9
        line.update(loci=p.n_loci, entries=p.n_entries)
        if a.multiplexed:
            mout = os.path.join(a.dir, "mout")
            mr = []
            for k in range(a.repeat + 1):
                t = {}
                bam_pileup.pileup_bams([mpath], mout, True, 0, 100, 30, 30, 0, a.threads, 3, times=t, cell_tag="CB",
                                       cells=barcodes)
                if k:
                    mr.append(t)
            m = dict(set_write_s=round(mux_s, 1), bam_bytes=os.path.getsize(mpath),
                     inflated_bytes=mr[0]["inflated_bytes"])
            for key in ("inflate_ms", "walk_ms", "upload_ms", "device_ms", "write_ms", "total_ms"):
                m[key] = round(med([r[key] for r in mr]), 2)
            m["bin_equal"] = open(mout + ".bin", "rb").read() == open(out + ".bin", "rb").read()
            m["map_equal"] = open(mout + ".map", "rb").read() == open(out + ".map", "rb").read()
            line["multiplexed"] = m
        if a.device_inflate:
            line["device_inflate"] = device_route(a, paths, out, med)
            if a.multiplexed:
                line["multiplexed"]["device_inflate"] = device_route(a, [mpath], mout, med, cell_tag="CB",
                                                                     cells=barcodes)
        if a.sam:
            line["sam"] = sam_route(a, sams, [msam] if msam else None, barcodes if msam else None, out,
                                    mout if msam else None, sam_s, med)
            if a.sam_gz:
                t0 = time.time()
                gzs, mgz = write_sam_gz_set(sams, msam)
                line["sam_gz"] = sam_route(a, gzs, [mgz] if mgz else None, barcodes if mgz else None, out,
                                           mout if mgz else None, time.time() - t0, med, prefix="g")
                line["sam_gz"]["gz_bytes"] = sum(os.path.getsize(p) for p in gzs)
                # the device inflate against the host zlib pool on BGZF bytes (the BAM route's inflate_GBps above)
                r = line["sam_gz"]["per_file"]
                r["inflate_GBps"] = r["text_bytes"] / (r["inflate_ms"] * 1e-3) / 1e9
    select = {}
    if a.require_flags is not None or a.exclude_flags is not None:
        select.update(require_flags=a.require_flags, exclude_flags=a.exclude_flags)
    if a.remove_duplicates:
        select["remove_duplicates"] = True
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        rt = []
        for k in range(a.repeat + 1):
            t = {}
            res, cells, max_len = bam_pileup.pileup_bams_resident(plan, paths, [0], 100, 30, 30, 0, a.threads, 3,
                                                                  times=t, **select)
            if k:
                rt.append(t)
    line["resident_total_ms"] = round(med([r["total_ms"] for r in rt]), 2)
    line["resident_device_ms"] = round(med([r["device_ms"] for r in rt]), 2)
    line["resident_device_ms_runs"] = [round(r["device_ms"], 2) for r in rt]
    if select:
        line["select"] = dict({k: str(v) for k, v in select.items()}, **bam_pileup.bam_select_stats())
    line.update(loci=res["n_loci"], entries=res["n_entries"], num_cells=cells, max_read_length=max_len)
    n_rec = a.cells * a.pairs * 2
    line["records"] = n_rec
    line["record_bytes"] = n_rec * 211  # uniform_cell_bam's fixed record size
    line["window_positions"] = int(a.mbp * 1_000_000)
    if "sam" in line or "device_inflate" in line:
        print_table(line)
    print(json.dumps(line), flush=True)


STEPS = ("inflate_ms", "walk_ms", "upload_ms", "device_ms", "write_ms", "total_ms")


def _refs_cell(args):
    """One cell of write_set copied onto n_refs chromosomes, with a .bai: per chromosome one chunk from its first
    record to behind its last, and the pseudo-bin with the record count."""
    from tests import bai_writer as bi
    from tests import bam_writer as bw
    src, dst, n_refs, mbp = args
    raw = bi.inflate(open(src, "rb").read())
    first = bi.record_spans(raw[:4096 + 8 + struct.unpack_from("<i", raw, 4)[0]])[0][0]
    size = 4 + struct.unpack_from("<i", raw, first)[0]  # uniform_cell_bam's records have one size
    recs = np.frombuffer(raw, dtype=np.uint8, offset=first).reshape(-1, size)
    L = int(mbp * 1_000_000)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%d\tLN:%d\n" % (r + 1, L) for r in range(n_refs))
    head = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", n_refs))
    for r in range(n_refs):
        name = b"%d\0" % (r + 1)
        head += struct.pack("<i", len(name)) + name + struct.pack("<i", L)
    body = []
    for r in range(n_refs):
        c = recs.copy()
        c[:, 4:8] = np.frombuffer(struct.pack("<i", r), dtype=np.uint8)    # RefID
        c[:, 24:28] = np.frombuffer(struct.pack("<i", r), dtype=np.uint8)  # next RefID
        body.append(c.tobytes())
    data = bw.bgzf(bytes(head) + b"".join(body))
    open(dst, "wb").write(data)
    table = bi.member_table(data)
    per = len(recs) * size
    out = bytearray(b"BAI\1" + struct.pack("<i", n_refs))
    for r in range(n_refs):
        beg = bi.voffset(table, len(head) + r * per)
        end = bi.voffset(table, len(head) + (r + 1) * per)
        out += struct.pack("<i", 2) + struct.pack("<IiQQ", 4681, 1, beg, end)
        out += struct.pack("<IiQQQQ", bi.PSEUDO_BIN, 2, beg, end, len(recs), 0) + struct.pack("<i", 0)
    open(dst + ".bai", "wb").write(bytes(out))
    return len(table)


def index_shape(a):
    """--refs N --index: N chromosomes per file, the middle one requested; index='off' against index='auto'."""
    paths, gen_s = write_set(a.dir, a.cells, a.pairs, a.mbp)
    d = os.path.join(a.dir, "refs%d" % a.refs)
    os.makedirs(d, exist_ok=True)
    rpaths = [os.path.join(d, os.path.basename(p)) for p in paths]
    stamp = os.path.join(d, "set.json")
    want = dict(cells=a.cells, pairs=a.pairs, mbp=a.mbp, refs=a.refs)
    if not (os.path.exists(stamp) and json.load(open(stamp)) == want):
        with Pool(16) as pool:
            members = sum(pool.map(_refs_cell, [(s, t, a.refs, a.mbp) for s, t in zip(paths, rpaths)], chunksize=4))
        json.dump(dict(want, members=members), open(stamp, "w"))
    from secedo_amd import bam_pileup

    med = lambda xs: float(np.median(xs))  # noqa: E731
    line = dict(workload="uniform_refs", cells=a.cells, pairs=a.pairs, mbp=a.mbp, refs=a.refs, threads=a.threads,
                requested=a.refs // 2, members=json.load(open(stamp)).get("members"),
                bam_bytes=sum(os.path.getsize(p) for p in rpaths))
    outs = {}
    for route in ("host", "device") if a.device_inflate else ("host",):
        for mode in ("off", "auto"):
            out = os.path.join(a.dir, "rout_%s_%s" % (route, mode))
            runs = []
            for k in range(a.repeat + 1):
                t = {}
                p = bam_pileup.pileup_bams(rpaths, out, True, a.refs // 2, 100, 30, 30, 0, a.threads, 3, times=t,
                                           inflate=route, index=mode)
                if k:
                    runs.append(t)
            r = {key: round(med([x[key] for x in runs]), 2) for key in STEPS}
            r["inflated_bytes"] = runs[0]["inflated_bytes"]
            rs = bam_pileup.bam_route_stats()
            r["members_read"] = rs["host_blocks"] + rs["device_blocks"]
            r["index_stats"] = bam_pileup.bam_index_stats()
            r["loci"] = p.n_loci
            outs[route, mode] = [open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt")]
            line["%s_%s" % (route, mode)] = r
        line["%s_outputs_equal" % route] = outs[route, "auto"] == outs[route, "off"]
    print(json.dumps(line), flush=True)


def _bgzip(args):
    """src -> dst as BGZF: members of 65280 bytes at zlib level 6, then the empty EOF member (what bgzip writes)"""
    src, dst = args
    data = open(src, "rb").read()
    with open(dst, "wb") as f:
        for o in list(range(0, len(data), 0xFF00)) + [len(data)]:
            piece = data[o:o + 0xFF00]
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            payload = c.compress(piece) + c.flush()
            f.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(payload) + 25) +
                    payload + struct.pack("<II", zlib.crc32(piece), len(piece)))
    return dst


def write_sam_gz_set(sams, msam):
    """Each SAM file of the set beside it as <name>.sam.gz -> (paths, multiplexed path or None)"""
    jobs = [(s, s + ".gz") for s in sams] + ([(msam, msam + ".gz")] if msam else [])
    jobs = [j for j in jobs if not os.path.exists(j[1])]
    with Pool(16) as pool:
        pool.map(_bgzip, jobs, chunksize=4)
    return [s + ".gz" for s in sams], (msam + ".gz" if msam else None)


def device_route(a, files, host_out, med, **kw):
    """The BAM files through inflate='device': step times (medians of --repeat runs after one untimed run), the route
    stats of the last run, and its outputs against the host route's (host_out)"""
    from secedo_amd import bam_pileup

    prefix = host_out + "_dev"
    runs = []
    for k in range(a.repeat + 1):
        t = {}
        bam_pileup.pileup_bams(files, prefix, True, 0, 100, 30, 30, 0, a.threads, 3, times=t, inflate="device", **kw)
        if k:
            runs.append(t)
    r = {key: round(med([x[key] for x in runs]), 2) for key in STEPS}
    r["inflated_bytes"] = runs[0]["inflated_bytes"]
    r["inflate_GBps"] = r["inflated_bytes"] / (r["inflate_ms"] * 1e-3) / 1e9
    r["route_stats"] = bam_pileup.bam_route_stats()
    for ext in (".bin", ".map", ".txt"):
        r[ext[1:] + "_equal"] = open(prefix + ext, "rb").read() == open(host_out + ext, "rb").read()
    return r


def sam_route(a, sams, msam, barcodes, out, mout, sam_s, med, prefix="s"):
    """The SAM route's step times (medians of --repeat runs after one untimed run), its outputs against the BAM
    route's (out / mout), and a table of both routes on stderr"""
    from secedo_amd import bam_pileup

    def timed(files, prefix, **kw):
        runs = []
        for k in range(a.repeat + 1):
            t = {}
            bam_pileup.pileup_bams(files, prefix, True, 0, 100, 30, 30, 0, a.threads, 3, times=t, **kw)
            if k:
                runs.append(t)
        r = {key: round(med([x[key] for x in runs]), 2) for key in STEPS}
        r["text_bytes"] = runs[0]["inflated_bytes"]
        r["text_read_GBps"] = r["text_bytes"] / (r["inflate_ms"] * 1e-3) / 1e9
        for ext in (".bin", ".map"):
            r[ext[1:] + "_equal"] = open(prefix + ext, "rb").read() == open(out_of[prefix] + ext, "rb").read()
        return r

    sout = os.path.join(a.dir, prefix + "out")
    out_of = {sout: out}
    res = dict(set_write_s=round(sam_s, 1), per_file=timed(sams, sout))
    if msam:
        smout = os.path.join(a.dir, prefix + "mout")
        out_of[smout] = mout
        res["multiplexed"] = timed(msam, smout, cell_tag="CB", cells=barcodes)
    return res


def print_table(line):
    rows = [("BAM per-file", line)]
    if "device_inflate" in line:
        rows.append(("BAM dev-inflate", line["device_inflate"]))
    if "sam" in line:
        rows.append(("SAM per-file", line["sam"]["per_file"]))
    if "multiplexed" in line:
        rows.append(("BAM multiplexed", line["multiplexed"]))
        if "device_inflate" in line["multiplexed"]:
            rows.append(("BAM mux dev-inf", line["multiplexed"]["device_inflate"]))
    if "sam" in line and "multiplexed" in line["sam"]:
        rows.append(("SAM multiplexed", line["sam"]["multiplexed"]))
    if "sam_gz" in line:
        rows.append(("SAM.gz per-file", line["sam_gz"]["per_file"]))
        if "multiplexed" in line["sam_gz"]:
            rows.append(("SAM.gz multiplex", line["sam_gz"]["multiplexed"]))
    print("%-16s" % "ms" + "".join("%11s" % k[:-3] for k in STEPS), file=sys.stderr)
    for name, r in rows:
        print("%-16s" % name + "".join("%11.1f" % r[k] for k in STEPS), file=sys.stderr)


if __name__ == "__main__":
    main()
