"""The device route for BAM input (inflate="device", SECEDO_BAM_INFLATE=device, --inflate device): the BGZF members
inflated and the records walked on the GPU give, byte for byte, what the host route gives on the same files; errors
carry the host route's code and message; the route stats say which way the blocks went."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_device_cases as cases
from tests import bam_writer as bw
from tests import bgzf_writer as gw
from tests import multiplex_bam as mb
from tests import sam_writer as sw
from tests.golden_util import GOLDEN
from tests.test_gpu_pileup_bam import FIXTURE_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAM = os.path.join(GOLDEN, "bam")
GOLDENS = ["test1", "test2", "test3", "soft_clipping", "hard_clipping", "insert_at_end"]
PARAMS = [(100, 30, 30, 0, 3), (100, 0, 0, 0, 0), (6, 20, 10, 50, 1), (100, 35, 0, 90, 2)]


def fx(name):
    return os.path.join(BAM, name + ".bam")


def files_of(out):
    return tuple(open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt"))


def pile(files, out, chromosome=0, params=(100, 0, 0, 0, 0), threads=4, **kw):
    max_cov, min_bq, min_mq, min_as, diff = params
    p = bam_pileup.pileup_bams(files, out, True, chromosome, max_cov, min_bq, min_mq, min_as, threads, diff, **kw)
    return p, files_of(out)


def same(files, tmp_path, tag="", **kw):
    """host route == device route on the files -> (the device pileup, the device route's stats)"""
    ph, fh = pile(files, str(tmp_path / ("h" + tag)), inflate="host", **kw)
    stats_h = bam_pileup.bam_route_stats()
    pd, fd = pile(files, str(tmp_path / ("d" + tag)), inflate="device", **kw)
    stats = bam_pileup.bam_route_stats()
    assert fd == fh
    assert pd.n_loci == ph.n_loci
    for k in ("chr_locus_off", "locus_pos", "locus_entry_off", "read_ids", "id_base"):
        assert np.array_equal(getattr(pd, k), getattr(ph, k)), k
    assert stats_h["device_records"] == 0 and stats_h["downloaded_record_bytes"] == 0
    return pd, stats


def raw_of(path_or_bytes):
    data = open(path_or_bytes, "rb").read() if isinstance(path_or_bytes, str) else path_or_bytes
    return gw.inflate_all(data)


def record_starts(raw):
    """-> (offset of the first record, [offset of every record], len(raw)) of inflated BAM bytes"""
    l_text = struct.unpack_from("<i", raw, 4)[0]
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    first, starts = o, []
    while o < len(raw):
        starts.append(o)
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    return first, starts, len(raw)


def aligned_bgzf(raw, limit=0xFF00, **kw):
    """htslib's rule: a member is flushed before a record that would not fit, so members start on records (a record
    longer than a member is cut)."""
    first, starts, n = record_starts(raw)
    cuts, at = [0], 0
    for s, e in zip(starts, starts[1:] + [n]):
        if e - at > limit and s > at:
            cuts.append(s)
            at = s
        while e - at > limit:
            at += limit
            cuts.append(at)
    cuts.append(n)
    return b"".join(gw.bgzf(raw[a:b], chunk=limit, eof=False, **kw) for a, b in zip(cuts, cuts[1:]) if b > a) + \
        gw.EOF_MEMBER


def with_empty_members(raw, chunk=3000):
    """members of `chunk` bytes with an empty member after every second one"""
    out = []
    for k, o in enumerate(range(0, len(raw), chunk)):
        out.append(gw.bgzf(raw[o:o + chunk], eof=False))
        if k % 2:
            out.append(gw.EOF_MEMBER)
    return b"".join(out) + gw.EOF_MEMBER


WRITERS = {
    "cut-ff00": lambda raw: gw.bgzf(raw),
    "chunk-4096": lambda raw: gw.bgzf(raw, chunk=4096),
    "chunk-1000": lambda raw: gw.bgzf(raw, chunk=1000),
    "stored": lambda raw: gw.bgzf(raw, level=0),
    "fixed": lambda raw: gw.bgzf(raw, strategy="fixed", chunk=8192),
    "aligned": lambda raw: aligned_bgzf(raw, limit=4096),
    "empty-members": with_empty_members,
}


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """bw.synthetic_set's cells, canonical -> (refs, cell records, bams, sams)."""
    d = tmp_path_factory.mktemp("synth_dev")
    refs, cells = mb.synthetic_cells(d / "raw", n_cells=8, pairs_per_cell=60, n_refs=2, seed=11)
    bams, sams = [], []
    for c, recs in enumerate(cells):
        b, s = sw.write_both(d, "cell_%03d" % c, refs, recs)
        bams.append(b)
        sams.append(s)
    return refs, cells, bams, sams


@pytest.fixture(scope="module")
def big(synth, tmp_path_factory):
    """every cell's records in one BAM: several members of 0xFF00 bytes"""
    refs, cells, _, _ = synth
    d = tmp_path_factory.mktemp("big_dev")
    path, _ = sw.write_both(d, "big", refs, sorted((r for c in cells for r in c), key=bw.sort_key))
    assert len(raw_of(path)) > 4 * 0xFF00
    return path


def header_blocks(path):
    """The leading BGZF members of the file that hold its header and reference list."""
    data = open(path, "rb").read()
    first = record_starts(raw_of(data))[0]
    o = got = k = 0
    while got < first:
        size = int.from_bytes(data[o + 16:o + 18], "little") + 1
        got += int.from_bytes(data[o + size - 4:o + size], "little")
        o += size
        k += 1
    return k


def n_members(path):
    data, o, k = open(path, "rb").read(), 0, 0
    while o < len(data):
        o += int.from_bytes(data[o + 16:o + 18], "little") + 1
        k += 1
    return k


# ---------------------------------------------------------------------------------------------- device == host

@pytest.mark.parametrize("case", range(len(FIXTURE_CASES)))
def test_fixture_cases(case, tmp_path):
    names, max_cov, mq, score, diff, n_loci = FIXTURE_CASES[case]
    files = [fx(n) for n in names]
    p, stats = same(files, tmp_path, params=(max_cov, 1, mq, score, diff))
    assert p.n_loci == n_loci
    assert stats["rewalked_segments"] == 0
    assert stats["host_blocks"] == sum(header_blocks(f) for f in files)
    assert stats["device_blocks"] == sum(n_members(f) for f in files) - stats["host_blocks"]
    assert stats["device_records"] == sum(bam_pileup.bam_scan(f)["n_records"] for f in files)


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("chromosome", [0, 1])
def test_synthetic_sets(synth, params, chromosome, tmp_path):
    _, _, bams, _ = synth
    p, _ = same(bams, tmp_path, chromosome=chromosome, params=params)
    if params[1] == 0:
        assert p.n_loci > 100


def _resident(files, i2g, **kw):
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, cells, max_len = bam_pileup.pileup_bams_resident(plan, files, [0, 1], 100, 20, 0, 0, 4, 1,
                                                              id_to_group=i2g, **kw)
        return {k: res[k].cpu().numpy() for k in ("chr", "pos", "off", "rid", "idb")}, cells, max_len


def test_resident_two_chromosomes_and_download_stats(synth, tmp_path):
    _, _, bams, _ = synth
    i2g = (np.arange(len(bams)) // 2).astype(np.uint16)
    gh, ch, lh = _resident(bams, i2g, inflate="host")
    gd, cd, ld = _resident(bams, i2g, inflate="device")
    both = bam_pileup.bam_route_stats()["downloaded_record_bytes"]
    assert (cd, ld) == (ch, lh) and gh["chr"][-1] > 0
    for k in gh:
        assert np.array_equal(gd[k], gh[k]), k
    # the bytes that came back are the runs of the requested chromosomes, no more
    sizes = [0, 0]
    total = 0
    for b in bams:
        raw = raw_of(b)
        _, starts, n = record_starts(raw)
        for s, e in zip(starts, starts[1:] + [n]):
            ref = struct.unpack_from("<i", raw, s + 4)[0]
            total += e - s
            if ref in (0, 1):
                sizes[ref] += e - s
    assert both == sum(sizes)
    pile(bams, str(tmp_path / "one"), chromosome=1, inflate="device")
    one = bam_pileup.bam_route_stats()["downloaded_record_bytes"]
    assert one == sizes[1] and 0 < one < both < total


def test_deterministic_and_pool_size(synth, tmp_path):
    _, _, bams, _ = synth
    outs = [pile(bams, str(tmp_path / ("d%d" % k)), threads=threads, inflate="device")[1]
            for k, threads in enumerate([1, 16, 16])]
    assert outs[0] == outs[1] == outs[2]


def test_tag_mode_barcodes_and_mixed_list(synth, tmp_path):
    refs, cells, bams, sams = synth
    barcodes = ["AAC%02d-1" % c for c in range(len(cells))]
    recs = [r for c in mb.tagged(cells, barcodes) for r in c]
    lanes, _ = sw.write_multiplexed(tmp_path, refs, recs, n_lanes=2, seed=4)
    for chromosome in (0, 1):
        same(lanes, tmp_path, tag="t%d" % chromosome, chromosome=chromosome, cell_tag="CB", cells=barcodes[::-1][:6])
    same(lanes, tmp_path, tag="all", cell_tag="CB", cells=barcodes)
    vh, nh = bam_pileup.bam_barcodes(lanes, "CB", [0, 1], 4, inflate="host")
    vd, nd = bam_pileup.bam_barcodes(lanes, "CB", [0, 1], 4, inflate="device")
    assert vd == vh == sorted(barcodes) and np.array_equal(nd, nh)
    # BAM, BGZF SAM and SAM in one list
    gz = str(tmp_path / "cell1.sam.gz")
    with open(gz, "wb") as f:
        f.write(gw.bgzf(open(sams[1], "rb").read(), chunk=4096))
    _, stats = same([bams[0], gz, sams[2]], tmp_path, tag="mix")
    assert pile(bams[:3], str(tmp_path / "b3"), inflate="host")[1] == files_of(str(tmp_path / "dmix"))
    assert stats["device_records"] == bam_pileup.bam_scan(bams[0])["n_records"]


# ---------------------------------------------------------------------------------------------- writers

def _rewritten(tmp_path, sources, how):
    paths = []
    for k, src in enumerate(sources):
        path = str(tmp_path / ("%s_%d.bam" % (how, k)))
        with open(path, "wb") as f:
            f.write(WRITERS[how](raw_of(src)))
        assert raw_of(path) == raw_of(src)
        paths.append(path)
    return paths


@pytest.mark.parametrize("how", sorted(WRITERS))
def test_writers(how, synth, big, tmp_path):
    _, _, bams, _ = synth
    want = pile(bams[:3] + [big], str(tmp_path / "want"), inflate="host")[1]
    paths = _rewritten(tmp_path, bams[:3] + [big], how)
    _, stats = same(paths, tmp_path)
    assert files_of(str(tmp_path / "d")) == want
    assert stats["host_blocks"] == sum(header_blocks(p) for p in paths)
    assert stats["device_blocks"] == sum(n_members(p) for p in paths) - stats["host_blocks"]
    assert stats["segments"] >= stats["device_blocks"] - 4
    if how == "aligned":
        assert stats["rewalked_segments"] == 0
    if how in ("cut-ff00", "chunk-1000"):
        assert stats["rewalked_segments"] > 0
    for p in paths:
        _scan_equal(p)
    # the goldens through the same writer
    g = _rewritten(tmp_path, [fx(n) for n in ("test1", "test2")], how)
    same(g, tmp_path, tag="g", params=(10, 1, 0, 0, 1))


def _scan_equal(path):
    a, b = bam_pileup.bam_scan(path), bam_pileup.bam_scan(path, device=True)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (path, k)
    return b


def test_scan_device(synth, tmp_path):
    _, _, bams, _ = synth
    for p in [fx(n) for n in GOLDENS] + bams[:2]:
        _scan_equal(p)
    for how in sorted(WRITERS):
        for p in _rewritten(tmp_path, bams[:1], how):
            _scan_equal(p)
    recs = [bw.Rec("a", 0, 50, [("M", 4)], "ACGT", qual=[40] * 4), bw.Rec("b", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4),
            bw.Rec("c", 1, 5, [("M", 4)], "ACGT", qual=[40] * 4), bw.Rec("u", -1, -1, [], "ACGT", qual=[30] * 4, flag=4),
            bw.Rec("d", 0, 70, [("M", 4)], "ACGT", qual=[40] * 4)]
    path = str(tmp_path / "unsorted.bam")
    bw.write_bam(path, [("1", 1000), ("2", 1000)], recs)
    got = _scan_equal(path)
    assert not got["sorted"] and got["n_records"] == 5 and got["n_unmapped"] == 1


def test_header_longer_than_a_block(tmp_path):
    refs = [("contig_%05d_with_a_long_name" % k, 100000 + k) for k in range(6000)]
    recs = [bw.Rec("r%d" % k, 0, 100 + k, [("M", 8)], "ACGTACGT", qual=[40] * 8) for k in range(50)]
    recs += [bw.Rec("s%d" % k, 1, 100 + k, [("M", 8)], "ACGTACGT", qual=[40] * 8) for k in range(5)]
    paths = []
    for k in range(2):
        path = str(tmp_path / ("long_%d.bam" % k))
        bw.write_bam(path, refs, recs)
        paths.append(path)
    assert header_blocks(paths[0]) >= 3
    _, stats = same(paths, tmp_path, params=(100, 0, 0, 0, 0))
    assert stats["host_blocks"] == 2 * header_blocks(paths[0])
    assert stats["device_blocks"] == 2 * (n_members(paths[0]) - header_blocks(paths[0]))
    _scan_equal(paths[0])


# ---------------------------------------------------------------------------------------------- batches and ranges

def test_small_batches_give_identical_outputs(synth, tmp_path, monkeypatch):
    refs, cells, bams, _ = synth
    recs = [r for c in mb.tagged(cells, ["B%02d" % c for c in range(len(cells))]) for r in c]
    big, _ = sw.write_both(tmp_path, "big", refs, sorted(recs, key=bw.sort_key))
    assert len(raw_of(big)) > 4 * 65536
    want_set = pile(bams, str(tmp_path / "ws"), inflate="host")[1]
    want_big = pile([big], str(tmp_path / "wb"), inflate="host")[1]
    want_tag = pile([big], str(tmp_path / "wt"), inflate="host", cell_tag="CB", cells=["B03", "B00", "B05"])[1]
    n_seg = None
    for batch in ("65536", "1000"):
        monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", batch)
        assert pile(bams, str(tmp_path / "s"), inflate="device")[1] == want_set
        assert bam_pileup.bam_route_stats()["batches"] > 1
        assert pile([big], str(tmp_path / "b"), inflate="device")[1] == want_big
        stats = bam_pileup.bam_route_stats()
        assert stats["batches"] >= 4 and stats["device_records"] == len(recs)
        assert n_seg is None or stats["segments"] == n_seg  # the same members, cut into more ranges
        n_seg = stats["segments"]
        assert pile([big], str(tmp_path / "t"), inflate="device", cell_tag="CB", cells=["B03", "B00", "B05"])[1] == want_tag
        assert pile([big, bams[0], big], str(tmp_path / "m"), inflate="device")[1] == \
            pile([big, bams[0], big], str(tmp_path / "mh"), inflate="host")[1]
        _scan_equal(big)


def test_102_files_go_through_in_batches(tmp_path, monkeypatch):
    paths = []
    for f in range(102):
        recs = [bw.Rec("shared", 0, 100, [("M", 8)], "ACGTACGT", qual=[40] * 8),
                bw.Rec("own%d" % f, 0, 104, [("M", 8)], "CCGTACGT" if f % 2 else "ACGTACGT", qual=[40] * 8)]
        path = str(tmp_path / ("f%03d.bam" % f))
        bw.write_bam(path, [("1", 1000)], recs)
        paths.append(path)
    got, stats = same(paths, tmp_path, params=(1000, 0, 0, 0, 0))
    assert stats["batches"] == 1 and stats["device_records"] == 204
    ids = {}
    b, e = int(got.locus_entry_off[0]), int(got.locus_entry_off[1])
    for rid, cb in zip(got.read_ids[b:e], got.id_base[b:e]):
        ids[int(cb) >> 2] = int(rid)
    assert ids[0] == ids[100] and ids[1] == ids[101] and ids[0] != ids[1]
    want = files_of(str(tmp_path / "h"))
    for batch in ("65536", "1000"):
        monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", batch)
        assert pile(paths, str(tmp_path / "x"), params=(1000, 0, 0, 0, 0), inflate="device")[1] == want
        stats = bam_pileup.bam_route_stats()
        assert 1 < stats["batches"] < 102  # several files to a launch, several launches
        assert stats["device_records"] == 204 and stats["host_blocks"] == 102


def test_a_file_without_a_member_left_shares_a_batch(tmp_path):
    """The middle file is one member that holds the header and every record, with no EOF member behind it: nothing of
    it is left to inflate on the device, and its carry is walked as one segment between two files that have members."""
    refs, paths, n_rec = [("1", 100000), ("2", 100000)], [], 0
    for f, chunk in enumerate((1000, None, 700)):
        recs = [bw.Rec("r%d_%d" % (f, k), k // 60, 100 + 7 * (k % 60) + f, [("M", 8)], "ACGTACGT"[f:] + "ACGTACGT"[:f],
                       qual=[40] * 8) for k in range(100 + f)]
        raw = raw_of(bw.bam_bytes(refs, recs))
        path = str(tmp_path / ("f%d.bam" % f))
        with open(path, "wb") as out:
            out.write(gw.bgzf(raw, chunk=chunk) if chunk else gw.bgzf(raw, eof=False))
        paths.append(path)
        n_rec += len(recs)
    assert [n_members(p) == header_blocks(p) for p in paths] == [False, True, False] and n_members(paths[1]) == 1
    for chromosome in (0, 1):
        _, stats = same(paths, tmp_path, tag=str(chromosome), chromosome=chromosome)
        assert stats["batches"] == 1 and stats["device_records"] == n_rec
        assert stats["host_blocks"] == sum(header_blocks(p) for p in paths)
        assert stats["device_blocks"] == sum(n_members(p) for p in paths) - stats["host_blocks"]
        assert stats["segments"] == stats["device_blocks"] + 1  # the middle file's carry
    for p in paths:
        _scan_equal(p)


# ---------------------------------------------------------------------------------------------- errors

def both_errors(files, **kw):
    """the host route's and the device route's error on the files: they must be equal -> the message"""
    errs = []
    for how in ("host", "device"):
        with pytest.raises(secedo_amd.SecedoError) as e:
            bam_pileup.pileup_bams(files, None, False, kw.get("chromosome", 0), 100, 0, kw.get("mq", 0), 0, 1, 0,
                                   inflate=how)
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1]
    return errs[1][1]


GOOD = bw.Rec("g", 0, 10, [("M", 4)], "ACGT", qual=[40] * 4)


def test_abort_cases_equal_the_host_routes(tmp_path):
    far = bw.Rec("x", 0, 999_000, [("M", 10), ("D", 2000), ("M", 10)], "A" * 20, qual=[40] * 20, mapq=5)
    cases = [[GOOD, bw.Rec("x", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4, flag=0x1)],
             [GOOD, bw.Rec("x", 0, 20, [("M", 4)], "ACGT", qual=[40] * 4, flag=0x3 | 0x200)],
             [GOOD, far],
             [GOOD, bw.Rec("x", 0, 20, [("M", 10), ("I", 5), ("S", 5)], "A" * 20, qual=[40] * 20)]]
    for k, recs in enumerate(cases):
        path = str(tmp_path / ("a%d.bam" % k))
        bw.write_bam(path, [("1", 3_000_000)], recs)
        assert "file 0, record" in both_errors([path])


def _many(n=400, ref=0):
    return [bw.Rec("f%d" % k, ref, 12 + k, [("M", 4)], "ACGT", qual=[40] * 4) for k in range(n)]


def _write(tmp_path, name, raw, **kw):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(gw.bgzf(raw, **kw))
    return path


def test_walk_errors_equal_the_host_routes(tmp_path):
    refs = [("1", 3_000_000), ("2", 3_000_000)]
    raw = raw_of(bw.bam_bytes(refs, _many()))
    first, starts, n = record_starts(raw)
    k = 250
    at = starts[k]
    cases = {
        "truncated": (raw[:n - 20], "record 399 is truncated"),
        "cut-in-size": (raw[:starts[399] + 2], "record 399 is truncated"),
        "overrun": (raw[:n - 3], "record 399 has a bad block_size"),
        "size-31": (raw[:at] + struct.pack("<I", 31) + raw[at + 4:], "record 250 has a bad block_size"),
        "longer": (raw[:at + 4 + 16] + struct.pack("<I", 5000) + raw[at + 4 + 20:], "record 250 is longer than"),
        "negative": (raw[:at + 8] + struct.pack("<i", -5) + raw[at + 12:], None),
        "magic": (raw[:8], "not a BAM file (magic)"),  # the magic and four more bytes: no header
        "short-header": (raw[:first - 3], "truncated reference list"),
        "short-text": (raw[:20], "truncated header"),
    }
    for name, (data, what) in cases.items():
        for kw in (dict(), dict(chunk=1000)):
            path = _write(tmp_path, name + ".bam", data, **kw)
            msg = both_errors([path])
            assert what is None or what in msg, (name, msg)
    recs = _many()
    recs[300], recs[301] = recs[301], recs[300]
    assert "record 301: input is not coordinate-sorted" in both_errors(
        [_write(tmp_path, "unsorted.bam", raw_of(bw.bam_bytes(refs, recs)), chunk=1000)])
    recs = _many()
    recs[200] = bw.Rec("x", 0, 212, [("M", 3)], "ACGT", qual=[40] * 4)
    assert "record 200: CIGAR and SEQ lengths differ" in both_errors(
        [_write(tmp_path, "cigar.bam", raw_of(bw.bam_bytes(refs, recs)), chunk=1000)])
    raw = raw_of(bw.bam_bytes(refs, _many()))
    cig = starts[200] + 4 + 32 + len("f200") + 1
    bad = raw[:cig] + struct.pack("<I", 4 << 4 | 11) + raw[cig + 4:]
    assert "record 200: invalid CIGAR op code 11" in both_errors([_write(tmp_path, "op.bam", bad)])
    # a record of another chromosome is not checked: no error on chromosome 0, an error on chromosome 1
    recs = _many(100) + [bw.Rec("x", 1, 5, [("M", 3)], "ACGT", qual=[40] * 4)]
    path = _write(tmp_path, "other.bam", raw_of(bw.bam_bytes(refs, recs)))
    same([path], tmp_path, tag="other")
    assert "record 100: CIGAR" in both_errors([path], chromosome=1)
    # the lowest file index comes first
    good = _write(tmp_path, "good.bam", raw_of(bw.bam_bytes(refs, _many())))
    files = [good, str(tmp_path / "cigar.bam"), str(tmp_path / "unsorted.bam")]
    assert "cigar.bam: record 200" in both_errors(files)


def test_block_errors(tmp_path):
    """The corrupt members are those of tests/bam_device_cases.py, which tests/test_bam_walk_cpu.py puts through the
    decoder on the host first."""
    raw = cases.block_error_bytes()
    _, starts, n = record_starts(raw)
    for how, k, data in cases.corrupt_bams():
        path = str(tmp_path / ("c_%s_%d.bam" % (how, k)))
        with open(path, "wb") as f:
            f.write(data)
        msg = both_errors([path])  # member 0 is the header's: the host inflates it on either route
        assert "BGZF block %d: " % k in msg and (how != "stored" or "CRC32 mismatch" in msg), msg
    # a record error after the bad member: the member comes first; before it: the record comes first
    path = str(tmp_path / "late.bam")
    with open(path, "wb") as f:
        f.write(cases.corrupt_with_record_error(2900))
    assert "BGZF block 3: " in both_errors([path])
    path = str(tmp_path / "early.bam")
    with open(path, "wb") as f:
        f.write(cases.corrupt_with_record_error(20))
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams([path], None, False, 0, 100, 0, 0, 0, 1, 0, inflate="device")
    assert e.value.code == -1 and "record 20 has a bad block_size" in str(e.value)
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.bam_scan(str(tmp_path / "late.bam"), device=True)
    assert "BGZF block 3: " in str(e.value)


@pytest.mark.parametrize("damage", range(len(gw.LISTING_DAMAGE)))
def test_a_file_whose_members_cannot_be_listed(tmp_path, damage):
    """Member 0 (the header's, which makes the file a BAM) is whole; the list breaks at member 1, on either route."""
    raw = gw.bgzf(raw_of(bw.bam_bytes([("1", 3_000_000)], _many())), chunk=4000)
    name, data, tail = gw.listing_damage(raw)[damage]
    path = str(tmp_path / (name + ".bam"))
    with open(path, "wb") as f:
        f.write(data)
    assert both_errors([path]) == gw.ERROR_PREFIX + path + tail


# ---------------------------------------------------------------------------------------------- surface

def test_cli_and_environment(synth, tmp_path):
    _, _, bams, _ = synth
    d = tmp_path / "in"
    d.mkdir()
    for k, b in enumerate(bams[:4]):
        os.symlink(b, str(d / ("cell_%d.bam" % k)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "secedo_amd.pileup_main", "-i", str(d), "--chromosomes", "1,2", "--min_base_quality",
            "20", "--min_map_quality", "0", "--min_different", "1"]
    outs = {}
    for name, extra, e in (("plain", [], {}), ("flag", ["--inflate", "device"], {}),
                           ("env", [], {"SECEDO_BAM_INFLATE": "device"})):
        o = str(tmp_path / name)
        r = subprocess.run(base + ["-o", o] + extra, env=dict(env, **e), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = [open("%s_%s.pileup%s" % (o, c, ext), "rb").read() for c in "12" for ext in (".bin", ".map", ".txt")]
        assert len(outs[name][0]) > 0
    assert outs["flag"] == outs["plain"] and outs["env"] == outs["plain"]
    code = ("import sys\n"
            "from secedo_amd import bam_pileup\n"
            "bam_pileup.pileup_bams([sys.argv[1]], None, False, 0, 100, 0, 0, 0, 1, 0)\n"
            "print(bam_pileup.bam_route_stats()['device_records'])\n")
    r = subprocess.run([sys.executable, "-c", code, bams[0]], env=dict(env, SECEDO_BAM_INFLATE="device"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and int(r.stdout.split()[-1]) > 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-c", code, bams[0]], env=dict(env, SECEDO_BAM_INFLATE="gpu"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "SECEDO_BAM_INFLATE=gpu: expected host or device" in r.stderr
    r = subprocess.run(base + ["-o", str(tmp_path / "bad"), "--inflate", "gpu"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "invalid choice" in r.stderr


def test_bad_values_are_refused(synth):
    _, _, bams, _ = synth
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams(bams[:1], None, False, 0, 100, 0, 0, 0, 1, 0, inflate="gpu")
    assert e.value.code == -1
    assert bam_pileup.lib().secedo_bam_set_inflate(7) == -1
    assert b"neither" in bam_pileup.lib().secedo_bam_last_error()
    # the keyword leaves the process setting as it found it
    bam_pileup.pileup_bams(bams[:1], None, False, 0, 100, 0, 0, 0, 1, 0, inflate="device")
    assert bam_pileup.bam_route_stats()["device_records"] > 0
    bam_pileup.pileup_bams(bams[:1], None, False, 0, 100, 0, 0, 0, 1, 0)
    assert bam_pileup.bam_route_stats()["device_records"] == 0
