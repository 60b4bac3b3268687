"""Reading BAM files through their .bai index (index="auto" / "require", SECEDO_BAM_INDEX, --index): every call gives,
byte for byte, what index="off" gives, on the host and on the device route; only the header's members and the members
of the requested chromosomes' spans are inflated; an index that does not fit its file is an error, the same on both
routes. The corrupt BAMs and the indexes that do not fit are built in tests/bam_index_cases.py;
tests/test_bam_index_cpu.py puts the same bytes through bgzf_inflate_test, bam_walk_test (each span from its entry to
its limit) and bam_index_test on the host, under the sanitizers, before a GPU sees them."""
import os
import shutil
import struct

import numpy as np
import pytest

import secedo_amd
from secedo_amd import _lib, bam_pileup
from tests import bai_writer as bi
from tests import bam_index_cases as ic
from tests import bam_writer as bw
from tests import bgzf_writer as gw
from tests import sam_writer as sw
from tests.golden_util import GOLDEN
from tests.test_bam_index_cpu import bad_indexes

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "bam")
GOLDENS = ["test1", "test2", "test3", "soft_clipping", "hard_clipping", "insert_at_end"]
ROUTES = ("host", "device")
REFS, reads, raw_bam, htslib_members, put = ic.REFS, ic.reads, ic.raw_bam, ic.htslib_members, ic.put


def expected_members(path, chromosomes):
    """From the member table and the writer's ranges: (the header's members + the members of the spans, all members)"""
    data = open(path, "rb").read()
    table = bi.member_table(data)
    spans = bi.record_spans(bi.inflate(data))
    first = spans[0][0] if spans else sum(m[2] for m in table)
    head = sum(1 for _c, _n, isize, start in table if start < first and isize)
    rng = bi.ranges(path)
    want = sorted((rng[c][0], rng[c][1]) for c in set(chromosomes) if c < len(rng) and rng[c][2])
    merged = []
    for beg, end in want:
        if merged and beg >> 16 <= merged[-1][1] >> 16:
            merged[-1][1] = max(merged[-1][1], end)
        else:
            merged.append([beg, end])
    n = sum(1 for beg, end in merged for coff, *_ in table
            if beg >> 16 <= coff and (coff < end >> 16 or (coff == end >> 16 and end & 0xFFFF)))
    return head + n, len(table), len(merged)


def full_read_members(path, route):
    """The members a full read inflates: every member on the host route; on the device route the header's members go
    through the host and every other member through the device, trailing empty members included"""
    return expected_members(path, [])[1]


def files_of(out):
    return tuple(open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt"))


def pile(files, out, chromosome, params=(100, 20, 0, 0, 1), threads=4, **kw):
    p = bam_pileup.pileup_bams(files, out, True, chromosome, params[0], params[1], params[2], params[3], threads,
                               params[4], **kw)
    return p, files_of(out)


def same_as_off(files, tmp_path, chromosome, tag="", indexed=None, **kw):
    """index="auto" and "require" against "off" on both routes -> {(route, mode): (route stats, index stats)}"""
    stats = {}
    for route in ROUTES:
        p0, f0 = pile(files, str(tmp_path / ("off" + route + tag)), chromosome, inflate=route, index="off", **kw)
        assert bam_pileup.bam_index_stats()["files_indexed"] == 0
        for mode in ("auto", "require"):
            p1, f1 = pile(files, str(tmp_path / (mode + route + tag)), chromosome, inflate=route, index=mode, **kw)
            stats[route, mode] = (bam_pileup.bam_route_stats(), bam_pileup.bam_index_stats())
            assert f1 == f0, (route, mode)
            for k in ("chr_locus_off", "locus_pos", "locus_entry_off", "read_ids", "id_base"):
                assert np.array_equal(getattr(p1, k), getattr(p0, k)), (route, mode, k)
            if indexed is not None:
                assert stats[route, mode][1]["files_indexed"] == indexed
        assert any(len(x) for x in f0) or chromosome == 3  # the comparison is not of nothing with nothing
    return stats


def check_members(stats, files, chromosomes):
    want = sum(expected_members(f, chromosomes)[0] for f in files)
    total = sum(expected_members(f, chromosomes)[1] for f in files)
    spans = sum(expected_members(f, chromosomes)[2] for f in files)
    for key, (route, index) in stats.items():
        assert route["host_blocks"] + route["device_blocks"] == want, (key, route, want)
        assert index["members"] + sum(expected_members(f, [])[0] for f in files) == want
        assert index["spans"] == spans and index["members_skipped"] == 0
    assert want < total
    return want, total


def barcodes_same(files, chromosomes, **kw):
    out = {}
    for route in ROUTES:
        v0, c0 = bam_pileup.bam_barcodes(files, "CB", chromosomes, 4, inflate=route, index="off", **kw)
        for mode in ("auto", "require"):
            v1, c1 = bam_pileup.bam_barcodes(files, "CB", chromosomes, 4, inflate=route, index=mode, **kw)
            out[route, mode] = (bam_pileup.bam_route_stats(), bam_pileup.bam_index_stats())
            assert v1 == v0 and np.array_equal(c1, c0), (route, mode)
        assert len(v0) == 3 or not chromosomes
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_with_their_committed_index(name, tmp_path):
    path = os.path.join(BAM, name + ".bam")
    for params in ((100, 30, 30, 0, 3), (100, 0, 0, 0, 0)):
        stats = same_as_off([path], tmp_path, 0, params=params, indexed=1)
    check_members(stats, [path], [0])


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    d = tmp_path_factory.mktemp("three")
    return put(d, "three.bam", htslib_members(raw_bam(reads()))), d


def test_three_references_htslib_members(three, tmp_path):
    path, _ = three
    for c in (0, 1, 2):
        want, total = check_members(same_as_off([path], tmp_path, c, tag=str(c), indexed=1), [path], [c])
        assert want * 2 < total
    # a reference without records: nothing beyond the header
    stats = same_as_off([path], tmp_path, 3, tag="e", indexed=1)
    for route, index in stats.values():
        assert index["spans"] == 0 and route["host_blocks"] + route["device_blocks"] == expected_members(path, [])[0]
    # one span, two disjoint spans, one merged span, through a call that takes several chromosomes
    for chromosomes, spans in (([1], 1), ([0, 2], 2), ([2, 0], 2), ([0, 1, 2], 1), ([1, 3, 1], 1)):
        assert expected_members(path, chromosomes)[2] == spans
        check_members(barcodes_same([path], chromosomes), [path], chromosomes)


def _resident(files, chromosomes, **kw):
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, cells, max_len = bam_pileup.pileup_bams_resident(plan, files, chromosomes, 100, 20, 0, 0, 4, 1, **kw)
        return {k: res[k].cpu().numpy() for k in ("chr", "pos", "off", "rid", "idb")}, cells, max_len


def test_resident_and_tag_mode(three, tmp_path):
    path, _ = three
    cells = ["cell0", "cell1", "cell2"]
    for route in ROUTES:
        for kw in ({}, dict(cell_tag="CB", cells=cells)):
            g0, c0, l0 = _resident([path], [0, 2], inflate=route, index="off", **kw)
            g1, c1, l1 = _resident([path], [0, 2], inflate=route, index="require", **kw)
            assert (c1, l1) == (c0, l0) and g0["chr"][-1] > 0
            assert bam_pileup.bam_index_stats()["spans"] == 2
            for k in g0:
                assert np.array_equal(g1[k], g0[k]), (route, k)
    stats = same_as_off([path], tmp_path, 1, tag="t", indexed=1, cell_tag="CB", cells=cells)
    check_members(stats, [path], [1])


@pytest.mark.parametrize("chunk", (16384, 1000))
def test_fixed_size_member_cuts(chunk, tmp_path):
    """runs begin and end mid-member; a block_size straddles the member boundary at a span's start and at a span's
    end; a record is longer than a member (chunk 1000)"""
    def build(pad_text, pad_tag):
        """the header text and reference 2's last record padded by so many bytes"""
        recs = reads(seed=21, long_every=40)  # the same records for both cuts
        last2 = max(k for k, r in enumerate(recs) if r.ref == 2)
        recs[last2].tags = recs[last2].tags + [("XP", "Z", "x" * pad_tag)]
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + \
            "@CO\t" + "x" * pad_text + "\n"
        raw = gw.inflate_all(bw.bam_bytes(REFS, recs, text=text))
        spans = bi.record_spans(raw)
        ref_of = [struct.unpack_from("<i", raw, s + 4)[0] for s, _e in spans]
        begs = {r: spans[ref_of.index(r)][0] for r in (0, 1, 2)}
        ends = {r: spans[len(ref_of) - 1 - ref_of[::-1].index(r)][1] for r in (0, 1, 2)}
        return raw, spans, begs, ends

    straddles = lambda o: (o % chunk) > chunk - 4  # noqa: E731  the four bytes of block_size cross a boundary
    _raw, _spans, begs, _ends = build(0, 0)
    pad_text = (chunk - 2 - begs[1]) % chunk
    _raw, _spans, _begs, ends = build(pad_text, 0)
    raw, spans, begs, ends = build(pad_text, (chunk - 2 - ends[2]) % chunk)
    assert straddles(begs[1]) and straddles(ends[2])
    assert begs[2] % chunk and ends[0] % chunk
    if chunk == 1000:
        assert max(e - s for s, e in spans) > chunk
    path = put(tmp_path, "cut.bam", gw.bgzf(raw, chunk=chunk))
    for c in (0, 1, 2):
        check_members(same_as_off([path], tmp_path, c, tag=str(c), indexed=1), [path], [c])
    check_members(barcodes_same([path], [0, 2]), [path], [0, 2])


def test_header_and_records_in_one_member(tmp_path):
    raw = raw_bam(reads(n=40))
    assert len(raw) < 0xFF00
    path = put(tmp_path, "one.bam", gw.bgzf(raw))
    for c in (0, 1, 2):
        stats = same_as_off([path], tmp_path, c, tag=str(c), indexed=1)
        for route, index in stats.values():
            assert index["spans"] == 1 and index["members"] == 1
            assert route["host_blocks"] + route["device_blocks"] == 2  # the one member, as header and as span


def test_small_batches(three, tmp_path, monkeypatch):
    raw = raw_bam(reads(n=2500, seed=9))
    path = put(tmp_path, "big.bam", htslib_members(raw, limit=16384))
    beg, end, _n = bi.ranges(path)[1]
    table = bi.member_table(open(path, "rb").read())
    span_bytes = sum(m[2] for m in table if beg >> 16 <= m[0] < end >> 16)
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", str(64 << 10))
    assert span_bytes > 3 * (64 << 10)
    stats = same_as_off([path], tmp_path, 1, indexed=1)
    check_members(stats, [path], [1])
    assert stats["device", "auto"][0]["batches"] >= 3
    check_members(barcodes_same([path], [0, 2]), [path], [0, 2])


def test_many_files_mixed_inputs(tmp_path):
    files, indexed = [], []
    for k in range(40):
        recs = reads(n=12, seed=100 + k)
        path = put(tmp_path, "cell_%02d.bam" % k, htslib_members(raw_bam(recs), limit=700), index=k % 2 == 0)
        files.append(path)
        indexed += [path] if k % 2 == 0 else []
    sam = str(tmp_path / "cell_40.sam")
    sw.write_sam(sam, REFS, sorted(reads(n=12, seed=77), key=bw.sort_key))
    files.append(sam)  # behind the BAMs, which are then one run of the list and fit one batch
    for route in ROUTES:
        p0, f0 = pile(files, str(tmp_path / ("off" + route)), 1, inflate=route, index="off")
        p1, f1 = pile(files, str(tmp_path / ("auto" + route)), 1, inflate=route, index="auto")
        index, rs = bam_pileup.bam_index_stats(), bam_pileup.bam_route_stats()
        assert f1 == f0 and len(f0[0]) > 0
        assert (index["files_indexed"], index["files_full"], index["rejected"], index["spans"]) == (20, 20, 0, 20)
        if route == "device":
            assert rs["batches"] == 1  # the files read in full and the indexed files' spans share it
        with pytest.raises(_lib.SecedoError) as e:
            pile(files, str(tmp_path / "req"), 1, inflate=route, index="require")
        assert e.value.code == _lib.E_INVALID_ARG and files[1] in str(e.value) and "no index file" in str(e.value)


def test_index_without_pseudo_bin(tmp_path):
    path = put(tmp_path, "plain.bam", htslib_members(raw_bam(reads())), pseudo_bin=False)
    assert all(int(c) == -1 for c in bam_pileup.bam_index_ranges(path)["count"])
    check_members(same_as_off([path], tmp_path, 1, indexed=1), [path], [1])


def test_rejected_index_files(three, tmp_path):
    src, _ = three
    path = str(tmp_path / "three.bam")
    shutil.copy(src, path)
    for name, data in bad_indexes(path).items():
        open(path + ".bai", "wb").write(data)
        for route in ROUTES:
            _p0, f0 = pile([path], str(tmp_path / "off"), 1, inflate=route, index="off")
            _p1, f1 = pile([path], str(tmp_path / "auto"), 1, inflate=route, index="auto")
            index, rs = bam_pileup.bam_index_stats(), bam_pileup.bam_route_stats()
            assert f1 == f0, name
            assert (index["files_indexed"], index["files_full"], index["rejected"]) == (0, 1, 1), name
            assert rs["host_blocks"] + rs["device_blocks"] == full_read_members(path, route), name
            with pytest.raises(_lib.SecedoError) as e:
                pile([path], str(tmp_path / "req"), 1, inflate=route, index="require")
            assert e.value.code == _lib.E_INVALID_ARG and path in str(e.value) and "no usable index" in str(e.value)


def errors_agree(path, chromosome, tmp_path, needle):
    msgs = []
    for route in ROUTES:
        for mode in ("auto", "require"):
            with pytest.raises(_lib.SecedoError) as e:
                pile([path], str(tmp_path / "err"), chromosome, inflate=route, index=mode)
            assert e.value.code == _lib.E_INVALID_ARG
            msgs.append(str(e.value))
    assert len(set(msgs)) == 1 and needle in msgs[0], msgs
    return msgs[0]


def test_index_that_does_not_match(three, tmp_path):
    """the builders are those of tests/bam_index_cases.py, whose bytes test_bam_index_cpu.py walks on the host first"""
    src, _d = three
    path = str(tmp_path / "three.bam")
    shutil.copy(src, path)
    mismatch = path + ": index does not match the file ("
    # the index of another BAM with the same header and the same members
    mine_bytes, other_bytes = ic.other_bam_pair()
    mine_path, other = put(tmp_path, "mine.bam", mine_bytes), put(tmp_path, "other.bam", other_bytes)
    assert [m[0] for m in bi.member_table(mine_bytes)] == [m[0] for m in bi.member_table(other_bytes)]
    assert bi.ranges(mine_path)[1][0] != bi.ranges(other)[1][0] and bi.ranges(mine_path)[1][1] == bi.ranges(other)[1][1]
    shutil.copy(other + ".bai", mine_path + ".bai")
    m = errors_agree(mine_path, 1, tmp_path, mine_path + ": index does not match the file (")
    assert m.endswith("); re-index it or use --index off")
    # a start moved one record later (the pseudo-bin still counts all), an end moved one record earlier, a start that
    # is no record start
    indexes, mine = ic.moved_indexes(path)
    wants = {"start-later": "has %d records between its start and end, the index counts %d" % (len(mine) - 1, len(mine)),
             "end-earlier-no-pseudo-bin": "the record at the end of reference 1 still has its RefID",
             "end-earlier": "", "start-inside-a-record": ""}
    for name, want in wants.items():
        open(path + ".bai", "wb").write(indexes[name])
        assert want in errors_agree(path, 1, tmp_path, mismatch), name
    # and the untouched index reads the file
    open(path + ".bai", "wb").write(indexes["good"])
    same_as_off([path], tmp_path, 1, indexed=1)


def test_defects_inside_and_outside_a_span(tmp_path):
    """tests/bam_index_cases.py's defect_bams (walked on the host by test_bam_index_cpu.py first): a corrupt member and
    a bad block_size inside the requested span are reported alike by both routes; outside every span they are not seen"""
    bams = ic.defect_bams()
    good = put(tmp_path, "good.bam", bams["good"])
    index = open(good + ".bai", "rb").read()
    table = bi.member_table(bams["good"])
    assert bi.ranges(good)[1][0] >> 16 > table[5][0]  # members 3 and 5 lie in reference 0's span only

    def variant(name, data):
        path = put(tmp_path, name, data, index=False)
        open(path + ".bai", "wb").write(index)
        return path

    bad_member = variant("member.bam", bams["member"])
    errors_agree(bad_member, 0, tmp_path, "BGZF block at byte %d: " % table[ic.DEFECT_MEMBER][0])
    bad_size = variant("size.bam", bams["size"])
    errors_agree(bad_size, 0, tmp_path, "index does not match the file (the record chain breaks: indexed record "
                                        "%d has a bad block_size)" % ic.DEFECT_RECORD)
    # outside reference 1's span both go unseen, and with the index off they are reported
    for path in (bad_member, bad_size):
        for route in ROUTES:
            p1, f1 = pile([path], str(tmp_path / "in"), 1, inflate=route, index="require")
            p0, f0 = pile([good], str(tmp_path / "ok"), 1, inflate=route, index="off")
            assert f1 == f0 and len(f0[0]) > 0
            with pytest.raises(_lib.SecedoError):
                pile([path], str(tmp_path / "off"), 1, inflate=route, index="off")


def test_cli_and_environment(three, tmp_path):
    import subprocess
    import sys
    path, _ = three
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    env.pop("SECEDO_BAM_INDEX", None)
    base = [sys.executable, "-m", "secedo_amd.pileup_main", "-i", path, "--chromosomes", "2", "--min_base_quality", "20",
            "--min_map_quality", "0", "--min_different", "1"]
    outs = {}
    for name, extra, e in (("plain", [], {}), ("flag", ["--index", "require"], {}),
                           ("env", [], {"SECEDO_BAM_INDEX": "auto"})):
        o = str(tmp_path / name)
        r = subprocess.run(base + ["-o", o] + extra, env=dict(env, **e), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = [open("%s_2.pileup%s" % (o, ext), "rb").read() for ext in (".bin", ".map", ".txt")]
    assert outs["flag"] == outs["plain"] and outs["env"] == outs["plain"] and len(outs["plain"][0]) > 0
    code = ("import sys\nfrom secedo_amd import bam_pileup\n"
            "bam_pileup.pileup_bams([sys.argv[1]], None, False, 1, 100, 0, 0, 0, 1, 0)\n"
            "print(bam_pileup.bam_index_stats()['files_indexed'])\n")
    r = subprocess.run([sys.executable, "-c", code, path], env=dict(env, SECEDO_BAM_INDEX="auto"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and int(r.stdout.split()[-1]) == 1, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-c", code, path], env=dict(env, SECEDO_BAM_INDEX="yes"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "SECEDO_BAM_INDEX=yes: expected off, auto or require" in r.stderr
