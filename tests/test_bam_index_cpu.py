"""The BAI reader (secedo_amd/csrc/bam_index.hpp) and the index switch, without a GPU: the ranges of the six golden
indexes against what the BAMs themselves say, the test writer (tests/bai_writer.py) against the goldens, the reader
under AddressSanitizer and UBSan on cut and mutated indexes (secedo_amd/csrc/build/bam_index_test), the ranges through
the library, the environment variable, the CLI flag, and the hostile BAMs and indexes of
tests/test_gpu_pileup_bam_index.py through bgzf_inflate_test, bam_walk_test and bam_index_test before a GPU sees them."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from secedo_amd import _lib, bam_pileup
from tests import bai_writer as bi
from tests import bam_index_cases as ic
from tests import bam_writer as bw
from tests.golden_util import GOLDEN
from tests.test_bam_walk_cpu import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_index_test")
BAM = os.path.join(GOLDEN, "bam")
GOLDENS = ["test1", "test2", "test3", "soft_clipping", "hard_clipping", "insert_at_end"]


def fx(name):
    return os.path.join(BAM, name + ".bam")


def program(*args):
    r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout


def program_ranges(index, bam=None, n_ref=None):
    """-> [(start, end, count)] or the rejection's reason (str)"""
    out = program("ranges", index, *([] if bam is None else [bam, n_ref]))
    if out.startswith("rejected: "):
        return out[len("rejected: "):].strip()
    res = []
    for line in out.splitlines():
        _ref, _r, beg, end, count = line.split()
        v = [int(c) << 16 | int(u) for c, u in (x.split(":") for x in (beg, end))]
        res.append((v[0], v[1], int(count)))
    return res


def test_test1_is_the_documented_example():
    assert bi.ranges(fx("test1")) == [(214 << 16, 311 << 16, 2)]


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_index_ranges_are_what_the_bam_says(name):
    """start = the virtual offset of the first record, end = the one behind the last, count = the records: each
    derived from the BAM alone (bam_writer.read_bam and the member table)"""
    want = bi.ranges(fx(name))
    n_ref = len(bw.read_bam(fx(name))[0])
    assert program_ranges(fx(name) + ".bai", fx(name), n_ref) == want
    assert bi.parse_ranges(open(fx(name) + ".bai", "rb").read()) == want
    got = bam_pileup.bam_index_ranges(fx(name))
    assert [(int(s), int(e), int(c)) for s, e, c in zip(got["start"], got["end"], got["count"])] == want


@pytest.mark.parametrize("name", GOLDENS)
def test_writer_gives_the_golden_ranges(name, tmp_path):
    for pseudo in (True, False):
        out = bi.write_bai(fx(name), str(tmp_path / ("%s_%d.bai" % (name, pseudo))), pseudo_bin=pseudo)
        want = [(s, e, c if pseudo else -1) for s, e, c in bi.ranges(fx(name))]
        assert program_ranges(out) == want
        assert bi.parse_ranges(open(out, "rb").read()) == want


def three_refs(path, n=60, empty_ref=True):
    refs = [("1", 100000), ("2", 100000), ("3", 100000)] + ([("4", 100000)] if empty_ref else [])
    recs = [bw.Rec("r%d_%d" % (ref, k), ref, 100 + 37 * k, [("M", 8)], "ACGTACGT", qual=[40] * 8)
            for ref in range(3) for k in range(n)]
    recs.append(bw.Rec("un", -1, -1, [], "ACGT", qual=[30] * 4, flag=0x4))
    bw.write_bam(str(path), refs, recs)
    return refs, recs


def test_multi_reference_ranges_and_empty_reference(tmp_path):
    bam = tmp_path / "three.bam"
    three_refs(bam)
    bi.write_bai(bam)
    want = bi.ranges(str(bam))
    assert want[3] == (0, 0, 0) and all(w[2] == 60 for w in want[:3])
    assert want[0][1] == want[1][0] and want[1][1] == want[2][0]  # one reference ends where the next starts
    got = program_ranges(str(bam) + ".bai", bam, 4)
    assert got[:3] == want[:3] and got[3][:2] == (0, 0)
    lib = bam_pileup.bam_index_ranges(str(bam))
    assert [int(x) for x in lib["start"]] == [w[0] for w in want]
    assert [int(x) for x in lib["end"]] == [w[1] for w in want]
    # <path without .bam>.bai is found too
    os.rename(str(bam) + ".bai", str(tmp_path / "three.bai"))
    assert [int(x) for x in bam_pileup.bam_index_ranges(str(bam))["start"]] == [w[0] for w in want]


def bad_indexes(bam):
    """-> {name: index bytes} that fail a file-level check against ``bam``"""
    good = bi.bai_bytes(str(bam))
    size = os.path.getsize(str(bam))
    first_chunk = 8 + 4 + 8  # n_bin, then bin and n_chunk of the first bin of reference 0
    beg = struct.unpack_from("<Q", good, first_chunk)[0]
    put = lambda v: good[:first_chunk] + struct.pack("<Q", v) + good[first_chunk + 8:]  # noqa: E731
    return {
        "magic": b"BAJ\1" + good[4:],
        "truncated": good[:len(good) // 2],
        "n_ref": good[:4] + struct.pack("<i", struct.unpack_from("<i", good, 4)[0] + 1) + good[8:] + b"\0" * 8,
        "past-the-file": put((size + 5) << 16),
        "not-a-member": put(((beg >> 16) + 1) << 16),
    }


def test_file_level_checks(tmp_path):
    bam = tmp_path / "three.bam"
    three_refs(bam, empty_ref=False)
    for name, data in bad_indexes(bam).items():
        (tmp_path / "bad.bai").write_bytes(data)
        why = program_ranges(tmp_path / "bad.bai", bam, 3)
        assert isinstance(why, str), (name, why)
        open(str(bam) + ".bai", "wb").write(data)
        with pytest.raises(_lib.SecedoError) as e:
            bam_pileup.bam_index_ranges(str(bam))
        assert e.value.code == _lib.E_INVALID_ARG and "no usable index" in str(e.value) and why in str(e.value), name
    os.remove(str(bam) + ".bai")
    with pytest.raises(_lib.SecedoError) as e:
        bam_pileup.bam_index_ranges(str(bam))
    assert "no index file" in str(e.value)


def test_reader_survives_cut_and_mutated_indexes(tmp_path):
    """every prefix of the index and seeded random mutations, each parsed from a heap block of its exact size: the
    program exits 0 only if no sanitizer reported"""
    bam = tmp_path / "three.bam"
    three_refs(bam)
    index = bi.write_bai(bam)
    out = program("mutate", index, bam, 4, 11, 4000).split()
    parsed, rejected = int(out[1]), int(out[3])
    assert parsed + rejected == os.path.getsize(index) + 1 + 4000
    assert rejected > 1000 and parsed > 0
    for name in GOLDENS:
        program("mutate", fx(name) + ".bai", fx(name), 1, 3, 500)
    # counts that would size an allocation: n_ref, n_bin, n_chunk and n_intv of 2^31 - 1 and 2^32 - 1
    good = open(index, "rb").read()
    for at in (4, 8, 16):
        for v in (0x7FFFFFFF, 0xFFFFFFFF):
            (tmp_path / "huge.bai").write_bytes(good[:at] + struct.pack("<I", v) + good[at + 4:])
            assert isinstance(program_ranges(tmp_path / "huge.bai"), str)


def test_environment_and_setter():
    """SECEDO_BAM_INDEX is read at every call until secedo_bam_set_index is called; an unknown value is an error"""
    code = ("import ctypes as C, os, sys\n"
            "l = C.CDLL(sys.argv[1]); l.secedo_bam_last_error.restype = C.c_char_p; m = C.c_int(-1)\n"
            "for v in ('', 'off', 'auto', 'require', 'yes', 'auto'):\n"
            "    os.environ['SECEDO_BAM_INDEX'] = v\n"
            "    rc = l.secedo_bam_get_index(C.byref(m))\n"
            "    print(v or '-', rc, m.value, l.secedo_bam_last_error().decode() if rc else '')\n"
            "print('set', l.secedo_bam_set_index(7), l.secedo_bam_set_index(2))\n"
            "os.environ['SECEDO_BAM_INDEX'] = 'yes'\n"
            "print('after', l.secedo_bam_get_index(C.byref(m)), m.value)\n")
    r = subprocess.run([sys.executable, "-c", code, bam_pileup.LIB_PATH], capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k != "SECEDO_BAM_INDEX"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert [l.split()[:3] for l in lines[:4]] == [["-", "0", "0"], ["off", "0", "0"], ["auto", "0", "1"],
                                                  ["require", "0", "2"]]
    assert lines[4].split()[1] == str(_lib.E_INVALID_ARG)
    assert "SECEDO_BAM_INDEX=yes: expected off, auto or require" in lines[4]
    assert lines[5].split()[:3] == ["auto", "0", "1"]
    assert lines[6].split() == ["set", str(_lib.E_INVALID_ARG), "0"]
    assert lines[7].split() == ["after", "0", "2"]


def test_python_keyword_is_checked_before_any_file_is_read():
    for call in (lambda: bam_pileup.pileup_bams(["/nonexistent.bam"], None, False, 0, 100, 0, 0, 0, 1, 0, index="on"),
                 lambda: bam_pileup.bam_barcodes(["/nonexistent.bam"], "CB", [0], index="on"),
                 lambda: bam_pileup.set_index("on")):
        with pytest.raises(_lib.SecedoError) as e:
            call()
        assert e.value.code == _lib.E_INVALID_ARG and "'off', 'auto' or 'require'" in str(e.value)
    assert set(bam_pileup.bam_index_stats()) == {"files_indexed", "files_full", "rejected", "spans", "members",
                                                 "members_skipped"}


def test_cli_flag_is_checked_before_torch(tmp_path):
    code = ("import sys; from secedo_amd import pileup_main as m\n"
            "try:\n    rc = m.main(sys.argv[1:])\nexcept SystemExit as e:\n    rc = 2\n"
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)")
    bam = tmp_path / "m.bam"
    bw.write_bam(str(bam), [("1", 100)], [])
    p = subprocess.run([sys.executable, "-c", code, "-i", str(bam), "-o", str(tmp_path / "o"), "--index", "always"],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert p.returncode == 2 and "torch imported" not in p.stderr and "invalid choice: 'always'" in p.stderr, p.stderr
    from secedo_amd import pileup_main
    assert pileup_main.parse_args(["-i", "x", "--index", "require"]).index == "require"
    assert pileup_main.parse_args(["-i", "x"]).index is None


# ---- the hostile inputs of tests/test_gpu_pileup_bam_index.py, on the host first (tests/bam_index_cases.py builds both)

def _inflate_statuses(tmp_path, data: bytes):
    """the BGZF bytes through secedo_amd/csrc/build/bgzf_inflate_test -> the status of every member"""
    exe = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bgzf_inflate_test")
    path, status = tmp_path / "in.bam", tmp_path / "status.txt"
    path.write_bytes(data)
    r = subprocess.run([exe, str(path), str(tmp_path / "out.bin"), str(status)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return [int(x) for x in status.read_text().split()]


def test_the_gpu_tests_hostile_bams_inflate_clean_here(tmp_path):
    """every BAM the index tests give a GPU with a defect in it, or with an index that does not fit, through the
    decoder the device runs, under the sanitizers: only the flipped member is bad (CRC32, the data is stored)"""
    bams = ic.defect_bams()
    mine, other = ic.other_bam_pair()
    for name, data in (("good", bams["good"]), ("size", bams["size"]), ("mine", mine), ("other", other),
                       ("three", ic.three_bam())):
        assert not any(_inflate_statuses(tmp_path, data)), name
    codes = _inflate_statuses(tmp_path, bams["member"])
    assert [k for k, c in enumerate(codes) if c] == [ic.DEFECT_MEMBER] and codes[ic.DEFECT_MEMBER] == 13


def test_the_gpu_tests_spans_walk_clean_here(tmp_path):
    """The bytes of every span those tests make the device walk, from the index's entry to its limit, through the
    segment walk and join of bam_walk.hpp under the sanitizers (bam_walk_test compares each with its serial walk):
    a span of a fitting index lands on its limit; a bad block_size, a start inside a record and another BAM's index
    give the serial walk's verdict without a read out of bounds."""
    bams = ic.defect_bams()
    good = ic.put(tmp_path, "good.bam", bams["good"])
    index = open(good + ".bai", "rb").read()
    assert program_ranges(good + ".bai", good, 2) == bi.ranges(good)
    # the good file: both references' spans are whole chains
    for c in (0, 1):
        raw, entry, limit, _starts = ic.span_of(bams["good"], index, c)
        n = bi.ranges(good)[c][2]
        assert {v[:1] + v[2:] for v in walk(tmp_path, raw[:limit], entry).values()} == {(n, 0, limit)}
    # block_size 31 in record 700: the chain breaks there, code kErrBlockSize
    raw, entry, limit, _starts = ic.span_of(bams["size"], index, 0)
    got = walk(tmp_path, raw[:limit], entry)
    assert {(v[0], v[2]) for v in got.values()} == {(ic.DEFECT_RECORD, 2)}
    # the flipped member: the device ends the span's bytes at that member's start and carries the cut record
    raw, entry, limit, starts = ic.span_of(bams["member"], index, 0)
    got = walk(tmp_path, raw[:starts[ic.DEFECT_MEMBER]], entry, final=False)
    assert {v[2] for v in got.values()} == {0}
    # indexes that are off by a record or enter inside one, and the index of another BAM
    three = ic.put(tmp_path, "three.bam", ic.three_bam())
    data = open(three, "rb").read()
    indexes, mine = ic.moved_indexes(three)
    verdicts = {}
    for name, idx in indexes.items():
        (tmp_path / "moved.bai").write_bytes(idx)
        assert not isinstance(program_ranges(tmp_path / "moved.bai", three, 4), str), name  # passes the file checks
        raw, entry, limit, _starts = ic.span_of(data, idx, 1)
        got = walk(tmp_path, raw[:limit], entry)
        assert len({v[:1] + v[2:] for v in got.values()}) == 1, name  # every segment size the same verdict
        verdicts[name] = next(iter(got.values()))
    assert verdicts["good"][0] == len(mine) and verdicts["good"][2] == 0
    assert verdicts["start-later"][0] == len(mine) - 1 and verdicts["end-earlier"][0] == len(mine) - 1
    mine_bam, other_bam = ic.other_bam_pair()
    other = ic.put(tmp_path, "other.bam", other_bam)
    raw, entry, limit, _starts = ic.span_of(mine_bam, open(other + ".bai", "rb").read(), 1)
    got = walk(tmp_path, raw[:limit], entry)
    assert len({v[:1] + v[2:] for v in got.values()}) == 1
