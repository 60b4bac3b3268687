"""The record walk of secedo_amd/csrc/bam_walk.hpp on the host: the code the GPU kernels run, built with g++ under
AddressSanitizer and UBSan (secedo_amd/csrc/build/bam_walk_test). The speculative segment walk and the join give
exactly the record starts of a serial walk (written separately in the test program), for segments larger and smaller
than a record, and on corrupted bytes they give the serial walk's verdict without reading or writing out of bounds."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_device_cases as cases
from tests import bam_writer as bw
from tests import bgzf_writer as gw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_walk_test")
SEGMENTS = (65536, 4096, 1000, 37)  # the last two are smaller than a record
CASE_TIMEOUT = 120


def first_record(raw: bytes) -> int:
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    return o


def walk(tmp_path, raw: bytes, start: int, final=True, segments=SEGMENTS):
    """-> {segment bytes: (records, re-walked segments, code, stop offset)}; the program compares with its serial walk"""
    path = tmp_path / "bytes.bin"
    path.write_bytes(raw)
    r = subprocess.run([EXE, str(path), str(start), "1" if final else "0"] + [str(s) for s in segments],
                       capture_output=True, text=True, timeout=CASE_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        seg, n, rewalked, code, stop = (int(x) for x in line.split())
        out[seg] = (n, rewalked, code, stop)
    assert sorted(out) == sorted(segments)
    return out


def n_records(raw, start):
    n, o = 0, start
    while o < len(raw):
        o += 4 + struct.unpack_from("<i", raw, o)[0]
        n += 1
    return n


def random_stream(rng, n=1500, longest=6000):
    """Records with random sizes and random bytes behind block_size; some longer than several segments."""
    out = []
    for k in range(n):
        bs = int(rng.integers(32, 300)) if k % 50 else int(rng.integers(300, longest))
        out.append(struct.pack("<I", bs) + rng.integers(0, 256, bs, dtype=np.uint8).tobytes())
    return b"".join(out)


def test_golden_bams(tmp_path):
    bams = gw.golden_bams()
    assert len(bams) == 6
    for bam in bams:
        raw = gw.inflate_all(open(bam, "rb").read())
        start = first_record(raw)
        want = n_records(raw, start)
        for seg, (n, _, code, stop) in walk(tmp_path, raw, start).items():
            assert (n, code, stop) == (want, 0, len(raw)), (bam, seg)


def test_bam_writer_sets(tmp_path):
    for path in bw.synthetic_set(tmp_path, n_cells=3, pairs_per_cell=40, n_refs=2, seed=5):
        raw = gw.inflate_all(open(path, "rb").read())
        start = first_record(raw)
        got = walk(tmp_path, raw, start)
        assert {v[0] for v in got.values()} == {n_records(raw, start)}
        assert got[37][1] > 0 and got[1000][1] > 0  # segments inside records were joined by a walk of their own
        # the bytes cut inside the last record, as a range that is not the file's last: carried, no error
        cut = walk(tmp_path, raw[:-7], start, final=False)
        assert {v[2] for v in cut.values()} == {0} and {v[0] for v in cut.values()} == {n_records(raw, start) - 1}
        assert {v[2] for v in walk(tmp_path, raw[:-7], start).values()} != {0}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_streams(seed, tmp_path):
    rng = np.random.default_rng(seed)
    raw = random_stream(rng)
    got = walk(tmp_path, raw, 0)
    assert {v[:1] + v[2:] for v in got.values()} == {(1500, 0, len(raw))}
    assert got[37][1] > 1000 and got[65536][1] >= 1


def test_empty_and_tiny(tmp_path):
    assert {v[0] for v in walk(tmp_path, b"", 0).values()} == {0}
    one = struct.pack("<I", 32) + bytes(32)
    assert {v[:1] + v[2:] for v in walk(tmp_path, one, 0).values()} == {(1, 0, 36)}
    assert {v[2] for v in walk(tmp_path, one[:-1], 0).values()} == {1}  # truncated
    assert {v[2] for v in walk(tmp_path, one[:-1], 0, final=False).values()} == {0}


@pytest.mark.parametrize("seed", [11, 12])
def test_corruptions_give_the_serial_verdict(seed, tmp_path):
    """block_size fields overwritten with hostile values, and the bytes at the speculative starts overwritten with
    values that look like block sizes: the program aborts on any difference from its serial walk, the sanitizers on
    any access out of bounds."""
    rng = np.random.default_rng(seed)
    base = random_stream(rng, n=600, longest=3000)
    starts, o = [], 0
    while o < len(base):
        starts.append(o)
        o += 4 + struct.unpack_from("<I", base, o)[0]
    start_set = set(starts)
    hostile = [0, 31, 32, 33, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFDC, len(base), len(base) - 4]
    n_err = 0
    for k in range(40):
        raw = bytearray(base)
        at = starts[int(rng.integers(0, len(starts)))]
        v = hostile[k % len(hostile)] if k % 3 else int(rng.integers(0, 1 << 32))
        if k % 2:
            v = max(0, len(base) - at - 4 + int(rng.integers(-3, 4)))  # ends at, just before or just past the bytes
        raw[at:at + 4] = struct.pack("<I", v & 0xFFFFFFFF)
        for seg in SEGMENTS:  # what a wave reads first in a segment
            for s in range(seg, len(raw) - 4, seg * int(rng.integers(1, 9))):
                if s not in start_set:
                    raw[s:s + 4] = struct.pack("<I", int(rng.choice([32, 40, 100, len(base), 0xFFFFFFFF, 0])))
        for final in (True, False):
            got = walk(tmp_path, bytes(raw), 0, final)
            assert len({v[:1] + v[2:] for v in got.values()}) == 1  # every segment size the same verdict
            n_err += any(v[2] for v in got.values())
    assert n_err > 10


def test_the_gpu_tests_corrupt_bams_are_clean_here(tmp_path):
    """Every corrupt BAM tests/test_gpu_pileup_bam_device.py gives the device goes through the same decoder here
    first, under the sanitizers: the first bad member is the one flipped, CRC32 for stored data."""
    inflate = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bgzf_inflate_test")
    files = cases.corrupt_bams() + [("late", 3, cases.corrupt_with_record_error(2900)),
                                    ("early", 3, cases.corrupt_with_record_error(20))]
    assert len(files) == 11
    for how, k, data in files:
        path, status = tmp_path / ("c_%s_%d.bam" % (how, k)), tmp_path / "status.txt"
        path.write_bytes(data)
        r = subprocess.run([inflate, str(path), str(tmp_path / "out.bin"), str(status)], capture_output=True,
                           text=True, timeout=CASE_TIMEOUT)
        assert r.returncode == 0, (how, k, r.stderr[-2000:])
        codes = [int(x) for x in status.read_text().split()]
        bad = [i for i, st in enumerate(codes) if st]
        assert bad == [k], (how, k, bad)
        if how == "stored":
            assert codes[k] == 13
