"""The DEFLATE decoder of secedo_amd/csrc/bgzf_inflate.hpp on the host: the code the GPU kernel runs, built with g++
under AddressSanitizer and UBSan (secedo_amd/csrc/build/bgzf_inflate_test). Round trips equal zlib byte for byte;
corrupted members end in a status code or fail their ISIZE / CRC32 check, never in a crash or a hang. Also the CLI's
.sam.gz discovery and the plain-gzip refusal, both without torch."""
import gzip
import os
import subprocess
import sys

import pytest

from secedo_amd import pileup_main
from tests import bgzf_writer as gw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bgzf_inflate_test")
CASE_TIMEOUT = 120  # seconds per run of the executable; a valid 200 KB file takes well under one


def run(path, tmp_path):
    """-> (status codes per member, bytes of the members with status 0)"""
    out, status = str(tmp_path / "out.bin"), str(tmp_path / "status.txt")
    r = subprocess.run([EXE, str(path), out, status], capture_output=True, text=True, timeout=CASE_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [int(x) for x in open(status).read().split()], open(out, "rb").read()


def test_round_trips_equal_zlib(tmp_path):
    cases = gw.round_trip_files(tmp_path)
    names = [c[0] for c in cases]
    assert len([n for n in names if n.endswith(".bam")]) == 6
    for name, path, want in cases:
        assert gw.inflate_all(open(path, "rb").read()) == want, name
        status, got = run(path, tmp_path)
        assert set(status) <= {0}, (name, status)
        assert got == want, name


def test_block_types_are_what_the_cases_claim():
    """BTYPE of the first block: level 0 stored, Z_FIXED fixed, levels 1 and 9 dynamic."""
    text = gw.sam_like_text(200)
    btype = lambda payload: (payload[0] >> 1) & 3
    assert btype(gw.deflate(text, 0)) == 0
    assert btype(gw.deflate(text, 6, "fixed")) == 1
    assert btype(gw.deflate(text, 1)) == 2 and btype(gw.deflate(text, 9)) == 2


def test_corruptions_end_in_a_status(tmp_path):
    cases = gw.corruptions()
    assert len(cases) >= 300
    path = tmp_path / "corrupt.gz"
    path.write_bytes(b"".join(gw.member(p, crc, isize) for p, crc, isize, _ in cases))
    status, got = run(path, tmp_path)
    assert len(status) == len(cases)
    o, n_ok, n_crc = 0, 0, 0
    for k, ((payload, crc, isize, piece), st) in enumerate(zip(cases, status)):
        if st == 0:  # inflated, ISIZE and CRC32 right: then the bytes are the original's
            assert got[o:o + isize] == piece, k
            o += isize
            n_ok += 1
        else:
            n_crc += st == 13
        # no false alarm either: what zlib inflates to the original bytes passes here
        assert (st == 0) == gw.zlib_verdict(payload, piece), (k, st)
    assert o == len(got)
    assert n_crc > 0, "no flip landed in stored data: the CRC check went untested"
    assert n_ok < len(cases) // 4


def test_the_gpu_tests_corrupt_files_are_clean_here(tmp_path):
    """Every corrupt file tests/test_gpu_pileup_samgz.py gives the device: the first bad member is the one flipped,
    with the status class zlib gives it (CRC32 for stored data)."""
    head = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:1\tLN:3000000\n@CO\tc\n"
    lines = ["g\t67\t1\t11\t60\t4M\t=\t11\t0\tACGT\tIIII\n", "x\t67\t1\t21\t60\t4Q\t=\t21\t0\tACGT\tIIII\n"]
    lines += ["f%d\t67\t1\t%d\t60\t4M\t=\t%d\t0\tACGT\tIIII\n" % (k, 12 + k, 12 + k) for k in range(6000)]
    text = (head + "".join(lines)).encode()
    for how, k, raw in gw.corrupt_files(text):
        path = tmp_path / ("c_%s_%d.gz" % (how, k))
        path.write_bytes(raw)
        status, _ = run(path, tmp_path)
        bad = [i for i, st in enumerate(status) if st]
        assert bad and bad[0] == k, (how, k, bad)
        if how == "stored":
            assert status[k] == 13
        if how == "two":
            assert bad == [2, 7]


def test_input_files_falls_back_to_sam_gz(tmp_path):
    d = tmp_path / "gz"
    (d / "sub").mkdir(parents=True)
    for p in ("b_1.sam.gz", "sub/a_2.sam.gz", "notes.txt.gz", "c.gz"):
        (d / p).write_text("")
    want = sorted([str(d / "b_1.sam.gz"), str(d / "sub" / "a_2.sam.gz")])
    assert pileup_main.input_files(str(d)) == want
    assert pileup_main.cell_map_lines(want) == ["b\t0\n", "a\t1\n"]
    (d / "x_3.sam").write_text("")
    assert pileup_main.input_files(str(d)) == [str(d / "x_3.sam")]
    (d / "y_4.bam").write_text("")
    assert pileup_main.input_files(str(d)) == [str(d / "y_4.bam")]
    single = str(d / "b_1.sam.gz")
    assert pileup_main.input_files(single) == [single]


def test_help_names_sam_gz(capsys):
    with pytest.raises(SystemExit):
        pileup_main.parse_args(["--help"])
    assert ".sam.gz" in capsys.readouterr().out


def test_plain_gzip_refusal_is_unchanged_and_needs_no_torch(tmp_path):
    path = tmp_path / "x.sam.gz"
    path.write_bytes(gzip.compress(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:1\tLN:3000000\n"))
    code = ("import ctypes as C, sys\n"
            "l = C.CDLL(sys.argv[1]); l.secedo_bam_last_error.restype = C.c_char_p\n"
            "files = (C.c_char_p * 1)(sys.argv[2].encode()); ids = (C.c_uint32 * 1)(0)\n"
            "n, b = C.c_uint32(0), C.c_uint64(0)\n"
            "rc = l.secedo_bam_barcodes(files, 1, b'CB', ids, 1, 1, C.byref(n), C.byref(b))\n"
            "assert 'torch' not in sys.modules, 'torch imported'\n"
            "print(rc, l.secedo_bam_last_error().decode())\n")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "secedo_amd", "libsecedo_bam.so"), str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == ("-1 %s: a gzip file that is not BGZF; decompress it to SAM or convert it to BAM "
                                "(samtools view -b)" % path)
