"""Record selection of ``pileup_bams`` without a GPU: the Python restatement of the flag filter and the duplicate
rules (tests/bam_select_ref.py) against an example worked out by hand, the parsing of flag masks, and the CLI's
validation of its three options before torch is imported."""
import os
import subprocess
import sys

import pytest

from secedo_amd import _lib, bam_pileup, pileup_main, sam_flags
from tests import bam_select_ref as sel
from tests import bam_writer as bw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_five_prime_ends_and_scores():
    F, R = 0x43, 0x93
    r = lambda cigar, flag, pos=1000: bw.Rec("x", 0, pos, cigar, "*", flag=flag)  # noqa: E731
    assert sel.five_prime(r([("M", 50)], F)) == (1000, 0)
    assert sel.five_prime(r([("S", 5), ("M", 45)], F, 1005)) == (1000, 0)
    assert sel.five_prime(r([("H", 3), ("M", 47)], F)) == (997, 0)
    assert sel.five_prime(r([("H", 2), ("S", 3), ("M", 45)], F, 3)) == (-2, 0)  # u is signed
    assert sel.five_prime(r([("M", 50)], R, 1200)) == (1249, 1)
    assert sel.five_prime(r([("M", 40), ("S", 10)], R, 1200)) == (1249, 1)
    assert sel.five_prime(r([("S", 9), ("M", 20), ("D", 5), ("I", 4), ("N", 10), ("=", 3), ("X", 2), ("S", 4),
                             ("H", 6)], R, 100)) == (100 + 40 - 1 + 10, 1)
    assert sel.score(bw.Rec("x", 0, 0, [("M", 4)], "ACGT", qual=[14, 15, 40, 0xFF])) == 55
    assert sel.score(bw.Rec("x", 0, 0, [("M", 4)], "ACGT", qual=None)) == 0


def test_worked_example():
    """T1 kept over T2 (same ends through the clips, score 3000 against 2700); T3 is T1 in another cell; the singles
    T4..T7 are not compared with pairs, T6 loses its tie with T4 to the ordinal; T8 has three records."""
    refs, files, want, want_stats = sel.worked_example()
    a = files[0]
    t2 = [r for r in a if r.name == "T2"]
    assert sorted(sel.five_prime(r) for r in t2) == [(1000, 0), (1249, 1)]
    assert sorted(sel.five_prime(r) for r in a if r.name == "T1") == [(1000, 0), (1249, 1)]
    assert sum(sel.score(r) for r in t2) == 2700 and sum(sel.score(r) for r in a if r.name == "T1") == 3000
    assert [r.name for r in a if r.name in ("T4", "T6")] == ["T4", "T6"]
    dropped, stats = sel.select(files, 0, remove_duplicates=True)
    assert dropped == want and {(f, files[f][k].name) for f, k in dropped} == {(0, "T2"), (0, "T6")}
    assert stats == want_stats
    assert sel.select(files, 0) == (set(), dict.fromkeys(sel.STAT_KEYS, 0))
    assert sel.select(files, 1, remove_duplicates=True)[0] == set()  # another chromosome
    kept = sel.without(files, dropped)
    assert [len(k) for k in kept] == [len(a) - 3, 2]
    assert sel.select(kept, 0, remove_duplicates=True)[0] == set()  # nothing more to drop


def test_filter_restatement_counts_require_first():
    recs = [bw.Rec("a", 0, 1, [("M", 1)], "A", qual=[30], flag=0x3),
            bw.Rec("b", 0, 2, [("M", 1)], "A", qual=[30], flag=0x1 | 0x400),  # fails both: counted under require
            bw.Rec("c", 0, 3, [("M", 1)], "A", qual=[30], flag=0x3 | 0x400),
            bw.Rec("d", 1, 3, [("M", 1)], "A", qual=[30], flag=0x0)]
    dropped, stats = sel.select([recs], 0, require=3, exclude=0x400)
    assert dropped == {(0, 1), (0, 2)}
    assert (stats["records"], stats["dropped_require"], stats["dropped_exclude"]) == (3, 1, 1)
    # a pair whose mate the filter removed is a single, and duplicates another single
    F = 0x43
    recs = [bw.Rec("p", 0, 10, [("M", 2)], "AC", qual=[30, 30], flag=F),
            bw.Rec("p", 0, 50, [("M", 2)], "AC", qual=[30, 30], flag=0x93 | 0x400),
            bw.Rec("s", 0, 10, [("M", 2)], "AC", qual=[30, 31], flag=F)]
    dropped, stats = sel.select([recs], 0, exclude=0x400, remove_duplicates=True)
    assert dropped == {(0, 1), (0, 0)} and stats["duplicate_records"] == 1 and stats["templates"] == 2


def test_flag_parsing():
    p = sam_flags.parse_flags
    assert p(3) == 3 and p("3") == 3 and p("0xF04") == 0xF04 and p("0Xf04") == 0xF04 and p("3844") == 0xF04
    assert p("SECONDARY,SUPPLEMENTARY,DUP,QCFAIL,UNMAP") == 0xF04 and p(" paired , Proper_Pair ") == 3
    assert p("QCFAIL") == 0x200 and p(None) == 0 and p(0xFFFF) == 0xFFFF
    assert [sam_flags.FLAG_NAMES[n] for n in ("PAIRED", "PROPER_PAIR", "UNMAP", "MUNMAP", "REVERSE", "MREVERSE",
                                              "READ1", "READ2", "SECONDARY", "QCFAIL", "DUP", "SUPPLEMENTARY")] == \
        [1 << k for k in range(12)]
    for bad in ("DUPLICATE", "DUP,", "", "0x", "0x10000", 65536, -1, "1.5", "DUP|UNMAP", True):
        with pytest.raises(ValueError):
            p(bad)
    assert sam_flags.parse_filter("3", "0xF04") == (3, 0xF04) and sam_flags.parse_filter(None, "DUP") == (0, 0x400)
    with pytest.raises(ValueError, match="share"):
        sam_flags.parse_filter("PAIRED,DUP", "DUP")


def test_python_keywords_are_checked_before_any_file_is_read():
    calls = (lambda: bam_pileup.pileup_bams(["/nonexistent.bam"], None, False, 0, 100, 0, 0, 0, 1, 0,
                                            exclude_flags="DUPE"),
             lambda: bam_pileup.pileup_bams(["/nonexistent.bam"], None, False, 0, 100, 0, 0, 0, 1, 0,
                                            require_flags=0x401, exclude_flags=0x400),
             lambda: bam_pileup.bam_barcodes(["/nonexistent.bam"], "CB", [0], require_flags=1 << 16))
    for call in calls:
        with pytest.raises(_lib.SecedoError) as e:
            call()
        assert e.value.code == _lib.E_INVALID_ARG and "nonexistent" not in str(e.value)


def _cli(*args):
    code = ("import sys; from secedo_amd import pileup_main as m\n"
            "try:\n    rc = m.main(sys.argv[1:])\nexcept SystemExit as e:\n    print(e, file=sys.stderr); rc = 2\n"
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)")
    return subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli_options_are_checked_before_torch(tmp_path):
    bam = tmp_path / "m.bam"
    bw.write_bam(str(bam), [("1", 100)], [])
    base = ["-i", str(bam), "-o", str(tmp_path / "o")]
    for extra, what in ((["--exclude_flags", "DUPLICATE"], "unknown flag 'DUPLICATE'"),
                        (["--require_flags", "0x10000"], "outside 0..0xFFFF"),
                        (["--require_flags", "3", "--exclude_flags", "PROPER_PAIR,DUP"], "share bits 0x2")):
        p = _cli(*base, *extra)
        assert p.returncode == 2 and "torch imported" not in p.stderr and what in p.stderr, p.stderr
    a = pileup_main.parse_args(base + ["--require_flags", "3", "--exclude_flags", "SECONDARY,DUP", "--remove_duplicates"])
    pileup_main.check_select_flags(a)
    assert (a.require_flags, a.exclude_flags, a.remove_duplicates) == (3, 0x500, True)
    a = pileup_main.parse_args(base)
    pileup_main.check_select_flags(a)
    assert (a.require_flags, a.exclude_flags, a.remove_duplicates) == (None, None, None)


def _getters(env):
    code = ("import ctypes as C\nfrom secedo_amd import bam_pileup\nl = bam_pileup.lib()\n"
            "rq, ex, m = C.c_uint32(9), C.c_uint32(9), C.c_int(9)\n"
            "print(l.secedo_bam_get_read_filter(C.byref(rq), C.byref(ex)), rq.value, ex.value,"
            " l.secedo_bam_get_duplicates(C.byref(m)), m.value)")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, **env))
    assert p.returncode == 0, p.stderr
    return [int(x) for x in p.stdout.split()]


def test_environment_decides_until_a_setter_is_called():
    assert _getters({}) == [_lib.OK, 0, 0, _lib.OK, 0]
    assert _getters({"SECEDO_BAM_REQUIRE_FLAGS": "3", "SECEDO_BAM_EXCLUDE_FLAGS": "0xF04",
                     "SECEDO_BAM_DUPLICATES": "remove"}) == [_lib.OK, 3, 0xF04, _lib.OK, 1]
    assert _getters({"SECEDO_BAM_REQUIRE_FLAGS": "3", "SECEDO_BAM_EXCLUDE_FLAGS": "2"})[0] == _lib.E_INVALID_ARG
    bad = _getters({"SECEDO_BAM_REQUIRE_FLAGS": "DUP", "SECEDO_BAM_DUPLICATES": "mark"})  # the C side reads numbers
    assert bad[0] == _lib.E_INVALID_ARG and bad[3] == _lib.E_INVALID_ARG


def test_setters_refuse_what_no_record_could_pass():
    import ctypes as C
    lib = bam_pileup.lib()
    rq, ex, mode = C.c_uint32(7), C.c_uint32(7), C.c_int(7)
    assert lib.secedo_bam_get_read_filter(C.byref(rq), C.byref(ex)) == _lib.OK
    assert lib.secedo_bam_get_duplicates(C.byref(mode)) == _lib.OK
    before = (rq.value, ex.value, mode.value)
    assert lib.secedo_bam_set_read_filter(0x401, 0x400) == _lib.E_INVALID_ARG
    assert lib.secedo_bam_set_read_filter(0, 0x10000) == _lib.E_INVALID_ARG
    assert lib.secedo_bam_set_duplicates(-1) == _lib.E_INVALID_ARG
    assert lib.secedo_bam_get_read_filter(C.byref(rq), C.byref(ex)) == _lib.OK
    assert lib.secedo_bam_get_duplicates(C.byref(mode)) == _lib.OK
    assert (rq.value, ex.value, mode.value) == before
    assert set(bam_pileup.bam_select_stats()) == set(sel.STAT_KEYS)
