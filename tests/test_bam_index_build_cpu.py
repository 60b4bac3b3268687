"""The BAI writer (secedo_amd/csrc/bam_index_build.hpp) and the index-building command lines, without a GPU: the host
builder under AddressSanitizer and UBSan (secedo_amd/csrc/build/bam_index_build_test) on what the device's index pass
would hand it for the six golden BAMs and the layout cases, whole and split at arbitrary range boundaries, against the
samtools-written indexes and tests/bai_expected.py; cut and empty inputs; the expected bytes themselves against the
goldens; and the command lines that are refused before torch is imported."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bai_expected as be
from tests import bai_writer as bi
from tests.golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_index_build_test")
BAM = os.path.join(GOLDEN, "bam")
GOLDENS = ["test1", "test2", "test3", "soft_clipping", "hard_clipping", "insert_at_end"]


def fx(name):
    return os.path.join(BAM, name + ".bam")


def program(*args):
    r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout


def built(tmp_path, text):
    """the builder's index for the input text -> (bytes, stats) or the rejection's reason"""
    (tmp_path / "in.txt").write_text(text)
    out = program("build", tmp_path / "in.txt", tmp_path / "out.bai")
    if out.startswith("rejected: "):
        return out[len("rejected: "):].strip()
    words = out.split()
    return (tmp_path / "out.bai").read_bytes(), dict(zip(words[0::2], (int(w) for w in words[1::2])))


@pytest.mark.parametrize("name", GOLDENS)
def test_expected_bytes_are_the_samtools_indexes(name):
    assert be.expected_bytes(fx(name)) == open(fx(name) + ".bai", "rb").read()


@pytest.mark.parametrize("name", GOLDENS)
def test_builder_gives_the_golden_indexes(name, tmp_path):
    want = open(fx(name) + ".bai", "rb").read()
    n = len(bi.layout(fx(name))[1])
    for cuts in ((), range(n), (n // 2,)):
        got, stats = built(tmp_path, be.builder_input(fx(name), cuts))
        assert got == want, (name, cuts)
        assert stats["bytes"] == len(want) and stats["joined"] == be.run_crossings(fx(name), cuts)


@pytest.mark.parametrize("how", sorted(be.LAYOUT_WRITERS))
def test_builder_gives_the_layout_cases(how, tmp_path):
    path = be.layout_bam(tmp_path, how)
    want = be.expected_bytes(path)
    n = len(bi.layout(path)[1])
    assert n > 900
    rng = np.random.default_rng(3)
    for cuts in ((), sorted(int(c) for c in rng.choice(n, 40, replace=False)), range(0, n, 7), range(n)):
        got, stats = built(tmp_path, be.builder_input(path, cuts))
        assert got == want, (how, list(cuts)[:5])
        assert stats["joined"] == be.run_crossings(path, cuts)
        assert not cuts or stats["joined"] > 0
    # the reader of bam_index.hpp restated reads the same ranges back
    got, own = bi.parse_ranges(want), bi.ranges(path)
    assert got[:3] == own[:3] and got[3] == (0, 0, -1) and own[3:4] == [(0, 0, 0)]  # no pseudo-bin without records


def test_layout_cases_hold_what_they_should(tmp_path):
    path = be.layout_bam(tmp_path, "cut-997")
    _table, recs, n_ref = bi.layout(path)
    on1 = [r for r in recs if r[0] == 1]
    windows = sorted({w for r in on1 for w in range(max(r[1], 0) >> 14, ((max(r[2], 1) - 1) >> 14) + 1)})
    assert n_ref == 4 and not [r for r in recs if r[0] == 3]
    assert any(b - a > 3 for a, b in zip(windows, windows[1:]))  # a gap the backward fill fills
    assert any(r[1] >> 14 != (r[2] - 1) >> 14 for r in on1) and any(r[1] >> 17 != (r[2] - 1) >> 17 for r in on1)
    assert sum(1 for r in on1 if r[5] & 4) == 1 and sum(1 for r in recs if r[0] < 0) == 5
    assert any(r[2] == r[1] + 1 and not r[5] & 4 for r in on1)  # the mapped record without a CIGAR
    want = be.expected_bytes(path)
    assert want != bi.bai_bytes(path)  # the fill direction shows


def test_builder_survives_cut_and_empty_inputs(tmp_path):
    """prefixes of a valid input, each parsed from a heap block of its exact size, and inputs that break the builder's
    rules: the program exits 0 only if no sanitizer reported"""
    path = be.layout_bam(tmp_path, "cut-997")
    text = be.builder_input(path, range(0, 1000, 50))
    (tmp_path / "in.txt").write_text(text)
    out = program("cuts", tmp_path / "in.txt", 97).split()
    assert int(out[1]) == 1 and int(out[3]) == (len(text) + 96) // 97
    (tmp_path / "small.txt").write_text(be.builder_input(fx("test1")))
    out = program("cuts", tmp_path / "small.txt", 1).split()
    assert int(out[1]) == 1 and int(out[3]) == os.path.getsize(tmp_path / "small.txt")
    assert built(tmp_path, "") == "no E line"
    assert built(tmp_path, "R 2\nE 0 0\n")[0] == b"BAI\1" + bytes([2, 0, 0, 0]) + bytes(16) + bytes(8)
    bad = {
        "ordinals": "R 1\nH 0 4681 0 100 5\nH 0 4682 0 200 5\nE 300 9\n",
        "refs": "R 2\nH 1 4681 0 100 0\nH 0 4681 0 200 1\nE 300 2\n",
        "ref-range": "R 1\nH 1 4681 0 100 0\nE 300 2\n",
        "bin": "R 1\nH 0 37450 0 100 0\nE 300 2\n",
        "window": "R 1\nH 0 4681 0 100 0\nW 0 32768 100\nE 300 2\n",
        "window-ref": "R 1\nH 0 4681 0 100 0\nW 1 0 100\nE 300 2\n",
        "orphan-window": "R 2\nH 0 4681 0 100 0\nW 1 0 100\nE 300 2\n",
        "count": "R 1\nH 0 4681 0 100 7\nE 300 7\n",
        "end": "R 1\nH 0 4681 0 100 0\nE 50 1\n",
        "past-total": "R 1\nM 0 0 10\nT 10 40\nH 0 4681 0 11 0\nE 10 1\n",
        "huge": "R 99999999999\n",
        "number": "R 1\nH 0 4681 0 1x0 0\nE 300 1\n",
    }
    for name, text in bad.items():
        assert isinstance(built(tmp_path, text), str), name
    # virtual offsets: the end of the data names the EOF member, else the file size
    got, _ = built(tmp_path, "R 1\nM 0 0 10\nM 30 10 0\nT 10 58\nH 0 4681 0 4 0\nW 0 0 4\nE 10 1\n")
    assert bi.parse_ranges(got) == [(4, 30 << 16, 1)]
    got, _ = built(tmp_path, "R 1\nM 0 0 10\nT 10 30\nH 0 4681 0 4 0\nW 0 0 4\nE 10 1\n")
    assert bi.parse_ranges(got) == [(4, 30 << 16, 1)]
    got, _ = built(tmp_path, "R 1\nM 0 0 10\nM 30 10 0\nM 58 10 7\nT 17 99\nH 0 4681 0 10 0\nW 0 0 10\nE 17 1\n")
    assert bi.parse_ranges(got) == [(58 << 16, 99 << 16, 1)]  # a boundary names the member that holds the next byte


def _cli(module, *args):
    code = ("import sys; from secedo_amd import %s as m\n"
            "try:\n    rc = m.main(sys.argv[1:])\nexcept SystemExit as e:\n"
            "    sys.stderr.write(str(e.code) + '\\n'); rc = 2\n"
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)" % module)
    return subprocess.run([sys.executable, "-c", code, *[str(a) for a in args]], capture_output=True, text=True,
                          timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))


def test_command_lines_are_checked_before_torch(tmp_path):
    bam = tmp_path / "m.bam"
    bam.write_bytes(open(fx("test1"), "rb").read())
    (tmp_path / "m.bam.bai").write_bytes(b"kept")
    for args, what in (((), "-i"), (("-i", tmp_path / "none.bam"), "does not exist"),
                       (("-i", bam, "--num_threads", "0"), "--num_threads"),
                       (("-i", bam, "--frobnicate"), "unrecognized"),
                       (("-i", bam), "m.bam.bai exists"), (("-i", tmp_path), "m.bam.bai exists")):
        p = _cli("index_main", *args)
        assert p.returncode == 2 and "torch imported" not in p.stderr and what in p.stderr, (args, p.stderr)
    assert (tmp_path / "m.bam.bai").read_bytes() == b"kept"
    empty = tmp_path / "empty"
    empty.mkdir()
    p = _cli("index_main", "-i", empty)
    assert p.returncode == 0 and "No BAM files" in p.stdout
    for args, what in ((("-i", bam, "-o", tmp_path / "o", "--build_index", "--index", "off"), "--index off"),
                       (("-i", tmp_path / "none", "-o", tmp_path / "o", "--build_index"), "does not exist"),
                       (("-i", bam, "-o", tmp_path / "o", "--build_index=yes"), "ignored explicit argument")):
        p = _cli("pileup_main", *args)
        assert p.returncode == 2 and "torch imported" not in p.stderr and what in p.stderr, (args, p.stderr)
    from secedo_amd import index_main, pileup_main
    assert pileup_main.parse_args(["-i", "x", "--build_index"]).build_index is True
    assert pileup_main.parse_args(["-i", "x"]).build_index is False
    assert pileup_main.is_bam(str(bam)) and not pileup_main.is_bam(str(tmp_path / "m.bam.bai"))
    assert index_main.input_files(str(tmp_path)) == [str(bam)]
