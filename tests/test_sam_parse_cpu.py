"""The SAM parser of secedo_amd/csrc/sam_parse.hpp without a GPU: tests/cpp/sam_parse_test.cpp runs it on the host under
ASan and UBSan (every line in a heap block of exactly its length, every record written into a block of exactly its
counted size) on every case of tests/sam_cases.py, and every number and byte it gives equals tests/sam_ref.py: the
newline count per vector, the line starts, (RefID, POS, size) per line, the error word and the records.

The restatement is checked on its own as well: against ``bw.encode_record`` where a case is made of ``bw.Rec``, against
the error word a case is built for, and its ``f`` values against the correctly rounded float32 in exact arithmetic."""
import os
import struct
import subprocess
from fractions import Fraction

import pytest

from tests import bam_writer as bw
from tests import sam_cases as sc
from tests import sam_ref as sr
from tests import sam_writer as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "sam_parse_test")


def case_bytes(c: sc.Case) -> bytes:
    out = struct.pack("<I", len(c.names))
    for n in c.names:
        out += struct.pack("<I", len(n)) + n.encode("latin-1")
    return out + bytes(c.selected) + struct.pack("<QBI", c.line_base, int(c.ends_file), len(c.text)) + c.text


def run_program(cases, tmp_path):
    """-> per case (count, start, [(ref, pos, size)], error word, lines written, records)."""
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(struct.pack("<I", len(cases)) + b"".join(case_bytes(c) for c in cases))
    r = subprocess.run([EXE, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout == "ok %d cases\n" % len(cases)
    raw, o, out = dst.read_bytes(), 0, []

    def take(fmt):
        nonlocal o
        v = struct.unpack_from(fmt, raw, o)
        o += struct.calcsize(fmt)
        return v

    for _ in cases:
        n16, = take("<I")
        cnt = list(take("<%dI" % n16))
        n_lines, = take("<I")
        start = list(take("<%dI" % (n_lines + 1)))
        info = [take("<iiQ") for _ in range(n_lines)]
        err, limit, n_bytes = take("<QIQ")
        out.append((cnt, start, info, err, limit, raw[o:o + n_bytes]))
        o += n_bytes
    assert o == len(raw)
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return dict(zip((c.name for c in sc.CASES), run_program(sc.CASES, tmp_path_factory.mktemp("sam_parse"))))


def expected(c: sc.Case):
    text = c.text
    padded = text + b"\0" * (-len(text) % 16)
    cnt = [padded[i:i + 16].count(b"\n") for i in range(0, len(padded), 16)]
    start = sr.split_lines(text, text.endswith(b"\n"))
    info, records, err = sr.parse_range(text, list(c.names), c.selected, c.line_base, c.ends_file)
    limit = len(info) if err == sr.NO_ERROR else (err >> 8) - c.line_base
    # the records of the lines below the first bad one
    n_written = sum(1 for _, _, size in info[:limit] if size)
    return cnt, start, info, err, limit, b"".join(records[:n_written])


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_host_parser_equals_the_restatement(results, name):
    c = sc.BY_NAME[name]
    got, want = results[name], expected(c)
    if c.error is not None:
        assert want[3] == c.error, "the restatement: line %d, code %d" % (want[3] >> 8, want[3] & 0xFF)
    parts = ("newline counts", "line starts", "RefID, POS, size", "error word", "lines written")
    for what, g, w in zip(parts, got, want):
        assert g == w, "%s (%s): %s" % (name, c.why, what)
    if got[5] != want[5]:  # name the first record that differs
        o = 0
        for k, (_, _, size) in enumerate(want[2][:want[4]]):
            assert got[5][o:o + size] == want[5][o:o + size], "%s (%s): the record of line %d: %r" % (
                name, c.why, k, c.text[want[1][k]:want[1][k + 1] - 1][:200])
            o += size
    assert got[5] == want[5]


def test_the_table_covers_what_it_claims():
    codes = {code for code, _, _ in sc.error_lines()}
    assert codes == set(range(1, 17))  # 17 needs a 2 GiB record
    assert max(len(c.text) for c in sc.CASES) > 130_000
    n_good = 0
    for c in sc.CASES:
        if c.product:
            info, records, err = sr.parse_range(c.text, list(c.names), c.selected, c.line_base, c.ends_file)
            assert err == sr.NO_ERROR, c.name
            n_good += sum(1 for ref, pos, size in info if size and pos >= 0)
    assert len(sc.product_lines()) == n_good > 150
    # the 300 names: one hash each, so no run of equal hashes is ever walked (see the module's docstring)
    many = sc.BY_NAME["300_sq"].names
    assert len({sc.fnv1a(n.encode()) for n in many}) == len(many) == 300


def test_restatement_equals_encode_record_on_the_covering_records():
    recs = sw.canonical(sc.covering_records())
    for ln, r in zip(sc.covering_lines(), recs):
        assert sr.parse_line(ln.decode("latin-1"), sc.NAMES) == bw.encode_record(r), r.name


def nearest_float32(text: str):
    """The float32 nearest to the decimal number, ties to even, in exact arithmetic -> (its bytes, whether a tie)."""
    x = Fraction(text.rstrip(".") if "e" not in text.lower() else text)
    sign, x = (0x80000000 if text.startswith("-") else 0), abs(x)
    lo, hi = 0, 0x7F800000  # bits of the largest float <= x, by bisection: the bits order as the values do
    value = lambda b: Fraction(2) ** 128 if b == 0x7F800000 else Fraction(  # noqa: E731
        struct.unpack("<f", struct.pack("<I", b))[0])  # 2^128: where the next float would be
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if value(mid) <= x:
            lo = mid
        else:
            hi = mid
    below, above = x - value(lo), value(hi) - x
    bits = lo if below < above or (below == above and lo % 2 == 0) else hi
    assert bits < 0x7F800000, "beyond the largest finite value"
    return struct.pack("<I", sign | bits), below == above


def test_restatement_floats_are_correctly_rounded():
    """Rounding the decimal text to double and then to float32 gives the correctly rounded float32 for every float of
    the table, the exact ties included."""
    ties = 0
    for what, text in sc.float_texts():
        got = sr.parse_aux("XF:f:" + text)[3:]
        assert (got, what.startswith("tie_")) == nearest_float32(text), (what, text)
        assert len(text.lstrip("+-0.").split("e")[0].split("E")[0].replace(".", "").rstrip("0")) <= 9, text
        ties += what.startswith("tie_")
    assert ties == 5 + 21
    for text, bits in (("2.65189e+08", 0x4D7CE768), ("16777217", 0x4B800000)):
        assert sr.parse_aux("XF:f:" + text)[3:] == struct.pack("<I", bits)
