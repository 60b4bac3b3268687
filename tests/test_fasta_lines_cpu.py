"""The line roles, the range carry and the contig assignment of secedo_amd/csrc/fasta_lines.hpp (what the device
route of the reference genome shares with the host), run as a host program under the address and undefined-behaviour
sanitizers (tests/cpp/fasta_lines_test.cpp) and compared with the restatement tests/variant_ref.py (Stream,
get_next_chromosome) and with the closed form of the roles: line 0 is a header; line i >= 1 is a header iff it starts
with '>' and line i - 1 is not one."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import fasta_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "secedo_amd", "csrc", "build", "fasta_lines_test")
N_CHR = 3
NEEDED = 2 * N_CHR + 1  # contigs the table keeps
RANGES = (1, 7, 64, 0)  # 0: the whole text


def _cases():
    rng = np.random.default_rng(20240)
    out = [(t, fc.vr.check_is_diploid(t)) for t in fc.QUIRKS.values()]
    out += [(fc.random_text(rng), False) for _ in range(2000)]
    out += [(fc.random_diploid_text(rng), True) for _ in range(500)]
    return out


CASES = _cases()


def _lines(text):
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def _closed_form(text):
    """-> (roles as a string of H / S, [(header_len, byte 1, seq_len)] of the first NEEDED contigs)"""
    roles, contigs = "", []
    for i, line in enumerate(_lines(text)):
        header = i == 0 or (line[:1] == b">" and roles[-1] != "H")
        roles += "H" if header else "S"
        if header:
            contigs.append([len(line), line[1] if len(line) > 1 else 0, 0])
        else:
            contigs[-1][2] += len(line)
    return roles, [tuple(c) for c in contigs[:NEEDED]]


def _expected(text):
    roles, contigs = _closed_form(text)
    head = "R %s | C%s" % (roles, "".join(" %d:%d:%d" % c for c in contigs))
    chroms = fc.restated(text, N_CHR)
    if isinstance(chroms, str):
        return head, chroms
    return head + " | G " + "".join("".join(chr(48 + g) for g in c) + ";" for c in chroms), None


EXPECTED = [_expected(t) for t, _ in CASES]


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("fasta_lines") / "cases.bin"
    with open(path, "wb") as f:
        for text, diploid in CASES:
            f.write(struct.pack("<IB", len(text), int(diploid)) + text)
    return str(path)


def _run(cases_file, rng_size, chunk):
    assert os.path.exists(PROGRAM), "build it with `make -C secedo_amd/csrc`"
    res = subprocess.run([PROGRAM, cases_file, str(rng_size), str(chunk), str(N_CHR)], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode(errors="replace")[-2000:]
    return res.stdout.decode("latin-1").split("\n")[:-1]


@pytest.mark.parametrize("chunk", [16, 3])
@pytest.mark.parametrize("range_size", RANGES)
def test_roles_contigs_and_assignment(cases_file, range_size, chunk):
    got = _run(cases_file, range_size, chunk)
    assert len(got) == len(CASES)
    for (text, _), line, (want, err) in zip(CASES, got, EXPECTED):
        if err is None:
            assert line == want, text
            continue
        head, _, message = line.partition(" | E ")
        assert head == want, text
        if err == "empty line":
            assert message == "reference genome: empty line where a contig header is expected", text
        else:
            assert message.startswith("Invalid reference genome. Maternal and paternal chromosome sizes don't match ("), text


def test_the_errors_stay_a_minority():
    random_cases = EXPECTED[len(fc.QUIRKS):]
    errors = sum(1 for _, err in random_cases if err is not None)
    assert 0 < errors <= len(random_cases) // 4, errors
