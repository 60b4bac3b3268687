"""The host code every BGZF reader shares (secedo_amd/csrc/bgzf_members.hpp), without a GPU, under AddressSanitizer and
UBSan (secedo_amd/csrc/build/bgzf_members_test): the member list of every golden BAM against the table Python makes of
the file's bytes, and the program's own groups of checks: the small files, the cut and mutated files, the payload span
and the descriptors of a range, the writers' member cuts of an extent, the words of a member that does not inflate, and
the zlib inflate of one member."""
import os
import struct
import subprocess

import pytest

from tests import bai_writer as bi
from tests import bgzf_writer as gw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bgzf_members_test")


def program(*args):
    r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout


def python_table(data: bytes):
    """-> [(coff, payload offset, clen, crc, isize, out)] from bai_writer.member_table and the file's bytes"""
    out = []
    for coff, size, isize, lin in bi.member_table(data):
        xlen = struct.unpack_from("<H", data, coff + 10)[0]
        crc, isize_field = struct.unpack_from("<II", data, coff + size - 8)
        assert isize_field == isize
        out.append((coff, 12 + xlen, size - 12 - xlen - 8, crc, isize, lin))
    return out


def listed(path):
    """-> (total, [(coff, payload offset, clen, crc, isize, out)]) or the refusal's words (str)"""
    lines = program("list", path).splitlines()
    if lines[0].startswith("rejected: "):
        return lines[0][len("rejected: "):]
    assert lines[0].startswith("total ")
    return int(lines[0].split()[1]), [tuple(int(x) for x in line.split()[1:]) for line in lines[1:]]


@pytest.mark.parametrize("bam", gw.golden_bams(), ids=os.path.basename)
def test_golden_bams_list_as_python_walks_them(bam):
    data = open(bam, "rb").read()
    want = python_table(data)
    assert len(want) >= 2 and want[-1][2:5] == (2, 0, 0)  # htslib ends a file with the empty member
    assert listed(bam) == (len(gw.inflate_all(data)), want)


def test_the_test_writers_files_and_the_three_refusals(tmp_path):
    raw = gw.bgzf(gw.sam_like_text(300), chunk=4096)
    path = tmp_path / "f.gz"
    path.write_bytes(raw)
    assert listed(path) == (len(gw.inflate_all(raw)), python_table(raw))
    for _name, data, tail in gw.listing_damage(raw):
        path.write_bytes(data)
        assert ": " + listed(path) == tail


@pytest.mark.parametrize("group", ["small", "hostile", "span", "cuts", "words", "inflate"])
def test_the_programs_own_checks(group):
    assert program(group).startswith("ok " + group)
