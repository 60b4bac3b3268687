"""The layout of a batch of the BAM device route (secedo_amd/csrc/bam_batch.hpp), without a GPU, under AddressSanitizer
and UBSan (secedo_amd/csrc/build/bam_batch_test): where every kernel of the route reads and writes, from member tables
alone. The program's groups: files read in full (one member, a file with nothing but its carry, three files in a batch,
empty members, a later range behind a device carry), spans of indexed files (entered mid-member, in one range and in
three, with and without the tail check, beside a file read in full), the index build's per-file table, the 4 GiB
limit, the range cut of bgzf_members.hpp with and without the folded tail of empty members, and the words of a record
defect, which the host walk and the device walk share."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_batch_test")


def program(*args):
    r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("group", ["files", "spans", "index", "limits", "ranges", "words"])
def test_the_programs_own_checks(group):
    assert program(group).startswith("ok " + group)


def test_an_unknown_group_is_refused():
    r = subprocess.run([EXE, "nothing"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr
