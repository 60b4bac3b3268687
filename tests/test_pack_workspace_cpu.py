"""The workspace of the device packing (secedo_amd/csrc/pack_workspace.hpp) on the host: every generation of every
arena carved over a malloc block of exactly the computed size, built with g++ under AddressSanitizer and UBSan
(secedo_amd/csrc/build/pack_workspace_test, tests/cpp/pack_workspace_test.cpp). The program checks that the views lie
inside their arenas one behind the other, are aligned for their element types and can be written at both ends, that the
cleared prefix of MISC is the scalars and the three id tables, and that FlagScratch's size and pointers agree."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "pack_workspace_test")


def test_every_view_lies_in_its_arena():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    shapes, views = (int(x) for x in r.stdout.split()[::2])
    # E x L x C x cells x id-space sizes of the grid; at least one view per generation and shape
    assert shapes == 6 * 3 * 3 * 5 * 2
    assert views > 40 * shapes
