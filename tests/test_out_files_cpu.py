"""The temp-then-rename file set of secedo_amd/csrc/out_files.hpp without a GPU: append and commit, what a call that
does not commit leaves behind, the refusals and their words, in both keep_open modes, as a program under the
sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "out_files_test")


def test_host_program_under_sanitizers():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and r.stderr == ""
