"""The rules of secedo_amd/csrc/bam_depth.hpp (secedo_bam_depth) without a GPU: the bin layout, the sort
key, the piece rule of `bases` mode, put_u64 and the line formats as a program under the sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_depth_test")


def test_host_program_under_sanitizers():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and r.stderr == ""
