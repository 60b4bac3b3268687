"""The rules of secedo_amd/csrc/genome_bins.hpp (secedo_variant_genome_bins) without a GPU: the byte
class, the name cut, the selection, the piece-to-bin mapping and the line format as a program under the sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "genome_bins_test")


def test_host_program_under_sanitizers():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and r.stderr == ""
