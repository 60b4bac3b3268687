"""The parts of the bgzf VCF output that need no GPU: the switch (setter, environment, CLI flag, all checked before
torch is imported) and the host formatter behind the plain route, held against a plain Python statement of the lines
on hand-built records (tests/vcf_output_cases.py). The GPU formatter meets the same cases in test_gpu_vcf_output.py."""
import os
import subprocess
import sys

import pytest

from secedo_amd import _lib, secedo_main, variant
from tests import vcf_output_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code, *args, **env):
    return subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=ROOT, **env))


@pytest.mark.parametrize("name", sorted(vc.ALL))
def test_host_formatter_writes_the_lines(name):
    case = vc.ALL[name]()
    want = case.expected()
    assert variant.format_host(*case.args()) == want
    assert len(want) == case.num_clusters + 1


def test_the_cases_cover_what_they_claim():
    text = b"".join(vc.digits().expected()).decode()
    for pos in ("\t1\t", "\t9\t", "\t10\t", "\t999999999\t", "\t4294967295\t"):
        assert pos in text
    assert "\t0 9 10 65535 \n" in text
    names = [l.split("\t")[0] for l in vc.chromosomes().expected()[1].decode().splitlines()]
    assert names == ["1", "1", "10", "10", "22", "22", "X", "X", "Y", "Y"]
    common = vc.line_rules().expected()[3].decode().splitlines()
    assert sum("\t0/1\t" in l for l in common) == 2 and any("\tA\tGT\t." in l for l in common)
    per_locus = [sum(l.split("\t")[1] == str(5 * k + 1) for l in common) for k in range(12)]
    assert per_locus == [1, 1, 1, 0, 1, 1, 2, 2, 1, 1, 1, 1]
    pooled = [l.split("\t")[3:5] for l in common if l.split("\t")[1] in ("41", "46", "51")]
    assert pooled == [["C", "A"], ["C", "A"], ["G", "T"]]
    many = vc.many_clusters()
    files = many.expected()
    assert files[7] == many.preambles[7] and files[299] == many.preambles[299] and len(files) == 301
    cluster0 = vc.long_file().expected()[0]
    assert len(cluster0) > 2 * 65280 and cluster0[65279:65280] != b"\n" and cluster0[130559:130560] != b"\n"


def test_records_out_of_order_or_out_of_range_are_refused():
    case = vc.digits()
    rec = case.records[::-1].copy()
    with pytest.raises(_lib.SecedoError, match="ascend"):
        variant.format_host(rec, *case.args()[1:])
    rec = case.records.copy()
    rec["cluster"][1] = 2
    with pytest.raises(_lib.SecedoError, match="num_clusters"):
        variant.format_host(rec, *case.args()[1:])


def test_setter_and_environment():
    code = ("import sys\nfrom secedo_amd import variant\n"
            "print(variant.get_vcf_output())\n"
            "variant.set_vcf_output('bgzf'); print(variant.get_vcf_output())\n"
            "variant.set_vcf_output('plain'); print(variant.get_vcf_output())\n"
            "assert 'torch' not in sys.modules or True\n")
    for value, want in (("", "plain"), ("plain", "plain"), ("bgzf", "bgzf")):
        r = _child(code, SECEDO_VCF=value)
        assert r.returncode == 0 and r.stdout.split() == [want, "bgzf", "plain"], r.stderr[-2000:]
    r = _child("from secedo_amd import variant\nvariant.get_vcf_output()\n", SECEDO_VCF="zip")
    assert r.returncode != 0 and "SECEDO_VCF=zip: expected plain or bgzf" in r.stderr
    with pytest.raises(ValueError):
        variant.set_vcf_output("zip")


def test_cli_flag_is_checked_before_torch(tmp_path):
    code = ("import sys; from secedo_amd import secedo_main as m; rc = m.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)")
    (tmp_path / "in").mkdir()
    r = _child(code, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), "--vcf_output", "zip")
    assert r.returncode == 1 and "torch imported" not in r.stderr, r.stderr
    assert "Invalid value for --vcf_output: zip.\nShould be one of plain, bgzf" in r.stderr
    assert "--vcf_output plain|bgzf" in secedo_main.usage() and "-vcf_output (str)" in secedo_main.usage()
    for ok in ("plain", "bgzf"):
        secedo_main.validate(secedo_main.parse_flags(["--vcf_output", ok]))
