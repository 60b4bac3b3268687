"""The parts of the per-cell allele counts that need no GPU: the mask rule of secedo_variant_allele_masks against the
restatement tests/allele_ref.py on hand-made records, the setting (setter, environment, the file-writing call's refusal
of an unknown value) and the CLI flags, checked before torch is imported. The kernels meet the restatement in
test_gpu_allele_counts.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from secedo_amd import _lib, secedo_main, variant
from tests import allele_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
POOLED, COMMON, CLUSTER = 0, 1, 2


def G(a, b=None):
    """The genotype code of bases a / b (letters)."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 5}
    return code[a] << 3 | code[a if b is None else b]


def _records(rows):
    rec = np.zeros(len(rows), dtype=variant.RECORD_DTYPE)
    for i, (locus, kind, cluster, genotype) in enumerate(rows):
        rec[i] = (locus, cluster, genotype, kind, (0, 0, 0, 0))
    return rec


def _child(code, *args, **env):
    return subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=ROOT, **env))


# name -> (reference genotype of locus 3, the records of locus 3, (ref_mask, alt_mask) letters expected under "all",
# whether the locus is a site under "cluster")
CASES = {
    "homozygous_ref_one_alt": (G("A"), [(3, COMMON, 0, G("C"))], ("A", "C"), False),
    "two_clusters_two_alts": (G("A"), [(3, CLUSTER, 1, G("C")), (3, CLUSTER, 4, G("T"))], ("A", "C,T"), True),
    "het_genotype_homozygous_ref": (G("G"), [(3, CLUSTER, 0, G("G", "T"))], ("G", "T"), True),
    "het_ref_losing_an_allele": (G("A", "C"), [(3, CLUSTER, 2, G("C"))], ("A", "C"), True),
    "het_ref_both_homozygous": (G("A", "C"), [(3, CLUSTER, 0, G("A")), (3, CLUSTER, 1, G("C"))], ("N", "A,C"), True),
    "ref_n": (G("N"), [(3, POOLED, 0, G("T")), (3, COMMON, 0, G("T"))], ("N", "T"), False),
    "pooled_only": (G("C"), [(3, POOLED, 0, G("A"))], ("C", "A"), False),
    "pooled_and_cluster": (G("C"), [(3, POOLED, 0, G("A")), (3, CLUSTER, 3, G("G"))], ("C", "A,G"), True),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("sites", ["all", "cluster"])
def test_masks_against_the_restatement(name, sites):
    ref3, rows, (ref_letters, alt_letters), in_cluster = CASES[name]
    # loci 1 and 5 carry a common record each, so the site's number is not 0 under "all"
    rec = _records([(1, COMMON, 0, G("T"))] + rows + [(5, COMMON, 0, G("G"))])
    locus_ref = np.asarray([0, G("A"), 0, ref3, 0, G("A"), 0], dtype=np.uint8)
    got = variant.allele_masks(rec, locus_ref, len(locus_ref), sites)
    want = ar.masks(rec, locus_ref, sites)
    assert [tuple(int(x) for x in row) for row in zip(got["site_locus"], got["ref_mask"], got["alt_mask"])] == want
    loci = [w[0] for w in want]
    assert loci == ([1, 3, 5] if sites == "all" else [3] if in_cluster else [])
    if 3 in loci:
        _, rm, am = want[loci.index(3)]
        assert (ar.letters(rm), ar.letters(am)) == (ref_letters, alt_letters) and am != 0 and rm & am == 0


def test_no_records_no_sites():
    for sites in ("all", "cluster"):
        got = variant.allele_masks(np.zeros(0, dtype=variant.RECORD_DTYPE), np.zeros(4, np.uint8), 4, sites)
        assert all(len(v) == 0 for v in got.values()) and ar.masks([], np.zeros(4, np.uint8), sites) == []


def test_bad_arguments_are_refused():
    rec = _records([(3, COMMON, 0, G("C")), (1, COMMON, 0, G("C"))])
    ref = np.zeros(4, np.uint8)
    with pytest.raises(_lib.SecedoError, match="ascend") as e:
        variant.allele_masks(rec, ref, 4)
    assert e.value.code == _lib.E_INVALID_ARG
    with pytest.raises(_lib.SecedoError, match="n_loci"):
        variant.allele_masks(rec[:1], ref, 3)
    with pytest.raises(ValueError):
        variant.allele_masks(rec[:1], ref, 4, "none")


def test_capacity_convention():
    import ctypes as C
    rec = _records([(l, COMMON, 0, G("C")) for l in range(5)])
    ref = np.zeros(5, np.uint8)
    n = C.c_uint32(0)
    rc = variant.lib().secedo_variant_allele_masks(_lib.ptr(rec), 5, _lib.ptr(ref), 5, 1, None, None, None, 0, C.byref(n))
    assert rc == _lib.E_LIMIT and n.value == 5


def test_setter_and_environment():
    code = ("from secedo_amd import variant\nprint(variant.get_allele_counts())\n"
            "variant.set_allele_counts('cluster'); print(variant.get_allele_counts())\n"
            "variant.set_allele_counts('all'); print(variant.get_allele_counts())\n"
            "variant.set_allele_counts('none'); print(variant.get_allele_counts())\n")
    for value, want in (("", "none"), ("none", "none"), ("all", "all"), ("cluster", "cluster")):
        r = _child(code, SECEDO_ALLELE_COUNTS=value)
        assert r.returncode == 0 and r.stdout.split() == [want, "cluster", "all", "none"], r.stderr[-2000:]
    r = _child("from secedo_amd import variant\nvariant.get_allele_counts()\n", SECEDO_ALLELE_COUNTS="every")
    assert r.returncode != 0 and "SECEDO_ALLELE_COUNTS=every: expected none, all or cluster" in r.stderr
    with pytest.raises(ValueError):
        variant.set_allele_counts("every")


def test_unknown_environment_value_fails_the_file_writing_call(tmp_path):
    """Refused with E_INVALID_ARG before a device is looked for or anything is written."""
    code = ("import sys, numpy as np\nfrom secedo_amd import _lib, variant\nfrom secedo_amd.pileup import FlatPileup\n"
            "p = FlatPileup(np.asarray([0, 1]), np.asarray([1]), np.asarray([0, 1], dtype=np.uint64),\n"
            "               np.zeros(1, np.uint32), np.zeros(1, np.uint32))\n"
            "try:\n    variant.variant_calling(p, [0], sys.argv[1], out_dir=sys.argv[2])\n"
            "except _lib.SecedoError as e:\n    print(e.code == _lib.E_INVALID_ARG, e)\n")
    out = tmp_path / "out"
    r = _child(code, os.path.join(DATA, "genome_female.fa"), str(out), SECEDO_ALLELE_COUNTS="sometimes")
    assert r.returncode == 0 and r.stdout.startswith("True") and "SECEDO_ALLELE_COUNTS=sometimes" in r.stdout, r.stderr
    assert not out.exists()


def test_cell_names_are_checked():
    with pytest.raises(_lib.SecedoError, match="empty or holds a tab"):
        variant.set_cell_names(["a", "b\tc"])
    with pytest.raises(_lib.SecedoError, match="cannot read"):
        variant.set_cell_names("/nonexistent/names.txt")
    variant.set_cell_names(["a", "b"])
    variant.set_cell_names(None)


def test_cli_flags_are_checked_before_torch(tmp_path):
    main = ("import sys; from secedo_amd import secedo_main as m; rc = m.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)")
    d = tmp_path / "in"
    d.mkdir()
    open(d / "s_1.pileup.bin", "wb").close()
    fa = os.path.join(DATA, "genome_female.fa")
    ok = ["-i", str(d), "--chromosomes=1"]
    for flags, words in ((["--allele_counts", "some", "--reference_genome", fa], "Should be one of none, all, cluster"),
                         (["--allele_counts=all"], "add --reference_genome"),
                         (["--allele_counts", "cluster"], "add --reference_genome"),
                         (["--cell_names", str(tmp_path / "missing"), "--reference_genome", fa],
                          "Cannot find cell names file")):
        p = _child(main, *(ok + flags))
        assert p.returncode == 1 and words in p.stderr and "torch imported" not in p.stderr, (flags, p.stderr)
    f = secedo_main.parse_flags(ok + ["--allele_counts=none"])
    secedo_main.validate(f)  # "none" needs no reference genome
    assert f.allele_counts == "none" and secedo_main.parse_flags(ok).allele_counts == ""
    text = secedo_main.usage()
    assert "--allele_counts none|all|cluster" in text and "--cell_names <file>" in text
    assert "-allele_counts (str)" in text and "-cell_names (str)" in text
