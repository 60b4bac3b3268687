"""The restatement tests/variant_ref.py against the COMPILED reference (oracle/_ref/ref_variant: the unmodified
variant_calling.cpp behind oracle/ref_variant_driver.cpp) on the cases of tests/variant_cases.py, and the recorded
results tests/golden/variant_reference.npz against what that program produces now. No GPU. Skipped when the program
is absent, as tests/test_oracle_vs_ref.py is. Integers and bytes only: no tolerance anywhere."""
import os

import numpy as np
import pytest

from oracle import bindings as ob
from tests import variant_cases as vc
from tests import variant_ref as vr

pytestmark = pytest.mark.skipif(not ob.have_ref_variant(), reason="oracle/_ref/ref_variant not built")


@pytest.fixture(scope="module")
def reference_tuples(tmp_path_factory):
    return vc.reference_tuples(str(tmp_path_factory.mktemp("tuples")))


@pytest.fixture(scope="module")
def reference_runs(tmp_path_factory):
    """{case: (returncode, log, files)} of the compiled reference, every case run once."""
    tmp = tmp_path_factory.mktemp("ref")
    return {c[0]: vc.run_reference(c, tmp) for c in vc.accepted() + vc.refused()}


def test_the_tuple_set_is_the_one_the_issue_names():
    counts = vc.tuple_set()
    n_exhaustive = len(vc.tuples_up_to(vc.EXHAUSTIVE_TOTAL))
    assert vc.EXHAUSTIVE_TOTAL >= 20 and len(counts) == n_exhaustive + 3000 + 3000 + len(vc.WRAP_TUPLES)
    assert len(vc.SETTINGS) == 12 and len(set(vc.SETTINGS)) == 12
    tail = [tuple(int(x) for x in c) for c in counts[-len(vc.WRAP_TUPLES):]]
    assert tail == vc.WRAP_TUPLES and (65535, 10, 0, 0) in tail and (32768, 32768, 9, 0) in tail
    sums = counts[n_exhaustive + 3000:n_exhaustive + 6000].astype(np.int64).sum(axis=1)
    assert (sums > 65535).any()  # the u16 sum wraps in the random part too


@pytest.mark.parametrize("setting", range(12))
def test_restatement_decisions_equal_the_reference(reference_tuples, setting):
    theta, prior, lht = vc.SETTINGS[setting]
    _, hom, gen, cov = reference_tuples
    counts = [[int(x) for x in c] for c in vc.tuple_set()]
    h = np.asarray([vr.likely_homozygous(c, theta) for c in counts], dtype=np.uint8)
    gc = [vr.most_likely_genotype(c, bool(lht), prior, theta) for c in counts]
    g = np.asarray([x[0] for x in gc], dtype=np.uint8)
    k = np.asarray([x[1] for x in gc], dtype=np.uint16)
    assert np.array_equal(h, hom[(1e-3, 0.01, 0.05).index(theta)])
    bad = np.nonzero(g != gen[setting])[0]
    assert len(bad) == 0, [counts[i] for i in bad[:5]]
    assert np.array_equal(k, cov)


@pytest.mark.parametrize("name", vc.accepted_names())
def test_restatement_files_equal_the_reference(reference_runs, tmp_path, name):
    case = vc.case_named(name)
    rc, log, ref_files = reference_runs[name]
    assert rc == 0, log
    fasta, mp = vc.write_genome(case, tmp_path)
    out = str(tmp_path / "restatement")
    vr.write_files(case[1], case[2], fasta, out, mp, case[5], case[6])
    mine = {k: vc.normalise(v, fasta) for k, v in vr.read_dir(out).items()}
    assert sorted(mine) == sorted(ref_files)
    for k in ref_files:
        assert mine[k] == ref_files[k], k
    assert any(vc.GENOME_MARK in v for v in mine.values())  # the preamble carries the genome's path: it was compared


def test_the_case_list_is_complete():
    assert [c[0] for c in vc.accepted()] == vc.accepted_names()
    assert sorted(c[0] for c in vc.refused()) == sorted(vc.REFUSED_EXPECT)
    assert max(len(c[1]) for c in vc.accepted()) == 24  # nothing here, or anywhere, has more than 24 chromosomes


@pytest.mark.parametrize("name", sorted(vc.REFUSED_EXPECT))
def test_reference_refuses_with_status_1_and_its_words(reference_runs, tmp_path, name):
    rc, log, files = reference_runs[name]
    assert rc == 1
    assert vc.mismatch_message(log) == vc.REFUSED_EXPECT[name]
    assert "cluster_0.vcf" in files  # it ends after the preambles are written
    case = vc.case_named(name)
    fasta, _ = vc.write_genome(case, tmp_path)
    with pytest.raises(ValueError, match="Maternal and paternal chromosome sizes don't match"):
        vr.calls(case[1], case[2], fasta, "", case[5], case[6])


def test_preconditions_hold_in_the_reference_output(reference_runs):
    """What each family is there for shows in what the reference wrote (the GPU test asserts the same on the recorded
    copy)."""
    files = reference_runs["wrap"][2]
    for name, line in vc.WRAP_EXPECT.items():
        assert line in files[name]
    files = reference_runs["many_clusters"][2]
    with_lines = [k for k, v in files.items() if k.startswith("cluster_") and
                  any(l and l[0] != "#" for l in v.splitlines())]
    assert len(with_lines) > 64
    for name, _, theta in vc.TIES_SETTINGS:
        files = reference_runs[name][2]
        for i, rule in enumerate(vc.ties_rules(theta)):
            assert vc.lines_at(files, i + 1) == vc.ties_expected(name, rule), (name, rule)
        scores = files["scores"].strip().split(",")
        for cell, want in vc.TIES_SCORES.items():
            assert scores[cell] == want, (name, cell)
    assert set(vc.ties_rules()) == set(vc.TIES_EXPECT)
    lines = reference_runs["extreme_24_chromosomes"][2]["cluster_1.vcf"].splitlines()
    assert any(l.startswith("X\t") for l in lines) and any(l.startswith("Y\t") for l in lines)


def test_driver_refuses_group_ids_past_14_bits(tmp_path):
    """A group id past the reference's u16 packing, or past `clusters`, is the driver's status, not a run."""
    from secedo_amd.pileup import FlatPileup
    p = vc.flat([[(1, [3 << 2, 20000 << 2 | 1])]])
    assert isinstance(p, FlatPileup)
    with pytest.raises(ValueError):
        vc.write_flat(str(tmp_path / "narrow.bin"), p, 20001)
    vc.write_flat(str(tmp_path / "p.bin"), p, 20001, wide=True)
    vc.write_clusters(str(tmp_path / "c.bin"), np.ones(20001, np.uint16))
    fasta = str(tmp_path / "g.fa")
    with open(fasta, "w") as f:
        f.write(">chr1\nACGT\n")
    out = str(tmp_path / "out")
    rc, _, files = ob.ref_variant_calling(tmp_path / "p.bin", tmp_path / "c.bin", fasta, "", 1e-3, 0.01, out)
    assert rc == ob.REF_VARIANT_BAD_GROUP and files == {} and not os.path.exists(out)
    vc.write_flat(str(tmp_path / "p2.bin"), vc.flat([[(1, [3 << 2, 9 << 2 | 1])]]), 4)
    vc.write_clusters(str(tmp_path / "c2.bin"), np.ones(4, np.uint16))
    rc, _, _ = ob.ref_variant_calling(tmp_path / "p2.bin", tmp_path / "c2.bin", fasta, "", 1e-3, 0.01, out)
    assert rc == ob.REF_VARIANT_BAD_GROUP and not os.path.exists(out)


def test_golden_file_is_current(reference_runs, reference_tuples):
    """tests/golden/variant_reference.npz holds what the reference program produces now, array for array."""
    results = {k: v[2] for k, v in reference_runs.items() if k in vc.accepted_names()}
    refusals = {k: (v[0], vc.mismatch_message(v[1])) for k, v in reference_runs.items() if k in vc.REFUSED_EXPECT}
    want = vc.golden_arrays(results, refusals, reference_tuples)
    have = vc.golden()
    assert sorted(have) == sorted(want)
    for k in want:
        assert np.array_equal(have[k], np.asarray(want[k])), k
    assert os.path.getsize(vc.GOLDEN) < 300 * 1024
