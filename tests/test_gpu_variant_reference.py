"""Variant calling on the GPU against the recorded results of the COMPILED reference
(tests/golden/variant_reference.npz, written by oracle/gen_golden.py variant_cases from oracle/_ref/ref_variant and
proved current by tests/test_variant_reference_cpu.py). Only the golden file and the seeded cases of
tests/variant_cases.py are read here. Integers and bytes: no tolerance anywhere.

Every case runs over the routes the project has: the FASTA read on the host and on the device, the VCF text written
plain and as bgzf (inflated and compared as the same bytes), the per-cell counters in LDS and as global atomics."""
import gzip
import os

import numpy as np
import pytest

from tests import variant_cases as vc
from tests import variant_ref as vr

pytestmark = pytest.mark.gpu

ROUTES = [(fasta, vcf) for fasta in ("host", "device") for vcf in ("plain", "bgzf")]
LDS_GROUPS = 16384  # the LDS counters hold at most this many groups (kLdsGroups); every case here fits


def _v():
    from secedo_amd import variant
    return variant


def _read(out_dir, fasta):
    """{file name as the plain route has it: normalised text} of a result directory of either output."""
    out = {}
    for n in sorted(os.listdir(out_dir)):
        raw = open(os.path.join(out_dir, n), "rb").read()
        if n.endswith(".vcf.gz"):
            raw, n = gzip.decompress(raw), n[:-3]
        out[n] = vc.normalise(raw.decode(), fasta)
    return out


# --- 1. the decision functions ----------------------------------------------------------------------------------------

def test_the_tuple_set_is_the_recorded_one():
    assert vc.tuple_digest(vc.tuple_set()) == str(vc.golden()["tuples_digest"])
    assert vc.golden()["tuples_gen"].shape == (len(vc.SETTINGS), len(vc.tuple_set()))


@pytest.mark.parametrize("setting", range(len(vc.SETTINGS)))
def test_decision_functions_equal_the_reference(setting):
    theta, prior, lht = vc.SETTINGS[setting]
    g = vc.golden()
    counts = vc.tuple_set()
    hom, gen = _v().genotypes_device(counts, bool(lht), prior, theta)
    want_hom = g["tuples_hom"][(1e-3, 0.01, 0.05).index(theta)]
    bad = np.nonzero(hom != want_hom)[0]
    assert len(bad) == 0, counts[bad[:5]]
    bad = np.nonzero(gen != g["tuples_gen"][setting])[0]
    assert len(bad) == 0, counts[bad[:5]]
    # the coverage the reference reports is the u16 sum: what the kernel's cov < 9 and cov > 15 see
    assert np.array_equal(g["tuples_cov"], counts.astype(np.uint32).sum(axis=1).astype(np.uint16))
    if setting == 0:  # the set reaches the wrap: a u16 coverage below 9 from counts far above it
        wrapped = (counts.astype(np.int64).sum(axis=1) > 65535) & (g["tuples_cov"] < 9)
        assert wrapped.any()


# --- 2. the files -----------------------------------------------------------------------------------------------------

_expected_counts = {}


def _counts_of(case, fasta, mp):
    """(mismatch, loci) per cell by the restatement, once per case."""
    name = case[0]
    if name not in _expected_counts:
        _, _, mismatch, loci = vr.calls(case[1], case[2], fasta, mp, case[5], case[6])
        _expected_counts[name] = (np.asarray(mismatch, dtype=np.uint32), np.asarray(loci, dtype=np.uint32))
    return _expected_counts[name]


def _check_preconditions(name, want):
    """What the case is there for shows in the recorded reference output."""
    if name == "wrap":
        for f, line in vc.WRAP_EXPECT.items():
            assert line in want[f]
    if name == "many_clusters":
        with_lines = [k for k, v in want.items() if k.startswith("cluster_") and
                      any(l and l[0] != "#" for l in v.splitlines())]
        assert len(with_lines) > 64
    if name.startswith("ties_"):
        theta = [s[2] for s in vc.TIES_SETTINGS if s[0] == name][0]
        for i, rule in enumerate(vc.ties_rules(theta)):
            assert vc.lines_at(want, i + 1) == vc.ties_expected(name, rule), rule
        scores = want["scores"].strip().split(",")
        for cell, token in vc.TIES_SCORES.items():
            assert scores[cell] == token
    if name == "extreme_24_chromosomes":
        lines = want["cluster_1.vcf"].splitlines()
        assert any(l.startswith("X\t") for l in lines) and any(l.startswith("Y\t") for l in lines)
    if name == "extreme_all_cluster_0":
        assert sorted(want) == ["cluster_0.vcf", "common.vcf", "scores", "variant"]
    if name == "fasta_empty_contig":
        assert not any(l.startswith("1\t") for v in want.values() for l in v.splitlines())


@pytest.mark.parametrize("name", vc.accepted_names())
def test_files_equal_the_reference(tmp_path, monkeypatch, name):
    case = vc.case_named(name)
    _, chromosomes, clusters, _, _, prior, theta = case
    want = vc.golden_files(name)
    assert want and "scores" in want and vc.GENOME_MARK in want["cluster_0.vcf"]
    _check_preconditions(name, want)
    fasta, mp = vc.write_genome(case, tmp_path)
    p = vc.flat(chromosomes)
    assert len(clusters) <= LDS_GROUPS
    v = _v()
    for counters in ("lds", "global"):
        monkeypatch.setenv("SECEDO_VARIANT_COUNTERS", counters)
        for fasta_route, vcf_output in ROUTES:
            out = str(tmp_path / ("%s_%s_%s" % (counters, fasta_route, vcf_output)))
            v.variant_calling(p, clusters, fasta, mp, prior, theta, out, fasta_route=fasta_route, vcf_output=vcf_output)
            if not mp:  # a map sends the device route back to the host (fasta_stats()["fell_back_for_map"])
                assert v.fasta_stats()["route"] == fasta_route
            assert v.vcf_stats()["output"] == vcf_output
            have = _read(out, fasta)
            assert sorted(have) == sorted(want), (counters, fasta_route, vcf_output)
            for k in want:
                assert have[k] == want[k], (counters, fasta_route, vcf_output, k)


@pytest.mark.parametrize("name", vc.accepted_names())
def test_mismatch_and_loci_counters(tmp_path, monkeypatch, name):
    """variant_calls' mismatch and loci arrays: against the reference's recorded `scores`, token for token, and against
    the counts the restatement derives from the case."""
    case = vc.case_named(name)
    _, chromosomes, clusters, _, _, prior, theta = case
    fasta, mp = vc.write_genome(case, tmp_path)
    want_mm, want_loci = _counts_of(case, fasta, mp)
    tokens = vc.golden_files(name)["scores"].rstrip("\n").split(",")
    assert len(tokens) == len(clusters)
    # the loci alone, straight from the case: every entry of a locus in front of its chromosome's end
    _, end = _v().reference_genotypes(fasta, vc.flat(chromosomes).chr_locus_off, vc.flat(chromosomes).locus_pos, mp)
    direct = np.zeros(len(clusters), dtype=np.uint32)
    p = vc.flat(chromosomes)
    for c in range(p.n_chr):
        b, e = int(p.locus_entry_off[int(p.chr_locus_off[c])]), int(p.locus_entry_off[int(end[c])])
        direct += np.bincount(p.id_base[b:e] >> 2, minlength=len(clusters)).astype(np.uint32)
    assert np.array_equal(direct, want_loci)
    for counters in ("lds", "global"):
        monkeypatch.setenv("SECEDO_VARIANT_COUNTERS", counters)
        for route in ("host", "device"):
            _, mm, loci = _v().variant_calls(p, clusters, fasta, mp, prior, theta, fasta_route=route)
            assert np.array_equal(loci, want_loci), (counters, route)
            assert np.array_equal(mm, want_mm), (counters, route)
            assert [vr.format_score(int(m), int(l)) for m, l in zip(mm, loci)] == tokens
    if name == "wrap":  # the cells of the cluster whose coverage wrapped to 0 still have the locus counted
        assert want_loci[600:].sum() == 20 + 65536 + 20 and want_mm.sum() == 5
    if name.startswith("ties_theta"):
        assert want_mm[vc.SCORE_CELL_COV9] == 0 and want_mm[vc.SCORE_CELL_COV10] == 1


# --- 3. what the reference refuses ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(vc.REFUSED_EXPECT))
def test_refused_genomes(tmp_path, name):
    """Unequal maternal and paternal contigs: the reference logs its words and exits with status 1; here the call is
    E_INVALID_ARG with the same words, on every route, and no output directory stays behind."""
    from secedo_amd import _lib
    g = vc.golden()
    at = list(g["refused_names"]).index(name)
    assert int(g["refused_status"][at]) == 1 and str(g["refused_message"][at]) == vc.REFUSED_EXPECT[name]
    case = vc.case_named(name)
    fasta, mp = vc.write_genome(case, tmp_path)
    for fasta_route, vcf_output in ROUTES:
        out = str(tmp_path / ("%s_%s" % (fasta_route, vcf_output)))
        with pytest.raises(_lib.SecedoError) as e:
            _v().variant_calling(vc.flat(case[1]), case[2], fasta, mp, case[5], case[6], out, fasta_route=fasta_route,
                                 vcf_output=vcf_output)
        assert e.value.code == _lib.E_INVALID_ARG and vc.REFUSED_EXPECT[name] in str(e.value), (fasta_route, vcf_output)
        assert not os.path.exists(out)
    # a directory that was there before the call stays
    out = tmp_path / "mine"
    out.mkdir()
    with pytest.raises(_lib.SecedoError):
        _v().variant_calling(vc.flat(case[1]), case[2], fasta, mp, case[5], case[6], str(out))
    assert out.is_dir() and os.listdir(out) == []
