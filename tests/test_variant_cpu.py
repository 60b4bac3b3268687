"""Host side of the variant calling (include/secedo_variant.h) and the restatement tests/variant_ref.py, without a
GPU: the reference's ReadFasta / ReadMap / ApplyMap / IsDiploid cases through the library's host entry points,
its MostLikelyGenotype / LikelyHomozygous known answers against the restatement (the two DISABLED_ cases stay
out, as in the reference), and the restatement against the expectations of its VariantCalling suite
(tests/test_variant_calling.cpp of the reference)."""
import os

import numpy as np
import pytest

from tests import variant_ref as vr

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
FEMALE = os.path.join(DATA, "genome_diploid_female.fa")
MALE = os.path.join(DATA, "genome_diploid_male.fa")
HAPLOID = os.path.join(DATA, "genome_female.fa")
MALE_MAP = os.path.join(DATA, "genome_diploid_male.map")
TEST_MAP = os.path.join(DATA, "test.map")


def _v():
    from secedo_amd import variant
    return variant


def _codes(s):
    return [vr.char_to_int(c) for c in s]


def _check(chr_data, paternal, maternal):
    assert len(chr_data) == len(paternal)
    assert [int(x) & 7 for x in chr_data] == _codes(paternal)
    assert [int(x) >> 3 for x in chr_data] == _codes(maternal)


# --- ReadFasta.* / IsDiploid.* ---------------------------------------------------------------------------------------

def test_read_fasta_empty_file(tmp_path):
    p = tmp_path / "empty.fa"
    p.write_bytes(b"")
    assert len(_v().read_chromosome(str(p), 0)) == 0


def test_read_fasta_female_genome():
    v = _v()
    _check(v.read_chromosome(FEMALE, 0), "CCCCCTTTTT", "AAAAAGGGGG")
    _check(v.read_chromosome(FEMALE, 1), "AAAAGGGG", "CCCCNNNN")


def test_read_fasta_female_genome_haploid():
    v = _v()
    assert not v.is_diploid(HAPLOID)
    _check(v.read_chromosome(HAPLOID, 0), "AAAAAGGGGG", "AAAAAGGGGG")
    _check(v.read_chromosome(HAPLOID, 1), "CCCCNNNN", "CCCCNNNN")


def test_read_fasta_male_genome():
    v = _v()
    assert v.is_diploid(MALE)
    _check(v.read_chromosome(MALE, 0), "CACCCTTTTT", "AAAAAGGGGG")
    _check(v.read_chromosome(MALE, 1), "CCCCNNNN", "CCCCNNNN")
    _check(v.read_chromosome(MALE, 2), "AAAAGGGG", "AAAAGGGG")


def test_read_fasta_male_genome_mapped():
    v = _v()
    _check(v.read_chromosome(MALE, 0, MALE_MAP), "NCACCCTTTTT", "ANAAAAGGGGG")
    _check(v.read_chromosome(MALE, 1, MALE_MAP), "CCCNNNN", "CCCNNNN")
    _check(v.read_chromosome(MALE, 2, MALE_MAP), "AAAGGG", "AAAGGG")


def test_fewer_contigs_keep_the_last_one():
    v = _v()
    assert np.array_equal(v.read_chromosome(HAPLOID, 2), v.read_chromosome(HAPLOID, 1))
    assert np.array_equal(v.read_chromosome(HAPLOID, 7), v.read_chromosome(HAPLOID, 1))


def test_is_diploid_haploid():
    assert not _v().is_diploid(HAPLOID)


def test_host_genome_equals_the_restatement():
    for fasta, mp in ((FEMALE, ""), (MALE, ""), (MALE, MALE_MAP), (HAPLOID, "")):
        data = open(fasta, "rb").read()
        f, chr_data = vr.Stream(data), []
        for i in range(4):
            chr_data = vr.get_next_chromosome(f, vr.read_map(mp), vr.check_is_diploid(data), chr_data)
            assert list(_v().read_chromosome(fasta, i, mp)) == chr_data, (fasta, mp, i)


# --- ReadMap.* / ApplyMap.* ------------------------------------------------------------------------------------------

def test_read_map_empty_name():
    assert _v().read_map("") == {}


def test_read_map_empty_file(tmp_path):
    p = tmp_path / "empty.map"
    p.write_text("")
    assert _v().read_map(str(p)) == {}


def test_read_map_file():
    m = _v().read_map(TEST_MAP)
    assert len(m) == 2 and len(m["1_maternal"]) == 6
    pat = m["1_paternal"]
    assert [e[0] for e in pat] == [63734, 66269, 82130, 91547, 285647, 289210, 708137]
    assert [e[2] for e in pat] == ["D", "I", "D", "I", "D", "I", "I"]
    assert [e[1] for e in pat] == [3, 1, 2, 1, 4, 1, 1]
    assert m == {k: [tuple(x) for x in e] for k, e in vr.read_map(TEST_MAP).items()}


def test_read_map_errors(tmp_path):
    from secedo_amd._lib import SecedoError
    bad = tmp_path / "bad.map"
    bad.write_text("1\t1_paternal\t1\t1\n")
    with pytest.raises(SecedoError):
        _v().read_map(str(bad))
    bad.write_text("1\t1_paternal\t1\t25\t2\t+\tDEL\t.\n")  # chromosome 25
    with pytest.raises(SecedoError):
        _v().read_map(str(bad))
    with pytest.raises(SecedoError):
        _v().read_map(str(tmp_path / "missing.map"))


@pytest.mark.parametrize("chromosome,entries,expected", [
    ([0, 0, 0, 0], [], [0, 0, 0, 0]),
    ([0, 0, 0, 0], [(0, 1, "D")], [5, 0, 0, 0, 0]),
    ([0, 0, 0, 0], [(2, 1, "D")], [0, 0, 5, 0, 0]),
    ([0, 1, 2, 3], [(0, 1, "I")], [1, 2, 3]),
    ([0, 1, 2, 3], [(2, 1, "I")], [0, 1, 3]),
    ([0, 1, 2, 3], [(0, 1, "D"), (2, 1, "I")], [5, 0, 1, 3]),
    ([0, 1, 2, 3], [(0, 1, "I"), (2, 1, "D")], [1, 5, 2, 3]),
], ids=["EmptyMap", "OneDeletionBeg", "OneDeletionMid", "OneInsertionBeg", "OneInsertionMid",
        "InsertionBegDeletionMid", "InsertionMidDeletionBeg"])
def test_apply_map(chromosome, entries, expected):
    assert list(_v().apply_map(entries, chromosome)) == expected
    assert vr.apply_map(entries, chromosome) == expected


# --- reference_genotypes ---------------------------------------------------------------------------------------------

def test_reference_genotypes_gather_and_chromosome_ends():
    v = _v()
    # chromosome 0: positions 1, 10, 11 (past the end: break), 2 (after the break: skipped too)
    # chromosome 1: position 0 (wraps: ends the chromosome at once), then 1
    ref, end = v.reference_genotypes(FEMALE, [0, 4, 6], [1, 10, 11, 2, 0, 1])
    assert list(end) == [2, 4]
    assert list(ref[:2]) == [(0 << 3) | 1, (2 << 3) | 3]
    assert list(ref[2:]) == [0, 0, 0, 0]
    # a third chromosome with a FASTA of two contigs keeps the second contig
    ref, end = v.reference_genotypes(HAPLOID, [0, 1, 2, 3], [1, 1, 8])
    assert list(ref) == [0, 9, 45] and list(end) == [1, 2, 3]


def test_reference_genotypes_errors(tmp_path):
    from secedo_amd._lib import SecedoError
    with pytest.raises(SecedoError):
        _v().reference_genotypes(str(tmp_path / "missing.fa"), [0, 1], [1])
    bad = tmp_path / "bad.fa"
    bad.write_text(">1_maternal\nAAAA\n>1_paternal\nAAA\n")
    with pytest.raises(SecedoError):
        _v().reference_genotypes(str(bad), [0, 1], [1])
    with pytest.raises(ValueError):
        vr.calls([[(1, [0])]], [0], str(bad))


# --- MostLikelyGenotype.* / LikelyHomozygous.* -----------------------------------------------------------------------

def _mlg(n, theta, lht=False):
    return vr.most_likely_genotype(n, lht, 1e-3, theta)[0]


def test_most_likely_genotype_kats():
    for b in range(4):
        n = [0, 0, 0, 0]
        n[b] = 10
        assert _mlg(n, 1e-3) == (b << 3) + b  # AllSame
        m = list(n)
        m[0 if b else 1] = 1
        assert _mlg(m, 1e-3) == (b << 3) + b  # OneDifferent
        m = list(n)
        m[0 if b else 1] = 2
        assert _mlg(m, 0.05) == (b << 3) + b  # TwoDifferent
    assert _mlg([10, 10, 0, 0], 0.05) in ((0 << 3) + 1, (1 << 3) + 0)  # EqualProportions
    assert _mlg([10, 13, 0, 0], 0.05) in ((0 << 3) + 1, (1 << 3) + 0)  # NearEqualProportions
    assert _mlg([5, 0, 0, 0], 0.05) == 255  # AllSameFewerThan9


def test_likely_homozygous_kats():
    assert vr.likely_homozygous([10, 0, 0, 0], 0.05) == 0
    assert vr.likely_homozygous([1, 10, 0, 0], 0.05) == (1 << 3) + 1
    assert vr.likely_homozygous([2, 10, 0, 0], 0.05) == vr.NO_GENOTYPE
    assert vr.likely_homozygous([5, 5, 5, 5], 0.05) == vr.NO_GENOTYPE


def test_tie_rules():
    # likely_homozygous: the lowest of tied maxima (std::max_element) -- cannot be homozygous with a tie, but the
    # index matters for cov - max; most_likely_genotype: the highest (stable argsort)
    assert vr.argsort4([3, 3, 3, 3]) == [0, 1, 2, 3]
    assert _mlg([0, 0, 9, 9], 0.01, True) == (3 << 3) | 2  # tied maxima: idx[3] is the higher base
    assert _mlg([3, 0, 0, 0], 0.01, True) == 0
    assert _mlg([2, 2, 0, 0], 0.01, True) == vr.NO_GENOTYPE  # cov 4: n3 = 2 < cov - 1
    assert _mlg([1, 0, 0, 1], 0.01, True) == (3 << 3) | 3  # cov 2: tied maxima -> the highest index


# --- VariantCalling.* on the restatement -----------------------------------------------------------------------------

def _vcf(path):
    out = []
    for line in open(path):
        if not line.strip() or line[0] == "#":
            continue
        c = line.rstrip("\n").split("\t")
        out.append((int(c[0]), int(c[1]), c[3][0], c[4][0], c[9]))
    return out


def _one(n, f):
    return [[(1, [f(i) for i in range(n)])]]


def test_restatement_variant_calling_suite(tmp_path):
    d = str(tmp_path / "Empty")
    vr.write_files([[]], [], FEMALE, d)
    assert not os.path.exists(os.path.join(d, "cluster_0.vcf"))

    d = str(tmp_path / "EmptyPos")
    vr.write_files([[]], [1, 1, 1, 2, 2, 2], FEMALE, d, "", 1e-3, 1e-3)
    assert _vcf(os.path.join(d, "cluster_0.vcf")) == []

    d = str(tmp_path / "OnePosOneVariant")
    vr.write_files(_one(10, lambda i: i << 2), [1] * 10, FEMALE, d, "", 1e-3, 1e-3)
    assert _vcf(os.path.join(d, "cluster_1.vcf")) == []
    assert [(r[2], r[3], r[4]) for r in _vcf(os.path.join(d, "common.vcf"))] == [("C", "A", "1/1")]

    d = str(tmp_path / "OnePosOneVariantHomozygous")
    vr.write_files([[(2, [i << 2 | 1 for i in range(10)])]], [1] * 10, MALE, d, "", 1e-3, 1e-3)
    assert [(r[2], r[3], r[4]) for r in _vcf(os.path.join(d, "common.vcf"))] == [("A", "C", "1/1")]

    d = str(tmp_path / "OnePosNoVariant")
    vr.write_files(_one(10, lambda i: i << 2 if i % 2 else i << 2 | 1), [1] * 10, FEMALE, d, "", 1e-3, 1e-3)
    assert _vcf(os.path.join(d, "cluster_1.vcf")) == []

    d = str(tmp_path / "OnePosTwoVariants")
    vr.write_files(_one(20, lambda i: i << 2 | 2 if i % 2 else i << 2 | 3), [1] * 19 + [2], FEMALE, d, "", 1e-3,
                   1e-3)
    assert [(r[2], r[3], r[4]) for r in _vcf(os.path.join(d, "cluster_1.vcf"))] == [("A", "G", "1/1"),
                                                                                    ("C", "T", "1/1")]

    d = str(tmp_path / "TwoPosTwoVariants")
    vr.write_files([[(1, [i << 2 if i % 2 else i << 2 | 3 for i in range(20)])], [(1, [i << 2 for i in range(20)])]],
                   [1] * 19 + [2], FEMALE, d, "", 1e-3, 1e-3)
    assert [(r[2], r[3], r[4]) for r in _vcf(os.path.join(d, "common.vcf"))] == [("C", "A", "1/1")]
    assert [(r[2], r[3], r[4]) for r in _vcf(os.path.join(d, "cluster_1.vcf"))] == [("C", "T", "1/1")]

    d = str(tmp_path / "HomozygousCommon")
    vr.write_files([[(1, [i << 2 for i in range(50)])], [(1, [i << 2 | 3 for i in range(50)])]],
                   [1] * 25 + [2] * 25, HAPLOID, d, "", 1e-3, 1e-3)
    assert _vcf(os.path.join(d, "cluster_1.vcf")) == [] and _vcf(os.path.join(d, "cluster_2.vcf")) == []
    assert [(r[2], r[3], r[4]) for r in _vcf(os.path.join(d, "common.vcf"))] == [("C", "T", "1/1")]
    assert sorted(os.listdir(d)) == ["cluster_0.vcf", "cluster_1.vcf", "cluster_2.vcf", "common.vcf", "scores",
                                     "variant"]
    assert open(os.path.join(d, "variant")).read() == ""
    assert open(os.path.join(d, "scores")).read() == ",".join(["0"] * 50) + "\n"


def test_scores_format():
    assert vr.format_score(0, 0) == "-nan"
    assert vr.format_score(1, 3) == "0.333333"
    assert vr.format_score(0, 5) == "0" and vr.format_score(1, 1) == "1"


# --- more than 24 chromosomes -----------------------------------------------------------------------------------------

def test_more_than_24_chromosomes_are_refused_before_anything_is_made(tmp_path):
    """The VCF lines name chromosomes 1..22, X, Y; the reference asserts on a line for a 25th (id_to_chromosome). The
    call is refused on its arguments alone: no GPU is touched and no directory is made."""
    from secedo_amd import _lib
    from tests import variant_cases as vc
    locus = [(1, [g << 2 for g in range(12)])]
    out = tmp_path / "out"
    with pytest.raises(_lib.SecedoError) as e:
        _v().variant_calling(vc.flat([locus] * 25), np.ones(12, np.uint16), HAPLOID, "", 1e-3, 0.01, str(out))
    assert e.value.code == _lib.E_INVALID_ARG and "more than 24 chromosomes (25)" in str(e.value)
    assert not out.exists()
    # no cells: nothing is done and nothing is an error, as in the reference
    _v().variant_calling(vc.flat([locus] * 25), np.zeros(0, np.uint16), HAPLOID, "", 1e-3, 0.01, str(out))
    assert not out.exists()
