"""Variant calling on the GPU (include/secedo_variant.h) against the reference's VariantCalling suite
(tests/test_variant_calling.cpp of the reference) and, byte for byte on every output file but ##fileDate, against
the restatement tests/variant_ref.py."""
import os

import numpy as np
import pytest

from secedo_amd.pileup import FlatPileup
from tests import variant_cases as vc
from tests import variant_ref as vr
from tests.clone_tree_gen import clone_tree

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
FEMALE = os.path.join(DATA, "genome_diploid_female.fa")
MALE = os.path.join(DATA, "genome_diploid_male.fa")
HAPLOID = os.path.join(DATA, "genome_female.fa")
MALE_MAP = os.path.join(DATA, "genome_diploid_male.map")


def _v():
    from secedo_amd import variant
    return variant


_flat = vc.flat


def _both(tmp_path, name, chromosomes, clusters, fasta, map_file="", prior=1e-3, theta=1e-3):
    """GPU files and restatement files for one case -> (gpu dir, {file: text} of the GPU, of the restatement)."""
    g, r = str(tmp_path / (name + "_gpu")), str(tmp_path / (name + "_ref"))
    _v().variant_calling(_flat(chromosomes), clusters, fasta, map_file, prior, theta, g)
    vr.write_files(chromosomes, clusters, fasta, r, map_file, prior, theta)
    if not os.path.exists(r):
        assert not os.path.exists(g)
        return g, {}, {}
    return g, vr.read_dir(g), vr.read_dir(r)


def _vcf(d, name):
    out = []
    for line in open(os.path.join(d, name)):
        if line.strip() and line[0] != "#":
            c = line.rstrip("\n").split("\t")
            out.append((c[3][0], c[4][0], c[9]))
    return out


# --- 1. the reference's VariantCalling.* ------------------------------------------------------------------------------

def test_empty(tmp_path):
    g, a, b = _both(tmp_path, "Empty", [[]], [], FEMALE)
    assert not os.path.exists(os.path.join(g, "cluster_0.vcf"))


def test_empty_pos(tmp_path):
    g, a, b = _both(tmp_path, "EmptyPos", [[]], [1, 1, 1, 2, 2, 2], FEMALE)
    assert a == b and _vcf(g, "cluster_0.vcf") == []
    assert a["scores"] == "-nan,-nan,-nan,-nan,-nan,-nan\n"


def test_one_pos_one_variant(tmp_path):
    g, a, b = _both(tmp_path, "OnePosOneVariant", [[(1, [i << 2 for i in range(10)])]], [1] * 10, FEMALE)
    assert a == b
    assert _vcf(g, "cluster_1.vcf") == [] and _vcf(g, "common.vcf") == [("C", "A", "1/1")]


def test_one_pos_one_variant_homozygous(tmp_path):
    g, a, b = _both(tmp_path, "OnePosOneVariantHomozygous", [[(2, [i << 2 | 1 for i in range(10)])]], [1] * 10, MALE)
    assert a == b and _vcf(g, "common.vcf") == [("A", "C", "1/1")]


def test_one_pos_no_variant(tmp_path):
    chroms = [[(1, [i << 2 if i % 2 else i << 2 | 1 for i in range(10)])]]
    g, a, b = _both(tmp_path, "OnePosNoVariant", chroms, [1] * 10, FEMALE)
    assert a == b and _vcf(g, "cluster_1.vcf") == []


def test_one_pos_two_variants(tmp_path):
    chroms = [[(1, [i << 2 | 2 if i % 2 else i << 2 | 3 for i in range(20)])]]
    g, a, b = _both(tmp_path, "OnePosTwoVariants", chroms, [1] * 19 + [2], FEMALE)
    assert a == b and _vcf(g, "cluster_1.vcf") == [("A", "G", "1/1"), ("C", "T", "1/1")]


def test_two_pos_two_variants(tmp_path):
    chroms = [[(1, [i << 2 if i % 2 else i << 2 | 3 for i in range(20)])], [(1, [i << 2 for i in range(20)])]]
    g, a, b = _both(tmp_path, "TwoPosTwoVariants", chroms, [1] * 19 + [2], FEMALE)
    assert a == b
    assert _vcf(g, "common.vcf") == [("C", "A", "1/1")] and _vcf(g, "cluster_1.vcf") == [("C", "T", "1/1")]


def test_homozygous_common(tmp_path):
    chroms = [[(1, [i << 2 for i in range(50)])], [(1, [i << 2 | 3 for i in range(50)])]]
    g, a, b = _both(tmp_path, "HomozygousCommon", chroms, [1] * 25 + [2] * 25, HAPLOID)
    assert a == b
    assert _vcf(g, "cluster_1.vcf") == [] and _vcf(g, "cluster_2.vcf") == []
    assert _vcf(g, "common.vcf") == [("C", "T", "1/1")]
    assert sorted(a) == ["cluster_0.vcf", "cluster_1.vcf", "cluster_2.vcf", "common.vcf", "scores", "variant"]
    assert a["variant"] == ""


# --- 2. the decision function -----------------------------------------------------------------------------------------

def _tuples_up_to(total):
    out = []
    for a in range(total + 1):
        for b in range(total + 1 - a):
            for c in range(total + 1 - a - b):
                for d in range(total + 1 - a - b - c):
                    out.append((a, b, c, d))
    return np.asarray(out, dtype=np.uint16)


@pytest.mark.parametrize("theta", [1e-3, 0.01, 0.05])
@pytest.mark.parametrize("prior", [1e-3, 0.2])
def test_decision_function_against_restatement(theta, prior):
    rng = np.random.default_rng(int(theta * 1e4) + int(prior * 100))
    counts = np.concatenate([_tuples_up_to(48), rng.integers(0, 250, (3000, 4)).astype(np.uint16),
                             (rng.dirichlet([5, 1, 0.3, 0.3], 3000) * rng.integers(9, 1000, 3000)[:, None])
                             .astype(np.uint16)])
    for lht in (False, True):
        h, g = _v().genotypes_device(counts, lht, prior, theta)
        eh = [vr.likely_homozygous([int(x) for x in c], theta) for c in counts]
        eg = [vr.most_likely_genotype([int(x) for x in c], lht, prior, theta)[0] for c in counts]
        assert np.array_equal(h, np.asarray(eh, dtype=np.uint8))
        bad = np.nonzero(g != np.asarray(eg, dtype=np.uint8))[0]
        assert len(bad) == 0, counts[bad[:5]]


# --- 3. seeded synthetic runs ------------------------------------------------------------------------------------------

def _fasta(path, contigs, diploid, male=False, rng=None):
    names = [str(i + 1) for i in range(len(contigs))]
    if male:
        names[-2:] = ["X", "Y"]
    with open(path, "w") as f:
        for i, (name, n) in enumerate(zip(names, contigs)):
            mat = "".join(rng.choice(list("ACGT"), n))
            if diploid and not (male and name in "XY"):
                pat = "".join(c if rng.random() < 0.9 else rng.choice(list("ACGT")) for c in mat)
                f.write(">%s_maternal\n%s\n>%s_paternal\n%s\n" % (name, _wrap(mat), name, _wrap(pat)))
            elif diploid:
                f.write(">%s_%s\n%s\n" % (name, "maternal" if name == "X" else "paternal", _wrap(mat)))
            else:
                f.write(">chr%s\n%s\n" % (name, _wrap(mat)))
    return path


def _wrap(s, w=60):
    return "\n".join(s[i:i + w] for i in range(0, len(s), w))


def _synthetic(rng, n_groups, n_clusters, contigs, n_chr, extra=True):
    clusters = rng.integers(0, n_clusters, n_groups).astype(np.uint16)
    clusters[: min(n_clusters, n_groups)] = np.arange(min(n_clusters, n_groups))
    chromosomes = []
    for c in range(n_chr):
        length = contigs[min(c, len(contigs) - 1)]
        pos = np.sort(rng.choice(np.arange(1, length + 1), min(length, 150), replace=False)).tolist()
        if extra and c == 1:
            pos = [0] + pos  # position 0 wraps: ends its chromosome at once
        if extra and c == 0:
            pos = pos + [length + 5, 3]  # past the end, then a locus after the break
        chrom = []
        for p in pos:
            cov = int(rng.choice([0, 3, 8, 12, 20, 30, 45, 70]))
            alleles = {int(k): rng.choice(4, 2) if rng.random() < 0.3 else np.repeat(rng.integers(4), 2)
                       for k in range(n_clusters)}
            groups = rng.integers(0, n_groups, cov)
            entries = []
            for g in groups:
                b = int(rng.choice(alleles[int(clusters[g])]))
                if rng.random() < 0.02:
                    b = int(rng.integers(4))
                entries.append(int(g) << 2 | b)
            chrom.append((p, entries))
        chromosomes.append(chrom)
    return chromosomes, clusters


@pytest.mark.parametrize("kind", ["diploid", "haploid", "male", "mapped", "fewer_contigs"])
def test_synthetic_against_restatement(tmp_path, kind):
    rng = np.random.default_rng(["diploid", "haploid", "male", "mapped", "fewer_contigs"].index(kind) + 11)
    if kind == "mapped":
        fasta, mp, contigs, n_chr = MALE, MALE_MAP, [11, 7, 6], 3
    else:
        contigs = [400, 300, 250, 200]
        fasta = _fasta(str(tmp_path / "g.fa"), contigs, kind != "haploid", kind == "male", rng)
        mp, n_chr = "", 6 if kind == "fewer_contigs" else 4
    chroms, clusters = _synthetic(rng, 300, 5, contigs, n_chr)
    for theta in (1e-3, 0.05):
        g, a, b = _both(tmp_path, "%s_%g" % (kind, theta), chroms, clusters, fasta, mp, 1e-3, theta)
        assert a == b, [k for k in a if a[k] != b.get(k)]
    assert sum(len(x) for x in a.values()) > 0


def test_long_loci_many_clusters_grouped(tmp_path):
    """Loci with more than 64 and more than 1000 entries, more than 64 clusters, cells in cluster 0, a cluster with
    coverage but no call, group ids that are not cell ids (more groups than clusters entries used)."""
    rng = np.random.default_rng(5)
    contigs = [500, 500]
    fasta = _fasta(str(tmp_path / "g.fa"), contigs, True, False, rng)
    n_groups, n_clusters = 2000, 90
    clusters = rng.integers(0, n_clusters, n_groups).astype(np.uint16)
    chroms = []
    for c in range(2):
        chrom = []
        for p in range(1, 60):
            cov = [70, 130, 1100, 20, 5, 300][p % 6]
            groups = rng.integers(0, n_groups, cov)
            alt = int(rng.integers(4))
            entries = [int(g) << 2 | (alt if clusters[g] % 3 == 0 else int(rng.integers(2)) if clusters[g] % 3 == 1
                                      else 2) for g in groups]
            chrom.append((p, entries))
        chroms.append(chrom)
    g, a, b = _both(tmp_path, "long", chroms, clusters, fasta, "", 1e-3, 0.01)
    assert a == b
    assert sum(1 for k in a if k.startswith("cluster_")) == n_clusters
    assert sum(len(x.splitlines()) for k, x in a.items() if k.startswith("cluster_")) > n_clusters * 6


def test_16_and_32_bit_layouts_agree(tmp_path):
    rng = np.random.default_rng(3)
    contigs = [300, 300]
    fasta = _fasta(str(tmp_path / "g.fa"), contigs, True, False, rng)
    chroms, clusters = _synthetic(rng, 200, 4, contigs, 2)
    p = _flat(chroms)
    v = _v()
    r16, m16, l16 = v.variant_calls(p, clusters, fasta)
    # the same pileup with every group id raised past 14 bits: 32-bit layout; clusters extended to match
    shift = 20000
    p32 = FlatPileup(p.chr_locus_off, p.locus_pos, p.locus_entry_off, p.read_ids, p.id_base + (shift << 2))
    cl32 = np.concatenate([np.zeros(shift, np.uint16), clusters])
    r32, m32, l32 = v.variant_calls(p32, cl32, fasta)
    assert len(r16) > 0 and np.array_equal(r16, r32)
    assert np.array_equal(m16, m32[shift:]) and np.array_equal(l16, l32[shift:]) and not l32[:shift].any()
    g16 = str(tmp_path / "a")
    v.variant_calling(p, clusters, fasta, "", 1e-3, 0.01, g16)
    v.variant_calling(p, clusters, fasta, "", 1e-3, 0.01, g16 + "2")
    a, b = vr.read_dir(g16), vr.read_dir(g16 + "2")  # two runs in one process give identical files
    assert a == b
    ref = str(tmp_path / "r")
    vr.write_files(chroms, clusters, fasta, ref, "", 1e-3, 0.01)
    assert a == vr.read_dir(ref)


def test_capacity(tmp_path):
    from secedo_amd import _lib
    rng = np.random.default_rng(4)
    fasta = _fasta(str(tmp_path / "g.fa"), [300], True, False, rng)
    chroms, clusters = _synthetic(rng, 100, 4, [300], 1, extra=False)
    v = _v()
    full, mm, lo = v.variant_calls(_flat(chroms), clusters, fasta)
    assert len(full) > 2
    with pytest.raises(_lib.SecedoError) as e:
        v.variant_calls(_flat(chroms), clusters, fasta, capacity=len(full) - 1)
    assert e.value.code == _lib.E_LIMIT and e.value.required == len(full)
    again, mm2, lo2 = v.variant_calls(_flat(chroms), clusters, fasta, capacity=e.value.required)
    assert np.array_equal(full, again) and np.array_equal(mm, mm2) and np.array_equal(lo, lo2)
    # the records are in the reference's write order
    key = [(int(r["locus"]), int(r["kind"]), int(r["cluster"])) for r in full]
    assert key == sorted(key)


def test_counter_modes_agree(tmp_path, monkeypatch):
    """The counted-entry counters privatised in LDS and as global atomics give the same outputs."""
    rng = np.random.default_rng(8)
    fasta = _fasta(str(tmp_path / "g.fa"), [300, 300], True, False, rng)
    chroms, clusters = _synthetic(rng, 500, 6, [300, 300], 2)
    out = {}
    for mode in ("lds", "global"):
        monkeypatch.setenv("SECEDO_VARIANT_COUNTERS", mode)
        out[mode] = _v().variant_calls(_flat(chroms), clusters, fasta)
    for a, b in zip(out["lds"], out["global"]):
        assert np.array_equal(a, b)
    _, _, mismatch, loci = vr.calls(chroms, clusters, fasta, "", 1e-3, 0.01)
    assert np.array_equal(out["lds"][1], mismatch) and np.array_equal(out["lds"][2], loci)


def test_group_id_past_clusters_is_an_error(tmp_path):
    from secedo_amd import _lib
    with pytest.raises(_lib.SecedoError) as e:
        _v().variant_calls(_flat([[(1, [7 << 2])]]), [1, 1], FEMALE)
    assert e.value.code == _lib.E_INVALID_ARG


# --- 6. end to end after divide_cluster_resident ------------------------------------------------------------------------

def test_clone_tree_end_to_end(tmp_path):
    import secedo_amd
    from secedo_amd import cluster
    n = 300
    p0, truth = clone_tree(n, n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)
    # positions 1.. (the generator's 0-based positions would end the chromosome at once)
    p = FlatPileup(p0.chr_locus_off, p0.locus_pos + 1, p0.locus_entry_off, p0.read_ids, p0.id_base)
    fasta = str(tmp_path / "tree.fa")
    with open(fasta, "w") as f:  # haploid reference: A everywhere (the A clone's base at the A|B loci)
        f.write(">chr1\n" + _wrap("A" * p.n_loci) + "\n")
    ident = np.arange(n)
    args = (500, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, ident.astype(np.uint32), n)
        cl, _, _ = cluster.divide_cluster_resident(plan, res, *args, "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40)
        d_res = str(tmp_path / "resident")
        secedo_amd.variant_calling_resident(plan, res, cl, fasta, "", 1e-3, 0.01, d_res)
    d_host = str(tmp_path / "host")
    secedo_amd.variant_calling(p, cl, fasta, "", 1e-3, 0.01, d_host)
    a = vr.read_dir(d_res)
    assert a == vr.read_dir(d_host)
    b_label = int(np.bincount(cl[truth == 0]).argmax())
    a_labels = {int(x) for x in cl[(truth == 1) | (truth == 2)]}
    assert b_label not in a_labels
    b_sites = {int(line.split("\t")[1]) for line in a["cluster_%d.vcf" % b_label].splitlines() if line[0] != "#"}
    ab_loci = set()  # the A|B loci: B cells read base 1 (C) where A cells read base 0
    for l in range(p.n_loci):
        e = p.id_base[int(p.locus_entry_off[l]):int(p.locus_entry_off[l + 1])]
        cells, bases = e >> 2, e & 3
        if ((bases[truth[cells] == 0] == 1).mean() if (truth[cells] == 0).any() else 0) > 0.8 and \
                ((bases[np.isin(truth[cells], (1, 2))] == 0).mean() if np.isin(truth[cells], (1, 2)).any() else 0) > 0.8:
            ab_loci.add(int(p.locus_pos[l]))
    assert len(b_sites & ab_loci) > 0.5 * len(ab_loci) > 0
    for lab in a_labels:
        sites = {int(line.split("\t")[1]) for line in a["cluster_%d.vcf" % lab].splitlines() if line[0] != "#"}
        assert not (sites & b_sites & ab_loci)
    ref = str(tmp_path / "ref")
    vr.write_files(vr.from_flat(p), cl, fasta, ref, "", 1e-3, 0.01)
    assert a == vr.read_dir(ref)


# --- 8. the compiled C++ entry point ----------------------------------------------------------------------------------

def test_cpp_entry_point_equals_python(tmp_path):
    """tests/cpp/variant_calling_test.cpp: secedo_amd::variant_calling of include/secedo_pipeline.hpp on
    reference-shaped PosData, against the Python entry point."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "variant_calling_test")
    lib = os.path.join(root, "secedo_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "variant_calling_test.cpp"), "-o", exe, "-L" + lib,
                    "-lsecedo_variant", "-Wl,-rpath," + lib], check=True)
    rng = np.random.default_rng(9)
    chroms, clusters = _synthetic(rng, 200, 5, [11, 7, 6], 3)
    p = _flat(chroms)
    vc.write_flat(str(tmp_path / "p.bin"), p, len(clusters))
    vc.write_clusters(str(tmp_path / "c.bin"), clusters)
    d_cpp, d_py = str(tmp_path / "cpp"), str(tmp_path / "py")
    subprocess.run([exe, str(tmp_path / "p.bin"), str(tmp_path / "c.bin"), MALE, MALE_MAP, "0.001", "0.01", d_cpp],
                   check=True)
    _v().variant_calling(p, clusters, MALE, MALE_MAP, 1e-3, 0.01, d_py)
    a = vr.read_dir(d_cpp)
    assert a == vr.read_dir(d_py) and len(a) == 5 + 3
