"""Per-cell allele counts at the called variants on the GPU (secedo_amd/csrc/allele_kernels.hip) against the
restatement tests/allele_ref.py: integers and bytes, no tolerance. The kernels alone on hand-made sites (the wave's
register sort at its chunk edges, the sorted route of deep loci, both id_base widths), then the files of both calling
functions, both outputs and many formatter ranges."""
import gzip
import os

import numpy as np
import pytest

from secedo_amd.pileup import FlatPileup
from tests import allele_ref as ar
from tests import variant_ref as vr
from tests.clone_tree_gen import clone_tree

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
HAPLOID = os.path.join(DATA, "genome_female.fa")
COMMON, CLUSTER = 1, 2


def _v():
    from secedo_amd import variant
    return variant


def _flat(chromosomes):
    chr_off, pos, off, idb = [0], [], [0], []
    for chrom in chromosomes:
        for p, entries in chrom:
            pos.append(p)
            idb.extend(entries)
            off.append(len(idb))
        chr_off.append(len(pos))
    idb = np.asarray(idb, dtype=np.uint32)
    return FlatPileup(np.asarray(chr_off), np.asarray(pos), np.asarray(off, dtype=np.uint64),
                      np.arange(len(idb), dtype=np.uint32), idb)


def _records(rows):
    rec = np.zeros(len(rows), dtype=_v().RECORD_DTYPE)
    for i, (locus, kind, cluster, genotype) in enumerate(rows):
        rec[i] = (locus, cluster, genotype, kind, (0, 0, 0, 0))
    return rec


def _check(p, rec, locus_ref, n_cells, sites="all"):
    """allele_counts equals the restatement; -> the restatement's (sites, pairs, totals)."""
    got = _v().allele_counts(p, rec, locus_ref, n_cells, sites)
    s = ar.masks(rec, locus_ref, sites)
    pairs, totals = ar.counts(p, s)
    want = ar.as_arrays(s, pairs, totals)
    for k in ("site_locus", "ref_mask", "alt_mask", "totals"):
        assert np.array_equal(got[k], want[k]), k
    bad = np.nonzero(got["pairs"] != want["pairs"])[0] if len(got["pairs"]) == len(want["pairs"]) else None
    assert bad is not None and len(bad) == 0, (len(got["pairs"]), len(want["pairs"]),
                                               None if bad is None else (got["pairs"][bad[:3]], want["pairs"][bad[:3]]))
    return s, pairs, totals


# --- 1. kernel edges: one site among non-site loci ---------------------------------------------------------------------

def _site_entries(rng, depth, how, n_cells):
    """`depth` entries of one locus in shuffled group order; the site's masks will be ref C, alt A|G (T is `other`)."""
    if how == "one_group":
        groups = np.full(depth, 7)
    elif how == "all_distinct":
        groups = rng.choice(n_cells, depth, replace=False)
    else:  # every group 1 to 5 times
        groups = []
        while len(groups) < depth:
            groups += [int(rng.integers(n_cells))] * int(rng.integers(1, 6))
        groups = rng.permutation(np.asarray(groups[:depth]))
    bases = rng.integers(0, 4, depth)  # all three classes
    return [int(g) << 2 | int(b) for g, b in zip(groups, bases)]


@pytest.mark.parametrize("how", ["repeats", "one_group", "all_distinct"])
@pytest.mark.parametrize("depth", [1, 63, 64, 65, 128, 129])
def test_one_site_at_the_chunk_edges(depth, how):
    rng = np.random.default_rng(depth * 10 + len(how))
    n_cells = 400
    filler = lambda k: [int(g) << 2 | int(rng.integers(4)) for g in rng.integers(0, n_cells, k)]  # noqa: E731
    p = _flat([[(1, filler(70)), (2, filler(5)), (3, _site_entries(rng, depth, how, n_cells)), (4, filler(200)),
                (5, [])]])
    locus_ref = np.asarray([0, 0, 1 << 3 | 1, 0, 0], dtype=np.uint8)
    rec = _records([(2, CLUSTER, 0, 0), (2, CLUSTER, 3, 2 << 3 | 2)])  # clusters call A/A and G/G under ref C/C
    s, pairs, totals = _check(p, rec, locus_ref, n_cells)
    assert s == [(2, 0b0010, 0b0101)] and sum(totals[0]) == depth
    if depth >= 63:
        assert all(t > 0 for t in totals[0])  # alt, ref and other all occur
    if how == "one_group":
        assert len(pairs) == 1 and pairs[0][1] == 7
    if how == "all_distinct":
        assert len(pairs) == depth


def test_a_group_past_the_cells_is_an_error():
    from secedo_amd import _lib
    p = _flat([[(1, [3 << 2, 9 << 2 | 1])]])
    with pytest.raises(_lib.SecedoError) as e:
        _v().allele_counts(p, _records([(0, COMMON, 0, 1 << 3 | 1)]), np.zeros(1, np.uint8), 9)
    assert e.value.code == _lib.E_INVALID_ARG


# --- 2. deep loci: the sorted route, both id_base widths -----------------------------------------------------------------

def test_deep_locus_16_bit():
    """3000 entries over 70 groups, beside wave-route sites before and after it."""
    rng = np.random.default_rng(1)
    groups = rng.choice(5000, 70, replace=False)
    deep = [int(g) << 2 | int(b) for g, b in zip(rng.choice(groups, 3000), rng.integers(0, 4, 3000))]
    shallow = lambda k: [int(g) << 2 | int(rng.integers(4)) for g in rng.integers(0, 5000, k)]  # noqa: E731
    p = _flat([[(1, shallow(100)), (2, deep), (3, shallow(128)), (4, shallow(140))]])
    assert int(p.id_base.max()) <= 0xFFFF
    rec = _records([(l, COMMON, 0, 3 << 3 | 3) for l in range(4)])
    s, pairs, totals = _check(p, rec, np.zeros(4, np.uint8), 5000)
    assert len(s) == 4 and sum(1 for q in pairs if q[0] == 1) == 70 and sum(totals[1]) == 3000
    st = _v().allele_stats()
    assert st["deep_sites"] == 2 and st["sites"] == 4 and st["entries_read"] == 3368 and st["pairs"] == len(pairs)


def test_deep_locus_32_bit():
    """40 000 entries over 20 000 groups whose ids pass 16383: id_base32."""
    rng = np.random.default_rng(2)
    n_cells = 70000
    groups = rng.choice(np.arange(30000, n_cells), 20000, replace=False)
    who = np.concatenate([groups, rng.choice(groups, 20000)])
    rng.shuffle(who)
    deep = (who.astype(np.uint32) << 2 | rng.integers(0, 4, len(who)).astype(np.uint32)).tolist()
    p = _flat([[(5, deep), (9, [int(g) << 2 | 1 for g in groups[:90]])]])
    assert int(p.id_base.max()) > 0xFFFF
    rec = _records([(0, CLUSTER, 1, 0 << 3 | 3), (1, COMMON, 0, 3 << 3 | 3)])
    s, pairs, totals = _check(p, rec, np.asarray([1 << 3 | 1, 1 << 3 | 1], np.uint8), n_cells)
    assert sum(1 for q in pairs if q[0] == 0) == 20000 and sum(totals[0]) == 40000
    _check(p, rec, np.asarray([1 << 3 | 1, 1 << 3 | 1], np.uint8), n_cells, "cluster")


# --- 3. several chromosomes: site numbers and CHROM ------------------------------------------------------------------------

def _wrap(s, w=60):
    return "\n".join(s[i:i + w] for i in range(0, len(s), w))


def _read(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            out[name] = f.read()
    return out


def _expected(p, clusters, fasta, selection, names=None, theta=0.01):
    """The restatement's files for the calls the GPU makes on p (its records are test_gpu_variant.py's subject)."""
    v = _v()
    rec, _, _ = v.variant_calls(p, clusters, fasta, "", 1e-3, theta)
    locus_ref, _ = v.reference_genotypes(fasta, p.chr_locus_off, p.locus_pos)
    return ar.files(p, rec, locus_ref, len(clusters), selection, names), rec


def test_sites_at_the_ends_of_chromosomes(tmp_path):
    """Three chromosomes of an all-A haploid genome; the first and last counted locus of each reads C in every cell
    (a call), the loci between read A (none); chromosome 1 goes on past its contig's end with loci that are not counted,
    right before chromosome 2's first site."""
    fasta = str(tmp_path / "g.fa")
    with open(fasta, "w") as f:
        for c in range(3):
            f.write(">chr%d\n%s\n" % (c + 1, _wrap("A" * 40)))
    n_cells = 30
    alt = lambda: [g << 2 | 1 for g in range(n_cells)]  # noqa: E731
    ref = lambda: [g << 2 | 0 for g in range(0, n_cells, 2)]  # noqa: E731
    chroms = [[(1, alt()), (7, ref()), (40, alt()), (41, alt()), (50, alt())],
              [(1, alt()), (2, ref()), (3, ref()), (30, alt())],
              [(5, alt()), (6, alt())]]
    p = _flat(chroms)
    clusters = np.asarray([0] * 15 + [1] * 15, dtype=np.uint16)
    d = str(tmp_path / "out")
    _v().variant_calling(p, clusters, fasta, "", 1e-3, 0.01, d, allele_counts="all")
    got = _read(os.path.join(d, "allele_counts"))
    want, rec = _expected(p, clusters, fasta, "all")
    assert got == want
    lines = [l.split("\t") for l in got["cellSNP.base.vcf"].decode().splitlines() if l[0] != "#"]
    assert [(l[0], l[1]) for l in lines] == [("1", "1"), ("1", "40"), ("2", "1"), ("2", "30"), ("3", "5"), ("3", "6")]
    assert all(l[3] == "A" and l[4] == "C" and l[7] == "AD=30;DP=30;OTH=0" for l in lines)


# --- 4. end to end on the clone tree ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The clone_tree pileup of test_gpu_variant.py, clustered once; the resident pileup is used inside the fixture."""
    import secedo_amd
    from secedo_amd import cluster
    tmp = tmp_path_factory.mktemp("allele_tree")
    n = 300
    p0, _ = clone_tree(n, n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)
    p = FlatPileup(p0.chr_locus_off, p0.locus_pos + 1, p0.locus_entry_off, p0.read_ids, p0.id_base)
    fasta = str(tmp / "tree.fa")
    with open(fasta, "w") as f:
        f.write(">chr1\n" + _wrap("A" * p.n_loci) + "\n")
    ident = np.arange(n)
    args = (500, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01)
    d_res = str(tmp / "resident")
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, ident.astype(np.uint32), n)
        cl, _, _ = cluster.divide_cluster_resident(plan, res, *args, "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40)
        secedo_amd.variant_calling_resident(plan, res, cl, fasta, "", 1e-3, 0.01, d_res, allele_counts="all")
    ref_dir = str(tmp / "ref")
    vr.write_files(vr.from_flat(p), cl, fasta, ref_dir, "", 1e-3, 0.01)
    return {"p": p, "cl": cl, "fasta": fasta, "resident": d_res, "ref": ref_dir, "tmp": tmp}


def _chrom_pos(text):
    return {tuple(l.split("\t")[:2]) for l in text.splitlines() if l and l[0] != "#"}


@pytest.mark.parametrize("selection", ["all", "cluster"])
def test_clone_tree_files(tree, selection):
    import secedo_amd
    d = str(tree["tmp"] / ("host_" + selection))
    secedo_amd.variant_calling(tree["p"], tree["cl"], tree["fasta"], "", 1e-3, 0.01, d, allele_counts=selection)
    got = _read(os.path.join(d, "allele_counts"))
    want, rec = _expected(tree["p"], tree["cl"], tree["fasta"], selection)
    assert sorted(got) == sorted(ar.NAMES)
    for name in ar.NAMES:
        assert got[name] == want[name], name
    # the sites against the VCFs the CPU restatement of the calls writes, not through the GPU's records
    cpu = set()
    for name in os.listdir(tree["ref"]):
        if name.endswith(".vcf") and (selection == "all" or name.startswith("cluster_")):
            with open(os.path.join(tree["ref"], name)) as f:
                cpu |= _chrom_pos(f.read())
    assert _chrom_pos(got["cellSNP.base.vcf"].decode()) == cpu and len(cpu) > 100
    st = secedo_amd.allele_stats()
    assert st["selection"] == selection and st["output"] == "plain" and st["sites"] == len(cpu)
    assert st["text_bytes"] == sum(len(got[n]) for n in ar.NAMES[:4]) and st["ranges"] == 1
    head = [int(x) for x in got["cellSNP.tag.DP.mtx"].decode().splitlines()[2].split("\t")]
    assert head == [st["sites"], 300, st["nnz_dp"]] and st["nnz_ad"] <= st["nnz_dp"] <= st["pairs"]
    if selection == "all":  # the resident call wrote the same files
        assert _read(os.path.join(tree["resident"], "allele_counts")) == got


def test_clone_tree_bgzf_inflates_to_the_plain_bytes(tree):
    import secedo_amd
    d = str(tree["tmp"] / "bgzf")
    secedo_amd.variant_calling(tree["p"], tree["cl"], tree["fasta"], "", 1e-3, 0.01, d, vcf_output="bgzf",
                               allele_counts="all")
    got = _read(os.path.join(d, "allele_counts"))
    plain = _read(os.path.join(tree["resident"], "allele_counts"))
    assert sorted(got) == sorted([n + ".gz" for n in ar.NAMES[:4]] + ["cellSNP.samples.tsv"])
    for name in ar.NAMES[:4]:
        assert gzip.decompress(got[name + ".gz"]) == plain[name], name
        assert got[name + ".gz"][-28:-26] == b"\x1f\x8b" and got[name + ".gz"][12:14] == b"BC"  # BGZF, EOF member last
    assert got["cellSNP.samples.tsv"] == plain["cellSNP.samples.tsv"]
    st = secedo_amd.allele_stats()
    assert st["output"] == "bgzf" and st["compressed_bytes"] == sum(len(got[n + ".gz"]) for n in ar.NAMES[:4])
    assert sorted(os.listdir(d)) == sorted(["allele_counts", "variant", "scores", "common.vcf.gz"] +
                                           ["cluster_%d.vcf.gz" % i for i in range(int(tree["cl"].max()) + 1)])


@pytest.mark.parametrize("output,batch,ranges", [("plain", 256, 100), ("bgzf", 1 << 20, 5)])
def test_clone_tree_many_ranges_same_bytes(tree, monkeypatch, output, batch, ranges):
    """A site to a range under 256 bytes; under bgzf, where every range is a run of the encoder, a few sites to one."""
    import secedo_amd
    monkeypatch.setenv("SECEDO_ALLELE_BATCH_BYTES", str(batch))
    d = str(tree["tmp"] / ("ranges_" + output))
    secedo_amd.variant_calling(tree["p"], tree["cl"], tree["fasta"], "", 1e-3, 0.01, d, vcf_output=output,
                               allele_counts="all")
    got = _read(os.path.join(d, "allele_counts"))
    plain = _read(os.path.join(tree["resident"], "allele_counts"))
    for name in ar.NAMES[:4]:
        assert (got[name] if output == "plain" else gzip.decompress(got[name + ".gz"])) == plain[name], name
    assert secedo_amd.allele_stats()["ranges"] > ranges


def test_cell_names(tree, tmp_path):
    import secedo_amd
    from secedo_amd import _lib
    names = ["AAAC-%d" % i for i in range(300)]
    d = str(tmp_path / "named")
    secedo_amd.variant_calling(tree["p"], tree["cl"], tree["fasta"], "", 1e-3, 0.01, d, allele_counts="cluster",
                               cell_names=names)
    with open(os.path.join(d, "allele_counts", "cellSNP.samples.tsv")) as f:
        assert f.read().split("\n") == names + [""]
    path = tmp_path / "names.txt"
    path.write_text("".join(n + "\n" for n in names[::-1]))
    secedo_amd.variant_calling(tree["p"], tree["cl"], tree["fasta"], "", 1e-3, 0.01, d, allele_counts="cluster",
                               cell_names=str(path))
    with open(os.path.join(d, "allele_counts", "cellSNP.samples.tsv")) as f:
        assert f.read().split("\n") == names[::-1] + [""]
    with pytest.raises(_lib.SecedoError, match="299 cell names for 300 cells") as e:
        secedo_amd.variant_calling(tree["p"], tree["cl"], tree["fasta"], "", 1e-3, 0.01, str(tmp_path / "short"),
                                   allele_counts="all", cell_names=names[:299])
    assert e.value.code == _lib.E_INVALID_ARG and not os.path.exists(tmp_path / "short" / "allele_counts")
    secedo_amd.variant_calling(tree["p"], tree["cl"], tree["fasta"], "", 1e-3, 0.01, d, allele_counts="cluster")
    with open(os.path.join(d, "allele_counts", "cellSNP.samples.tsv")) as f:  # the names were for their call only
        assert f.read().split("\n")[:2] == ["cell_0", "cell_1"]


def test_cli_writes_what_the_call_writes(tmp_path):
    """secedo_main with --allele_counts and --cell_names on a .bin pileup and a given clustering, against
    variant_calling on the same pileup read by the host reader."""
    import secedo_amd
    from secedo_amd import secedo_main
    from tests.pileup_file_writer import clone_tree_files
    p0, truth = clone_tree(300, n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)
    p = FlatPileup(p0.chr_locus_off, p0.locus_pos + 1, p0.locus_entry_off, p0.read_ids, p0.id_base)  # positions from 1
    clone_tree_files(str(tmp_path / "bin"), p, ("1",))
    hp, _, _ = secedo_amd.read_pileup(str(tmp_path / "bin" / "s_1.pileup.bin"), secedo_amd.get_grouping(), None, 100,
                                      None, True)
    flat = FlatPileup(np.asarray([0] + [hp.n_loci] * 24, np.uint32), hp.locus_pos, hp.locus_entry_off, hp.read_ids,
                      hp.id_base)
    cl = np.where(truth == 0, 1, 2).astype(np.uint16)  # not 0: the calls never compare cluster 0 with the others
    (tmp_path / "clustering").write_text(",".join(str(int(c)) for c in cl) + "\n")
    names = ["bc%03d" % i for i in range(300)]
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    fa = str(tmp_path / "g.fa")
    with open(fa, "w") as f:
        f.write(">chr1\n" + _wrap("A" * (int(hp.locus_pos.max()) + 10)) + "\n")
    ov, od = str(tmp_path / "ov") + "/", str(tmp_path / "od")
    assert secedo_main.main(["-i", str(tmp_path / "bin"), "-o", ov, "--chromosomes=1", "--reference_genome=" + fa,
                             "--clustering=" + str(tmp_path / "clustering"), "--allele_counts", "cluster",
                             "--cell_names", str(tmp_path / "names.txt")]) == 0
    secedo_amd.variant_calling(flat, cl, fa, "", 1e-3, 0.01, od, allele_counts="cluster", cell_names=names)
    got = _read(os.path.join(ov, "allele_counts"))
    assert got == _read(os.path.join(od, "allele_counts")) and sorted(got) == sorted(ar.NAMES)
    assert len(got["cellSNP.base.vcf"].splitlines()) > 100 and got["cellSNP.samples.tsv"].startswith(b"bc000\nbc001\n")


# --- 5. off is off -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["default", "none"])
def test_off_is_off(tmp_path, how):
    import secedo_amd
    chroms = [[(1, [i << 2 for i in range(50)])], [(1, [i << 2 | 3 for i in range(50)])]]
    d = str(tmp_path / "out")
    kw = {} if how == "default" else {"allele_counts": "none"}
    secedo_amd.variant_calling(_flat(chroms), [1] * 25 + [2] * 25, HAPLOID, "", 1e-3, 1e-3, d, **kw)
    assert sorted(os.listdir(d)) == ["cluster_0.vcf", "cluster_1.vcf", "cluster_2.vcf", "common.vcf", "scores",
                                     "variant"]
    st = secedo_amd.allele_stats()
    assert st.pop("selection") == "none" and st.pop("output") == "plain" and all(v == 0 for v in st.values()), st
