"""The bgzf VCF output on the GPU: the formatter kernels against the host formatter of the plain route on hand-built
records (tests/vcf_output_cases.py), and variant_calling(..., vcf_output="bgzf") against the plain route end to end:
every .vcf.gz inflates to the bytes of its .vcf (but for ##fileDate), `variant` and `scores` are the same files."""
import gzip
import os
import shutil

import numpy as np
import pytest

import secedo_amd
from secedo_amd import _lib, secedo_main, variant
from secedo_amd.pileup import FlatPileup
from tests import bgzf_deflate_cases as dc
from tests import variant_ref as vr
from tests import vcf_output_cases as vc
from tests.clone_tree_gen import clone_tree
from tests.test_gpu_variant import FEMALE, MALE, MALE_MAP, _fasta, _flat, _synthetic, _wrap

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


# --- 1. the formatter against the host ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(vc.ALL))
def test_formatter_equals_the_plain_routes_text(name):
    case = vc.ALL[name]()
    want = variant.format_host(*case.args())
    assert want == case.expected()
    assert variant.format_device(*case.args()) == want


def test_formatter_without_preambles_and_with_one_chromosome():
    case = vc.line_rules()
    case.preambles = None
    assert variant.format_device(*case.args()) == variant.format_host(*case.args())


def test_a_line_straddles_the_cut_and_the_file_still_inflates():
    case = vc.long_file()
    files = variant.format_device(*case.args())
    text = files[0]
    assert len(text) > 2 * dc.CUT and text[dc.CUT - 1:dc.CUT] != b"\n"
    raws = variant.bgzf_deflate_many(files)
    for raw, data in zip(raws, files):
        dc.check_file(raw, data, with_tokens=False)
    assert variant.vcf_stats()["stored_blocks"] == 0


# --- 2. end to end -----------------------------------------------------------------------------------------------

def _read_plain(d):
    return {n: vr.strip_date(open(os.path.join(d, n)).read()) for n in sorted(os.listdir(d))}


def _read_bgzf(d):
    """{name as the plain route has it: text}; every .vcf.gz checked as a BGZF file on the way."""
    out = {}
    for n in sorted(os.listdir(d)):
        raw = open(os.path.join(d, n), "rb").read()
        if n.endswith(".vcf.gz"):
            data = gzip.decompress(raw)
            dc.check_file(raw, data, with_tokens=False)
            out[n[:-3]] = vr.strip_date(data.decode())
        else:
            out[n] = raw.decode()
    return out


def _compare(tmp_path, name, p, clusters, fasta, map_file="", theta=0.01):
    plain, bgzf = str(tmp_path / (name + "_plain")), str(tmp_path / (name + "_bgzf"))
    variant.variant_calling(p, clusters, fasta, map_file, 1e-3, theta, plain)
    assert variant.vcf_stats()["output"] == "plain"
    times = variant.variant_calling(p, clusters, fasta, map_file, 1e-3, theta, bgzf, vcf_output="bgzf")
    st = variant.vcf_stats()
    a, b = _read_plain(plain), _read_bgzf(bgzf)
    assert a == b, [k for k in a if a[k] != b.get(k)]
    names = os.listdir(bgzf)
    assert not [n for n in names if n.endswith(".vcf")] and not [n for n in os.listdir(plain) if n.endswith(".gz")]
    n_vcf = sum(n.endswith(".vcf.gz") for n in names)
    assert n_vcf == int(max(clusters)) + 2 and sorted(set(names) - {"scores", "variant"}) == sorted(
        n for n in names if n.endswith(".vcf.gz"))
    # the stats are those of the files
    text = {n: gzip.decompress(open(os.path.join(bgzf, n), "rb").read()) for n in names if n.endswith(".vcf.gz")}
    assert st["output"] == "bgzf" and st["files"] == n_vcf
    assert st["text_bytes"] == sum(map(len, text.values()))
    assert st["blocks"] == sum(-(-len(t) // dc.CUT) for t in text.values()) and st["stored_blocks"] == 0
    assert st["compressed_bytes"] == sum(os.path.getsize(os.path.join(bgzf, n)) for n in text)
    assert times["write_ms"] > 0 and variant.get_vcf_output() == "plain"  # the keyword was a scoped override
    return a, bgzf


@pytest.mark.parametrize("kind", ["diploid", "haploid", "mapped"])
def test_synthetic_bgzf_equals_plain(tmp_path, kind):
    rng = np.random.default_rng(["diploid", "haploid", "mapped"].index(kind) + 31)
    if kind == "mapped":
        fasta, mp, contigs, n_chr = MALE, MALE_MAP, [11, 7, 6], 3
    else:
        contigs = [400, 300, 250, 200]
        fasta, mp, n_chr = _fasta(str(tmp_path / "g.fa"), contigs, kind != "haploid", False, rng), "", 4
    chroms, clusters = _synthetic(rng, 300, 5, contigs, n_chr)
    a, _ = _compare(tmp_path, kind, _flat(chroms), clusters, fasta, mp)
    assert sum(len(x) for x in a.values()) > 1000


def test_long_grouped_loci_and_many_clusters(tmp_path):
    rng = np.random.default_rng(6)
    fasta = _fasta(str(tmp_path / "g.fa"), [500, 500], True, False, rng)
    n_groups, n_clusters = 2000, 90
    clusters = rng.integers(0, n_clusters, n_groups).astype(np.uint16)
    chroms = []
    for c in range(2):
        chrom = []
        for p in range(1, 60):
            cov = [70, 130, 1100, 20, 5, 300][p % 6]
            groups = rng.integers(0, n_groups, cov)
            alt = int(rng.integers(4))
            chrom.append((p, [int(g) << 2 | (alt if clusters[g] % 3 == 0 else int(rng.integers(2))
                                             if clusters[g] % 3 == 1 else 2) for g in groups]))
        chroms.append(chrom)
    a, _ = _compare(tmp_path, "long", _flat(chroms), clusters, fasta)
    assert sum(1 for k in a if k.startswith("cluster_")) == int(clusters.max()) + 1


def test_clone_tree_resident_and_both_id_layouts(tmp_path):
    n = 300
    p0, truth = clone_tree(n, n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)
    p = FlatPileup(p0.chr_locus_off, p0.locus_pos + 1, p0.locus_entry_off, p0.read_ids, p0.id_base)
    fasta = str(tmp_path / "tree.fa")
    with open(fasta, "w") as f:
        f.write(">chr1\n" + _wrap("A" * p.n_loci) + "\n")
    clusters = (truth % 3).astype(np.uint16)
    a, d16 = _compare(tmp_path, "tree", p, clusters, fasta)
    assert sum(len(x) for x in a.values()) > 1000
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, np.arange(n, dtype=np.uint32), n)
        d_res = str(tmp_path / "resident")
        secedo_amd.variant_calling_resident(plan, res, clusters, fasta, "", 1e-3, 0.01, d_res, vcf_output="bgzf")
    assert _read_bgzf(d_res) == a
    shift = 20000  # every group id past 14 bits: the 32-bit layout
    p32 = FlatPileup(p.chr_locus_off, p.locus_pos, p.locus_entry_off, p.read_ids, p.id_base + (shift << 2))
    d32 = str(tmp_path / "wide")
    variant.variant_calling(p32, np.concatenate([np.zeros(shift, np.uint16), clusters]), fasta, "", 1e-3, 0.01, d32,
                            vcf_output="bgzf")
    b = _read_bgzf(d32)
    assert {k: v for k, v in b.items() if k != "scores"} == {k: v for k, v in a.items() if k != "scores"}
    # but for the date, the files of two routes into one layout are the same bytes
    for n_ in os.listdir(d_res):
        if n_.endswith(".gz"):
            assert gzip.decompress(open(os.path.join(d_res, n_), "rb").read()).count(b"\n") == \
                gzip.decompress(open(os.path.join(d16, n_), "rb").read()).count(b"\n")


def test_the_setting_and_the_environment_route_a_call(tmp_path, monkeypatch):
    p = _flat([[(1, [i << 2 for i in range(10)])]])
    variant.set_vcf_output("bgzf")
    try:
        variant.variant_calling(p, [1] * 10, FEMALE, "", 1e-3, 1e-3, str(tmp_path / "a"))
        assert sorted(os.listdir(tmp_path / "a")) == ["cluster_0.vcf.gz", "cluster_1.vcf.gz", "common.vcf.gz", "scores",
                                                      "variant"]
        variant.variant_calling(p, [1] * 10, FEMALE, "", 1e-3, 1e-3, str(tmp_path / "b"), vcf_output="plain")
        assert "common.vcf" in os.listdir(tmp_path / "b") and variant.get_vcf_output() == "bgzf"
    finally:
        variant.set_vcf_output("plain")
    common = gzip.decompress((tmp_path / "a" / "common.vcf.gz").read_bytes()).decode()
    assert common == open(tmp_path / "b" / "common.vcf").read() and common.count("\n") == 1
    assert (tmp_path / "a" / "scores").read_bytes() == (tmp_path / "b" / "scores").read_bytes()
    # no cells: nothing is written on either route
    variant.variant_calling(_flat([[]]), [], FEMALE, "", 1e-3, 1e-3, str(tmp_path / "none"), vcf_output="bgzf")
    assert not os.path.exists(tmp_path / "none")


def test_errors_equal_the_plain_routes(tmp_path):
    p = _flat([[(1, [i << 2 for i in range(10)])]])

    def message(out_dir, output, clusters=(1,) * 10, fasta=FEMALE, pileup=p):
        with pytest.raises(_lib.SecedoError) as e:
            variant.variant_calling(pileup, list(clusters), fasta, "", 1e-3, 1e-3, out_dir, vcf_output=output)
        return e.value.code, str(e.value)
    # a directory where the first file should go: neither root nor a user can open it for writing
    for output, name in (("plain", "cluster_0.vcf"), ("bgzf", "cluster_0.vcf.gz")):
        os.makedirs(tmp_path / output / name)
    a, b = message(str(tmp_path / "plain"), "plain"), message(str(tmp_path / "bgzf"), "bgzf")
    assert "cannot write " + str(tmp_path / "plain" / "cluster_0.vcf") in a[1]
    assert b == (a[0], a[1].replace(str(tmp_path / "plain" / "cluster_0.vcf"), str(tmp_path / "bgzf" / "cluster_0.vcf.gz")))
    # out_dir is a file; the reference genome is missing; a group id past the clusters
    blocker = tmp_path / "file"
    blocker.write_text("x")
    assert message(str(blocker / "o"), "bgzf") == message(str(blocker / "o"), "plain")
    missing = str(tmp_path / "no.fa")
    assert message(str(tmp_path / "m"), "bgzf", fasta=missing) == message(str(tmp_path / "m"), "plain", fasta=missing)
    wide = _flat([[(1, [7 << 2] * 12)]])
    assert message(str(tmp_path / "g"), "bgzf", (1, 1), pileup=wide) == message(str(tmp_path / "g"), "plain", (1, 1), pileup=wide)


# --- 3. the command line -----------------------------------------------------------------------------------------

def test_cli_writes_vcf_gz(tmp_path):
    d = tmp_path / "ten"
    d.mkdir()
    shutil.copy(os.path.join(DATA, "ten_rows.pileup.bin"), d / "s_22.pileup.bin")
    flags = ["-i", str(d), "--chromosomes=22", "--reference_genome=" + os.path.join(DATA, "genome_diploid_female.fa")]
    a, b = str(tmp_path / "plain") + "/", str(tmp_path / "bgzf") + "/"
    assert secedo_main.main(flags + ["-o", a]) == 0
    assert secedo_main.main(flags + ["-o", b, "--vcf_output", "bgzf"]) == 0
    assert variant.vcf_stats()["output"] == "bgzf"
    want = {k: v for k, v in _read_plain(a).items() if k.endswith(".vcf") or k in ("variant", "scores")}
    got = {k: v for k, v in _read_bgzf(b).items() if k in want}
    assert "common.vcf" in want and "cluster_0.vcf" in want and got == want
    assert not [n for n in os.listdir(b) if n.endswith(".vcf")]
    assert secedo_main.main(flags + ["-o", b, "--vcf_output", "zip"]) == 1
