"""The files divide_cluster writes (include/secedo_cluster.h) and the secedo CLI end to end
(python -m secedo_amd.secedo_main) on planted clone trees, on the reference's own binary fixtures, with and
without variant calling."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import cluster, secedo_main
from tests import golden_util as gu
from tests.clone_tree_gen import clone_tree
from tests.pileup_file_writer import clone_tree_files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(gu.GOLDEN, "data")
TREE = dict(n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)
NO_POS = 16383


def _read_vec(path):
    text = open(path).read()
    assert text.endswith("\n")
    return np.asarray([int(x) for x in text.strip().split(",")], dtype=np.int64)


def _tree_args():
    p, truth = clone_tree(300, **dict(dict(f_ab=0.5, f_a12=0.05), **TREE))
    ident = np.arange(300)
    return p, truth, (500, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01)


def test_divide_cluster_files(tmp_path):
    p, truth, args = _tree_args()
    out = str(tmp_path / "out") + "/"
    cl, idx, recs = cluster.divide_cluster(p, *args, 1, out, "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40,
                                           write_files=True)
    cl0, idx0, recs0 = cluster.divide_cluster(p, *args, 1, str(tmp_path / "unused"), "ADD_MIN", "BIC", "SPECTRAL6",
                                              False, True, 40)
    assert np.array_equal(cl, cl0) and idx == idx0 and recs == recs0
    assert not os.path.exists(tmp_path / "unused")  # defaults write nothing
    assert [r["marker"] for r in recs] == ["", "A", "AA", "AB", "B"]
    expect = {"clustering"}
    for r in recs:
        m = r["marker"]
        expect.add("significant_positions" + m)
        if r["eigenvalues"]:
            expect |= {"sim_mat_eigenvalues%s.csv" % m, "sim_mat_eigenvectors_norm%s.csv" % m}
        if r["num_clusters"] > 1:
            expect.add("spectral_clustering" + m)
        if r["em"] == "run":
            expect.add("expectation_maximization" + m)
    assert set(os.listdir(out)) == expect
    assert "expectation_maximization" in expect and "expectation_maximizationA" not in expect
    assert np.array_equal(_read_vec(out + "clustering"), cl)
    for r in recs:
        m = r["marker"]
        if r["eigenvalues"]:
            vals = [float(x) for x in open(out + "sim_mat_eigenvalues%s.csv" % m).read().split()]
            assert vals == r["eigenvalues"]
            rows = [list(map(float, l.split())) for l in open(out + "sim_mat_eigenvectors_norm%s.csv" % m)]
            assert len(rows) == r["cells"] and all(len(x) == 7 for x in rows)
            assert np.allclose(np.linalg.norm(np.asarray(rows), axis=1), 1.0, atol=1e-12)
    # the top level's labels: every cell in the sub-cluster, labels 0/1 before EM, truncated probabilities after
    sc = _read_vec(out + "spectral_clustering")
    assert len(sc) == 300 and set(sc.tolist()) <= {0, 1}
    em = _read_vec(out + "expectation_maximization")
    assert len(em) == 300 and set(em.tolist()) <= {0, 1}
    # below the top level, the cells outside the sub-cluster are NO_POS
    sa = _read_vec(out + "spectral_clusteringA")
    assert (sa == NO_POS).sum() == 300 - recs[1]["cells"] and set(sa[sa != NO_POS].tolist()) <= {0, 1}
    # the top level's significant positions are the filter's kept positions
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, np.arange(300, dtype=np.uint32), 300)
        f, _ = secedo_amd.filter_resident(plan, res, np.arange(300), 0.01)
        kept = f["pos"].cpu().numpy()[:f["n_loci"]]
    lines = open(out + "significant_positions").read().splitlines()
    assert [l.split("\t")[0] for l in lines] == ["1"] * len(lines)
    assert np.array_equal(np.asarray([int(l.split("\t")[1]) for l in lines]), kept)


def _fasta(path, n_contigs=24, length=4000, seed=0):
    rng = np.random.default_rng(seed)
    with open(path, "w") as fh:
        for i in range(n_contigs):
            s = "".join(rng.choice(list("ACGT"), length))
            fh.write(">chr%d\n%s\n" % (i + 1, "\n".join(s[j:j + 60] for j in range(0, length, 60))))
    return path


def _outputs(d):
    return {os.path.relpath(f, d): open(f, "rb").read() for f in glob.glob(os.path.join(d, "**"), recursive=True)
            if os.path.isfile(f)}


def _variant_files(d):
    return {k: v for k, v in _outputs(d).items() if k.endswith(".vcf") or k in ("variant", "scores")}


def test_cli_clone_tree(tmp_path):
    p, truth, _ = _tree_args()
    clone_tree_files(str(tmp_path / "bin"), p, ("1", "2", "X"))
    clone_tree_files(str(tmp_path / "text"), p, ("1", "2", "X"), text=True)
    fa = _fasta(str(tmp_path / "g.fa"))
    flags = ["--chromosomes=1,2,X", "--min_cluster_size=40", "--expectation_maximization"]
    ob = str(tmp_path / "ob") + "/"
    assert secedo_main.main(["-i", str(tmp_path / "bin"), "-o", ob, "--compute_read_stats"] + flags) == 0
    ot = str(tmp_path / "ot") + "/"
    assert secedo_main.main(["-i", str(tmp_path / "text"), "-o", ot] + flags) == 0
    got = _read_vec(ob + "clustering")
    # the top split separates the planted clones A and B exactly (B is cluster 2, A is split into 3 and 4)
    assert (got[truth == 0] == 2).all() and set(got[(truth == 1) | (truth == 2)].tolist()) <= {3, 4}
    files = set(os.listdir(ob))
    assert {"significant_positions" + m for m in ("", "A", "AA", "AB", "B")} <= files
    assert [f for f in files if f.startswith("expectation_maximization")] == ["expectation_maximization"]
    assert _outputs(ob) == _outputs(ot)  # the .bin and the .pileup runs write identical files
    # the same clustering from the host-read pileup in 24 slots
    slots = {0: "1", 1: "2", 22: "X"}
    chr_off, pos, off, rid, idb, base = [0], [], [np.zeros(1, np.uint64)], [], [], 0
    for s in range(24):
        n = 0
        if s in slots:
            hp, _, ml = secedo_amd.read_pileup(str(tmp_path / "bin" / ("s_%s.pileup.bin" % slots[s])),
                                               secedo_amd.get_grouping(), None, 100, None, True)
            pos.append(hp.locus_pos)
            off.append(np.asarray(hp.locus_entry_off[1:], np.uint64) + np.uint64(base))
            rid.append(hp.read_ids)
            idb.append(hp.id_base)
            base += hp.n_entries
            n = hp.n_loci
        chr_off.append(chr_off[-1] + n)
    flat = secedo_amd.FlatPileup(np.asarray(chr_off, np.uint32), np.concatenate(pos), np.concatenate(off),
                                 np.concatenate(rid), np.concatenate(idb))
    ident = np.arange(300)
    cl, _, recs = cluster.divide_cluster(flat, 0, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01, 8, "",
                                         "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40, 4)
    assert np.array_equal(cl, got) and [r["marker"] for r in recs] == ["", "A", "AA", "AB", "B"]
    # variant calling on the same resident pileup: identical to a direct variant_calling call
    ov = str(tmp_path / "ov") + "/"
    assert secedo_main.main(["-i", str(tmp_path / "bin"), "-o", ov, "--compute_read_stats",
                             "--reference_genome=" + fa] + flags) == 0
    od = str(tmp_path / "od") + "/"
    secedo_amd.variant_calling(flat, cl, fa, "", 1e-3, 0.01, od)
    vc = _variant_files(ov)
    assert vc and vc == _variant_files(od)
    # --clustering skips the clustering and gives the same VCFs
    oc = str(tmp_path / "oc") + "/"
    assert secedo_main.main(["-i", str(tmp_path / "bin"), "-o", oc, "--clustering=" + ob + "clustering",
                             "--reference_genome=" + fa] + flags) == 0
    assert _variant_files(oc) == vc
    bad = tmp_path / "short"
    bad.write_text("1,2,3\n")
    assert secedo_main.main(["-i", str(tmp_path / "bin"), "-o", oc, "--clustering=" + str(bad)] + flags) == 1


def test_cli_reference_fixtures(tmp_path):
    ref = np.load(os.path.join(gu.GOLDEN, "ref_files_pipeline.npz"))
    d = tmp_path / "ten"
    d.mkdir()
    shutil.copy(os.path.join(DATA, "ten_rows.pileup.bin"), d / "s_22.pileup.bin")
    out = str(tmp_path / "o10") + "/"
    assert secedo_main.main(["-i", str(d), "-o", out, "--chromosomes=22"]) == 0
    lines = open(out + "significant_positions").read().splitlines()
    assert all(l.startswith("22\t") for l in lines)
    assert np.array_equal(np.asarray([int(l.split("\t")[1]) for l in lines]), ref["ten_rows__kept_pos"])
    assert os.path.exists(out + "sim_mat_eigenvalues.csv")
    d6 = tmp_path / "six"
    d6.mkdir()
    shutil.copy(os.path.join(DATA, "six_cells.pileup.bin"), d6 / "s_22.pileup.bin")
    out6 = str(tmp_path / "o6") + "/"
    assert secedo_main.main(["-i", str(d6), "-o", out6, "--chromosomes=22"]) == 0
    assert open(out6 + "significant_positions").read() == "" and not os.path.exists(out6 + "clustering")


def test_cli_child_process(tmp_path):
    p, _, _ = _tree_args()
    clone_tree_files(str(tmp_path / "bin"), p, ("1", "2"))
    out = str(tmp_path / "o") + "/"
    proc = subprocess.run([sys.executable, "-m", "secedo_amd.secedo_main", "-i", str(tmp_path / "bin"), "-o", out,
                           "--chromosomes", "1,2", "--min_cluster_size", "40", "--expectation_maximization"],
                          cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert os.path.exists(out + "clustering") and "level" in proc.stdout
