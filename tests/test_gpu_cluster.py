"""Spectral clustering and divide_cluster on the GPU (include/secedo_cluster.h) against the numpy
restatements of tests/kmeans_ref.py and the reference's own SpectralClustering / DivideClusters suites
(tests/test_spectral_clustering.cpp:28-270 of the reference)."""
import math
import os

import numpy as np
import pytest

from tests.clone_tree_gen import clone_tree, purity
from tests.kmeans_ref import gmm_learn, kmeans_run

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _planted(n_blocks, size=30, seed=3):
    rng = np.random.default_rng(seed)
    n = n_blocks * size
    a = rng.uniform(0, 5, (n, n))
    for b in range(n_blocks):
        a[b * size:(b + 1) * size, b * size:(b + 1) * size] = rng.uniform(100, 200, (size, size))
    a = np.triu(a, 1)
    return a + a.T


def _eigvecs(a):
    import secedo_amd
    t = _torch()
    vals, vecs, _ = secedo_amd.smallest_eigenpairs(t.from_numpy(a).cuda(), min(20, len(a)), min(7, len(a)))
    return vecs  # n x 7 float64 on the device


def _inputs():
    z = np.load(os.path.join(GOLDEN, "spectral_reference_inputs.npz"))
    return [("two", z["two_clusters"]), ("three", z["three_clusters"]), ("planted4", _planted(4))]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_kmeans_parity_with_the_numpy_restatement(case):
    from secedo_amd import cluster
    name, a = _inputs()[case]
    vecs = _eigvecs(a)
    pts = vecs[:, :3].contiguous()
    host = pts.cpu().numpy()
    for K in range(1, 5):
        labels, inertia, _ = cluster.kmeans_device(pts, K)
        ref_labels, ref_inertia, _ = kmeans_run(host, K)
        assert np.array_equal(labels, ref_labels), (name, K)
        assert math.isclose(inertia, ref_inertia, rel_tol=1e-12, abs_tol=1e-300), (name, K, inertia, ref_inertia)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_gmm_against_closed_form_and_restatement(case):
    from secedo_amd import cluster
    name, a = _inputs()[case]
    vecs = _eigvecs(a)
    pts = vecs[:, 1:6].contiguous()
    X = pts.cpu().numpy()
    n, d = X.shape
    # one component: the ML Gaussian
    mu = X.mean(axis=0)
    cov = (X - mu).T @ (X - mu) / n
    _, logdet = np.linalg.slogdet(cov)
    avg = -0.5 * (d * math.log(2 * math.pi) + logdet + d)
    npar = d * (d + 1) // 2 + d
    m = cluster.gmm_device(pts, 1)
    assert m["status"] == 1
    assert math.isclose(m["avg_log_p"], avg, rel_tol=1e-10)
    assert math.isclose(m["aic"], 2 * npar - 2 * n * avg, rel_tol=1e-10)
    assert math.isclose(m["bic"], npar * math.log(n) - 2 * n * avg, rel_tol=1e-10)
    for K in range(2, 5):
        m = cluster.gmm_device(pts, K)
        r = gmm_learn(X, K)
        assert m["status"] == r["status"], (name, K)
        for key in ("avg_log_p", "aic", "bic"):
            if r["status"]:
                assert math.isclose(m[key], r[key], rel_tol=1e-9), (name, K, key, m[key], r[key])
            else:
                assert m[key] == r[key]


SC_PARAMS = [("SPECTRAL2", "AIC", False), ("FIEDLER", "AIC", False), ("SPECTRAL2", "BIC", False),
             ("FIEDLER", "BIC", False), ("FIEDLER", "AIC", True), ("FIEDLER", "BIC", True)]
# the reference instantiates SPECTRAL2 with use_arma_kmeans too: Armadillo's random k-means is not provided
ARMA_SPECTRAL = [("SPECTRAL2", "AIC", True), ("SPECTRAL2", "BIC", True)]


@pytest.mark.parametrize("params", SC_PARAMS)
def test_reference_one_cluster(params):
    from secedo_amd import cluster
    rng = np.random.default_rng(1243)
    done = 0
    for _ in range(3):
        a = np.triu(1 + rng.uniform(-1e-3, 1e-3, (100, 100)), 1)
        a = a + a.T
        nc, _, _ = cluster.spectral_clustering(a, *params)
        done += nc == 1
    assert done > 1


@pytest.mark.parametrize("params", SC_PARAMS)
def test_reference_two_and_three_clusters(params):
    from secedo_amd import cluster
    z = np.load(os.path.join(GOLDEN, "spectral_reference_inputs.npz"))
    if params[0] not in ("SPECTRAL2", "SPECTRAL6"):
        return  # the reference returns early for the other methods
    nc, c, _ = cluster.spectral_clustering(z["two_clusters"], *params)
    assert nc == 2
    mismatches = sum(abs(c[i] - c[i + 1]) > 1e-3 for i in range(49)) + sum(abs(c[i] - c[i + 1]) > 1e-3
                                                                         for i in range(50, 99))
    assert mismatches < 4
    assert abs(c[0] - c[-1]) == 1.0
    nc, c, _ = cluster.spectral_clustering(z["three_clusters"], *params)
    assert nc in (2, 3)
    for i in range(nc):
        count = int((c == i).sum())
        assert abs(count) < 2 or abs(count - 33) < 2 or abs(count - 66) < 2


@pytest.mark.parametrize("params", SC_PARAMS)
def test_reference_all_zero(params):
    from secedo_amd import cluster
    cluster.spectral_clustering(np.zeros((99, 99)), *params)


@pytest.mark.parametrize("params", ARMA_SPECTRAL)
def test_arma_kmeans_with_spectral_is_rejected(params):
    from secedo_amd import _lib, cluster
    with pytest.raises(_lib.SecedoError) as e:
        cluster.spectral_clustering(np.zeros((9, 9)), *params)
    assert e.value.code == _lib.E_INVALID_ARG


def test_decision_matches_restatement_and_is_deterministic():
    from secedo_amd import cluster
    from tests.kmeans_ref import decide
    for name, a in _inputs():
        vecs = _eigvecs(a)
        host = vecs.cpu().numpy()
        for t in ("FIEDLER", "SPECTRAL2", "SPECTRAL6"):
            for term in ("AIC", "BIC"):
                nc, c, rec = cluster.spectral_clustering_device(vecs, t, term)
                nc2, c2, rec2 = cluster.spectral_clustering_device(vecs, t, term)
                assert nc == nc2 and rec == rec2 and bool((c == c2).all())
                rnc, rlab, rrec = decide(host, t, term)
                assert nc == rnc, (name, t, term)
                assert np.array_equal(c.cpu().numpy(), rlab), (name, t, term)
                assert rec["cluster_count"] == rrec["cluster_count"]


def _shaped():
    from secedo_amd.pileup import FlatPileup
    z = np.load(os.path.join(GOLDEN, "divide_clusters_shaped.npz"))
    return FlatPileup(z["chr_locus_off"], z["locus_pos"], z["locus_entry_off"], z["read_ids"], z["id_base"])


DC_PARAMS = [("SPECTRAL6", "AIC", False), ("SPECTRAL2", "AIC", False), ("FIEDLER", "AIC", False),
             ("SPECTRAL2", "BIC", False), ("FIEDLER", "BIC", False), ("FIEDLER", "AIC", True),
             ("FIEDLER", "BIC", True)]


@pytest.mark.parametrize("params", DC_PARAMS)
def test_reference_divide_clusters_two_clusters(params):
    """DivideClusters.TwoClusters exactly as the reference calls it: the termination argument is the literal
    "BIC" whatever the parameter says (test_spectral_clustering.cpp:258). The parameter's own termination is
    run as well (test_divide_clusters_with_the_parameter_termination)."""
    _divide_shaped(params[0], "BIC", params[2])


@pytest.mark.parametrize("params", [p for p in DC_PARAMS if p[1] == "AIC"])
def test_divide_clusters_with_the_parameter_termination(params):
    _divide_shaped(*params)


def _divide_shaped(t, term, arma):
    import secedo_amd
    from secedo_amd import cluster
    p = _shaped()
    ident = np.arange(100)
    args = (500, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.05)
    cl, idx, recs = cluster.divide_cluster(p, *args, 4, "data/", "ADD_MIN", term, t, arma, False, 101, 4, "")
    assert cl.max() == 2
    assert (cl[:50] == cl[0]).all() and (cl[50:] == cl[-1]).all() and cl[0] != cl[-1]
    assert idx == 3 and len(recs) == 1 and recs[0]["child_states"] == ["too_small", "too_small"]
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, ident.astype(np.uint32), 100)
        cl2, idx2, recs2 = cluster.divide_cluster_resident(plan, res, *args, "ADD_MIN", term, t, arma, False, 101)
    assert np.array_equal(cl, cl2) and idx == idx2 and recs == recs2


def _tree(n=300, **kw):
    kw = dict(dict(f_ab=0.5, f_a12=0.05), **kw)
    p, truth = clone_tree(n, **kw)
    ident = np.arange(n)
    return p, truth, (500, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01)


# ((A1, A2), B): B the larger clone, the A1 | A2 loci rarer than the A | B loci, six mixed cells
TREE = dict(n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)


def test_clone_tree_recursion():
    """((A1, A2), B) with the reference's numbering: the top level splits A from B (labels 1 and 2, EM refines
    the two-way split), A is split again below it (labels 3 and 4; EM skipped there, its group ids reach past
    the sub-cluster's size), and every level below stops."""
    from secedo_amd import cluster
    p, truth, args = _tree(**TREE)
    cl, idx, recs = cluster.divide_cluster(p, *args, 1, "", "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40)
    assert [r["marker"] for r in recs] == ["", "A", "AA", "AB", "B"]
    top, a = recs[0], recs[1]
    assert top["stop_reason"] == "split" and top["num_clusters"] == 2 and top["cluster_idx"] == 1
    assert top["em"] == "run" and top["em_iterations"] >= 1 and top["child_states"] == ["recursed"] * 2
    assert a["stop_reason"] == "split" and a["num_clusters"] == 2 and a["cluster_idx"] == 3
    assert a["em"] == "skipped" and a["n_vectors"] == 7 and a["kept_loci"] > 0 and len(a["eigenvalues"]) == 20
    assert a["cells"] == top["child_sizes"][0] and recs[4]["cells"] == top["child_sizes"][1]
    assert sum(a["child_sizes"]) == a["cells"]
    assert all(r["stop_reason"] != "split" and r["cluster_idx"] == 5 for r in recs[2:])
    assert idx == 5
    # the full label vector of the clones: B one top-level cluster, A1 and A2 the child labels 3 and 4
    assert (cl[truth == 0] == 2).all()
    assert {int(cl[truth == 1][0]), int(cl[truth == 2][0])} == {3, 4}
    assert (cl[truth == 1] == cl[truth == 1][0]).all() and (cl[truth == 2] == cl[truth == 2][0]).all()
    assert purity(cl, truth) == 1.0
    cl2, idx2, recs2 = cluster.divide_cluster(p, *args, 1, "", "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40)
    assert np.array_equal(cl, cl2) and idx == idx2 and recs == recs2  # bit-identical
    # without EM the top split is not refined, and the tree is not recovered
    cl0, _, recs0 = cluster.divide_cluster(p, *args, 1, "", "ADD_MIN", "BIC", "SPECTRAL6", False, False, 40)
    assert recs0[0]["em"] == "not_run" and purity(cl0, truth) < 1.0


def test_unassigned_cells_by_the_005_rule():
    """After EM a cell joins child c only when |p - c| < 0.05. Cells without a single read keep the EM's prior
    (the likelihoods of both sides are equal), which lies in between: they get cluster id 0."""
    from secedo_amd import cluster
    p, truth, args = _tree(**dict(TREE, mixed_cov=0.0))
    cl, idx, recs = cluster.divide_cluster(p, *args, 1, "", "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40)
    assert recs[0]["em"] == "run"
    assert (cl[truth == 3] == 0).all() and (cl[truth < 3] != 0).all()
    assert sum(recs[0]["child_sizes"]) == 300 - int((cl == 0).sum())


def test_clone_tree_stop_reasons():
    from secedo_amd import cluster
    p, truth, args = _tree()
    # min_cluster_size larger than any child: one level, every child too small
    cl, idx, recs = cluster.divide_cluster(p, *args, 1, "", "ADD_MIN", "BIC", "SPECTRAL2", False, False, 1000)
    assert len(recs) == 1 and recs[0]["child_states"] == ["too_small"] * recs[0]["num_clusters"]
    # between the child sizes (75, 75, 150): the clone of 150 recurses and stops on its coverage
    cl, idx, recs = cluster.divide_cluster(p, *args, 1, "", "ADD_MIN", "BIC", "SPECTRAL2", False, False, 140)
    assert sorted(recs[0]["child_states"]) == ["recursed", "too_small", "too_small"] and len(recs) == 2
    assert recs[1]["cells"] == 150 and recs[1]["stop_reason"] == "coverage" and recs[1]["coverage"] < 9
    # a child too large relative to the rest (:424-426), on the ((A1, A2), B) tree: its top children are 117 and
    # 183 cells; with 120, the first is too small and the second leaves 300 - 183 < 120 for the rest
    p2, _, args2 = _tree(**TREE)
    cl, idx, recs = cluster.divide_cluster(p2, *args2, 1, "", "ADD_MIN", "BIC", "SPECTRAL6", False, True, 120)
    assert recs[0]["child_states"] == ["too_small", "too_large"] and len(recs) == 1
    # little coverage: the GMM with one component wins at the top level
    p3, _, args3 = _tree(300, cov_lo=0.005, cov_hi=0.02, seed=5)
    cl, idx, recs = cluster.divide_cluster(p3, *args3, 1, "", "ADD_MIN", "BIC", "SPECTRAL2", False, False, 50)
    assert len(recs) == 1 and recs[0]["stop_reason"] == "one_cluster" and idx == 1 and not cl.any()


def _write_pileup(path, p, n_cells):
    with open(path, "wb") as f:
        np.asarray([len(p.chr_locus_off) - 1, p.n_loci, p.n_entries, n_cells], dtype=np.uint64).tofile(f)
        np.asarray(p.chr_locus_off, dtype=np.uint32).tofile(f)
        np.asarray(p.locus_pos, dtype=np.uint32).tofile(f)
        np.asarray(p.locus_entry_off, dtype=np.uint64).tofile(f)
        np.asarray(p.read_ids, dtype=np.uint32).tofile(f)
        np.asarray(p.id_base, dtype=np.uint16).tofile(f)


def test_cpp_entry_points_equal_the_python_ones(tmp_path):
    """tests/cpp/divide_cluster_test.cpp: secedo_amd::divide_cluster and secedo_amd::spectral_clustering of
    include/secedo_pipeline.hpp on reference-shaped PosData / Matd, against the Python entry points."""
    import subprocess
    from secedo_amd import cluster
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "divide_cluster_test")
    lib = os.path.join(root, "secedo_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "divide_cluster_test.cpp"), "-o", exe, "-L" + lib,
                    "-lsecedo_cluster", "-lsecedo_simmat", "-Wl,-rpath," + lib], check=True)

    def run(*args):
        out = subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True).stdout.split()
        return out

    # the reference's DivideClusters input: 2 clusters, 50 / 50
    _write_pileup(tmp_path / "shaped.bin", _shaped(), 100)
    out = run("divide", tmp_path / "shaped.bin", "SPECTRAL2", "BIC", 0, 0, 101, 0.05)
    ident = np.arange(100)
    cl, idx, recs = cluster.divide_cluster(_shaped(), 500, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.05, 4,
                                           "data/", "ADD_MIN", "BIC", "SPECTRAL2", False, False, 101, 4, "")
    got = np.asarray(out[2:], dtype=np.uint16)
    assert int(out[0]) == idx == 3 and int(out[1]) == len(recs) and np.array_equal(got, cl)
    assert got.max() == 2 and (got[:50] == got[0]).all() and (got[50:] == got[-1]).all()
    # the recursion with EM
    p, truth, args = _tree(**TREE)
    _write_pileup(tmp_path / "tree.bin", p, 300)
    out = run("divide", tmp_path / "tree.bin", "SPECTRAL6", "BIC", 0, 1, 40, 0.01)
    cl, idx, recs = cluster.divide_cluster(p, *args, 1, "", "ADD_MIN", "BIC", "SPECTRAL6", False, True, 40)
    assert int(out[0]) == idx and int(out[1]) == len(recs)
    assert np.array_equal(np.asarray(out[2:], dtype=np.uint16), cl)
    # spectral_clustering on a Matd
    a = np.load(os.path.join(GOLDEN, "spectral_reference_inputs.npz"))["two_clusters"]
    with open(tmp_path / "m.bin", "wb") as f:
        np.asarray([len(a)], dtype=np.uint64).tofile(f)
        a.astype(np.float64).tofile(f)
    out = run("spectral", tmp_path / "m.bin", "SPECTRAL6", "AIC", 0)
    nc, c, _ = cluster.spectral_clustering(a, "SPECTRAL6", "AIC")
    assert int(out[0]) == nc == 2 and np.array_equal(np.asarray(out[1:], dtype=np.float64), c)
