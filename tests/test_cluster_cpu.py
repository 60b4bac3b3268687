"""The clustering library (include/secedo_cluster.h) without a GPU: exports, string parsing, argument checks
that must fail before any device is touched, and the numpy KMeans::run restatement on hand-made cases."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from secedo_amd import _lib, cluster
from tests.kmeans_ref import kmeans_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("secedo_")}


def _declared(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return set(re.findall(r"^(?:const\s+)?\w+\s*\*?\s*(secedo_\w+)\s*\(", text, re.M))


def test_simmat_exports_unchanged_and_cluster_exports_its_header():
    simmat = _exports(_lib.LIB_PATH)
    assert simmat == set(_lib.SIGNATURES)
    assert not any("cluster" in s for s in simmat)
    assert _exports(cluster.LIB_PATH) == _declared("secedo_cluster.h") == set(cluster.SIGNATURES)


def test_importing_the_package_does_not_load_the_cluster_library():
    import sys
    code = ("import secedo_amd, sys; from secedo_amd import cluster; "
            "assert cluster._cl is None; assert callable(secedo_amd.divide_cluster)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_parsers():
    assert [cluster.clustering_type(s) for s in ("FIEDLER", "SPECTRAL2", "SPECTRAL6")] == [0, 1, 2]
    with pytest.raises(_lib.SecedoError) as e:
        cluster.clustering_type("SPECTRAL3")
    assert e.value.code == _lib.E_INVALID_ARG and "SPECTRAL3" in str(e.value)
    # parse_termination: "AIC" is AIC, anything else BIC (spectral_clustering.cpp:30-32)
    assert cluster.termination("AIC") == 0 and cluster.termination("BIC") == 1 and cluster.termination("x") == 1


def _expect_invalid(fn, text):
    with pytest.raises(_lib.SecedoError) as e:
        fn()
    assert e.value.code == _lib.E_INVALID_ARG, str(e.value)
    assert text in str(e.value)


def test_invalid_arguments_fail_before_the_device():
    a = np.zeros((4, 4))
    _expect_invalid(lambda: cluster.spectral_clustering(a, "SPECTRAL2", "BIC", use_arma_kmeans=True), "use_arma_kmeans")
    _expect_invalid(lambda: cluster.spectral_clustering(a, "SPECTRAL6", "AIC", use_arma_kmeans=True), "use_arma_kmeans")
    _expect_invalid(lambda: cluster.spectral_clustering(a, "KMEANS"), "KMEANS")
    _expect_invalid(lambda: cluster.spectral_clustering(np.zeros((0, 0))), "no cells")
    from tests.clone_tree_gen import clone_tree
    p, _ = clone_tree(20, n_loci=50)
    ident = np.arange(20)
    args = (p, 500, ident.astype(np.uint16))
    rest = (0.01, 0.5, 0.05, 1, "", "ADD_MIN", "BIC", "SPECTRAL2")
    _expect_invalid(lambda: cluster.divide_cluster(*args, ident, ident[:0], *rest), "no cells")
    bad = ident.copy()
    bad[[3, 4]] = bad[[4, 3]]  # id_to_pos swapped against pos_to_id
    _expect_invalid(lambda: cluster.divide_cluster(*args, bad, ident, *rest), "inconsistent")
    _expect_invalid(lambda: cluster.divide_cluster(*args, ident, ident, 0.01, 0.5, 0.05, 1, "", "ADD_MIN", "BIC",
                                                   "SPECTRAL6", True), "use_arma_kmeans")


def test_fiedler_with_arma_kmeans_is_accepted_and_needs_the_gpu():
    # accepted (no effect with FIEDLER): without a GPU the call gets as far as the device check
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: covered by tests/test_gpu_cluster.py")
    except ImportError:
        pass
    with pytest.raises(_lib.SecedoError) as e:
        cluster.spectral_clustering(np.zeros((4, 4)), "FIEDLER", "AIC", use_arma_kmeans=True)
    assert e.value.code == _lib.E_NO_DEVICE


def test_kmeans_ref_empty_cluster_and_initial_zero_labels():
    # rows 0 and 1 coincide: both seed centroids are equal and every point goes to cluster 0 (first on ties).
    # That equals the initial all-zero labels, so pass 1 is already `done`; cluster 1 is empty and keeps the
    # zero centroid, and the inertia uses the centroid recomputed after that pass
    pts = np.array([[5.0, 5.0], [5.0, 5.0], [0.1, 0.0], [0.0, 0.1], [5.1, 5.0]])
    labels, inertia, passes = kmeans_run(pts, 2)
    assert list(labels) == [0, 0, 0, 0, 0] and passes == 1
    c0 = pts.sum(axis=0) / 5
    w = np.array([1.0, 1.2])
    assert math.isclose(inertia, sum(((p - c0) * w) @ ((p - c0) * w) for p in pts), rel_tol=1e-14)


def test_kmeans_ref_iteration_cap_recomputes_the_centroids():
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [10.0, 0.0], [11.0, 0.0]])
    labels1, inertia1, passes1 = kmeans_run(pts, 2, max_iter=1)
    # one pass: seeds rows 0, 1 -> labels [0, 1, 1, 1]; centroids recomputed from them, inertia uses those
    assert list(labels1) == [0, 1, 1, 1] and passes1 == 1
    c1 = pts[1:].mean(axis=0)
    assert math.isclose(inertia1, sum(((p - c1) ** 2).sum() for p in pts[1:]), rel_tol=1e-14)
    labels, inertia, _ = kmeans_run(pts, 2)
    assert list(labels) == [0, 0, 1, 1] and math.isclose(inertia, 1.0, rel_tol=1e-14)


def test_kmeans_ref_k_equals_n_and_beyond():
    pts = np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 7.0]])
    labels, inertia, _ = kmeans_run(pts, 3)
    assert list(labels) == [0, 1, 2] and inertia == 0
    assert kmeans_run(pts, 4)[1] == math.inf  # defined here: the reference never returns


def test_kmeans_ref_weights_coordinate_one():
    # equidistant in plain Euclid, not with coordinate 1 scaled by 1.2: the point joins the x-neighbour
    pts = np.array([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]])
    labels, _, _ = kmeans_run(pts, 2)
    assert labels[2] == 0
