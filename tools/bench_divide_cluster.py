#!/usr/bin/env python3
"""bench_divide_cluster.py -- the divide_cluster recursion (include/secedo_cluster.h) on the GPU, one JSON line
per workload:

    tree_2000, tree_8000   the clone tree ((A1, A2), B) of tests/clone_tree_gen.py at about 2000 / 8000 cells
    shaped                 the two-clone input of the reference's DivideClusters test (tests/golden)
    decision_8000, decision_32000
                           the decision step alone (secedo_spectral_clustering_device: both launches and the
                           read-back of the decision) on an n x 7 eigenvector-like block of four planted clusters

A recursion line holds every level's step times (filter, matrix, eigenpairs, decision, EM, partition; wall ms,
each step ended by a stream synchronisation), the total wall time of the call and the purity of the final
labels against the planted clones. The first call of a process pays for allocations and code loading, so every
workload runs once untimed first. Run every step under a time limit (timeout -k 10 ...)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from secedo_amd import cluster  # noqa: E402
from secedo_amd.pileup import FlatPileup  # noqa: E402
from tests.clone_tree_gen import clone_tree, purity  # noqa: E402

# clone-tree parameters of tests/test_gpu_cluster.py: B 60 % of the cells, the A1 | A2 loci rarer than the A | B
# loci, 2 % mixed cells; SPECTRAL6 with EM
TREE = dict(f_ab=0.35, f_a12=0.12)


def recursion(name, p, truth, min_cluster_size, theta, termination="BIC", clustering="SPECTRAL2", em=False):
    n = len(truth)
    ident = np.arange(n)
    args = (p, 500, ident.astype(np.uint16), ident, ident, 0.01, 0.5, theta, 1, "", "ADD_MIN", termination,
            clustering, False, em, min_cluster_size)
    cluster.divide_cluster(*args)  # warm-up
    t0 = time.perf_counter()
    cl, idx, recs = cluster.divide_cluster(*args, with_times=True)
    total = (time.perf_counter() - t0) * 1e3
    levels = [dict(marker=r["marker"], cells=r["cells"], kept_loci=r["kept_loci"], stop=r["stop_reason"],
                   num_clusters=r["num_clusters"], em=r["em"], **{k: round(v, 3) for k, v in r["times"].items()})
              for r in recs]
    print(json.dumps(dict(workload=name, cells=n, clustering=clustering, termination=termination, em=em,
                          levels=levels, total_ms=round(total, 3), cluster_idx=idx,
                          purity=purity(cl, truth))), flush=True)


def decision(n, reps=5):
    import torch
    rng = np.random.default_rng(n)
    centres = rng.normal(0, 1, (4, 7))
    x = centres[rng.integers(0, 4, n)] + rng.normal(0, 0.05, (n, 7))
    x /= np.linalg.norm(x, axis=0)
    ev = torch.from_numpy(x).cuda()
    cluster.spectral_clustering_device(ev, "SPECTRAL6", "BIC")  # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nc, _, rec = cluster.spectral_clustering_device(ev, "SPECTRAL6", "BIC")
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(workload="decision_%d" % n, cells=n, decision_ms_median=round(float(np.median(times)), 3),
                          decision_ms_min=round(min(times), 3), target_ms=2.0, num_clusters=nc,
                          cluster_count=rec["cluster_count"], kmeans_iterations=rec["kmeans_iterations"],
                          label_iterations=rec["label_iterations"])), flush=True)


def main(which):
    if "tree_2000" in which:
        p, truth = clone_tree(2000, n_b=1200, n_mixed=40, n_loci=4000, cov_lo=0.02, cov_hi=0.1, **TREE)
        recursion("tree_2000", p, truth, 100, 0.01, clustering="SPECTRAL6", em=True)
    if "tree_8000" in which:
        p, truth = clone_tree(8000, n_b=4800, n_mixed=160, n_loci=3000, cov_lo=0.01, cov_hi=0.04, **TREE)
        recursion("tree_8000", p, truth, 400, 0.01, clustering="SPECTRAL6", em=True)
    if "shaped" in which:
        z = np.load(os.path.join(ROOT, "tests", "golden", "divide_clusters_shaped.npz"))
        p = FlatPileup(z["chr_locus_off"], z["locus_pos"], z["locus_entry_off"], z["read_ids"], z["id_base"])
        recursion("shaped", p, np.repeat([0, 1], 50), 101, 0.05)
    for n in (8000, 32000):
        if "decision_%d" % n in which:
            decision(n)


if __name__ == "__main__":
    main(sys.argv[1:] or ["tree_2000", "tree_8000", "shaped", "decision_8000", "decision_32000"])
