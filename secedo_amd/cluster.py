"""Spectral clustering and the divide_cluster recursion (include/secedo_cluster.h, libsecedo_cluster.so).

Host-side mirror of the reference's ``spectral_clustering(similarity, ...)`` and ``divide_cluster(...)``
(spectral_clustering.cpp:117-299, :311-434): the decision step (k-means for the cluster count, GMMs with
AIC / BIC for termination, the labels) runs on the GPU (secedo_amd/csrc/cluster_kernels.hip), and so does
every heavy step of a recursion level. The library is loaded on first use, after torch (see _lib.py).
No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .pileup import FlatPileup, flatten

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsecedo_cluster.so")

CLUSTERING_TYPES = ("FIEDLER", "SPECTRAL2", "SPECTRAL6")
MAX_CLUSTERS = 4
STOP_REASONS = ("split", "coverage", "one_cluster")
CHILD_STATES = ("recursed", "too_small", "too_large")
EM_STATES = ("not_run", "run", "skipped")

_vp = C.c_void_p
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)


class Model(C.Structure):
    _fields_ = [("inertia", C.c_double), ("avg_log_p", C.c_double), ("aic", C.c_double), ("bic", C.c_double),
                ("status", C.c_uint32), ("iterations", C.c_uint32)]


class Decision(C.Structure):
    _fields_ = [("kmeans", Model * MAX_CLUSTERS), ("gmm", Model * MAX_CLUSTERS), ("cluster_count", C.c_uint32),
                ("num_clusters", C.c_uint32), ("label_iterations", C.c_uint32), ("n_vectors", C.c_uint32)]


class Level(C.Structure):
    _fields_ = [("marker", C.c_char * 64), ("n_cells", C.c_uint32), ("stop_reason", C.c_uint32),
                ("kept_loci", C.c_uint64), ("coverage", C.c_double), ("eigenvalues", C.c_double * 20),
                ("n_eigenvalues", C.c_uint32), ("num_clusters", C.c_uint32), ("decision", Decision),
                ("em_state", C.c_uint32), ("em_iterations", C.c_uint32), ("cluster_idx", C.c_uint32),
                ("child_size", C.c_uint32 * MAX_CLUSTERS), ("child_state", C.c_uint32 * MAX_CLUSTERS),
                ("step_ms", C.c_double * 6)]

STEPS = ("filter_ms", "matrix_ms", "eigenpairs_ms", "decision_ms", "em_ms", "partition_ms")


SIGNATURES = {
    "secedo_cluster_type_from_string": (C.c_int, [C.c_char_p]),
    "secedo_termination_from_string": (C.c_int, [C.c_char_p]),
    "secedo_cluster_last_error": (C.c_char_p, []),
    "secedo_spectral_clustering_device": (C.c_int, [C.c_int, _vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                                    _vp, _u32p, C.POINTER(Decision), _vp]),
    "secedo_spectral_clustering": (C.c_int, [C.c_int, _vp, C.c_uint32, C.c_int, C.c_int, C.c_int, _vp, _u32p,
                                             C.POINTER(Decision), _vp]),
    "secedo_cluster_kmeans_device": (C.c_int, [C.c_int, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp,
                                               C.POINTER(Model), _vp]),
    "secedo_cluster_gmm_device": (C.c_int, [C.c_int, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Model), _vp]),
    "secedo_divide_cluster_device": (C.c_int, [C.c_int, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.c_uint32,
                                               C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp, C.c_uint32, _vp,
                                               C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, _vp,
                                               _u16p, C.POINTER(Level), C.c_uint32, _u32p, _vp]),
    "secedo_divide_cluster": (C.c_int, [C.c_int, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp,
                                        C.c_uint32, _vp, C.c_uint32, _vp, C.c_uint32, C.c_double, C.c_double,
                                        C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                        C.c_uint32, C.c_char_p, _vp, _u16p, C.POINTER(Level), C.c_uint32, _u32p]),
}
# the same two recursions writing the reference's output files: one more argument, out_dir, at the end
SIGNATURES["secedo_divide_cluster_files_device"] = (C.c_int, SIGNATURES["secedo_divide_cluster_device"][1] +
                                                    [C.c_char_p])
SIGNATURES["secedo_divide_cluster_files"] = (C.c_int, SIGNATURES["secedo_divide_cluster"][1] + [C.c_char_p])

_cl = None


def lib():
    global _cl
    if _cl is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `make -C secedo_amd/csrc` (there is no fallback "
                              "implementation)" % LIB_PATH)
        try:
            import torch  # noqa: F401  -- one HIP runtime per process: torch's, as in _lib.py
        except ImportError:
            pass
        _lib.lib()  # the product library first: libsecedo_cluster.so links it
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _cl = l
    return _cl


def check(rc):
    if rc == _lib.OK:
        return
    msg = lib().secedo_cluster_last_error().decode(errors="replace")
    if rc == _lib.E_INVALID_NORMALIZATION:
        raise _lib.InvalidNormalization(msg)
    raise _lib.SecedoError(rc, msg)


def clustering_type(name: str) -> int:
    rc = lib().secedo_cluster_type_from_string(name.encode())
    if rc < 0:
        check(rc)
    return rc


def termination(name: str) -> int:
    return lib().secedo_termination_from_string(name.encode())


def _model(m: Model) -> dict:
    return dict(inertia=m.inertia, avg_log_p=m.avg_log_p, aic=m.aic, bic=m.bic, status=int(m.status),
                iterations=int(m.iterations))


def decision_dict(d: Decision) -> dict:
    k = [_model(m) for m in d.kmeans]
    g = [_model(m) for m in d.gmm]
    return dict(inertia=[m["inertia"] for m in k], kmeans_iterations=[m["iterations"] for m in k],
                gmm_status=[m["status"] for m in g], avg_log_p=[m["avg_log_p"] for m in g],
                aic=[m["aic"] for m in g], bic=[m["bic"] for m in g], em_iterations_gmm=[m["iterations"] for m in g],
                cluster_count=int(d.cluster_count), num_clusters=int(d.num_clusters),
                label_iterations=int(d.label_iterations), n_vectors=int(d.n_vectors))


def _level_dict(r: Level) -> dict:
    nc = int(r.num_clusters) if r.stop_reason == 0 else 0
    out = decision_dict(r.decision)
    out.update(marker=r.marker.decode(), cells=int(r.n_cells), kept_loci=int(r.kept_loci), coverage=r.coverage,
               eigenvalues=list(r.eigenvalues[:r.n_eigenvalues]), num_clusters=int(r.num_clusters),
               stop_reason=STOP_REASONS[r.stop_reason], em=EM_STATES[r.em_state],
               em_iterations=int(r.em_iterations), cluster_idx=int(r.cluster_idx),
               child_sizes=list(r.child_size[:nc]), child_states=[CHILD_STATES[s] for s in r.child_state[:nc]])
    return out


def _records(recs, n, with_times):
    out = [_level_dict(recs[i]) for i in range(n)]
    if with_times:  # wall times differ from run to run; the rest of a record is reproducible
        for o, i in zip(out, range(n)):
            o["times"] = dict(zip(STEPS, recs[i].step_ms))
    return out


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def spectral_clustering(similarity, clustering_type_name: str = "SPECTRAL6", termination_name: str = "BIC",
                        use_arma_kmeans: bool = False, device: int = 0):
    """spectral_clustering(similarity, clustering, termination, out_dir, marker, use_arma_kmeans, &cluster)
    (spectral_clustering.cpp:117-299) -> (num_clusters, cluster as float64 ndarray, record dict).
    `similarity`: n x n symmetric, zero diagonal (host array)."""
    a = np.ascontiguousarray(similarity, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("similarity must be square")
    t, term = clustering_type(clustering_type_name), termination(termination_name)
    n = a.shape[0]
    cluster = np.zeros(max(n, 1), dtype=np.float64)
    vals = np.zeros(20, dtype=np.float64)
    nc, dec = C.c_uint32(0), Decision()
    check(lib().secedo_spectral_clustering(device, _lib.ptr(a), n, t, term, int(bool(use_arma_kmeans)),
                                           _lib.ptr(cluster), C.byref(nc), C.byref(dec), _lib.ptr(vals)))
    rec = decision_dict(dec)
    rec["eigenvalues"] = list(vals[:min(20, n)])
    return int(nc.value), cluster[:n], rec


def spectral_clustering_device(eigenvectors, clustering_type_name="SPECTRAL6", termination_name="BIC",
                               use_arma_kmeans=False):
    """The decision step alone on a (n x k) float64 CUDA tensor of eigenvectors (as smallest_eigenpairs returns
    them) -> (num_clusters, cluster tensor, record dict)."""
    import torch
    ev = eigenvectors.t().contiguous()  # column-major n x k
    n, k = eigenvectors.shape
    out = torch.empty(n, dtype=torch.float64, device=eigenvectors.device)
    nc, dec = C.c_uint32(0), Decision()
    check(lib().secedo_spectral_clustering_device(
        eigenvectors.device.index or 0, ev.data_ptr(), n, k, clustering_type(clustering_type_name),
        termination(termination_name), int(bool(use_arma_kmeans)), out.data_ptr(), C.byref(nc), C.byref(dec),
        _stream(eigenvectors.device)))
    return int(nc.value), out, decision_dict(dec)


def kmeans_device(points, K, max_iter=100):
    """KMeans::run(points, K, max_iter, tries) (util/kmeans.cpp) on a (n x dims) float64 CUDA tensor ->
    (labels as int64 ndarray, inertia, iterations)."""
    import torch
    x = points.t().contiguous()
    n, dims = points.shape
    lab = torch.empty(n, dtype=torch.int32, device=points.device)
    m = Model()
    check(lib().secedo_cluster_kmeans_device(points.device.index or 0, x.data_ptr(), n, dims, K, max_iter,
                                             lab.data_ptr(), C.byref(m), _stream(points.device)))
    return lab.cpu().numpy().astype(np.int64), m.inertia, int(m.iterations)


def gmm_device(points, K):
    """gmm_full::learn(data, K, eucl_dist, random_subset, 10, 5, 1e-10) + avg_log_p / AIC / BIC on a (n x dims)
    float64 CUDA tensor (one sample per row) -> dict."""
    x = points.t().contiguous()
    n, dims = points.shape
    m = Model()
    check(lib().secedo_cluster_gmm_device(points.device.index or 0, x.data_ptr(), n, dims, K, C.byref(m),
                                          _stream(points.device)))
    return _model(m)


def _norm(normalization):
    from .similarity_matrix import to_enum
    return to_enum(normalization)


def _id_maps(id_to_group, id_to_pos, pos_to_id, clusters):
    g = np.ascontiguousarray(id_to_group, dtype=np.uint16)
    i2p = np.ascontiguousarray(id_to_pos, dtype=np.uint32)
    p2i = np.ascontiguousarray(pos_to_id, dtype=np.uint32)
    cl = np.zeros(len(g), dtype=np.uint16) if clusters is None else np.array(clusters, dtype=np.uint16)
    return g, i2p, p2i, cl


def divide_cluster(pds, max_read_length, id_to_group, id_to_pos, pos_to_id, mutation_rate, homozygous_rate,
                   seq_error_rate, num_threads=1, out_dir="", normalization="ADD_MIN", termination_name="BIC",
                   clustering_type_name="SPECTRAL6", use_arma_kmeans=False, use_expectation_maximization=False,
                   min_cluster_size=500, cell_proportion=4, marker="", clusters=None, cluster_idx=1, device=0,
                   with_times=False, *, write_files=False):
    """divide_cluster(...) (spectral_clustering.cpp:311-434) in the reference's argument order, the pileup uploaded
    once. `num_threads` is accepted and unused; `out_dir` is ignored unless write_files is set, when the reference's
    output files are written there (include/secedo_cluster.h lists them). The records carry what the reference
    logs; with_times adds each level's step times. -> (clusters as uint16 ndarray per cell id, cluster_idx, list of
    level records)."""
    del num_threads
    p = pds if isinstance(pds, FlatPileup) else flatten(pds)
    g, i2p, p2i, cl = _id_maps(id_to_group, id_to_pos, pos_to_id, clusters)
    idb = np.ascontiguousarray(p.id_base)
    b16 = b32 = None
    if idb.dtype == np.uint16 or len(idb) == 0 or int(idb.max()) <= 0xFFFF:
        b16 = np.ascontiguousarray(idb, dtype=np.uint16)
    else:
        b32 = np.ascontiguousarray(idb, dtype=np.uint32)
    chr_off = np.ascontiguousarray(p.chr_locus_off, dtype=np.uint32)
    pos = np.ascontiguousarray(p.locus_pos, dtype=np.uint32)
    off = np.ascontiguousarray(p.locus_entry_off, dtype=np.uint64)
    rid = np.ascontiguousarray(p.read_ids, dtype=np.uint32)
    t, term = clustering_type(clustering_type_name), termination(termination_name)
    cap = 4 * len(p2i) + 16
    recs = (Level * cap)()
    n_rec, idx = C.c_uint32(0), C.c_uint16(cluster_idx)
    fn, extra = lib().secedo_divide_cluster, ()
    if write_files:
        fn, extra = lib().secedo_divide_cluster_files, (os.fsencode(str(out_dir)),)
    check(fn(
        device, _lib.ptr(chr_off), len(chr_off) - 1, _lib.ptr(pos), _lib.ptr(off), _lib.ptr(rid), _lib.ptr(b16),
        _lib.ptr(b32), max_read_length, _lib.ptr(g), len(g), _lib.ptr(i2p), len(i2p), _lib.ptr(p2i), len(p2i),
        mutation_rate, homozygous_rate, seq_error_rate, _norm(normalization), term, t, int(bool(use_arma_kmeans)),
        int(bool(use_expectation_maximization)), min_cluster_size, cell_proportion, marker.encode(),
        _lib.ptr(cl), C.byref(idx), recs, cap, C.byref(n_rec), *extra))
    return cl, int(idx.value), _records(recs, n_rec.value, with_times)


def divide_cluster_resident(plan, res, max_read_length, id_to_group, id_to_pos, pos_to_id, mutation_rate,
                            homozygous_rate, seq_error_rate, normalization="ADD_MIN", termination_name="BIC",
                            clustering_type_name="SPECTRAL6", use_arma_kmeans=False,
                            use_expectation_maximization=False, min_cluster_size=500, cell_proportion=4, marker="",
                            clusters=None, cluster_idx=1, with_times=False, out_dir=None):
    """divide_cluster on a pileup already resident in HBM (`res` from SimilarityMatrixPlan.upload, on
    plan.device, in the plan's current stream) -> (clusters, cluster_idx, records). With an out_dir the reference's
    output files are written there (include/secedo_cluster.h lists them)."""
    g, i2p, p2i, cl = _id_maps(id_to_group, id_to_pos, pos_to_id, clusters)
    t, term = clustering_type(clustering_type_name), termination(termination_name)
    idb = C.c_void_p(res["idb"].data_ptr())
    cap = 4 * len(p2i) + 16
    recs = (Level * cap)()
    n_rec, idx = C.c_uint32(0), C.c_uint16(cluster_idx)
    fn, extra = lib().secedo_divide_cluster_device, ()
    if out_dir is not None:
        fn, extra = lib().secedo_divide_cluster_files_device, (os.fsencode(str(out_dir)),)
    check(fn(
        plan.device, C.c_void_p(res["chr"].data_ptr()), res["n_chr"], C.c_void_p(res["pos"].data_ptr()),
        C.c_void_p(res["off"].data_ptr()), C.c_void_p(res["rid"].data_ptr()), idb if res["idb_is16"] else None,
        None if res["idb_is16"] else idb, res["n_loci"], res["n_entries"], max_read_length, _lib.ptr(g), len(g),
        _lib.ptr(i2p), len(i2p), _lib.ptr(p2i), len(p2i), mutation_rate, homozygous_rate, seq_error_rate,
        _norm(normalization), term, t, int(bool(use_arma_kmeans)), int(bool(use_expectation_maximization)),
        min_cluster_size, cell_proportion, marker.encode(), _lib.ptr(cl), C.byref(idx), recs, cap, C.byref(n_rec),
        plan._stream(), *extra))
    return cl, int(idx.value), _records(recs, n_rec.value, with_times)
