"""GPU loader of the reference's binary pileup files (include/secedo_pileup.h, libsecedo_pileup.so).

``read_pileups_resident`` reads several ``.bin`` files (one per chromosome slot) straight into HBM: the host reads
the files in bounded chunks and walks the record headers, the GPU decodes the records
(secedo_amd/csrc/pileup_device.hip). Per file the result equals ``read_pileup`` on that file bit for bit. Text
``.pileup`` files keep going through the host reader. No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .pileup import FlatPileup

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsecedo_pileup.so")

MAX_CELLS = 16384  # cell ids are 14 bits in a .bin file


class LoadInfo(C.Structure):
    _fields_ = [("n_loci", C.c_uint64), ("n_entries", C.c_uint64)]


class Times(C.Structure):
    _fields_ = [("read_ms", C.c_double), ("walk_ms", C.c_double), ("upload_ms", C.c_double),
                ("device_ms", C.c_double), ("total_ms", C.c_double)]


_vp = C.c_void_p
_u32 = C.c_uint32

SIGNATURES = {
    "secedo_pileup_load_last_error": (C.c_char_p, []),
    "secedo_pileup_load_device": (C.c_int, [C.POINTER(C.c_char_p), _u32, _vp, _u32, _vp, _u32, _u32,
                                            C.POINTER(_vp), _vp, C.c_int, C.c_uint64, C.POINTER(LoadInfo), _vp, _vp,
                                            C.POINTER(Times)]),
    "secedo_pileup_load_fetch": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "secedo_pileup_load_release": (None, []),
}

_pl = None


def lib():
    global _pl
    if _pl is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `make -C secedo_amd/csrc` (there is no fallback "
                              "implementation)" % LIB_PATH)
        try:
            import torch  # noqa: F401  -- one HIP runtime per process: torch's, as in _lib.py
        except ImportError:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _pl = l
    return _pl


def check(rc):
    if rc == _lib.OK:
        return
    raise _lib.SecedoError(rc, lib().secedo_pileup_load_last_error().decode(errors="replace"))


def _call(files, slots, n_slots, id_to_group, max_coverage, positions, compute_read_stats, staging_bytes):
    names = [os.fsencode(str(f)) for f in files]
    n = len(names)
    arr = (C.c_char_p * max(n, 1))(*names)
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    if len(sl) != n:
        raise ValueError("one slot per file")
    i2g = np.ascontiguousarray(np.arange(MAX_CELLS) if id_to_group is None else id_to_group, dtype=np.uint16)
    keep = []
    pos_ptrs = (_vp * max(n, 1))()
    n_pos = np.zeros(max(n, 1), dtype=np.uint64)
    if positions is not None:
        if len(positions) != n:
            raise ValueError("one position list (or None) per file")
        for i, p in enumerate(positions):
            if p is None or len(p) == 0:
                continue
            a = np.ascontiguousarray(p, dtype=np.uint32)
            keep.append(a)
            pos_ptrs[i] = a.ctypes.data
            n_pos[i] = len(a)
    info, t = LoadInfo(), Times()
    num_cells = np.zeros(max(n, 1), dtype=np.uint32)
    max_len = np.zeros(max(n, 1), dtype=np.uint32)
    check(lib().secedo_pileup_load_device(
        arr, n, _lib.ptr(sl), n_slots, _lib.ptr(i2g), len(i2g), max_coverage,
        pos_ptrs if positions is not None else None, _lib.ptr(n_pos) if positions is not None else None,
        int(bool(compute_read_stats)), staging_bytes, C.byref(info), _lib.ptr(num_cells), _lib.ptr(max_len),
        C.byref(t)))
    return info, t, num_cells[:n], max_len[:n], i2g


def _times(t: Times) -> dict:
    return {k: float(getattr(t, k)) for k, _ in Times._fields_}


def read_pileups(files: Sequence[str], slots: Sequence[int], n_slots: int = 24, id_to_group=None,
                 max_coverage: int = 100, positions=None, compute_read_stats: bool = False, staging_bytes: int = 0,
                 times: Optional[dict] = None, per_file: Optional[dict] = None) -> FlatPileup:
    """The GPU loader with the result copied back to the host -> FlatPileup of n_slots chromosomes (for tests and
    tools; the pipeline keeps the pileup resident with read_pileups_resident)."""
    info, t, nc, ml, _ = _call(files, slots, n_slots, id_to_group, max_coverage, positions, compute_read_stats,
                               staging_bytes)
    L, E = int(info.n_loci), int(info.n_entries)
    chr_off = np.zeros(n_slots + 1, dtype=np.uint32)
    pos = np.zeros(max(L, 1), dtype=np.uint32)
    off = np.zeros(L + 1, dtype=np.uint64)
    rid = np.zeros(max(E, 1), dtype=np.uint32)
    idb = np.zeros(max(E, 1), dtype=np.uint16)
    try:
        check(lib().secedo_pileup_load_fetch(_lib.ptr(chr_off), _lib.ptr(pos), _lib.ptr(off), _lib.ptr(rid),
                                             _lib.ptr(idb)))
    finally:
        lib().secedo_pileup_load_release()
    if times is not None:
        times.update(_times(t))
    if per_file is not None:
        per_file.update(num_cells=[int(x) for x in nc], max_read_length=[int(x) for x in ml])
    return FlatPileup(chr_off, pos[:L], off, rid[:E], idb[:E].astype(np.uint32))


def read_pileups_resident(plan, files: Sequence[str], slots: Sequence[int], n_slots: int = 24, id_to_group=None,
                          max_coverage: int = 100, positions=None, compute_read_stats: bool = False,
                          staging_bytes: int = 0, times: Optional[dict] = None, per_file: Optional[dict] = None):
    """``.bin`` files[i] into chromosome slot slots[i] (distinct, < n_slots), straight into HBM on ``plan``'s
    device. id_to_group: cell id -> group (None: the identity over 16384 cells); positions: None or one sorted
    position list (or None) per file, as read_pileup's ``positions``; staging_bytes: bytes read per chunk
    (0 = 64 MiB).

    -> (res, num_cells, max_read_length) like pileup_bams_resident: ``res`` is the resident pileup dict of
    SimilarityMatrixPlan.upload; num_cells and max_read_length are the maxima over the files of what read_pileup
    reports (max_read_length 1000 when compute_read_stats is off). ``per_file`` (a dict) receives the per-file
    values, ``times`` the step times in ms (read, walk, upload, device, total)."""
    import torch

    dev = "cuda:%d" % plan.device
    with torch.cuda.device(plan.device):
        info, t, nc, ml, i2g = _call(files, slots, n_slots, id_to_group, max_coverage, positions,
                                     compute_read_stats, staging_bytes)
        L, E = int(info.n_loci), int(info.n_entries)
        chr_t = torch.empty(n_slots + 1, dtype=torch.int32, device=dev)
        pos_t = torch.empty(max(L, 1), dtype=torch.int32, device=dev)
        off_t = torch.empty(L + 1, dtype=torch.int64, device=dev)
        rid_t = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        idb_t = torch.empty(max(E, 1), dtype=torch.int16, device=dev)
        torch.cuda.synchronize(dev)
        try:
            check(lib().secedo_pileup_load_fetch(C.c_void_p(chr_t.data_ptr()), C.c_void_p(pos_t.data_ptr()),
                                                 C.c_void_p(off_t.data_ptr()), C.c_void_p(rid_t.data_ptr()),
                                                 C.c_void_p(idb_t.data_ptr())))
        finally:
            lib().secedo_pileup_load_release()
    if times is not None:
        times.update(_times(t))
    if per_file is not None:
        per_file.update(num_cells=[int(x) for x in nc], max_read_length=[int(x) for x in ml])
    num_cells = int(nc.max()) if len(nc) else 1
    max_read_length = int(ml.max()) if len(ml) else 0
    n_groups = int(i2g.max()) + 1 if len(i2g) else 1
    g2p = np.arange(n_groups, dtype=np.uint32)
    res = dict(chr=chr_t, pos=pos_t, off=off_t, rid=rid_t, idb=idb_t, idb_is16=True,
               g2p=torch.from_numpy(g2p.view(np.int32)).to(dev), n_chr=n_slots, n_loci=L, n_entries=E,
               n_groups=len(g2p))
    return res, num_cells, max_read_length
