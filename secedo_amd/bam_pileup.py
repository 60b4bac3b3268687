"""Pileup creation from BAM or SAM files (include/secedo_bam.h, libsecedo_bam.so).

Host-side mirror of the reference's ``pileup_bams(bam_files, out_pileup, write_text_file, chromosome_id,
max_coverage, min_base_quality, min_map_quality, min_alignment_score, num_threads, min_different)``
(pileup.cpp:235-348). The host inflates the BGZF blocks and walks the records; the per-record decode, the read
name numbering, the base counts, the locus rule and the entry placement run on the GPU
(secedo_amd/csrc/bam_kernels.hip). ``bam_scan`` needs no GPU. No CPU fallback for the pileup itself.

Every file list may hold BAM, coordinate-sorted SAM and BGZF-compressed SAM (``bgzip``'s .sam.gz) files, told apart by
content (BGZF whose text starts with ``BAM\\1``: BAM; other BGZF: compressed SAM; plain gzip is refused; anything else:
SAM text). A SAM file's lines are parsed on the GPU (secedo_amd/csrc/sam_kernels.hip) into the records of the BAM that
``samtools view -b`` writes from it, so results equal that BAM's; errors name its line. A BGZF SAM file is inflated on
the GPU too (secedo_amd/csrc/bgzf_kernels.hip) and gives what its text gives; ``bgzf_inflate`` is that inflate alone.

Multiplexed BAMs (one file, many cells named by a barcode tag such as 10x's ``CB:Z``): ``cell_tag`` and ``cells``
on ``pileup_bams`` / ``pileup_bams_resident`` make cell c the records whose tag value is ``cells[c]``;
``bam_barcodes`` lists the values found and their record counts.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .pileup import FlatPileup
from .sam_flags import parse_filter

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsecedo_bam.so")

MAX_FILES = 16384


class ScanInfo(C.Structure):
    _fields_ = [("n_ref", C.c_uint32), ("sorted", C.c_uint32), ("n_records", C.c_uint64),
                ("n_unmapped", C.c_uint64), ("n_blocks", C.c_uint64), ("inflated_bytes", C.c_uint64),
                ("l_text", C.c_uint32), ("reserved", C.c_uint32)]


class Times(C.Structure):
    _fields_ = [("inflate_ms", C.c_double), ("inflated_bytes", C.c_double), ("walk_ms", C.c_double),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("write_ms", C.c_double),
                ("total_ms", C.c_double)]


class ResultInfo(C.Structure):
    _fields_ = [("n_loci", C.c_uint64), ("n_entries", C.c_uint64), ("n_chr", C.c_uint32),
                ("num_cells", C.c_uint32), ("max_read_length", C.c_uint32), ("reserved", C.c_uint32)]


class RouteInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("host_blocks", "device_blocks", "device_records", "segments",
                                          "rewalked_segments", "uploaded_bytes", "downloaded_record_bytes",
                                          "batches")]


class IndexInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("files_indexed", "files_full", "rejected", "spans", "members",
                                          "members_skipped")]


class BuildInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("files", "records", "chunks", "bins", "windows", "index_bytes",
                                          "joined_runs", "reserved")]


class SelectInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records", "dropped_require", "dropped_exclude", "templates",
                                          "large_templates", "duplicate_templates", "duplicate_records", "reserved")]


class SplitInfo(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("files", "clusters", "cells", "records", "dropped_records", "text_bytes",
                                           "compressed_bytes", "members", "stored_members")] +
                [(k, C.c_double) for k in ("order_ms", "gather_ms", "deflate_ms", "download_ms", "write_ms")])


class SplitRgInfo(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("tagged_records", "replaced_records", "unparsed_records", "added_bytes",
                                           "removed_bytes")] + [("reserved", C.c_uint64 * 3)])


class DepthInfo(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("files", "cells", "chromosomes", "bins", "clusters", "records", "counted",
                                           "dropped_barcode", "dropped_require", "dropped_exclude",
                                           "dropped_duplicate", "dropped_mapq", "out_of_range", "pieces", "pairs",
                                           "text_bytes", "compressed_bytes", "members", "ranges")] +
                [(k, C.c_double) for k in ("order_ms", "count_ms", "format_ms", "deflate_ms", "download_ms",
                                           "write_ms")])


INFLATE_MODES = {"host": 0, "device": 1}
DEPTH_MODES = {"reads": 0, "bases": 1}      # SECEDO_BAM_DEPTH_READS, _BASES
DEPTH_OUTPUTS = {"plain": 0, "bgzf": 1}     # SECEDO_BAM_DEPTH_PLAIN, _BGZF
DEPTH_DUPLICATES = {"off": 0, "remove": 1}  # SECEDO_BAM_DUPLICATES_KEEP, _REMOVE
INDEX_MODES = {"off": 0, "auto": 1, "require": 2}
SPLIT_DUPLICATES = {"off": 0, "remove": 1, "mark": 2}  # SECEDO_BAM_DUPLICATES_KEEP, _REMOVE, _MARK

_vp = C.c_void_p
_u32 = C.c_uint32
_files_t = C.POINTER(C.c_char_p)

SIGNATURES = {
    "secedo_bam_last_error": (C.c_char_p, []),
    "secedo_bam_scan": (C.c_int, [C.c_char_p, _u32, C.POINTER(ScanInfo), _vp, _u32]),
    "secedo_pileup_bams": (C.c_int, [_files_t, _u32, C.c_char_p, C.c_int, _u32, _u32, _u32, _u32, _u32, _u32,
                                     C.c_uint16, C.POINTER(ResultInfo), C.POINTER(Times)]),
    "secedo_pileup_bams_device": (C.c_int, [_files_t, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _u32, C.c_uint16,
                                            _vp, _u32, C.POINTER(ResultInfo), C.POINTER(Times)]),
    "secedo_pileup_bams_cells": (C.c_int, [_files_t, _u32, C.c_char_p, C.c_int, _u32, _u32, _u32, _u32, _u32, _u32,
                                           C.c_uint16, C.c_char_p, _files_t, _u32, C.POINTER(ResultInfo),
                                           C.POINTER(Times)]),
    "secedo_pileup_bams_cells_device": (C.c_int, [_files_t, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _u32,
                                                  C.c_uint16, _vp, _u32, C.c_char_p, _files_t, _u32,
                                                  C.POINTER(ResultInfo), C.POINTER(Times)]),
    "secedo_bam_barcodes": (C.c_int, [_files_t, _u32, C.c_char_p, _vp, _u32, _u32, C.POINTER(_u32),
                                      C.POINTER(C.c_uint64)]),
    "secedo_bam_barcodes_fetch": (C.c_int, [_vp, _vp, _vp]),
    "secedo_bam_fetch": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "secedo_bam_release": (None, []),
    "secedo_bam_set_inflate": (C.c_int, [C.c_int]),
    "secedo_bam_get_inflate": (C.c_int, [C.POINTER(C.c_int)]),
    "secedo_bam_route_stats": (C.c_int, [C.POINTER(RouteInfo)]),
    "secedo_bam_set_index": (C.c_int, [C.c_int]),
    "secedo_bam_get_index": (C.c_int, [C.POINTER(C.c_int)]),
    "secedo_bam_index_stats": (C.c_int, [C.POINTER(IndexInfo)]),
    "secedo_bam_set_read_filter": (C.c_int, [_u32, _u32]),
    "secedo_bam_get_read_filter": (C.c_int, [C.POINTER(_u32), C.POINTER(_u32)]),
    "secedo_bam_set_duplicates": (C.c_int, [C.c_int]),
    "secedo_bam_get_duplicates": (C.c_int, [C.POINTER(C.c_int)]),
    "secedo_bam_select_stats": (C.c_int, [C.POINTER(SelectInfo)]),
    "secedo_bam_index_ranges": (C.c_int, [C.c_char_p, C.POINTER(_u32), _vp, _vp, _vp, _u32]),
    "secedo_bam_scan_device": (C.c_int, [C.c_char_p, _u32, C.POINTER(ScanInfo), _vp, _u32]),
    "secedo_bam_index_build": (C.c_int, [_files_t, _u32, _files_t, C.c_int, _u32, C.POINTER(BuildInfo)]),
    "secedo_bam_split_clusters": (C.c_int, [_files_t, _u32, _vp, _u32, _vp, _u32, C.c_char_p, _files_t, _u32,
                                            C.c_char_p, C.c_int, _u32, C.POINTER(SplitInfo), C.POINTER(Times)]),
    "secedo_bam_split_stats": (C.c_int, [C.POINTER(SplitInfo)]),
    "secedo_bam_split_clusters_rg": (C.c_int, [_files_t, _u32, _vp, _u32, _vp, _u32, C.c_char_p, _files_t, _u32,
                                               C.c_char_p, C.c_int, _u32, C.POINTER(SplitInfo), C.POINTER(Times),
                                               _files_t, _u32, C.POINTER(SplitRgInfo)]),
    "secedo_bam_split_rg_stats": (C.c_int, [C.POINTER(SplitRgInfo)]),
    "secedo_bam_split_clusters_select": (C.c_int, [_files_t, _u32, _vp, _u32, _vp, _u32, C.c_char_p, _files_t, _u32,
                                                   C.c_char_p, C.c_int, _u32, C.POINTER(SplitInfo), C.POINTER(Times),
                                                   _files_t, _u32, C.POINTER(SplitRgInfo), C.c_int, _u32, _u32,
                                                   C.c_int, C.POINTER(SelectInfo)]),
    "secedo_bam_split_select_stats": (C.c_int, [C.POINTER(SelectInfo)]),
    "secedo_bam_depth": (C.c_int, [_files_t, _u32, _vp, _u32, C.c_char_p, _files_t, _u32, _u32, C.c_int, _u32, _u32,
                                   _u32, C.c_int, _vp, _u32, _files_t, _u32, C.c_char_p, C.c_int, C.c_int, _u32,
                                   C.POINTER(DepthInfo), C.POINTER(Times)]),
    "secedo_bam_depth_fetch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "secedo_bam_depth_stats": (C.c_int, [C.POINTER(DepthInfo)]),
    "secedo_bam_depth_chromosomes": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.POINTER(C.c_uint64)]),
    "secedo_bgzf_inflate": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint64)]),
    "secedo_bgzf_inflate_fetch": (C.c_int, [_vp]),
}

_bl = None


def lib():
    global _bl
    if _bl is None:
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
        _bl = l
    return _bl


def check(rc):
    if rc == _lib.OK:
        return
    raise _lib.SecedoError(rc, lib().secedo_bam_last_error().decode(errors="replace"))


def _files(bam_files):
    names = [os.fsencode(str(f)) for f in bam_files]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    return arr, len(names)


def _encode(value) -> bytes:
    return value if isinstance(value, bytes) else str(value).encode("utf-8", "surrogateescape")


def _tag(cell_tag) -> bytes:
    """The two tag characters (the library checks them); anything not two characters long is refused here."""
    t = _encode(cell_tag)
    if len(t) != 2:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "a tag is two characters [A-Za-z][A-Za-z0-9], got %r" % cell_tag)
    return t


def _cells(cell_tag, cells):
    """-> (tag bytes, barcode array, count) of tag mode, or (None, None, 0) without cell_tag."""
    if cell_tag is None:
        if cells is not None:
            raise _lib.SecedoError(_lib.E_INVALID_ARG, "cells needs cell_tag")
        return None, None, 0
    if cells is None:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "cell_tag needs the barcode list cells")
    vals = [_encode(c) for c in cells]
    return _tag(cell_tag), (C.c_char_p * max(len(vals), 1))(*vals), len(vals)


class _route:
    """The BAM route of the calls inside the block: ``inflate`` is "host" (zlib pool and record walk on the host),
    "device" (BGZF inflate and record walk on the GPU) or None for the process setting (secedo_bam_set_inflate, else
    the environment variable SECEDO_BAM_INFLATE). ``index`` likewise: "off", "auto" or "require" (``pileup_bams``), or
    None for the process setting (secedo_bam_set_index, else SECEDO_BAM_INDEX). The settings are per process; the block
    restores what it found."""

    def __init__(self, inflate, index=None):
        if inflate is not None and inflate not in INFLATE_MODES:
            raise _lib.SecedoError(_lib.E_INVALID_ARG, "inflate is 'host' or 'device', got %r" % (inflate,))
        if index is not None and index not in INDEX_MODES:
            raise _lib.SecedoError(_lib.E_INVALID_ARG, "index is 'off', 'auto' or 'require', got %r" % (index,))
        self.inflate = inflate
        self.index = index

    def __enter__(self):
        if self.inflate is not None:
            before = C.c_int(0)
            check(lib().secedo_bam_get_inflate(C.byref(before)))
            self.before = before.value
            check(lib().secedo_bam_set_inflate(INFLATE_MODES[self.inflate]))
        if self.index is not None:
            before = C.c_int(0)
            check(lib().secedo_bam_get_index(C.byref(before)))
            self.index_before = before.value
            check(lib().secedo_bam_set_index(INDEX_MODES[self.index]))

    def __exit__(self, *exc):
        if self.index is not None:
            check(lib().secedo_bam_set_index(self.index_before))
        if self.inflate is not None:
            check(lib().secedo_bam_set_inflate(self.before))
        return False


class _select:
    """The record selection of the calls inside the block: ``require_flags`` / ``exclude_flags`` (an int, or a string:
    decimal, 0x hex or samtools' names, see sam_flags.py) and ``remove_duplicates`` (bool). None keeps the process
    setting of each (secedo_bam_set_read_filter / secedo_bam_set_duplicates, else the environment); giving one of the
    two masks sets both, the other to 0. The settings are per process; the block restores what it found."""

    def __init__(self, require_flags=None, exclude_flags=None, remove_duplicates=None):
        self.filter = None
        if require_flags is not None or exclude_flags is not None:
            try:
                self.filter = parse_filter(require_flags, exclude_flags)
            except ValueError as e:
                raise _lib.SecedoError(_lib.E_INVALID_ARG, str(e))
        self.dup = None if remove_duplicates is None else int(bool(remove_duplicates))

    def __enter__(self):
        if self.filter is not None:
            rq, ex = _u32(0), _u32(0)
            check(lib().secedo_bam_get_read_filter(C.byref(rq), C.byref(ex)))
            self.filter_before = (rq.value, ex.value)
            check(lib().secedo_bam_set_read_filter(*self.filter))
        if self.dup is not None:
            before = C.c_int(0)
            check(lib().secedo_bam_get_duplicates(C.byref(before)))
            self.dup_before = before.value
            check(lib().secedo_bam_set_duplicates(self.dup))

    def __exit__(self, *exc):
        if self.dup is not None:
            check(lib().secedo_bam_set_duplicates(self.dup_before))
        if self.filter is not None:
            check(lib().secedo_bam_set_read_filter(*self.filter_before))
        return False


def bam_select_stats() -> dict:
    """What the last pileup or barcode call on this thread selected, summed over its chromosomes: records that reached
    the flag filter, dropped_require, dropped_exclude (a record is counted once, ``require`` first), templates formed
    by the duplicate removal, large_templates (three or more records, left alone), duplicate_templates and
    duplicate_records dropped. All zero when neither option was on: no pass ran."""
    info = SelectInfo()
    check(lib().secedo_bam_select_stats(C.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in SelectInfo._fields_ if k != "reserved"}


def set_inflate(inflate: str) -> None:
    """Sets the process-wide BAM route: "host" or "device" (see ``pileup_bams``'s ``inflate``)."""
    if inflate not in INFLATE_MODES:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "inflate is 'host' or 'device', got %r" % (inflate,))
    check(lib().secedo_bam_set_inflate(INFLATE_MODES[inflate]))


def set_index(index: str) -> None:
    """Sets the process-wide use of .bai indexes: "off", "auto" or "require" (see ``pileup_bams``'s ``index``)."""
    if index not in INDEX_MODES:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "index is 'off', 'auto' or 'require', got %r" % (index,))
    check(lib().secedo_bam_set_index(INDEX_MODES[index]))


def bam_index_stats() -> dict:
    """What the last pileup or barcode call on this thread did with the indexes of its BAM files: files_indexed,
    files_full (read in full under "auto"), rejected (of those, index files that failed the file-level checks), spans
    and members read through an index, members_skipped (0 for an indexed file: it is never listed in full)."""
    info = IndexInfo()
    check(lib().secedo_bam_index_stats(C.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in IndexInfo._fields_}


def bam_index_ranges(path, max_refs: int = 4096) -> dict:
    """What the .bai beside the BAM ``path`` (<path>.bai, else <path without .bam>.bai) says of each reference ->
    dict(start, end: np.uint64 virtual offsets (coffset << 16 | uoffset), both 0 for a reference without records;
    count: np.int64 records from the pseudo-bin, -1 where the index has none). The file-level checks against the BAM
    are made; a missing or rejected index raises SecedoError. No GPU."""
    n = C.c_uint32(0)
    beg = np.zeros(max_refs, dtype=np.uint64)
    end = np.zeros(max_refs, dtype=np.uint64)
    cnt = np.zeros(max_refs, dtype=np.uint64)
    check(lib().secedo_bam_index_ranges(os.fsencode(str(path)), C.byref(n), _lib.ptr(beg), _lib.ptr(end),
                                        _lib.ptr(cnt), max_refs))
    k = min(int(n.value), max_refs)
    return dict(start=beg[:k].copy(), end=end[:k].copy(), count=cnt[:k].view(np.int64).copy())


def index_file_of(path) -> Optional[str]:
    """The index file the readers would open for the BAM ``path``: <path>.bai, else <path without .bam>.bai; None
    when neither exists."""
    path = os.fspath(path)
    names = [path + ".bai"] + ([path[:-4] + ".bai"] if len(path) > 4 and path.endswith(".bam") else [])
    return next((n for n in names if os.path.exists(n)), None)


def bam_index_build(files: Sequence[str], out_paths: Optional[Sequence[Optional[str]]] = None,
                    overwrite: bool = False, num_threads: int = 1) -> dict:
    """Writes a .bai index for each of the coordinate-sorted BAM ``files`` in one pass on the GPU: the members are
    inflated and the records walked there (the device route, whatever ``set_inflate`` says), many small files to a
    batch, and per record its end on the reference, its bin, the (RefID, bin) runs and the 16 kb windows are found
    there too (secedo_amd/csrc/bam_index_kernels.hip). ``out_paths[f]`` names the index of file f; None, or a None
    entry, means ``<bam>.bai``. An existing output raises unless ``overwrite``. -> dict(files, records, chunks, bins,
    windows, index_bytes, joined_runs) over the indexes written. A file that cannot be indexed (not coordinate-sorted,
    SAM, a corrupt member, a reference or record past 2^29) raises SecedoError naming it and leaves nothing behind;
    the files in front of it in the list keep their indexes. ``bam_route_stats()`` says what the call did."""
    if isinstance(files, (str, bytes, os.PathLike)):
        files = [files]
    arr, n = _files(files)
    outs = None
    if out_paths is not None:
        if len(out_paths) != n:
            raise _lib.SecedoError(_lib.E_INVALID_ARG, "out_paths needs one entry per file (%d), got %d"
                                   % (n, len(out_paths)))
        outs = (C.c_char_p * max(n, 1))(*[None if o is None else os.fsencode(str(o)) for o in out_paths])
    try:
        import torch  # noqa: F401  -- the HIP runtime torch initialises, as for the pileup calls
    except ImportError:
        pass
    info = BuildInfo()
    check(lib().secedo_bam_index_build(arr, n, outs, int(bool(overwrite)), num_threads, C.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in BuildInfo._fields_ if k != "reserved"}


def read_clustering(path) -> list:
    """The cluster of each cell from the comma-separated ``clustering`` file ``secedo_main`` writes; anything but
    cluster numbers in [0, 65535] raises ValueError."""
    with open(path) as f:
        fields = [x.strip() for x in f.read().replace("\n", ",").split(",")]
    out = []
    for x in fields:
        if not x:
            continue
        if not x.isdigit() or int(x) > 65535:
            raise ValueError("%s: %r is not a cluster number in [0, 65535]" % (path, x))
        out.append(int(x))
    if not out:
        raise ValueError("%s lists no cell" % path)
    return out


def _split_dict(info: SplitInfo) -> dict:
    return {k: (int if t is C.c_uint64 else float)(getattr(info, k)) for k, t in SplitInfo._fields_}


def split_stats() -> dict:
    """What the last ``split_clusters`` call on this thread did, a failed one up to its failure: files, clusters,
    cells, records written, dropped_records, text_bytes, compressed_bytes, members, stored_members and the stage
    times order_ms, gather_ms, deflate_ms, download_ms, write_ms."""
    info = SplitInfo()
    check(lib().secedo_bam_split_stats(C.byref(info)))
    return _split_dict(info)


def _split_rg_dict(info: SplitRgInfo) -> dict:
    return {k: int(getattr(info, k)) for k, _ in SplitRgInfo._fields_ if k != "reserved"}


def split_rg_stats() -> dict:
    """What the last ``split_clusters(..., read_groups=True)`` call on this thread edited, a failed one up to its
    failure: tagged_records, replaced_records (their own RG field was removed), unparsed_records (the aux area did not
    parse: nothing removed), added_bytes, removed_bytes. All zero after a call without ``read_groups``."""
    info = SplitRgInfo()
    check(lib().secedo_bam_split_rg_stats(C.byref(info)))
    return _split_rg_dict(info)


def _select_dict(info: SelectInfo) -> dict:
    return {k: int(getattr(info, k)) for k, _ in SelectInfo._fields_ if k != "reserved"}


def split_select_stats() -> dict:
    """What the last ``split_clusters`` call on this thread selected (``require_flags``, ``exclude_flags``,
    ``duplicates``), a failed one up to its failure, with the keys of ``bam_select_stats()``: records that reached the
    flag filter, dropped_require, dropped_exclude, templates, large_templates, and duplicate_templates /
    duplicate_records chosen, whether marked or removed. All zero after a call with the three options off.
    ``bam_select_stats()`` itself is the pileup's and is not touched by a split call."""
    info = SelectInfo()
    check(lib().secedo_bam_split_select_stats(C.byref(info)))
    return _select_dict(info)


def split_clusters(bam_files: Sequence[str], clustering, out_dir, chromosome_ids: Sequence[int], *, cell_tag=None,
                   cells=None, inflate=None, index=None, bai: bool = False, overwrite: bool = False,
                   num_threads: int = 8, times: Optional[dict] = None, read_groups: bool = False,
                   cell_names: Optional[Sequence[str]] = None, require_flags=None, exclude_flags=None,
                   duplicates: str = "off") -> dict:
    """Writes ``<out_dir>/cluster_<k>.bam`` for every k in 0..max(clustering): the records of the cells of cluster k
    on the chromosomes ``chromosome_ids`` (RefIDs), merged in coordinate order (RefID, Position, input file, record),
    byte for byte as they are in the input; a k no cell has gives a header-only file. The pseudo-bulk BAMs of the
    subclones. ``clustering``: the cluster of each cell, a sequence or the path of the comma-separated file
    ``secedo_main`` writes. The cell of a record is its file's index, or with ``cell_tag`` / ``cells`` the index of its
    Z-typed tag value in ``cells`` as in ``pileup_bams`` (other records are dropped and counted). The inputs go through
    the pileup's input layer: BAM, SAM and bgzipped SAM, ``inflate`` and ``index`` as in ``pileup_bams``; the flag
    filter, the duplicate removal and the quality rules do not apply. Cell to cluster, the order, the gather of the
    records into per-cluster streams and the DEFLATE run on the GPU; the bytes of every file are fixed (see
    include/secedo_bam.h). All inputs must share one reference list. An existing output raises unless ``overwrite``; a
    failed call leaves no file behind. ``bai``: also write ``cluster_<k>.bam.bai`` with ``bam_index_build``.
    ``read_groups``: name each read's cell in the files (secedo_bam_split_clusters_rg): every record gets
    ``RG:Z:<name of its cell>`` as its last field in place of the RG field it had, and cluster k's header gets
    ``@RG ID:<name> SM:cluster_<k>`` per cell of the cluster in place of the inputs' @RG lines; the edit runs on the
    GPU inside the gather. ``cell_names``: one name per cell (1 to 254 bytes in 0x21..0x7E, no two equal); None names a
    cell by its file's base name without .bam / .sam / .sam.gz, or by its barcode. The files are multiplexed BAMs that
    ``pileup_bams(..., cell_tag="RG", cells=names)`` reads back cell by cell.
    ``require_flags`` / ``exclude_flags`` (an int, or a string as for ``pileup_bams``, see sam_flags.py) and
    ``duplicates`` ("off", "mark" or "remove") select records while each record's cell is still known
    (secedo_bam_split_clusters_select): a record is written iff ``(flag & require) == require and (flag & exclude) ==
    0``, and among those duplicates are decided per cell and chromosome exactly as ``pileup_bams(...,
    remove_duplicates=True)`` decides them; "remove" leaves them out, "mark" writes them with 0x400 set in their FLAG
    and changes nothing else. Two reads of one cluster with the same ends from two cells are no duplicates, which no
    tool can tell once the files are merged. These are this call's own options: the process-wide filter and duplicate
    settings of the pileup calls, and their environment variables, never apply to ``split_clusters``.
    -> the dict of ``split_stats()``, with ``read_groups`` also the keys of ``split_rg_stats()``, with any of the three
    selection options on also those of ``split_select_stats()`` (its ``records``, the records that reached the filter,
    as ``filter_records``: ``records`` stays the records written); ``times`` (a dict) receives the step times in ms."""
    if cell_names is not None and not read_groups:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "cell_names needs read_groups")
    if duplicates not in SPLIT_DUPLICATES:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "duplicates is 'off', 'mark' or 'remove', got %r" % (duplicates,))
    try:
        require, exclude = parse_filter(require_flags, exclude_flags)
    except ValueError as e:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, str(e))
    select = bool(require or exclude or SPLIT_DUPLICATES[duplicates])
    arr, n = _files(bam_files)
    if isinstance(clustering, (str, bytes, os.PathLike)):
        try:
            clustering = read_clustering(clustering)
        except ValueError as e:
            raise _lib.SecedoError(_lib.E_INVALID_ARG, str(e))
    cl = np.asarray(clustering)
    if cl.ndim != 1 or cl.size == 0 or not np.issubdtype(cl.dtype, np.integer) or cl.min() < 0 or cl.max() > 65535:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "clustering is a non-empty sequence of cluster numbers in [0, 65535]")
    cl = np.ascontiguousarray(cl, dtype=np.uint16)
    tag, bcs, n_bcs = _cells(cell_tag, cells)
    ids = np.ascontiguousarray(chromosome_ids, dtype=np.uint32)
    try:
        import torch  # noqa: F401  -- the HIP runtime torch initialises, as for the pileup calls
    except ImportError:
        pass
    info, t, rg, sel = SplitInfo(), Times(), SplitRgInfo(), SelectInfo()
    args = (arr, n, _lib.ptr(ids) if len(ids) else None, len(ids), _lib.ptr(cl), len(cl), tag, bcs, n_bcs,
            os.fsencode(str(out_dir)), int(bool(overwrite)), num_threads, C.byref(info), C.byref(t))
    with _route(inflate, index):
        names = None if cell_names is None else [_encode(x) for x in cell_names]
        names_arr = None if names is None else (C.c_char_p * max(len(names), 1))(*names)
        if select:
            check(lib().secedo_bam_split_clusters_select(*args, names_arr, 0 if names is None else len(names),
                                                         C.byref(rg), int(bool(read_groups)), require, exclude,
                                                         SPLIT_DUPLICATES[duplicates], C.byref(sel)))
        elif read_groups:
            check(lib().secedo_bam_split_clusters_rg(*args, names_arr, 0 if names is None else len(names),
                                                     C.byref(rg)))
        else:
            check(lib().secedo_bam_split_clusters(*args))
    if times is not None:
        times.update(_times(t))
    if bai:
        outs = [os.path.join(str(out_dir), "cluster_%d.bam" % k) for k in range(int(info.clusters))]
        bam_index_build(outs, overwrite=True, num_threads=max(1, min(int(num_threads), 16)))
    out = _split_dict(info)
    if read_groups:
        out.update(_split_rg_dict(rg))
    if select:  # "records" is the split's own key (records written): the filter's count goes by filter_records
        out.update(("filter_records" if k == "records" else k, v) for k, v in _select_dict(sel).items())
    return out


def _depth_dict(info: DepthInfo) -> dict:
    return {k: (int if ty is C.c_uint64 else float)(getattr(info, k)) for k, ty in DepthInfo._fields_}


def depth_stats() -> dict:
    """What the last ``bin_depth`` call on this thread did, a failed one up to its failure: files, cells, chromosomes,
    bins, clusters, records (after the barcode step), counted (after all five steps), dropped_barcode,
    dropped_require, dropped_exclude, dropped_duplicate, dropped_mapq, out_of_range, pieces, pairs, text_bytes,
    compressed_bytes, members, ranges and the stage times order_ms, count_ms, format_ms, deflate_ms, download_ms,
    write_ms."""
    info = DepthInfo()
    check(lib().secedo_bam_depth_stats(C.byref(info)))
    return _depth_dict(info)


def bin_depth(files: Sequence[str], bin_size: int, chromosome_ids: Sequence[int], out_dir=None, mode: str = "reads",
              min_map_quality: int = 30, require_flags=None, exclude_flags=None, duplicates: str = "off",
              cell_tag=None, cells=None, clustering=None, cell_names: Optional[Sequence[str]] = None,
              output: str = "plain", overwrite: bool = False, times: Optional[dict] = None, *, inflate=None,
              index=None, num_threads: int = 8, reference_genome=None) -> dict:
    """Per-cell read depth in fixed genomic bins: the bins x cells count matrix copy-number tools start from, counted
    on the GPU (secedo_bam_depth; the rules and the bytes of the files are in include/secedo_bam.h). ``files`` are the
    inputs of ``pileup_bams`` (BAM, SAM, bgzipped SAM; ``inflate`` and ``index`` as there), one cell per file, or with
    ``cell_tag`` / ``cells`` multiplexed files whose records name their cell by a barcode. Chromosome ``c`` of
    ``chromosome_ids`` (RefIDs, any order) has ``ceil(LN_c / bin_size)`` bins; global bin numbers run over the
    requested chromosomes in ascending id. A record is selected by, in this order, its barcode, ``require_flags`` /
    ``exclude_flags`` (as for ``split_clusters``), ``duplicates`` ("off" or "remove": per cell and chromosome, the
    pileup's rule), ``MapQuality >= min_map_quality`` and ``0 <= Position < LN_c``; these are this call's own, the
    process-wide filter and duplicate settings never apply. ``mode`` "reads": each surviving record adds 1 to the bin
    of its Position; "bases": it adds to every bin it touches the reference positions there that an M, = or X op of
    its CIGAR covers. ``clustering`` (a sequence, or the file ``secedo_main`` writes) adds the per-cluster sums.
    ``out_dir``: also write ``<out_dir>/depth/`` (depth.bins.bed, depth.counts.mtx, depth.samples.tsv,
    depth.cells.tsv and with a clustering depth.clusters.tsv; ``output="bgzf"`` writes the .mtx and the two longer
    .tsv as .gz); existing files raise unless ``overwrite``; a failed call leaves nothing behind. ``cell_names``: one
    name per cell; None names a cell by its barcode or its file's base name. ``reference_genome`` (a FASTA, plain,
    gzip or bgzip): after the depth, ``genome_bins`` runs on it with the requested chromosomes' @SQ names and LN as
    ``contigs`` and ``lengths``, so a genome with other names or lengths raises and says why; the result gains ``gc``
    (uint32 [bins, 6]: a, c, g, t, other, masked, row for row with the bins) and ``out_dir`` gains
    ``depth/depth.gc.tsv`` (``.gz`` under ``output="bgzf"``), whose first three columns are depth.bins.bed's. When the
    genome step fails, what the depth step of this call wrote is removed again.
    -> dict of numpy arrays: bin_chrom, bin_start, bin_end [bins]; pair_bin, pair_cell (0-based, uint32), pair_value
    (uint64) [pairs], ordered by bin and then cell; cells [n_cells, 5] uint64 (records, counted, sum, nonzero_bins,
    max_value); cluster_sums [bins, K] uint64 (with a clustering); names (list of str); stats (``depth_stats()``).
    ``times`` (a dict) receives the input layer's step times in ms."""
    if mode not in DEPTH_MODES:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "mode is 'reads' or 'bases', got %r" % (mode,))
    if output not in DEPTH_OUTPUTS:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "output is 'plain' or 'bgzf', got %r" % (output,))
    if duplicates not in DEPTH_DUPLICATES:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "duplicates is 'off' or 'remove', got %r" % (duplicates,))
    if not isinstance(bin_size, (int, np.integer)) or bin_size < 0 or bin_size > 0xFFFFFFFF:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "bin_size is an integer in [1, 2^32 - 1], got %r" % (bin_size,))
    if not isinstance(min_map_quality, (int, np.integer)) or not 0 <= min_map_quality <= 255:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "min_map_quality is an integer in [0, 255], got %r"
                               % (min_map_quality,))
    try:
        require, exclude = parse_filter(require_flags, exclude_flags)
    except ValueError as e:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, str(e))
    if isinstance(files, (str, bytes, os.PathLike)):
        files = [files]
    arr, n = _files(files)
    cl = None
    if clustering is not None:
        if isinstance(clustering, (str, bytes, os.PathLike)):
            try:
                clustering = read_clustering(clustering)
            except ValueError as e:
                raise _lib.SecedoError(_lib.E_INVALID_ARG, str(e))
        cl = np.asarray(clustering)
        if cl.ndim != 1 or cl.size == 0 or not np.issubdtype(cl.dtype, np.integer) or cl.min() < 0 or cl.max() > 65535:
            raise _lib.SecedoError(_lib.E_INVALID_ARG,
                                   "clustering is a non-empty sequence of cluster numbers in [0, 65535]")
        cl = np.ascontiguousarray(cl, dtype=np.uint16)
    tag, bcs, n_bcs = _cells(cell_tag, cells)
    ids = np.ascontiguousarray(chromosome_ids, dtype=np.uint32)
    gc_path, had_dir = None, False
    if reference_genome is not None and out_dir is not None:
        had_dir = os.path.isdir(os.path.join(str(out_dir), "depth"))
        gc_path = os.path.join(str(out_dir), "depth", "depth.gc.tsv")
        gc_target = gc_path + (".gz" if output == "bgzf" else "")
        if not overwrite and os.path.exists(gc_target):  # before anything runs
            raise _lib.SecedoError(_lib.E_INVALID_ARG, "%s exists; pass overwrite to replace it" % gc_target)
    names = None if cell_names is None else [_encode(x) for x in cell_names]
    names_arr = None if names is None else (C.c_char_p * max(len(names), 1))(*names)
    try:
        import torch  # noqa: F401  -- the HIP runtime torch initialises, as for the pileup calls
    except ImportError:
        pass
    info, t = DepthInfo(), Times()
    with _route(inflate, index):
        check(lib().secedo_bam_depth(arr, n, _lib.ptr(ids) if len(ids) else None, len(ids), tag, bcs, n_bcs,
                                     int(bin_size), DEPTH_MODES[mode], int(min_map_quality), require, exclude,
                                     DEPTH_DUPLICATES[duplicates], _lib.ptr(cl), 0 if cl is None else len(cl),
                                     names_arr, 0 if names is None else len(names),
                                     None if out_dir is None else os.fsencode(str(out_dir)), DEPTH_OUTPUTS[output],
                                     int(bool(overwrite)), num_threads, C.byref(info), C.byref(t)))
    if times is not None:
        times.update(_times(t))
    n_bins, n_pairs, n_cells, k = int(info.bins), int(info.pairs), int(info.cells), int(info.clusters)
    out = dict(bin_chrom=np.zeros(n_bins, np.uint32), bin_start=np.zeros(n_bins, np.uint32),
               bin_end=np.zeros(n_bins, np.uint32), pair_bin=np.zeros(n_pairs, np.uint32),
               pair_cell=np.zeros(n_pairs, np.uint32), pair_value=np.zeros(n_pairs, np.uint64),
               cells=np.zeros((n_cells, 5), np.uint64), cluster_sums=np.zeros((n_bins, k), np.uint64))
    check(lib().secedo_bam_depth_fetch(*[_lib.ptr(out[key]) for key in ("bin_chrom", "bin_start", "bin_end",
                                                                        "pair_bin", "pair_cell", "pair_value",
                                                                        "cells", "cluster_sums")]))
    if cl is None:
        del out["cluster_sums"]
    if cell_names is not None:
        out["names"] = [str(x) for x in cell_names]
    elif cell_tag is not None:
        out["names"] = [x.decode("utf-8", "surrogateescape") if isinstance(x, bytes) else str(x) for x in cells]
    else:
        out["names"] = [default_cell_name(f) for f in files]
    out["stats"] = _depth_dict(info)
    if reference_genome is not None:
        try:
            out["gc"] = _depth_gc(reference_genome, int(bin_size), gc_path, output, overwrite)
        except Exception:
            if out_dir is not None:  # a failed call leaves nothing behind: what the depth step of this call wrote
                _remove_depth_files(os.path.join(str(out_dir), "depth"), output, cl is not None, not had_dir)
            raise
    return out


def depth_chromosomes():
    """The requested chromosomes of the last ``bin_depth`` call on this thread, in ascending id (the order of the
    bins) -> (names, lengths): their @SQ names (list of str) and LN (uint32 array)."""
    n_bytes = C.c_uint64(0)
    check(lib().secedo_bam_depth_chromosomes(None, 0, None, None, C.byref(n_bytes)))
    info = DepthInfo()
    check(lib().secedo_bam_depth_stats(C.byref(info)))
    n = int(info.chromosomes)
    raw = np.zeros(max(int(n_bytes.value), 1), np.uint8)
    off, ln = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32)
    check(lib().secedo_bam_depth_chromosomes(_lib.ptr(raw), int(n_bytes.value), _lib.ptr(off), _lib.ptr(ln), None))
    data = raw.tobytes()
    return [data[int(off[i]):int(off[i + 1])].decode("utf-8", "surrogateescape") for i in range(n)], ln


def _depth_gc(reference_genome, bin_size, gc_path, output, overwrite):
    """The genome step of ``bin_depth``: the composition of the depth call's bins, refused unless the genome has the
    BAM header's chromosome names and lengths."""
    from .variant import genome_bins

    names, ln = depth_chromosomes()
    try:
        g = genome_bins(reference_genome, bin_size, contigs=names, lengths=ln, out_path=gc_path, output=output,
                        overwrite=overwrite)
    except _lib.SecedoError as e:
        raise _lib.SecedoError(e.code, "reference_genome %s does not fit the BAM header (its @SQ names and LN are the "
                               "contigs and lengths asked for): %s" % (reference_genome, str(e).split(": ", 1)[-1]))
    return g["counts"]


def _remove_depth_files(depth_dir, output, clustered, made_dir):
    """Removes what secedo_bam_depth wrote under ``depth_dir`` for this output kind, and the directory if asked."""
    gz = ".gz" if output == "bgzf" else ""
    names = ["depth.bins.bed", "depth.samples.tsv", "depth.counts.mtx" + gz, "depth.cells.tsv" + gz]
    if clustered:
        names.append("depth.clusters.tsv" + gz)
    for name in names:
        path = os.path.join(depth_dir, name)
        if os.path.exists(path):
            os.unlink(path)
    if made_dir and os.path.isdir(depth_dir) and not os.listdir(depth_dir):
        os.rmdir(depth_dir)


def default_cell_name(path) -> str:
    """The name a per-file cell gets without ``cell_names``: the file's base name without the first of .sam.gz, .bam,
    .sam that it ends in."""
    base = os.path.basename(os.fspath(path))
    for ext in (".sam.gz", ".bam", ".sam"):
        if base.endswith(ext):
            return base[:-len(ext)]
    return base


def bam_route_stats() -> dict:
    """What the last pileup, barcode or scan call on this thread did: members inflated on the host and on the device,
    records walked on the device, walk segments and how many of them were re-walked, compressed bytes uploaded, record
    bytes downloaded, device inflate launches."""
    info = RouteInfo()
    check(lib().secedo_bam_route_stats(C.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in RouteInfo._fields_}


def bam_barcodes(files: Sequence[str], tag: str, chromosome_ids: Sequence[int], num_threads: int = 1, *,
                 inflate=None, index=None, require_flags=None, exclude_flags=None):
    """The distinct Z-typed values of ``tag`` over the records of the given chromosomes of ``files`` (BAM or SAM),
    sorted bytewise -> (values [str], counts np.uint64: records per value). Needs the GPU. ``inflate``: the BAM
    route, and ``index``: the use of .bai indexes, both as in ``pileup_bams``. ``require_flags`` / ``exclude_flags``:
    only records that pass the flag filter are counted, as in ``pileup_bams``."""
    arr, n = _files(files)
    ids = np.ascontiguousarray(chromosome_ids, dtype=np.uint32)
    n_val, n_bytes = C.c_uint32(0), C.c_uint64(0)
    t = _tag(tag)
    try:
        import torch  # noqa: F401  -- the HIP runtime torch initialises, as for the pileup calls
    except ImportError:
        pass
    with _route(inflate, index), _select(require_flags, exclude_flags):
        check(lib().secedo_bam_barcodes(arr, n, t, _lib.ptr(ids) if len(ids) else None, len(ids), num_threads,
                                        C.byref(n_val), C.byref(n_bytes)))
    k = int(n_val.value)
    buf = C.create_string_buffer(max(int(n_bytes.value), 1))
    off = np.zeros(k + 1, dtype=np.uint64)
    counts = np.zeros(max(k, 1), dtype=np.uint64)
    check(lib().secedo_bam_barcodes_fetch(C.cast(buf, C.c_void_p), _lib.ptr(off), _lib.ptr(counts)))
    raw = buf.raw
    values = [raw[int(off[i]):int(off[i + 1])].decode("utf-8", "surrogateescape") for i in range(k)]
    return values, counts[:k].copy()


def bgzf_inflate(path) -> np.ndarray:
    """The inflated bytes of a BGZF file (BAM, bgzipped SAM, ...) -> np.uint8. Every member is inflated on the GPU,
    its ISIZE and CRC32 checked there; a bad member raises SecedoError naming its block. Needs the GPU."""
    try:
        import torch  # noqa: F401  -- the HIP runtime torch initialises, as for the pileup calls
    except ImportError:
        pass
    n = C.c_uint64(0)
    check(lib().secedo_bgzf_inflate(os.fsencode(str(path)), C.byref(n)))
    out = np.zeros(int(n.value), dtype=np.uint8)
    check(lib().secedo_bgzf_inflate_fetch(_lib.ptr(out) if len(out) else None))
    lib().secedo_bam_release()
    return out


def bam_scan(path, num_threads: int = 1, max_refs: int = 4096, device: bool = False) -> dict:
    """Header and record summary of one BAM file: n_ref, sorted, n_records, n_unmapped, n_blocks, inflated_bytes,
    l_text and records_per_ref (one count per @SQ entry). No GPU, unless ``device``: then the members are inflated
    and the records walked on the GPU, with the same result."""
    info = ScanInfo()
    per = np.zeros(max_refs, dtype=np.uint64)
    if device:
        try:
            import torch  # noqa: F401  -- the HIP runtime torch initialises, as for the pileup calls
        except ImportError:
            pass
    scan = lib().secedo_bam_scan_device if device else lib().secedo_bam_scan
    check(scan(os.fsencode(str(path)), num_threads, C.byref(info), _lib.ptr(per), max_refs))
    out = {k: int(getattr(info, k)) for k, _ in ScanInfo._fields_ if k != "reserved"}
    out["sorted"] = bool(info.sorted)
    out["records_per_ref"] = per[:min(info.n_ref, max_refs)].copy()
    return out


def _times(t: Times) -> dict:
    return {k: float(getattr(t, k)) for k, _ in Times._fields_}


def _fetch_host(info: ResultInfo) -> FlatPileup:
    chr_off = np.zeros(info.n_chr + 1, dtype=np.uint32)
    pos = np.zeros(max(info.n_loci, 1), dtype=np.uint32)
    off = np.zeros(info.n_loci + 1, dtype=np.uint64)
    rid = np.zeros(max(info.n_entries, 1), dtype=np.uint32)
    idb = np.zeros(max(info.n_entries, 1), dtype=np.uint16)
    check(lib().secedo_bam_fetch(_lib.ptr(chr_off), _lib.ptr(pos), _lib.ptr(off), _lib.ptr(rid), _lib.ptr(idb)))
    lib().secedo_bam_release()
    return FlatPileup(chr_off, pos[:info.n_loci], off, rid[:info.n_entries],
                      idb[:info.n_entries].astype(np.uint32))


def pileup_bams(bam_files: Sequence[str], out_pileup: Optional[str], write_text_file: bool, chromosome_id: int,
                max_coverage: int, min_base_quality: int, min_map_quality: int, min_alignment_score: int,
                num_threads: int, min_different: int, times: Optional[dict] = None, *, cell_tag=None,
                cells=None, inflate=None, index=None, require_flags=None, exclude_flags=None,
                remove_duplicates=None) -> FlatPileup:
    """The reference's pileup_bams() on BAM or SAM files -> a one-chromosome FlatPileup (id_base = cell << 2 |
    base). Writes <out_pileup>.bin/.map/.txt unless out_pileup is None. ``times`` (a dict) receives the step times in ms.

    With ``cell_tag`` (e.g. "CB") the files are multiplexed: cell c is the records whose Z-typed ``cell_tag`` value
    is ``cells[c]``; the result equals this call on the per-cell split files.

    ``inflate``: the route BAM files take. "host" (the default setting) inflates them with zlib in a host pool and
    walks the records on the host; "device" uploads the compressed bytes, inflates them and walks the records on the
    GPU, and gives the same result; None keeps the process setting (``set_inflate``, SECEDO_BAM_INFLATE).

    ``index``: whether BAM files are read through their .bai index (<path>.bai, else <path without .bam>.bai). "off"
    (the default setting) opens no index and reads every BGZF member; "auto" reads of a BAM with a usable index only
    the members that hold the chromosome's records, and any other BAM in full; "require" raises for a BAM without a
    usable index. For coordinate-sorted BAMs with a matching index the result is the same; an index that does not
    match its BAM raises. None keeps the process setting (``set_index``, SECEDO_BAM_INDEX). ``bam_index_stats()`` says
    what the call did.

    ``require_flags`` / ``exclude_flags``: a record is used iff (flag & require) == require and (flag & exclude) == 0,
    as samtools' -f / -F. Each is an int or a string (decimal, 0x hex, or a comma list of samtools' names such as
    "SECONDARY,SUPPLEMENTARY,DUP,QCFAIL,UNMAP"). ``remove_duplicates``: among the records the filter kept, per cell, templates
    (records of one read name) with the same unclipped 5' ends and strands are duplicates; the one with the highest
    sum of base qualities >= 15 stays (ties: the earliest). Dropped records take no read id and pass no check, so the
    result equals this call with the options off on the files without them. The defaults (None) keep the process
    settings, which are off unless the environment sets them. ``bam_select_stats()`` says what the call dropped."""
    arr, n = _files(bam_files)
    tag, bcs, n_bcs = _cells(cell_tag, cells)
    info, t = ResultInfo(), Times()
    out = None if out_pileup is None else os.fsencode(str(out_pileup))
    with _route(inflate, index), _select(require_flags, exclude_flags, remove_duplicates):
        if tag is None:
            check(lib().secedo_pileup_bams(arr, n, out, int(bool(write_text_file)), chromosome_id, max_coverage,
                                           min_base_quality, min_map_quality, min_alignment_score, num_threads,
                                           min_different, C.byref(info), C.byref(t)))
        else:
            check(lib().secedo_pileup_bams_cells(arr, n, out, int(bool(write_text_file)), chromosome_id,
                                                 max_coverage, min_base_quality, min_map_quality,
                                                 min_alignment_score, num_threads, min_different, tag, bcs, n_bcs,
                                                 C.byref(info), C.byref(t)))
    if times is not None:
        times.update(_times(t))
    return _fetch_host(info)


def pileup_bams_resident(plan, bam_files: Sequence[str], chromosome_ids: Sequence[int], max_coverage: int = 100,
                         min_base_quality: int = 30, min_map_quality: int = 30, min_alignment_score: int = 0,
                         num_threads: int = 8, min_different: int = 3, id_to_group=None, group_id_to_pos=None,
                         times: Optional[dict] = None, *, cell_tag=None, cells=None, inflate=None, index=None,
                         require_flags=None, exclude_flags=None, remove_duplicates=None):
    """Several chromosomes in one pass over the BAM or SAM files, straight into HBM on ``plan``'s device.

    -> (res, num_cells, max_read_length): ``res`` is the resident pileup dict of SimilarityMatrixPlan.upload,
    which filter_resident, divide_cluster_resident and variant_calling_resident take; num_cells and
    max_read_length are what read_pileup would report on the written .bin files (maxima over chromosomes).
    ``cell_tag`` / ``cells``: multiplexed files, as in pileup_bams; id_to_group then maps barcode indices.
    ``inflate``: the BAM route, and ``index``: the use of .bai indexes, both as in pileup_bams; ``require_flags``,
    ``exclude_flags`` and ``remove_duplicates`` likewise (duplicates are found per chromosome)."""
    import torch

    ids = np.ascontiguousarray(chromosome_ids, dtype=np.uint32)
    arr, n = _files(bam_files)
    tag, bcs, n_bcs = _cells(cell_tag, cells)
    i2g = None if id_to_group is None else np.ascontiguousarray(id_to_group, dtype=np.uint16)
    info, t = ResultInfo(), Times()
    dev = "cuda:%d" % plan.device
    with torch.cuda.device(plan.device), _route(inflate, index), \
            _select(require_flags, exclude_flags, remove_duplicates):
        i2g_p, n_i2g = (_lib.ptr(i2g), len(i2g)) if i2g is not None else (None, 0)
        if tag is None:
            check(lib().secedo_pileup_bams_device(arr, n, _lib.ptr(ids), len(ids), max_coverage, min_base_quality,
                                                  min_map_quality, min_alignment_score, num_threads, min_different,
                                                  i2g_p, n_i2g, C.byref(info), C.byref(t)))
        else:
            check(lib().secedo_pileup_bams_cells_device(arr, n, _lib.ptr(ids), len(ids), max_coverage,
                                                        min_base_quality, min_map_quality, min_alignment_score,
                                                        num_threads, min_different, i2g_p, n_i2g, tag, bcs, n_bcs,
                                                        C.byref(info), C.byref(t)))
        L, E = int(info.n_loci), int(info.n_entries)
        chr_t = torch.from_numpy(np.zeros(len(ids) + 1, dtype=np.int32)).to(dev)
        pos_t = torch.empty(max(L, 1), dtype=torch.int32, device=dev)
        off_t = torch.empty(L + 1, dtype=torch.int64, device=dev)
        rid_t = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        idb_t = torch.empty(max(E, 1), dtype=torch.int16, device=dev)
        torch.cuda.synchronize(dev)
        check(lib().secedo_bam_fetch(C.c_void_p(chr_t.data_ptr()), C.c_void_p(pos_t.data_ptr()),
                                     C.c_void_p(off_t.data_ptr()), C.c_void_p(rid_t.data_ptr()),
                                     C.c_void_p(idb_t.data_ptr())))
        lib().secedo_bam_release()
    if times is not None:
        times.update(_times(t))
    num_cells = int(info.num_cells)
    if group_id_to_pos is None:
        n_groups = int(i2g.max()) + 1 if i2g is not None and len(i2g) else num_cells
        group_id_to_pos = np.arange(n_groups, dtype=np.uint32)
    g2p = np.ascontiguousarray(group_id_to_pos, dtype=np.uint32)
    res = dict(chr=chr_t, pos=pos_t, off=off_t, rid=rid_t, idb=idb_t, idb_is16=True,
               g2p=torch.from_numpy(g2p.view(np.int32)).to(dev), n_chr=len(ids), n_loci=L, n_entries=E,
               n_groups=len(g2p))
    return res, num_cells, int(info.max_read_length)
