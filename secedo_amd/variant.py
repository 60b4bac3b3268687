"""Variant calling after the clustering (include/secedo_variant.h, libsecedo_variant.so).

Host-side mirror of the reference's ``variant_calling(pos_data, clusters, reference_genome, map_file,
hetero_prior, theta, out_dir)`` (variant_calling.cpp:323-461): the per-locus genotype calls and the per-cell
counters run on the GPU (secedo_amd/csrc/variant_kernels.hip); the FASTA / map reading and the VCF text are
host code in the library. ``reference_genotypes`` and the FASTA / map helpers need no GPU. No CPU fallback for
the calls.

The reference genome may be plain text, BGZF or plain gzip (told by content). Its parse and the per-locus gather
run on the host by default; ``set_fasta_route("device")``, the environment ``SECEDO_FASTA=device`` or the
``fasta_route`` keyword of the calling functions move them to the GPU (a BGZF file always goes there), where the
text never lives on the host. ``fasta_stats()`` says what the last call did.

The VCF files are plain text written by the host by default. ``set_vcf_output("bgzf")``, the environment
``SECEDO_VCF=bgzf`` or the ``vcf_output`` keyword of the calling functions write ``cluster_<i>.vcf.gz`` and
``common.vcf.gz`` instead: the lines are formatted on the GPU from the records where the calls left them, cut into BGZF
members and deflated there (secedo_amd/csrc/bgzf_deflate_kernels.hip), and only compressed bytes come back. Each file
inflates to the bytes the plain route writes. ``vcf_stats()`` says what the last call wrote; ``bgzf_deflate`` is the
encoder alone, the mirror of ``secedo_amd.bgzf_inflate``.

``set_vcf_index("tbi")``, the environment ``SECEDO_VCF_INDEX=tbi`` or the ``vcf_index`` keyword of the calling
functions make the bgzf output also write ``<file>.vcf.gz.tbi``, the tabix index region queries need, from a line pass
over the text where the formatter left it (secedo_amd/csrc/tabix_kernels.hip). ``tabix_build(files)`` indexes
bgzip-compressed VCFs that exist: their compressed bytes are inflated and indexed on the GPU, many small files to a
batch. Both give the same bytes for the same file; ``tabix_stats()`` says what the last of either did.

``set_allele_counts("all" | "cluster")``, the environment ``SECEDO_ALLELE_COUNTS`` or the ``allele_counts`` keyword of
the calling functions add ``<out_dir>/allele_counts/``: the sparse sites x cells matrices of alternate-allele, total and
other read counts at the called variants (``cellSNP.tag.AD.mtx``, ``.DP.mtx``, ``.OTH.mtx``), the sites as
``cellSNP.base.vcf`` and the cells as ``cellSNP.samples.tsv`` (``cell_names``: a list or a file of names), counted and
formatted on the GPU (secedo_amd/csrc/allele_kernels.hip) and compressed to ``.gz`` under the bgzf output. "all" takes
every locus with a call, "cluster" the loci where clusters differ. ``allele_masks`` (no GPU) and ``allele_counts`` give
the sites and the (site, cell) pairs as arrays; ``allele_stats()`` says what the last call did. Off by default.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from .pileup import FlatPileup, flatten

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsecedo_variant.so")

NO_GENOTYPE = 255
KINDS = ("pooled", "common", "cluster")

_vp = C.c_void_p
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_f64p = C.POINTER(C.c_double)


class Record(C.Structure):
    _fields_ = [("locus", C.c_uint32), ("cluster", C.c_uint16), ("genotype", C.c_uint8), ("kind", C.c_uint8),
                ("counts", C.c_uint16 * 4)]


class Times(C.Structure):
    _fields_ = [("fasta_ms", C.c_double), ("gather_ms", C.c_double), ("device_ms", C.c_double),
                ("write_ms", C.c_double), ("kernel_ms", C.c_double)]


class FastaInfo(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("route", C.c_uint32), ("fell_back_for_map", C.c_uint32),
                ("reserved", C.c_uint32), ("host_inflated_bytes", C.c_uint64), ("device_members", C.c_uint64),
                ("uploaded_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("ranges", C.c_uint64),
                ("contigs", C.c_uint64), ("contigs_used", C.c_uint64), ("inflate_ms", C.c_double),
                ("upload_ms", C.c_double), ("parse_gather_ms", C.c_double)]


class VcfInfo(C.Structure):
    _fields_ = [("output", C.c_uint32), ("reserved", C.c_uint32), ("files", C.c_uint64), ("text_bytes", C.c_uint64),
                ("compressed_bytes", C.c_uint64), ("blocks", C.c_uint64), ("stored_blocks", C.c_uint64),
                ("format_ms", C.c_double), ("deflate_ms", C.c_double), ("download_ms", C.c_double),
                ("write_ms", C.c_double), ("deflate_kernel_ms", C.c_double)]


class TabixInfo(C.Structure):
    _fields_ = [("files", C.c_uint64), ("lines", C.c_uint64), ("data_lines", C.c_uint64), ("names", C.c_uint64),
                ("bins", C.c_uint64), ("chunks", C.c_uint64), ("windows", C.c_uint64), ("ranges", C.c_uint64),
                ("index_bytes", C.c_uint64), ("compressed_bytes", C.c_uint64), ("pass_ms", C.c_double),
                ("build_ms", C.c_double), ("deflate_ms", C.c_double), ("write_ms", C.c_double)]


class AlleleInfo(C.Structure):
    _fields_ = [("selection", C.c_uint32), ("output", C.c_uint32), ("sites", C.c_uint64), ("deep_sites", C.c_uint64),
                ("entries_read", C.c_uint64), ("pairs", C.c_uint64), ("nnz_ad", C.c_uint64), ("nnz_dp", C.c_uint64),
                ("nnz_oth", C.c_uint64), ("text_bytes", C.c_uint64), ("compressed_bytes", C.c_uint64),
                ("ranges", C.c_uint64), ("count_ms", C.c_double), ("format_ms", C.c_double),
                ("deflate_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double),
                ("count_kernel_ms", C.c_double)]


class GenomeBinsInfo(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("output", C.c_uint32), ("contigs", C.c_uint64), ("selected", C.c_uint64),
                ("duplicate_names", C.c_uint64), ("bins", C.c_uint64), ("bases", C.c_uint64),
                ("name_bytes", C.c_uint64), ("ranges", C.c_uint64), ("uploaded_bytes", C.c_uint64),
                ("device_members", C.c_uint64), ("fasta_bytes", C.c_uint64), ("text_bytes", C.c_uint64),
                ("compressed_bytes", C.c_uint64), ("members", C.c_uint64), ("upload_ms", C.c_double),
                ("parse_ms", C.c_double), ("count_ms", C.c_double), ("format_ms", C.c_double),
                ("deflate_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


FASTA_ROUTES = ("host", "device")
GENOME_BINS_OUTPUTS = ("plain", "bgzf")
GENOME_BINS_COLUMNS = ("a", "c", "g", "t", "other", "masked")
ALLELE_COUNTS = ("none", "all", "cluster")
PAIR_DTYPE = np.dtype([("site", np.uint32), ("group", np.uint32), ("ad", np.uint32), ("rd", np.uint32),
                       ("oth", np.uint32)])
VCF_OUTPUTS = ("plain", "bgzf")
VCF_INDEXES = ("none", "tbi")
BGZF_CUT = 0xFF00  # text bytes per BGZF member at the most
FASTA_KINDS = ("text", "bgzf", "gzip")

RECORD_DTYPE = np.dtype([("locus", np.uint32), ("cluster", np.uint16), ("genotype", np.uint8), ("kind", np.uint8),
                         ("counts", np.uint16, (4,))])

SIGNATURES = {
    "secedo_variant_last_error": (C.c_char_p, []),
    "secedo_variant_reference_genotypes": (C.c_int, [C.c_char_p, C.c_char_p, _vp, C.c_uint32, _vp, C.c_uint32, _vp,
                                                     _vp, _f64p]),
    "secedo_variant_set_fasta_route": (C.c_int, [C.c_int]),
    "secedo_variant_get_fasta_route": (C.c_int, []),
    "secedo_variant_fasta_stats": (C.c_int, [C.POINTER(FastaInfo)]),
    "secedo_variant_reference_genotypes_device": (C.c_int, [C.c_int, C.c_char_p, C.c_char_p, _vp, _vp, C.c_uint32, _vp,
                                                            C.c_uint32, _vp, _vp, C.POINTER(Times), _vp]),
    "secedo_variant_set_vcf_output": (C.c_int, [C.c_int]),
    "secedo_variant_get_vcf_output": (C.c_int, []),
    "secedo_variant_vcf_stats": (C.c_int, [C.POINTER(VcfInfo)]),
    "secedo_variant_set_vcf_index": (C.c_int, [C.c_int]),
    "secedo_variant_get_vcf_index": (C.c_int, []),
    "secedo_variant_tabix_build": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.c_int, _vp]),
    "secedo_variant_tabix_stats": (C.c_int, [C.POINTER(TabixInfo)]),
    "secedo_variant_format_host": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint32,
                                             C.c_char_p, _vp, _vp, C.c_uint64, _vp]),
    "secedo_variant_format_device": (C.c_int, [C.c_int, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, C.c_uint32,
                                               C.c_uint32, C.c_char_p, _vp, _vp, C.c_uint64, _vp]),
    "secedo_variant_bgzf_deflate": (C.c_int, [C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp]),
    "secedo_variant_set_allele_counts": (C.c_int, [C.c_int]),
    "secedo_variant_get_allele_counts": (C.c_int, []),
    "secedo_variant_set_cell_names": (C.c_int, [C.POINTER(C.c_char_p), C.c_uint32]),
    "secedo_variant_set_cell_names_file": (C.c_int, [C.c_char_p]),
    "secedo_variant_allele_masks": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint32, C.c_int, _vp, _vp, _vp, C.c_uint32,
                                              _u32p]),
    "secedo_variant_allele_counts_device": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp,
                                                      C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, C.c_uint32, _u32p, _vp,
                                                      C.c_uint64, _u64p, _vp]),
    "secedo_variant_allele_stats": (C.c_int, [C.POINTER(AlleleInfo)]),
    "secedo_variant_genome_bins": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), _vp, C.c_uint32,
                                             C.c_char_p, C.c_int, C.c_int, C.POINTER(GenomeBinsInfo)]),
    "secedo_variant_genome_bins_fetch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "secedo_variant_genome_bins_stats": (C.c_int, [C.POINTER(GenomeBinsInfo)]),
    "secedo_variant_is_diploid": (C.c_int, [C.c_char_p]),
    "secedo_variant_read_chromosome": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32, _vp, C.c_uint64, _u64p]),
    "secedo_variant_read_map": (C.c_int, [C.c_char_p, _vp, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint32, _u32p]),
    "secedo_variant_apply_map": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, _u64p]),
    "secedo_variant_calls_device": (C.c_int, [C.c_int, _vp, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64,
                                              _vp, C.c_uint32, _vp, _vp, C.c_double, C.c_double, _vp, C.c_uint32,
                                              _u32p, _vp, _vp, _f64p, _vp]),
    "secedo_variant_genotypes_device": (C.c_int, [C.c_int, _vp, C.c_uint32, C.c_int, C.c_double, C.c_double, _vp,
                                                  _vp]),
    "secedo_variant_calling": (C.c_int, [C.c_int, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_char_p,
                                         C.c_char_p, C.c_double, C.c_double, C.c_char_p, C.POINTER(Times)]),
    "secedo_variant_calling_device": (C.c_int, [C.c_int, _vp, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint32,
                                                C.c_uint64, _vp, C.c_uint32, C.c_char_p, C.c_char_p, C.c_double,
                                                C.c_double, C.c_char_p, C.POINTER(Times), _vp]),
}

_vl = None


def lib():
    global _vl
    if _vl is None:
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
        _vl = l
    return _vl


def check(rc):
    if rc == _lib.OK:
        return
    raise _lib.SecedoError(rc, lib().secedo_variant_last_error().decode(errors="replace"))


def _b(s):
    return None if s is None else os.fsencode(str(s))


def _flat(pos_data):
    p = pos_data if isinstance(pos_data, FlatPileup) else flatten(pos_data)
    idb = np.ascontiguousarray(p.id_base)
    if p.n_entries == 0 or int(idb.max()) <= 0xFFFF:
        return p, np.ascontiguousarray(idb, dtype=np.uint16), None
    return p, None, np.ascontiguousarray(idb, dtype=np.uint32)


def set_fasta_route(route):
    """The process-wide route of the FASTA parse and gather: "host" or "device" (see the module docstring)."""
    if route not in FASTA_ROUTES:
        raise ValueError("fasta route must be 'host' or 'device', not %r" % (route,))
    check(lib().secedo_variant_set_fasta_route(FASTA_ROUTES.index(route)))


def get_fasta_route() -> str:
    rc = lib().secedo_variant_get_fasta_route()
    if rc < 0:
        check(rc)
    return FASTA_ROUTES[rc]


@contextlib.contextmanager
def _route(route):
    """A scoped override of the FASTA route; None leaves the setting alone. Afterwards the route that held before is
    set explicitly, so the environment is no longer consulted in this process."""
    if route is None:
        yield
        return
    before = get_fasta_route()
    set_fasta_route(route)
    try:
        yield
    finally:
        set_fasta_route(before)


def set_vcf_output(output):
    """The process-wide kind of VCF output: "plain" (cluster_<i>.vcf, common.vcf) or "bgzf" (the same text as
    .vcf.gz, formatted and deflated on the GPU; see the module docstring)."""
    if output not in VCF_OUTPUTS:
        raise ValueError("vcf output must be 'plain' or 'bgzf', not %r" % (output,))
    check(lib().secedo_variant_set_vcf_output(VCF_OUTPUTS.index(output)))


def get_vcf_output() -> str:
    rc = lib().secedo_variant_get_vcf_output()
    if rc < 0:
        check(rc)
    return VCF_OUTPUTS[rc]


@contextlib.contextmanager
def _output(output):
    """A scoped override of the VCF output, as _route is of the FASTA route."""
    if output is None:
        yield
        return
    before = get_vcf_output()
    set_vcf_output(output)
    try:
        yield
    finally:
        set_vcf_output(before)


def set_vcf_index(index):
    """The process-wide index of the bgzf VCF output: "none", or "tbi" (<file>.vcf.gz.tbi beside each file, built on
    the GPU; see the module docstring). "tbi" with plain output makes the file-writing calls fail."""
    if index not in VCF_INDEXES:
        raise ValueError("vcf index must be 'none' or 'tbi', not %r" % (index,))
    check(lib().secedo_variant_set_vcf_index(VCF_INDEXES.index(index)))


def get_vcf_index() -> str:
    rc = lib().secedo_variant_get_vcf_index()
    if rc < 0:
        check(rc)
    return VCF_INDEXES[rc]


@contextlib.contextmanager
def _index(index):
    """A scoped override of the VCF index, as _route is of the FASTA route."""
    if index is None:
        yield
        return
    before = get_vcf_index()
    set_vcf_index(index)
    try:
        yield
    finally:
        set_vcf_index(before)


def set_allele_counts(selection):
    """The process-wide selection of the per-cell allele counts: "none" (the default: nothing is added), "all" (every
    locus with a call) or "cluster" (the loci where clusters differ); see the module docstring."""
    if selection not in ALLELE_COUNTS:
        raise ValueError("allele counts must be 'none', 'all' or 'cluster', not %r" % (selection,))
    check(lib().secedo_variant_set_allele_counts(ALLELE_COUNTS.index(selection)))


def get_allele_counts() -> str:
    rc = lib().secedo_variant_get_allele_counts()
    if rc < 0:
        check(rc)
    return ALLELE_COUNTS[rc]


def set_cell_names(names):
    """The lines of cellSNP.samples.tsv: a list of names, the path of a file with one name per line, or None for
    cell_<i>. Their count must be the length of `clusters` of the file-writing call."""
    if names is None:
        check(lib().secedo_variant_set_cell_names(None, 0))
    elif isinstance(names, (str, bytes, os.PathLike)):
        check(lib().secedo_variant_set_cell_names_file(_b(names)))
    else:
        enc = [str(x).encode() for x in names]
        check(lib().secedo_variant_set_cell_names((C.c_char_p * max(len(enc), 1))(*enc), len(enc)))


@contextlib.contextmanager
def _alleles(selection, cell_names):
    """A scoped override of the allele-count selection, as _route is of the FASTA route; cell names given for the call
    are dropped after it."""
    before = None if selection is None else get_allele_counts()
    if selection is not None:
        set_allele_counts(selection)
    try:
        if cell_names is not None:
            set_cell_names(cell_names)
        yield
    finally:
        if cell_names is not None:
            set_cell_names(None)
        if before is not None:
            set_allele_counts(before)


def allele_stats() -> dict:
    """What the allele counting of the last file-writing call of this thread (or allele_counts) did
    (secedo_variant_allele_info), selection and output as words. All zero ("none") when it was off."""
    info = AlleleInfo()
    check(lib().secedo_variant_allele_stats(C.byref(info)))
    out = {name: getattr(info, name) for name, _ in AlleleInfo._fields_}
    out["selection"], out["output"] = ALLELE_COUNTS[info.selection], VCF_OUTPUTS[info.output]
    return out


def _selection(sites):
    if sites not in ALLELE_COUNTS[1:]:
        raise ValueError("sites must be 'all' or 'cluster', not %r" % (sites,))
    return ALLELE_COUNTS.index(sites)


def allele_masks(records, locus_ref, n_loci, sites="all") -> dict:
    """The sites of `records` (RECORD_DTYPE, write order) and their base masks, on the host (no GPU): {"site_locus"
    u32[S], "ref_mask" u8[S], "alt_mask" u8[S]}; bit b of a mask = base b, A,C,G,T = 0..3."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    ref = np.ascontiguousarray(locus_ref, dtype=np.uint8)
    if len(ref) < n_loci:
        raise ValueError("locus_ref is shorter than n_loci")
    cap = max(len(rec), 1)
    loc, rm, am = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    n = C.c_uint32(0)
    check(lib().secedo_variant_allele_masks(_lib.ptr(rec) if len(rec) else None, len(rec),
                                            _lib.ptr(ref) if len(ref) else None, n_loci, _selection(sites),
                                            _lib.ptr(loc), _lib.ptr(rm), _lib.ptr(am), cap, C.byref(n)))
    return {"site_locus": loc[:n.value], "ref_mask": rm[:n.value], "alt_mask": am[:n.value]}


def allele_counts(pos_data, records, locus_ref, n_cells, sites="all", device=0) -> dict:
    """The per-cell allele counts alone, on the GPU: allele_masks' arrays, "totals" u32[S, 3] (the sums of ad, rd, oth
    per site) and "pairs" (PAIR_DTYPE, site then group ascending: the (site, cell) pairs with at least one read)."""
    import torch
    p, b16, b32 = _flat(pos_data)
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    dev = "cuda:%d" % device
    d_off = _dev(p.locus_entry_off, np.int64, dev)
    d_idb = _dev(b16, np.int16, dev) if b16 is not None else _dev(b32, np.int32, dev)
    d_ref = _dev(np.ascontiguousarray(locus_ref, dtype=np.uint8), np.uint8, dev)
    idb = C.c_void_p(d_idb.data_ptr())
    cap = max(len(rec), 1)
    loc, rm, am = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    tot = np.zeros((cap, 3), np.uint32)
    pairs = np.zeros(1, dtype=PAIR_DTYPE)
    n_sites, n_pairs = C.c_uint32(0), C.c_uint64(0)
    for capacity in (0, None):  # the first call asks for the number of pairs
        if capacity is None:
            capacity = n_pairs.value
            pairs = np.zeros(max(capacity, 1), dtype=PAIR_DTYPE)
        rc = lib().secedo_variant_allele_counts_device(
            device, C.c_void_p(d_off.data_ptr()), idb if b16 is not None else None, None if b16 is not None else idb,
            p.n_loci, _lib.ptr(rec) if len(rec) else None, len(rec), C.c_void_p(d_ref.data_ptr()), n_cells,
            _selection(sites), _lib.ptr(loc), _lib.ptr(rm), _lib.ptr(am), _lib.ptr(tot), cap, C.byref(n_sites),
            _lib.ptr(pairs), capacity, C.byref(n_pairs), _stream(device))
        if rc != _lib.E_LIMIT:
            break
    check(rc)
    torch.cuda.synchronize(device)
    s = n_sites.value
    return {"site_locus": loc[:s], "ref_mask": rm[:s], "alt_mask": am[:s], "totals": tot[:s],
            "pairs": pairs[:n_pairs.value]}


def tabix_stats() -> dict:
    """What the last index-writing call of this thread did (secedo_variant_tabix_info): a file-writing call under
    "tbi", or tabix_build. All zero after a call that wrote no index."""
    info = TabixInfo()
    check(lib().secedo_variant_tabix_stats(C.byref(info)))
    return {name: getattr(info, name) for name, _ in TabixInfo._fields_}


def tabix_build(files, overwrite=False, device=0) -> dict:
    """<file>.tbi for every bgzip-compressed VCF of `files` (a path or a list of paths), built on the GPU: the
    compressed bytes are uploaded, inflated there (ISIZE and CRC32 checked) and indexed, many small files to a batch.
    An index that exists is an error unless overwrite; when a file fails, the files in front of it keep their indexes.
    -> tabix_stats()."""
    if isinstance(files, (str, bytes, os.PathLike)):
        files = [files]
    paths = [_b(f) for f in files]
    arr = (C.c_char_p * max(len(paths), 1))(*paths)
    check(lib().secedo_variant_tabix_build(device, arr, len(paths), int(bool(overwrite)), _stream(device)))
    return tabix_stats()


def vcf_stats() -> dict:
    """What the last file-writing call of this thread (or bgzf_deflate) did (secedo_variant_vcf_info), the output as a
    word."""
    info = VcfInfo()
    check(lib().secedo_variant_vcf_stats(C.byref(info)))
    out = {name: getattr(info, name) for name, _ in VcfInfo._fields_ if name != "reserved"}
    out["output"] = VCF_OUTPUTS[info.output]
    return out


def bgzf_deflate_many(inputs, device=0):
    """Every input (bytes-like) compressed on the GPU in one launch -> a list of complete BGZF files (bytes): members
    of at most 0xFF00 input bytes and the EOF member; an empty input gives the EOF member alone."""
    datas = [bytes(d) for d in inputs]
    off = np.zeros(len(datas) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    data = np.frombuffer(b"".join(datas), dtype=np.uint8)
    cap = int(sum(len(d) + 31 * (-(-len(d) // BGZF_CUT)) + 28 for d in datas))
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    out_off = np.zeros(len(datas) + 1, dtype=np.uint64)
    check(lib().secedo_variant_bgzf_deflate(device, _lib.ptr(data) if len(data) else None, _lib.ptr(off), len(datas),
                                            _lib.ptr(out), cap, _lib.ptr(out_off), _stream(device)))
    return [out[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(len(datas))]


def bgzf_deflate(data, device=0) -> bytes:
    """The BGZF encoder alone, on the GPU: `data` (bytes-like) -> a complete BGZF file, as `bgzip` would cut it. The
    mirror of secedo_amd.bgzf_inflate(path)."""
    return bgzf_deflate_many([data], device)[0]


def _format(fn, records, chr_locus_off, locus_pos, locus_ref, num_clusters, preambles):
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    off = np.ascontiguousarray(chr_locus_off, dtype=np.uint32)
    pos = np.ascontiguousarray(locus_pos, dtype=np.uint32)
    ref = np.ascontiguousarray(locus_ref, dtype=np.uint8)
    pre = [bytes(p) for p in (preambles or [b""] * num_clusters)]
    if len(pre) != num_clusters:
        raise ValueError("one preamble per cluster")
    pre_off = np.zeros(num_clusters + 1, dtype=np.uint64)
    pre_off[1:] = np.cumsum([len(p) for p in pre], dtype=np.uint64)
    file_off = np.zeros(num_clusters + 2, dtype=np.uint64)
    cap = int(pre_off[-1]) + 2 * 82 * len(rec)  # a record is at most two lines of 82 bytes
    text = np.zeros(max(cap, 1), dtype=np.uint8)
    check(fn(_lib.ptr(rec) if len(rec) else None, len(rec), _lib.ptr(off), len(off) - 1,
             _lib.ptr(pos) if len(pos) else None, _lib.ptr(ref) if len(ref) else None, len(pos), num_clusters,
             b"".join(pre), _lib.ptr(pre_off), _lib.ptr(text), cap, _lib.ptr(file_off)))
    return [text[int(file_off[i]):int(file_off[i + 1])].tobytes() for i in range(num_clusters + 1)]


def format_host(records, chr_locus_off, locus_pos, locus_ref, num_clusters, preambles=None):
    """The VCF text of `records` (RECORD_DTYPE, write order) as the plain route builds it -> [cluster_0, ...,
    cluster_<num_clusters - 1>, common] as bytes; preambles: the cluster files' first bytes. No GPU."""
    return _format(lib().secedo_variant_format_host, records, chr_locus_off, locus_pos, locus_ref, num_clusters,
                   preambles)


def format_device(records, chr_locus_off, locus_pos, locus_ref, num_clusters, preambles=None, device=0):
    """The same text by the formatter kernels of the bgzf route."""
    fn = lib().secedo_variant_format_device
    return _format(lambda *a: fn(device, *a), records, chr_locus_off, locus_pos, locus_ref, num_clusters, preambles)


def fasta_stats() -> dict:
    """What the last FASTA-reading call of this thread did (secedo_variant_fasta_info), kind and route as words."""
    info = FastaInfo()
    check(lib().secedo_variant_fasta_stats(C.byref(info)))
    out = {name: getattr(info, name) for name, _ in FastaInfo._fields_ if name != "reserved"}
    out["kind"], out["route"] = FASTA_KINDS[info.kind], FASTA_ROUTES[info.route]
    return out


def reference_genotypes(reference_genome, chr_locus_off, locus_pos, map_file="", device=None):
    """The reference genotype of every locus (maternal << 3 | paternal, N = 5) and each chromosome's end (the
    first locus with position - 1 >= its contig's length) -> (locus_ref u8[L], chr_locus_end u32[C]), host arrays.
    device=None: the host function, no GPU. device=<id>: secedo_variant_reference_genotypes_device on copies of the
    offsets and positions in that GPU's memory, by the route the file and the setting ask for."""
    off = np.ascontiguousarray(chr_locus_off, dtype=np.uint32)
    pos = np.ascontiguousarray(locus_pos, dtype=np.uint32)
    ref = np.zeros(max(len(pos), 1), dtype=np.uint8)
    end = np.zeros(max(len(off) - 1, 1), dtype=np.uint32)
    if device is not None:
        import torch
        dev = "cuda:%d" % device
        d_off, d_pos = _dev(off, np.int32, dev), _dev(pos, np.int32, dev)
        d_ref = torch.zeros(max(len(pos), 1), dtype=torch.uint8, device=dev)
        check(lib().secedo_variant_reference_genotypes_device(
            device, _b(reference_genome), _b(map_file), C.c_void_p(d_off.data_ptr()), _lib.ptr(off), len(off) - 1,
            C.c_void_p(d_pos.data_ptr()), len(pos), C.c_void_p(d_ref.data_ptr()), _lib.ptr(end), None,
            _stream(device)))
        return d_ref.cpu().numpy()[:len(pos)].copy(), end[:len(off) - 1]
    check(lib().secedo_variant_reference_genotypes(_b(reference_genome), _b(map_file), _lib.ptr(off), len(off) - 1,
                                                   _lib.ptr(pos), len(pos), _lib.ptr(ref), _lib.ptr(end), None))
    return ref[:len(pos)], end[:len(off) - 1]


def is_diploid(fasta) -> bool:
    rc = lib().secedo_variant_is_diploid(_b(fasta))
    if rc < 0:
        check(rc)
    return bool(rc)


def read_chromosome(fasta, index, map_file=""):
    """What get_next_chromosome leaves in chr_data after its (index + 1)-th call -> u8 genotype codes."""
    n = C.c_uint64(0)
    rc = lib().secedo_variant_read_chromosome(_b(fasta), _b(map_file), index, None, 0, C.byref(n))
    if rc not in (_lib.OK, _lib.E_LIMIT):
        check(rc)
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    check(lib().secedo_variant_read_chromosome(_b(fasta), _b(map_file), index, _lib.ptr(out), len(out), C.byref(n)))
    return out[:n.value]


def read_map(map_file):
    """read_map -> {contig name: [(start_pos, len, tr, chromosome_id), ...]} in file order."""
    n = C.c_uint32(0)
    rc = lib().secedo_variant_read_map(_b(map_file), None, 0, None, None, None, None, 0, C.byref(n))
    if rc not in (_lib.OK, _lib.E_LIMIT):
        check(rc)
    k, width = max(n.value, 1), 256
    names = C.create_string_buffer(k * width)
    start, length = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    tr, chrom = C.create_string_buffer(k), np.zeros(k, np.uint8)
    check(lib().secedo_variant_read_map(_b(map_file), names, width, _lib.ptr(start), _lib.ptr(length), tr,
                                        _lib.ptr(chrom), k, C.byref(n)))
    out = {}
    for i in range(n.value):
        name = names.raw[i * width:(i + 1) * width].split(b"\0", 1)[0].decode()
        out.setdefault(name, []).append((int(start[i]), int(length[i]), tr.raw[i:i + 1].decode(), int(chrom[i])))
    return out


def apply_map(map_entries, chr_data):
    """apply_map on one contig: map_entries = [(start_pos, len, tr), ...] -> u8 array."""
    m = list(map_entries)
    start = np.asarray([e[0] for e in m] or [0], dtype=np.uint32)
    length = np.asarray([e[1] for e in m] or [0], dtype=np.uint32)
    tr = C.create_string_buffer("".join(e[2] for e in m).encode() or b"\0")
    data = np.ascontiguousarray(chr_data, dtype=np.uint8)
    n = C.c_uint64(0)
    cap = int(len(data) + sum(e[1] for e in m if e[2] == "D")) + 1
    out = np.zeros(cap, dtype=np.uint8)
    check(lib().secedo_variant_apply_map(_lib.ptr(start), _lib.ptr(length), tr, len(m), _lib.ptr(data), len(data),
                                         _lib.ptr(out), cap, C.byref(n)))
    return out[:n.value]


def genotypes_device(counts, likely_homozygous_total, hetero_prior, theta, device=0):
    """likely_homozygous(counts[i], theta) and most_likely_genotype(counts[i], ..., likely_homozygous_total,
    hetero_prior, theta) as the kernel evaluates them; counts: (n, 4) -> (homozygous u8[n], genotype u8[n])."""
    c = np.ascontiguousarray(counts, dtype=np.uint16).reshape(-1, 4)
    n = c.shape[0]
    h, g = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    check(lib().secedo_variant_genotypes_device(device, _lib.ptr(c), n, int(bool(likely_homozygous_total)),
                                                hetero_prior, theta, _lib.ptr(h), _lib.ptr(g)))
    return h[:n], g[:n]


def _dev(a, t, dev):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    return torch.from_numpy(a.view(t)).to(dev)


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def variant_calls(pos_data, clusters, reference_genome, map_file="", hetero_prior=1e-3, theta=0.01, capacity=None,
                  device=0, with_kernel_ms=False, fasta_route=None):
    """The device calls alone -> (records as a RECORD_DTYPE array in write order, mismatch u32[n], loci u32[n]).
    `capacity` (default: enough) bounds the records; SecedoError(E_LIMIT) when more are needed, its
    `required` attribute the count. fasta_route: None reads the reference genome with the host function, "host" or
    "device" through secedo_variant_reference_genotypes_device under that route."""
    import torch
    p, b16, b32 = _flat(pos_data)
    cl = np.ascontiguousarray(clusters, dtype=np.uint16)
    with _route(fasta_route):
        ref, end = reference_genotypes(reference_genome, p.chr_locus_off, p.locus_pos, map_file,
                                       None if fasta_route is None else device)
    dev = "cuda:%d" % device
    d_chr = _dev(p.chr_locus_off, np.int32, dev)
    d_pos = _dev(p.locus_pos, np.int32, dev)
    d_off = _dev(p.locus_entry_off, np.int64, dev)
    d_idb = _dev(b16, np.int16, dev) if b16 is not None else _dev(b32, np.int32, dev)
    d_cl = _dev(cl, np.int16, dev)
    d_ref = _dev(ref, np.uint8, dev)
    n = len(cl)
    d_mm = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    d_loci = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    cap = int(p.n_entries) * 2 + p.n_loci + 16 if capacity is None else int(capacity)
    recs = (Record * max(cap, 1))()
    n_rec, kms = C.c_uint32(0), C.c_double(0)
    idb = C.c_void_p(d_idb.data_ptr())
    rc = lib().secedo_variant_calls_device(
        device, C.c_void_p(d_chr.data_ptr()), p.n_chr, C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_off.data_ptr()),
        idb if b16 is not None else None, None if b16 is not None else idb, p.n_loci, p.n_entries,
        C.c_void_p(d_cl.data_ptr()), n, C.c_void_p(d_ref.data_ptr()), _lib.ptr(end), hetero_prior, theta, recs, cap,
        C.byref(n_rec), C.c_void_p(d_mm.data_ptr()), C.c_void_p(d_loci.data_ptr()), C.byref(kms), _stream(device))
    if rc == _lib.E_LIMIT:
        err = _lib.SecedoError(rc, lib().secedo_variant_last_error().decode(errors="replace"))
        err.required = int(n_rec.value)
        raise err
    check(rc)
    out = np.frombuffer(recs, dtype=RECORD_DTYPE, count=n_rec.value).copy()
    mm = d_mm.cpu().numpy().view(np.uint32)[:n].copy()
    lo = d_loci.cpu().numpy().view(np.uint32)[:n].copy()
    if with_kernel_ms:
        return out, mm, lo, kms.value
    return out, mm, lo


def _times(t):
    return dict(fasta_ms=t.fasta_ms, gather_ms=t.gather_ms, device_ms=t.device_ms, write_ms=t.write_ms,
                kernel_ms=t.kernel_ms)


def variant_calling(pos_data, clusters, reference_genome, map_file="", hetero_prior=1e-3, theta=0.01,
                    out_dir="variant_calling", device=0, fasta_route=None, vcf_output=None, vcf_index=None,
                    allele_counts=None, cell_names=None):
    """variant_calling(pos_data, clusters, reference_genome, map_file, hetero_prior, theta, out_dir): writes
    cluster_<i>.vcf, common.vcf, variant and scores under out_dir as the reference does. fasta_route ("host",
    "device"; None: the setting) overrides the FASTA route for this call, vcf_output ("plain", "bgzf"; None: the
    setting) the kind of VCF files, vcf_index ("none", "tbi"; None: the setting) whether the bgzf files get a tabix
    index, allele_counts ("none", "all", "cluster"; None: the setting) whether out_dir/allele_counts/ is written, with
    cell_names (a list or a file; None: the names set, else cell_<i>) in its samples file. -> step times (ms)."""
    p, b16, b32 = _flat(pos_data)
    cl = np.ascontiguousarray(clusters, dtype=np.uint16)
    t = Times()
    with _route(fasta_route), _output(vcf_output), _index(vcf_index), _alleles(allele_counts, cell_names):
        check(lib().secedo_variant_calling(device, _lib.ptr(p.chr_locus_off), p.n_chr, _lib.ptr(p.locus_pos),
                                           _lib.ptr(p.locus_entry_off), _lib.ptr(b16), _lib.ptr(b32), _lib.ptr(cl),
                                           len(cl), _b(reference_genome), _b(map_file), hetero_prior, theta,
                                           _b(out_dir), C.byref(t)))
    return _times(t)


def variant_calling_resident(plan, res, clusters, reference_genome, map_file="", hetero_prior=1e-3, theta=0.01,
                             out_dir="variant_calling", fasta_route=None, vcf_output=None, vcf_index=None,
                             allele_counts=None, cell_names=None):
    """variant_calling on the pileup `res` resident in HBM (SimilarityMatrixPlan.upload, as divide_cluster_resident
    takes it), in the plan's current stream. fasta_route, vcf_output, vcf_index, allele_counts and cell_names as in
    variant_calling. -> step times (ms)."""
    cl = np.ascontiguousarray(clusters, dtype=np.uint16)
    idb = C.c_void_p(res["idb"].data_ptr())
    t = Times()
    with _route(fasta_route), _output(vcf_output), _index(vcf_index), _alleles(allele_counts, cell_names):
        check(lib().secedo_variant_calling_device(
            plan.device, C.c_void_p(res["chr"].data_ptr()), res["n_chr"], C.c_void_p(res["pos"].data_ptr()),
            C.c_void_p(res["off"].data_ptr()), idb if res["idb_is16"] else None, None if res["idb_is16"] else idb,
            res["n_loci"], res["n_entries"], _lib.ptr(cl), len(cl), _b(reference_genome), _b(map_file), hetero_prior,
            theta, _b(out_dir), C.byref(t), plan._stream()))
    return _times(t)


def _genome_bins_dict(info: GenomeBinsInfo) -> dict:
    out = {k: (float if ty is C.c_double else int)(getattr(info, k)) for k, ty in GenomeBinsInfo._fields_}
    out["kind"] = FASTA_KINDS[out["kind"]]
    out["output"] = GENOME_BINS_OUTPUTS[out["output"]]
    return out


def genome_bins_stats() -> dict:
    """What the last ``genome_bins`` call on this thread did, a failed one up to its failure: kind, output, contigs,
    selected, duplicate_names, bins, bases, name_bytes, ranges, uploaded_bytes, device_members, fasta_bytes,
    text_bytes, compressed_bytes, members and the stage times upload_ms, parse_ms, count_ms, format_ms, deflate_ms,
    download_ms, write_ms."""
    info = GenomeBinsInfo()
    check(lib().secedo_variant_genome_bins_stats(C.byref(info)))
    return _genome_bins_dict(info)


def _name_bytes(x) -> bytes:
    return x if isinstance(x, bytes) else str(x).encode("utf-8", "surrogateescape")


def genome_bins(fasta, bin_size: int, contigs=None, lengths=None, out_path=None, output: str = "plain",
                overwrite: bool = False) -> dict:
    """The composition of a reference genome per bin, counted on the GPU: what a copy-number tool regresses depth on
    (GC) and filters bins by (N, soft-masked repeats); the companion of ``bin_depth``
    (secedo_variant_genome_bins; the rules and the bytes of the file are in include/secedo_variant.h). ``fasta`` is
    plain, gzip or bgzip-compressed. Every header line starts a contig, named by the header's bytes after its first up
    to the first space, tab or '\\r'; of two contigs with one name the first counts. ``contigs`` None: all contigs in
    file order; else the listed names in the listed order, matched exactly (no ``chr`` aliasing), a missing one raises.
    ``lengths`` (with ``contigs``): the length each listed contig must have, else the call raises. Contig ``k`` has
    ``ceil(L_k / bin_size)`` bins, numbered in selection order: the bins of ``bin_depth`` for the same names and
    lengths. ``out_path``: also write that file (``output="bgzf"``: ``<out_path>.gz``), a header line and one line
    per bin ``name start end a c g t other masked``, tab-separated; an existing file raises unless ``overwrite``.
    -> dict: names (list of str), contig_lengths uint64 [selected], bin_contig (the position in ``names``), bin_start,
    bin_end uint32 [bins], counts uint32 [bins, 6] (a, c, g, t, other, masked: masked counts bytes 'a'..'z' in
    addition to their class, so a + c + g + t + other == bin_end - bin_start), stats (``genome_bins_stats()``)."""
    if output not in GENOME_BINS_OUTPUTS:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "output is 'plain' or 'bgzf', got %r" % (output,))
    if not isinstance(bin_size, (int, np.integer)) or bin_size < 0 or bin_size > 0xFFFFFFFF:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "bin_size is an integer in [1, 2^32 - 1], got %r" % (bin_size,))
    if lengths is not None and contigs is None:
        raise _lib.SecedoError(_lib.E_INVALID_ARG, "lengths needs contigs")
    names_arr, len_arr, n = None, None, 0
    if contigs is not None:
        if isinstance(contigs, (str, bytes)):
            contigs = [contigs]
        names = [_name_bytes(x) for x in contigs]
        n = len(names)
        names_arr = (C.c_char_p * max(n, 1))(*names)
        if lengths is not None:
            len_arr = np.ascontiguousarray(lengths, dtype=np.uint64)
            if len_arr.shape != (n,):
                raise _lib.SecedoError(_lib.E_INVALID_ARG, "%d lengths for %d contigs" % (len_arr.size, n))
    info = GenomeBinsInfo()
    check(lib().secedo_variant_genome_bins(_b(fasta), int(bin_size), names_arr, _lib.ptr(len_arr), n, _b(out_path),
                                           GENOME_BINS_OUTPUTS.index(output), int(bool(overwrite)), C.byref(info)))
    n_sel, n_bins = int(info.selected), int(info.bins)
    raw = np.zeros(max(int(info.name_bytes), 1), np.uint8)
    off = np.zeros(n_sel + 1, np.uint64)
    out = dict(contig_lengths=np.zeros(n_sel, np.uint64), bin_contig=np.zeros(n_bins, np.uint32),
               bin_start=np.zeros(n_bins, np.uint32), bin_end=np.zeros(n_bins, np.uint32),
               counts=np.zeros((n_bins, len(GENOME_BINS_COLUMNS)), np.uint32))
    check(lib().secedo_variant_genome_bins_fetch(_lib.ptr(raw), _lib.ptr(off), *[_lib.ptr(out[k]) for k in (
        "contig_lengths", "bin_contig", "bin_start", "bin_end", "counts")]))
    data = raw.tobytes()
    out["names"] = [data[int(off[i]):int(off[i + 1])].decode("utf-8", "surrogateescape") for i in range(n_sel)]
    out["stats"] = _genome_bins_dict(info)
    return out
