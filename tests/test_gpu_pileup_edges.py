"""The BAM pileup kernels on the edge cases of tests/pileup_edge_cases.py. For every family pileup_bams() equals the
Python restatement of the reference (tests/pileup_bam_ref.py) on .bin, .map, .txt up to 16 entries and the returned
arrays, and its .bin and .map have the SHA-256 the compiled reference's had (tests/golden/pileup_edges.npz), which
closes kernel = restatement = reference without the reference being here. Then the device inflate route, SAM text,
the resident path, the reference's aborts as errors that disturb nothing, and a repeated run.

Every file is accepted by bam_pileup.bam_scan (host only) before a kernel sees it; the error files are valid BAMs
whose records the reference's asserts refuse."""
import dataclasses
import hashlib
import os
import struct

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_writer as bw
from tests import multiplex_bam as mb
from tests import pileup_bam_ref as ref
from tests import pileup_edge_cases as pe
from tests import sam_writer as sw
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu

ARRAYS = ("chr_locus_off", "locus_pos", "locus_entry_off", "read_ids", "id_base")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "pileup_edges.npz"))
    return {str(n): {k: z[k][i].item() for k in z.files if k != "name"} for i, n in enumerate(z["name"])}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Every family's files, written once, each accepted by the host-only scan."""
    d = tmp_path_factory.mktemp("edges_gpu")
    with pe.cached_records():
        out = {f: pe.build(f, d) for f in pe.FAMILIES}
        for path in sorted({p for cs in out.values() for c in cs for p in c.files}):
            assert bam_pileup.bam_scan(path)["sorted"], path
        yield out


def files_of(out):
    return tuple(open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt"))


def pile(case, out, files=None, **kw):
    max_cov, min_bq, min_mq, min_as, diff = case.params
    got = bam_pileup.pileup_bams(list(files or case.files), out, True, 0, max_cov, min_bq, min_mq, min_as, 4, diff,
                                 **kw)
    return got, files_of(out)


def check(case, out, golden, **kw):
    """pileup_bams on the case against the restatement and the reference's recorded digests -> (pileup, files)"""
    got, (bin_bytes, map_bytes, txt) = pile(case, out, **kw)
    want = pe.run_restatement(case)
    assert bin_bytes == want.bin_bytes(), case.name
    assert map_bytes == want.map_text().encode(), case.name
    assert pe.txt_upto16(txt.decode()) == pe.txt_upto16(want.txt_text()), case.name
    assert got.n_loci == len(want.loci), case.name
    assert got.locus_pos.tolist() == [l[0] for l in want.loci], case.name
    assert got.locus_entry_off.tolist() == np.cumsum([0] + [len(l[1]) for l in want.loci]).tolist(), case.name
    assert got.read_ids.tolist() == [r for l in want.loci for r in l[1]], case.name
    assert got.id_base.tolist() == [b for l in want.loci for b in l[2]], case.name
    rec = golden[case.name]
    assert rec["status"] == 0, case.name
    assert hashlib.sha256(bin_bytes).hexdigest() == rec["bin_sha"], case.name
    assert hashlib.sha256(map_bytes).hexdigest() == rec["map_sha"], case.name
    assert (got.n_loci, got.n_entries) == (rec["n_loci"], rec["n_entries"]), case.name
    if pe.family_of(case.name) in pe.SMALL_FAMILIES:
        assert pe.txt_upto16(txt.decode()) == rec["txt"], case.name
    return got, (bin_bytes, map_bytes, txt)


def clean(cs):
    return [c for c in cs if c.kind == pe.CLEAN]


@pytest.mark.parametrize("family", [f for f in pe.FAMILIES if f != "wrap"])
def test_family_equals_restatement_and_reference(family, cases, golden, tmp_path):
    for k, c in enumerate(clean(cases[family])):
        check(c, str(tmp_path / ("o%d" % k)), golden)


@pytest.mark.parametrize("k", pe.WRAP_K)
def test_wrap_equals_restatement_and_reference(k, cases, golden, tmp_path):
    """65,536 + k arrivals at one position: the u16 counter wraps, the last k arrivals are the entries."""
    mine = [c for c in cases["wrap"] if "/k%d@" % k in c.name]
    assert len(mine) == len(pe.WRAP_PARAMS)
    for n, c in enumerate(mine):
        got, _ = check(c, str(tmp_path / ("w%d" % n)), golden)
        if k == 5 and c.params == (100, 0, 0, 0, 3):
            assert got.read_ids.tolist() == [65536, 65537, 65538, 65539, 65540]


def test_wrap_twice_gives_the_same_bytes(cases, tmp_path):
    c = next(c for c in cases["wrap"] if c.name == pe.case_name("wrap", "k5", (100, 0, 0, 0, 3)))
    (a, fa), (b, fb) = pile(c, str(tmp_path / "a")), pile(c, str(tmp_path / "b"))
    assert fa == fb and a.n_loci == b.n_loci == 1
    for k in ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("family", ["cigars", "wrap", "window", "tags"])
def test_device_route_gives_the_same(family, cases, golden, tmp_path):
    mine = clean(cases[family])
    if family == "wrap":
        mine = [c for c in mine if "/k5@" in c.name]
    for k, c in enumerate(mine):
        host, fh = pile(c, str(tmp_path / ("h%d" % k)), inflate="host")
        dev, fd = check(c, str(tmp_path / ("d%d" % k)), golden, inflate="device")
        stats = bam_pileup.bam_route_stats()
        assert fd == fh, c.name
        for a in ARRAYS:
            assert np.array_equal(getattr(dev, a), getattr(host, a)), (c.name, a)
        assert stats["device_records"] > 0, c.name


def sam_expressible(records):
    """The records SAM text holds exactly, their aux blocks as tags: stored qualities up to 93 or none at all, no cut
    aux field, and every integer of the type a SAM reader stores for its value."""
    out = []
    for r in records:
        if r.qual is not None and any(q > 93 for q in r.qual):
            continue
        if r.aux is not None:
            try:
                tags = mb.parse_aux(r.aux)
            except (KeyError, ValueError, IndexError, struct.error):
                continue  # a storage type or a layout that is no aux field
            if b"".join(bw._tag(*t) for t in tags) != r.aux or not all(t[0].isalnum() for t in tags):
                continue
            r = dataclasses.replace(r, tags=tags, aux=None)
        if sw.canonical([r])[0].tags == r.tags:
            out.append(r)
    return out


def sam_case(family, cases):
    """-> (records, params list) of the family's one file"""
    if family == "cigars":
        walked, _ = pe.classify_cigars()
        return [pe.read("c%04d" % i, 100 + pe.SLOT * i, cg, i) for i, cg in walked], [pe.OPEN]
    if family == "quality":
        return pe.quality_records(), [c.params for c in cases["quality"]]
    return pe.tag_records(), [c.params for c in cases["tags"]]


@pytest.mark.parametrize("family,at_least", [("cigars", 2286), ("quality", 7), ("tags", 9)])
def test_sam_text_gives_the_same(family, at_least, cases, tmp_path):
    records, params = sam_case(family, cases)
    kept = sam_expressible(records)
    assert len(kept) >= at_least
    bam, sam = sw.write_both(tmp_path, family, [("1", 3_000_000)], sorted(kept, key=bw.sort_key))
    assert bam_pileup.bam_scan(bam)["n_records"] == len(kept)
    for k, p in enumerate(params):
        c = pe.Case("%s/sam@%d" % (family, k), (bam, bam), p, pe.CLEAN)
        pb, fb = pile(c, str(tmp_path / ("b%d" % k)))
        ps, fs = pile(c, str(tmp_path / ("s%d" % k)), files=(sam, sam))
        want = pe.run_restatement(c)
        assert fb[0] == want.bin_bytes() and fb[1] == want.map_text().encode(), c.name
        assert fs == fb, c.name
        assert pb.n_loci > 0
        for a in ARRAYS:
            assert np.array_equal(getattr(ps, a), getattr(pb, a)), (c.name, a)


def test_window_resident_equals_file_route(cases, golden, tmp_path):
    """Loci on both sides of position 2^24, the start of the second device window, straight into HBM."""
    for k, c in enumerate(cases["window"]):
        got, _ = check(c, str(tmp_path / ("f%d" % k)), golden)
        assert int(got.locus_pos.min()) < pe.WINDOW < int(got.locus_pos.max())
        max_cov, min_bq, min_mq, min_as, diff = c.params
        with secedo_amd.SimilarityMatrixPlan(0) as plan:
            res, cells, _max_len = bam_pileup.pileup_bams_resident(plan, list(c.files), [0], max_cov, min_bq, min_mq,
                                                                   min_as, 4, diff)
            dev = {a: res[a].cpu().numpy() for a in ("chr", "pos", "off", "rid", "idb")}
        L, E = got.n_loci, got.n_entries
        assert (res["n_loci"], res["n_entries"], cells) == (L, E, 2)
        assert dev["chr"].tolist() == [0, L]
        assert np.array_equal(dev["pos"][:L].view(np.uint32), got.locus_pos)
        assert np.array_equal(dev["off"][:L + 1].view(np.uint64), got.locus_entry_off)
        assert np.array_equal(dev["rid"][:E].view(np.uint32), got.read_ids)
        assert np.array_equal(dev["idb"][:E].view(np.uint16).astype(np.uint32), got.id_base)


def error_cases(cases, which):
    if which == "chunks":
        return [c for c in cases["chunks"] if c.kind == pe.ABORT]
    return [c for c in cases["cigars"] if c.kind != pe.CLEAN and c.name.startswith("cigars/" + which)]


@pytest.mark.parametrize("which,count", [("insert_not_last", 8), ("deletion", 8), ("quality_index", 8), ("chunks", 1)])
def test_aborts_are_errors_that_disturb_nothing(which, count, cases, golden, tmp_path):
    """What the reference's asserts refuse (and the quality index past the quality string, which it reads) is a
    SecedoError naming the record; the next call on a good file gives the right bytes."""
    mine = error_cases(cases, which)
    assert len(mine) == count
    good = cases["tags"][1]
    for k, c in enumerate(mine):
        with pytest.raises(ref.RefAbort):
            pe.run_restatement(c)
        if c.kind == pe.ABORT:
            assert golden[c.name]["status"] == pe.ABORT_STATUS
        with pytest.raises(secedo_amd.SecedoError) as e:
            pile(c, str(tmp_path / ("e%d" % k)))
        assert e.value.code == -1 and "file 0, record 1" in str(e.value), (c.name, str(e.value))
        check(good, str(tmp_path / ("g%d" % k)), golden)
