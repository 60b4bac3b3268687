"""The edge cases of tests/pileup_edge_cases.py on the CPU: the Python restatement of the reference's pileup_bams()
(tests/pileup_bam_ref.py) equals what the compiled reference gave on every case, as committed in
tests/golden/pileup_edges.npz, and, where oracle/_ref/ref_pileup is built, what it gives when run afresh, byte for
byte on .bin and .map; an assert of the reference is a RefAbort of the restatement and the reverse. The cases where
the reference reads past the quality string are undefined behaviour there: the restatement raises, nothing is
compared."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import pileup_bam_ref as ref
from tests import pileup_edge_cases as pe
from tests.golden_util import GOLDEN


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "pileup_edges.npz"))
    return {str(n): {k: z[k][i].item() for k in z.files if k != "name"} for i, n in enumerate(z["name"])}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("edges")
    with pe.cached_records():
        yield {f: pe.build(f, d) for f in pe.FAMILIES}


def restatement(case):
    """-> the restatement's Pileup, or None where it raises RefAbort"""
    try:
        return pe.run_restatement(case)
    except ref.RefAbort:
        return None


def test_every_defined_case_is_recorded(cases, golden):
    names = [c.name for f in pe.FAMILIES for c in cases[f]]
    assert len(set(names)) == len(names)
    assert set(golden) == {c.name for f in pe.FAMILIES for c in cases[f] if c.kind != pe.UNDEFINED}


@pytest.mark.parametrize("family", pe.FAMILIES)
def test_restatement_equals_recorded_reference(family, cases, golden):
    for c in cases[family]:
        got = restatement(c)
        if c.kind != pe.CLEAN:
            assert got is None, c.name
            if c.kind == pe.ABORT:
                assert golden[c.name]["status"] == pe.ABORT_STATUS, c.name
            continue
        want = golden[c.name]
        assert want["status"] == 0 and got is not None, c.name
        s = pe.summary_of_restatement(got)
        assert (s["bin_sha"], s["map_sha"]) == (want["bin_sha"], want["map_sha"]), c.name
        assert (s["n_loci"], s["n_entries"]) == (want["n_loci"], want["n_entries"]), c.name
        assert s["n_loci"] == len(got.loci)
        if family in pe.SMALL_FAMILIES:
            assert s["txt"] == want["txt"], c.name


def test_cigar_family_conditions(cases, golden):
    walked, aborting = pe.classify_cigars()
    assert len(pe.all_cigars()) == 2835 and len(walked) >= 2000
    assert {cigar[0][0] for _, cigar in walked} == set("MIDNSHP=X")
    assert {cigar[-1][0] for _, cigar in walked} == set("MIDNSHP=X")
    assert len(aborting[pe.INSERT_NOT_LAST]) >= 60
    assert len(aborting[pe.DELETION]) >= 12
    assert len(aborting[pe.QUALITY_INDEX]) >= 400
    kinds = [c.kind for c in cases["cigars"]]
    assert kinds.count(pe.CLEAN) == 1 and kinds.count(pe.ABORT) == 16 and kinds.count(pe.UNDEFINED) == 8
    whole = golden[cases["cigars"][0].name]
    assert (len(walked), whole["n_loci"]) == (2286, 5836)


def test_wrap_keeps_the_last_arrivals(cases, golden):
    by = {c.name: c for c in cases["wrap"]}
    for k in (0, 1):
        for p in pe.WRAP_PARAMS:
            assert golden[pe.case_name("wrap", "k%d" % k, p)]["n_loci"] == 0
    got = restatement(by[pe.case_name("wrap", "k5", (100, 0, 0, 0, 3))])
    assert got.loci == [(pe.WRAP_POS + 1, [65536, 65537, 65538, 65539, 65540], [0, 1, 2, 3, 0])]
    assert golden[pe.case_name("wrap", "k5", (100, 0, 0, 0, 3))]["n_entries"] == 5
    assert golden[pe.case_name("wrap", "k5", (100, 0, 0, 0, 4))]["n_loci"] == 0
    assert golden[pe.case_name("wrap", "k5", (3, 0, 0, 0, 0))]["n_loci"] == 0


def test_families_reach_what_they_are_for(cases, golden):
    """The loci lie where each family means them to: on both sides of the second device window's start, behind the
    chunk's end only when another record opens the next chunk, and so on."""
    win = restatement(cases["window"][0])
    pos = [p - 1 for p, _, _ in win.loci]
    assert min(pos) < pe.WINDOW - 1 and pe.WINDOW - 1 in pos and pe.WINDOW in pos and max(pos) > pe.WINDOW
    ch = {c.name.split("/")[1].split("@")[0]: c for c in cases["chunks"]}
    assert max(p for p, _, _ in restatement(ch["cut_off"]).loci) == 1_000_000  # 1-based: position 999,999
    assert max(p for p, _, _ in restatement(ch["carried_over"]).loci) == 1_000_020
    assert max(p for p, _, _ in restatement(ch["999_past"]).loci) == 1_001_000
    assert ch["1000_past"].kind == pe.ABORT and restatement(ch["1000_past"]) is None
    q = {c.params[1]: golden[c.name]["n_loci"] for c in cases["quality"]}
    assert q[0] > q[1] > q[20] > q[21] > q[94] > q[95] == q[96] == q[200] > 0
    t = {c.params[3]: golden[c.name]["n_loci"] for c in cases["tags"]}
    assert t[0] == 3 * len(pe.TAG_LAYOUTS) and t[0] > t[50] > t[51] > 0
    codes = restatement(cases["seq"][0])
    assert [p for p, _, _ in codes.loci] == [102, 103, 105, 109, 117, 201]  # A C G T of the sixteen codes, A, one base


@pytest.mark.skipif(not pe.have_reference(), reason="oracle/_ref/ref_pileup not built")
@pytest.mark.parametrize("family", pe.FAMILIES)
def test_reference_run_afresh_equals_restatement(family, cases, tmp_path):
    # the reference reads past the quality string in the UNDEFINED cases: whatever it does there is not compared
    todo = [c for c in cases[family] if c.kind != pe.UNDEFINED]
    outs = [str(tmp_path / ("ref%d" % k)) for k in range(len(todo))]
    with ThreadPoolExecutor(max_workers=4) as pool:  # each run is a process of its own, most of it allocation
        statuses = list(pool.map(lambda co: pe.run_reference(co[0], co[1], timeout=120), zip(todo, outs)))
    for c, out, status in zip(todo, outs, statuses):
        got = restatement(c)
        assert status in (0, pe.ABORT_STATUS), (c.name, status)
        assert (status == pe.ABORT_STATUS) == (got is None), (c.name, status)
        if got is not None:
            assert open(out + ".bin", "rb").read() == got.bin_bytes(), c.name
            assert open(out + ".map", "rb").read() == got.map_text().encode(), c.name
            assert pe.txt_upto16(open(out + ".txt").read()) == pe.txt_upto16(got.txt_text()), c.name
