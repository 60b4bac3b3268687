"""secedo_bam_split_clusters without a GPU: the host logic of secedo_amd/csrc/bam_split.hpp as a program under the
sanitizers, the refusals of ``python -m secedo_amd.split_main`` (made before torch is imported), and
tests/split_expected.py against itself: inflating the file it expects and reading it back gives the records of the
cluster's cells in (RefID, Position, file, record) order."""
import gzip
import json
import os
import subprocess
import sys

import pytest

from tests import bam_writer as bw
from tests import split_expected as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bam_split_test")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bam")


def test_host_program_under_sanitizers():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok ") and r.stderr == ""


# ---- the CLI's refusals

WRAPPER = ("import json, sys\n"
           "from secedo_amd import split_main\n"
           "try:\n"
           "    code = split_main.main(sys.argv[1:])\n"
           "except SystemExit as e:\n"
           "    code = e.code\n"
           "print(json.dumps({'code': code, 'torch': 'torch' in sys.modules}))\n")


def refused(args):
    """-> the reason ``main`` gave up with; torch must not have been imported by then."""
    r = subprocess.run([sys.executable, "-c", WRAPPER] + [str(a) for a in args], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["torch"] is False
    assert isinstance(out["code"], str) and "\n" not in out["code"], out
    return out["code"]


@pytest.fixture()
def cli_inputs(tmp_path):
    cells = tmp_path / "cells"
    cells.mkdir()
    for k, name in enumerate(("test1", "test2", "hard_clipping")):
        (cells / ("cell_%d.bam" % k)).write_bytes(open(os.path.join(GOLDEN, name + ".bam"), "rb").read())
    clustering = tmp_path / "clustering"
    clustering.write_text("1,0,1\n")
    out = tmp_path / "out"
    out.mkdir()
    return cells, clustering, out


def test_cli_refusals(cli_inputs, tmp_path):
    cells, clustering, out = cli_inputs
    base = ["-i", cells, "-o", out, "--chromosomes", "1"]
    assert "does not exist" in refused(base + ["--clustering", tmp_path / "missing"])
    short = tmp_path / "short"
    short.write_text("1,0\n")
    why = refused(base + ["--clustering", short])
    assert "lists 2 cells" in why and "has 3" in why
    assert "--cell_tag needs --cells" in refused(base + ["--clustering", clustering, "--cell_tag", "CB"])
    barcodes = tmp_path / "barcodes.tsv"
    barcodes.write_text("AAA\nCCC\nGGG\n")
    assert "Invalid --cell_tag" in refused(base + ["--clustering", clustering, "--cell_tag", "C!", "--cells", barcodes])
    assert "--cells needs --cell_tag" in refused(base + ["--clustering", clustering, "--cells", barcodes])
    why = refused(base + ["--clustering", short, "--cell_tag", "CB", "--cells", barcodes])
    assert "lists 2 cells" in why and "has 3" in why  # tag mode: the cells are the barcodes
    not_dir = tmp_path / "file"
    not_dir.write_text("")
    assert "is not a directory" in refused(["-i", cells, "-o", not_dir, "--clustering", clustering])
    assert "is not a directory" in refused(["-i", cells, "-o", tmp_path / "nowhere", "--clustering", clustering])
    (out / "cluster_1.bam").write_bytes(b"kept")
    why = refused(base + ["--clustering", clustering])
    assert "cluster_1.bam exists" in why and "--overwrite" in why
    assert (out / "cluster_1.bam").read_bytes() == b"kept"
    bad = tmp_path / "bad"
    bad.write_text("1,x,0\n")
    assert "not a cluster number" in refused(base + ["--clustering", bad])


def test_cli_exit_code_and_one_line(cli_inputs, tmp_path):
    cells, _clustering, out = cli_inputs
    r = subprocess.run([sys.executable, "-m", "secedo_amd.split_main", "-i", str(cells), "-o", str(out),
                        "--clustering", str(tmp_path / "missing")], capture_output=True, text=True, cwd=ROOT,
                       timeout=120)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.strip().count("\n") == 0 and "does not exist" in r.stderr


# ---- split_expected against itself

def records_back(raw: bytes, tmp_path, name):
    path = tmp_path / name
    path.write_bytes(raw)
    return bw.read_bam(str(path))


def check_expected(sources, clustering, chromosome_ids, tmp_path, tag=None, barcodes=None):
    """Every expected file is a BAM of whole members that holds exactly its cluster's records, in order."""
    files, dropped = se.expected_files(sources, clustering, chromosome_ids, tmp_path, tag, barcodes)
    assert len(files) == max(clustering) + 1
    index = None if tag is None else {b.encode(): c for c, b in enumerate(barcodes)}
    seen = 0
    for k, raw in enumerate(files):
        assert raw.endswith(se.EOF) and all(isize <= se.CUT for isize, _ in se.member_sizes(raw))
        refs, recs = records_back(raw, tmp_path, "expected_%d.bam" % k)
        assert refs == sources[0].refs
        text = gzip.decompress(raw)[8:].split(b"\0")[0].decode(errors="replace")
        assert "@CO\tsecedo_amd cluster %d: %d of %d cells\n" % (k, clustering.count(k), len(clustering)) in text
        want = []
        for f, s in enumerate(sources):
            for i, rec in enumerate(s.records):
                ref, pos = se.ref_pos(rec)
                cell = f if index is None else index.get(se.z_value(rec, tag))
                if ref in chromosome_ids and cell is not None and clustering[cell] == k:
                    want.append((ref, pos, f, i, rec))
        want.sort(key=lambda r: r[:4])
        assert [(r["ref"], r["pos"]) for r in recs] == [(w[0], w[1]) for w in want]
        inflated = gzip.decompress(raw)
        assert inflated.endswith(b"".join(w[4] for w in want))
        assert [(r["ref"], r["pos"]) for r in recs] == sorted((r["ref"], r["pos"]) for r in recs)
        seen += len(recs)
    mapped = sum(1 for s in sources for rec in s.records if se.ref_pos(rec)[0] in chromosome_ids)
    assert seen + dropped == mapped
    return files, dropped


def test_expected_on_golden_bams(tmp_path):
    names = ("test1", "test2", "hard_clipping", "soft_clipping", "insert_at_end")
    sources = [se.source_of_bam(os.path.join(GOLDEN, n + ".bam")) for n in names]
    assert all(len(s.records) == 2 for s in sources)
    files, _ = check_expected(sources, [1, 0, 1, 3, 0], [0], tmp_path)
    refs, recs = records_back(files[2], tmp_path, "empty.bam")  # no cell has 2: header only
    assert recs == [] and len(se.member_sizes(files[2])) == 2
    # the input's @CO lines are not carried, the one @CO line is the cluster's
    text = gzip.decompress(files[0])[8:].split(b"\0")[0].decode(errors="replace")
    assert text.count("@CO\t") == 1 and text.startswith("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:1\tLN:2\n")


def test_source_of_bam_matches_the_writer(tmp_path):
    cells = se.cell_records(n_cells=2, pairs=5)
    path = tmp_path / "cell.bam"
    bw.write_bam(str(path), se.REFS, cells[1])
    a, b = se.source_of_bam(str(path)), se.source_of_recs(se.REFS, cells[1])
    assert (a.text, a.refs, a.records) == (b.text, b.refs, b.records)


def test_expected_on_the_synthetic_sets(tmp_path):
    cells = se.cell_records()
    sources = [se.source_of_recs(se.REFS, c) for c in cells]
    files, dropped = check_expected(sources, se.CLUSTERING, [0, 1], tmp_path)
    assert dropped == 0
    # the multiplexed file gives the same files in tag mode, and drops exactly the extra records
    recs, n_extra = se.multiplexed_records(cells)
    tagged, dropped = check_expected([se.source_of_recs(se.REFS, recs)], se.CLUSTERING, [0, 1], tmp_path, "CB",
                                     se.BARCODES)
    assert tagged == files and dropped == n_extra == 9
    # @RG lines: merged in order of first appearance
    texts = [se.default_text(se.REFS) + "@RG\tID:%s\tSM:s\n" % i for i in ("b", "a", "b")]
    rg = [se.source_of_recs(se.REFS, cells[c], texts[c]) for c in range(3)]
    raw = se.expected_files(rg, [0, 0, 1], [0], tmp_path)[0][0]
    text = gzip.decompress(raw)[8:].split(b"\0")[0].decode(errors="replace")
    assert "\n@RG\tID:b\tSM:s\n@RG\tID:a\tSM:s\n@PG\tID:secedo_amd.split" in text
