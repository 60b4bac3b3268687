"""Building .bai indexes on the GPU (secedo_amd.bam_index_build, secedo_bam_index_build): the index written equals,
byte for byte, the samtools-written ones of tests/golden/bam and what tests/bai_expected.py derives from the BAM alone,
whatever the member layout and however many ranges or batches the files take; the project's own reader and
``pileup_bams(index="require")`` read it back; errors name the file and leave nothing behind."""
import gzip
import os
import shutil
import subprocess
import sys

import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bai_expected as be
from tests import bai_writer as bi
from tests import bam_device_cases as cases
from tests import bam_writer as bw
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAM = os.path.join(GOLDEN, "bam")
GOLDENS = ["test1", "test2", "test3", "soft_clipping", "hard_clipping", "insert_at_end"]
SMALL_BATCH = "1000"  # tests/test_gpu_pileup_bam_device.py's smallest SECEDO_BAM_BATCH_BYTES


def no_temporaries(directory):
    return not [n for n in os.listdir(str(directory)) if ".tmp." in n]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """the layout-case file written three ways -> {how: (path, expected index bytes)}"""
    d = tmp_path_factory.mktemp("layout_index")
    out = {}
    for how in sorted(be.LAYOUT_WRITERS):
        path = be.layout_bam(d, how)
        out[how] = (path, be.expected_bytes(path))
    return out


def test_reference_held_vectors(tmp_path):
    paths = []
    for name in GOLDENS:
        paths.append(str(tmp_path / (name + ".bam")))
        shutil.copy(os.path.join(BAM, name + ".bam"), paths[-1])
    info = secedo_amd.bam_index_build(paths)
    stats = bam_pileup.bam_route_stats()
    for name, path in zip(GOLDENS, paths):
        assert open(path + ".bai", "rb").read() == open(os.path.join(BAM, name + ".bam.bai"), "rb").read(), name
    assert info["files"] == 6 and stats["batches"] == 1 and stats["device_records"] == info["records"]
    assert info["index_bytes"] == sum(os.path.getsize(p + ".bai") for p in paths)
    assert info["records"] == sum(len(bw.read_bam(p)[1]) for p in paths)
    # out_paths, with an entry left to the default; the process's host route does not matter
    os.remove(paths[0] + ".bai")
    with bam_pileup._route("host"):
        secedo_amd.bam_index_build(paths[:2], out_paths=[None, str(tmp_path / "other.bai")], num_threads=4)
    assert open(str(tmp_path / "other.bai"), "rb").read() == open(paths[1] + ".bai", "rb").read()
    assert open(paths[0] + ".bai", "rb").read() == open(os.path.join(BAM, "test1.bam.bai"), "rb").read()
    assert bam_pileup.bam_route_stats()["device_blocks"] > 0 and no_temporaries(tmp_path)


@pytest.mark.parametrize("batch", [None, SMALL_BATCH])
@pytest.mark.parametrize("how", sorted(be.LAYOUT_WRITERS))
def test_layout_cases(how, batch, layout, tmp_path, monkeypatch):
    path, want = layout[how]
    if batch:
        monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", batch)
    out = str(tmp_path / "out.bai")
    info = secedo_amd.bam_index_build([path], out_paths=[out])
    stats = bam_pileup.bam_route_stats()
    assert open(out, "rb").read() == want
    n = len(bi.layout(path)[1])
    assert info["records"] == n == stats["device_records"] and info["index_bytes"] == len(want)
    if batch:
        assert stats["batches"] > 1  # the file took several ranges
        assert info["joined_runs"] > 0  # and a (RefID, bin) run crossed a range boundary
    else:
        assert stats["batches"] == 1 and info["joined_runs"] == 0


def test_many_files_one_call(tmp_path):
    paths = bw.synthetic_set(tmp_path, n_cells=40, pairs_per_cell=40, seed=23)
    info = secedo_amd.bam_index_build(paths, num_threads=8)
    stats = bam_pileup.bam_route_stats()
    for p in paths:
        assert open(p + ".bai", "rb").read() == be.expected_bytes(p), p
    assert info["files"] == 40 and stats["batches"] < 40
    assert stats["device_records"] == info["records"] == sum(len(bw.read_bam(p)[1]) for p in paths)


def files_of(out):
    return tuple(open(out + ext, "rb").read() for ext in (".bin", ".map", ".txt"))


def test_round_trip_through_the_reader(layout, tmp_path):
    paths = []
    for how, (path, _want) in sorted(layout.items()):
        paths.append(str(tmp_path / os.path.basename(path)))
        shutil.copy(path, paths[-1])
    secedo_amd.bam_index_build(paths)
    for p in paths:
        got = bam_pileup.bam_index_ranges(p)
        want = bi.ranges(p)
        assert [(int(s), int(e)) for s, e in zip(got["start"], got["end"])] == [w[:2] for w in want]
        # a reference without records has no pseudo-bin: the reader reports no count for it
        assert [int(c) for c in got["count"]] == [w[2] if w[2] else -1 for w in want]
    for chromosome in (0, 3):  # with records, and the one without
        for route in ("host", "device"):
            outs = {}
            for index in ("off", "require"):
                out = str(tmp_path / ("p_%d_%s_%s" % (chromosome, route, index)))
                p = bam_pileup.pileup_bams(paths, out, True, chromosome, 100, 0, 0, 0, 4, 0, inflate=route,
                                           index=index)
                outs[index] = files_of(out)
                assert (p.n_loci > 0) == (chromosome == 0)
                if index == "require":
                    assert bam_pileup.bam_index_stats()["files_indexed"] == len(paths)
            assert outs["off"] == outs["require"], (chromosome, route)


def test_pileup_main_build_index(layout, tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    for k, (how, (path, _want)) in enumerate(sorted(layout.items())):
        shutil.copy(path, str(d / ("cell%d_x.bam" % k)))
    kept = str(d / "cell1_x.bam.bai")
    bi.write_bai(str(d / "cell1_x.bam"))  # forward fill: not the bytes the builder would write
    os.utime(kept, (1_000_000_000, 1_000_000_000))
    before = (open(kept, "rb").read(), os.stat(kept).st_mtime_ns)
    assert before[0] != be.expected_bytes(str(d / "cell1_x.bam"))
    run = lambda *a: subprocess.run([sys.executable, "-m", "secedo_amd.pileup_main", "-i", str(d), "--chromosomes",  # noqa: E731
                                     "1", "--min_base_quality", "0", "--min_map_quality", "0", "--min_different", "0",
                                     *a], capture_output=True, text=True, timeout=600,
                                    env=dict(os.environ, PYTHONPATH=ROOT))
    p = run("-o", str(tmp_path / "off"), "--index", "off")
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(str(d))) == ["cell0_x.bam", "cell1_x.bam", "cell1_x.bam.bai", "cell2_x.bam"]
    p = run("-o", str(tmp_path / "req"), "--index", "require", "--build_index")
    assert p.returncode == 0 and "Indexed 2 of 3 input files" in p.stdout, (p.stdout, p.stderr[-2000:])
    assert files_of(str(tmp_path / "req_1.pileup")) == files_of(str(tmp_path / "off_1.pileup"))
    assert (open(kept, "rb").read(), os.stat(kept).st_mtime_ns) == before
    for k in (0, 2):
        bam = str(d / ("cell%d_x.bam" % k))
        assert open(bam + ".bai", "rb").read() == be.expected_bytes(bam)
    assert no_temporaries(d)
    # index_main on the directory (it refuses existing indexes before the GPU is touched: the CPU tests) replaces them
    im = lambda *a: subprocess.run([sys.executable, "-m", "secedo_amd.index_main", "-i", str(d), *a],  # noqa: E731
                                   capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    p = im("--overwrite", "--num_threads", "4")
    assert p.returncode == 0 and len([l for l in p.stdout.splitlines() if l.endswith(" bytes")]) == 3, p.stderr[-2000:]
    assert open(kept, "rb").read() == be.expected_bytes(str(d / "cell1_x.bam"))


def build_error(files, **kw):
    with pytest.raises(secedo_amd.SecedoError) as e:
        secedo_amd.bam_index_build(files, **kw)
    assert e.value.code == -1, str(e.value)
    return str(e.value)


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def test_errors(tmp_path):
    refs = [("1", 3_000_000), ("2", 3_000_000)]
    good = write(tmp_path, "good.bam", bw.bam_bytes(refs, cases.many()))
    # not coordinate-sorted: the record is named
    recs = cases.many()
    recs[300], recs[301] = recs[301], recs[300]
    unsorted = write(tmp_path, "unsorted.bam", bw.bam_bytes(refs, recs))
    msg = build_error([unsorted])
    assert "unsorted.bam: record 301: input is not coordinate-sorted" in msg
    assert not os.path.exists(unsorted + ".bai") and no_temporaries(tmp_path)
    assert not bam_pileup.bam_scan(unsorted, device=True)["sorted"]  # in scan mode it is no error
    # SAM text and plain gzip
    assert "a SAM file cannot be indexed" in build_error([write(tmp_path, "t.sam", b"@HD\tVN:1.6\n")])
    assert "not BGZF" in build_error([write(tmp_path, "t.sam.gz", gzip.compress(b"@HD\tVN:1.6\n"))])
    # a corrupt member, a broken record chain: secedo_bam_scan_device's message
    broken = [data for _how, _k, data in cases.corrupt_bams()] + [cases.corrupt_with_record_error(20)]
    for k, data in enumerate(broken):
        path = write(tmp_path, "corrupt_%d.bam" % k, data)
        with pytest.raises(secedo_amd.SecedoError) as e:
            bam_pileup.bam_scan(path, device=True)
        assert build_error([path]) == str(e.value) and ("BGZF block" in str(e.value) or k == len(broken) - 1)
        assert not os.path.exists(path + ".bai")
    assert "record 20 has a bad block_size" in str(e.value) and no_temporaries(tmp_path)
    # what BAI cannot hold: a reference longer than 2^29; a record that ends past 2^29
    at = (1 << 29) - 30
    rec = bw.Rec("late", 0, at, [("M", 60)], "ACGT" * 15, qual=[40] * 60)
    msg = build_error([write(tmp_path, "long.bam", bw.bam_bytes([("1", (1 << 29) + 1)], [rec]))])
    assert "long.bam: reference 0" in msg and "BAI" in msg
    msg = build_error([write(tmp_path, "past.bam", bw.bam_bytes([("1", 1 << 29)], cases.many(100) + [rec]))])
    assert "past.bam: record 100 ends past" in msg and "BAI" in msg
    rec = bw.Rec("fits", 0, at, [("M", 30)], "ACGT" * 7 + "AC", qual=[40] * 30)
    fits = write(tmp_path, "fits.bam", bw.bam_bytes([("1", 1 << 29)], [rec]))
    secedo_amd.bam_index_build([fits])
    assert open(fits + ".bai", "rb").read() == be.expected_bytes(fits)
    # an existing output
    secedo_amd.bam_index_build([good])
    want = be.expected_bytes(good)
    assert open(good + ".bai", "rb").read() == want
    open(good + ".bai", "wb").write(b"mine")
    assert "good.bam.bai exists" in build_error([good])
    assert open(good + ".bai", "rb").read() == b"mine"
    secedo_amd.bam_index_build([good], overwrite=True)
    assert open(good + ".bai", "rb").read() == want
    # the second of three files is bad: the first keeps its finished index, the third gets none
    first, third = write(tmp_path, "first.bam", open(good, "rb").read()), write(tmp_path, "third.bam",
                                                                              open(good, "rb").read())
    for bad in (unsorted, str(tmp_path / "corrupt_4.bam"), str(tmp_path / "missing.bam"), str(tmp_path / "past.bam")):
        msg = build_error([first, bad, third])
        assert os.path.basename(bad) in msg
        assert open(first + ".bai", "rb").read() == be.expected_bytes(first)
        assert not os.path.exists(third + ".bai") and not os.path.exists(bad + ".bai")
        os.remove(first + ".bai")
    assert no_temporaries(tmp_path)
