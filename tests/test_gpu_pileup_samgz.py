"""BGZF-compressed SAM (.sam.gz) on the GPU: the device inflate (secedo_amd.bgzf_inflate) equals zlib byte for byte, and
a .sam.gz gives what its text gives as a plain SAM file and what the BAM of the same records gives (.bin/.map/.txt,
resident arrays, num_cells, max_read_length, barcodes), whatever the compression level, strategy, member size, range
size and pool size; errors name the same line, and a corrupt block is reported by its index ahead of any parse error.
The corrupt inputs are ones the host build of the same decoder (tests/test_bgzf_inflate_cpu.py) already handles."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import bam_pileup
from tests import bam_writer as bw
from tests import bgzf_writer as gw
from tests import multiplex_bam as mb
from tests import sam_writer as sw
from tests.test_gpu_pileup_bam import FIXTURE_CASES
from tests.test_gpu_pileup_sam import BAM, GOOD, HEAD, _resident, files_of, fixture_sam, pile, same

pytestmark = pytest.mark.gpu

# how the .sam.gz of a test is written: stored blocks, fixed Huffman, and 4 KiB members (lines across many members)
WRITERS = {"l6": dict(level=6), "stored": dict(level=0), "fixed": dict(level=6, strategy="fixed"),
           "4k": dict(level=6, chunk=4096), "l1-flush": dict(level=1, flush=True)}


def gz_of(sam, directory, how="l6", name=None):
    path = os.path.join(str(directory), name or (os.path.basename(sam) + ".gz"))
    with open(path, "wb") as f:
        f.write(gw.bgzf(open(sam, "rb").read(), **WRITERS[how]))
    return path


def test_bgzf_inflate_equals_zlib(tmp_path):
    for name, path, want in gw.round_trip_files(tmp_path):
        got = secedo_amd.bgzf_inflate(path)
        assert got.dtype == np.uint8 and got.tobytes() == want, name


def test_bgzf_inflate_in_small_ranges(tmp_path, monkeypatch):
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", "65536")
    for name, path, want in gw.round_trip_files(tmp_path):
        assert secedo_amd.bgzf_inflate(path).tobytes() == want, name


@pytest.mark.parametrize("how", ["l6", "stored", "fixed", "4k"])
@pytest.mark.parametrize("case", range(len(FIXTURE_CASES)))
def test_fixture_cases_from_sam_gz(case, how, tmp_path):
    names, max_cov, mq, score, diff, n_loci = FIXTURE_CASES[case]
    bams = [os.path.join(BAM, n + ".bam") for n in names]
    sams = [fixture_sam(n, tmp_path) for n in names]
    gzs = [gz_of(s, tmp_path, how, "%d_%s.sam.gz" % (k, how)) for k, s in enumerate(sams)]
    params = (max_cov, 1, mq, score, diff)
    p = same(bams, gzs, tmp_path, params=params)
    assert p.n_loci == n_loci
    assert pile(sams, str(tmp_path / "plain"), params=params)[1] == files_of(str(tmp_path / "s"))


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """The synthetic cells of test_gpu_pileup_sam.py as BAM, SAM and .sam.gz (level 6, stored, fixed, 4 KiB members)."""
    d = tmp_path_factory.mktemp("synth_samgz")
    refs, cells = mb.synthetic_cells(d / "raw", n_cells=8, pairs_per_cell=60, n_refs=2, seed=11)
    bams, sams = [], []
    for c, recs in enumerate(cells):
        b, s = sw.write_both(d, "cell_%03d" % c, refs, recs)
        bams.append(b)
        sams.append(s)
    gzs = {}
    for how in ("l6", "stored", "fixed", "4k"):
        os.mkdir(d / how)
        gzs[how] = [gz_of(s, d / how, how) for s in sams]
    return refs, cells, bams, sams, gzs


@pytest.mark.parametrize("how", ["l6", "stored", "fixed", "4k"])
@pytest.mark.parametrize("params", [(100, 30, 30, 0, 3), (100, 0, 0, 0, 0), (6, 20, 10, 50, 1), (100, 35, 0, 90, 2)])
@pytest.mark.parametrize("chromosome", [0, 1])
def test_synthetic_sets_from_sam_gz(synth, params, chromosome, how, tmp_path):
    _, _, bams, sams, gzs = synth
    p = same(bams, gzs[how], tmp_path, chromosome=chromosome, params=params)
    assert pile(sams, str(tmp_path / "plain"), chromosome=chromosome, params=params)[1] == files_of(str(tmp_path / "s"))
    if params[1] == 0:
        assert p.n_loci > 100


def test_small_ranges_give_identical_outputs(synth, tmp_path, monkeypatch):
    refs, cells, _, _, _ = synth
    recs = [r for c in mb.tagged(cells, ["B%02d" % c for c in range(len(cells))]) for r in c]
    bam, sam = sw.write_both(tmp_path, "big", refs, sorted(recs, key=bw.sort_key))
    assert os.path.getsize(sam) > 4 * 65536
    want = pile([bam], str(tmp_path / "w"))[1]
    gzs = [gz_of(sam, tmp_path, how, "big_%s.sam.gz" % how) for how in ("l6", "4k", "stored", "l1-flush")]
    for gz in gzs:
        assert pile([gz], str(tmp_path / "full"))[1] == want
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", "65536")
    for gz in gzs:
        assert pile([gz], str(tmp_path / "r"))[1] == want
    assert pile([bam, gzs[0], sam], str(tmp_path / "m"))[1] == pile([bam, bam, bam], str(tmp_path / "mb"))[1]
    monkeypatch.setenv("SECEDO_BAM_BATCH_BYTES", "1000")  # every range one member, most lines carried
    assert pile([gzs[1]], str(tmp_path / "t"))[1] == want


def test_resident_two_chromosomes(synth):
    _, _, bams, _, gzs = synth
    i2g = (np.arange(len(bams)) // 2).astype(np.uint16)
    gb, cb, lb = _resident(bams, i2g)
    gs, cs, ls = _resident(gzs["l6"], i2g)
    assert (cs, ls) == (cb, lb) and gb["chr"][-1] > 0
    for k in gb:
        assert np.array_equal(gs[k], gb[k]), k


def test_mixed_list(synth, tmp_path):
    _, _, bams, sams, gzs = synth
    same(bams[:4], [bams[0], sams[1], gzs["l6"][2], gzs["4k"][3]], tmp_path)


def test_tag_mode_and_barcodes(synth, tmp_path):
    refs, cells, _, _, _ = synth
    barcodes = ["AAC%02d-1" % c for c in range(len(cells))]
    recs = [r for c in mb.tagged(cells, barcodes) for r in c]
    bams, sams = sw.write_multiplexed(tmp_path, refs, recs, n_lanes=1, seed=4)
    gzs = [gz_of(s, tmp_path) for s in sams]
    listed = barcodes[::-1][:6]
    for chromosome in (0, 1):
        same(bams, gzs, tmp_path, chromosome=chromosome, cell_tag="CB", cells=listed)
    vb, cb = bam_pileup.bam_barcodes(bams, "CB", [0, 1], 4)
    vs, cs = bam_pileup.bam_barcodes(gzs, "CB", [0, 1], 4)
    assert vs == vb == sorted(barcodes) and np.array_equal(cs, cb)


@pytest.mark.parametrize("threads", [1, 16])
def test_pool_sizes(synth, tmp_path, threads):
    _, _, bams, _, gzs = synth
    same(bams, gzs["l6"], tmp_path, threads=threads)


def _err(files):
    with pytest.raises(secedo_amd.SecedoError) as e:
        bam_pileup.pileup_bams(files, None, False, 0, 100, 0, 0, 0, 1, 0)
    return e.value


BAD = "x\t67\t1\t21\t60\t4Q\t=\t21\t0\tACGT\tIIII\n"


def test_a_bad_line_names_the_same_line(tmp_path):
    filler = "".join("f%d\t67\t1\t%d\t60\t4M\t=\t%d\t0\tACGT\tIIII\n" % (k, 12 + k, 12 + k) for k in range(3000))
    plain = tmp_path / "e.sam"
    plain.write_text(HEAD + GOOD + filler + BAD + GOOD.replace("\t11\t", "\t5000\t"))
    for how in ("l6", "4k"):
        gz = gz_of(str(plain), tmp_path, how, "e_%s.sam.gz" % how)
        want, got = _err([str(plain)]), _err([gz])
        assert got.code == want.code == -1 and ", line 3005" in str(want)
        assert str(got) == str(want).replace(str(plain), gz)
    # a header-only and an empty-bodied file are fine, a bad @SQ names its line
    gz = tmp_path / "h.sam.gz"
    gz.write_bytes(gw.bgzf(("@HD\tVN:1.6\n@SQ\tSN:1\n" + GOOD).encode()))
    assert "line 2" in str(_err([str(gz)]))


def error_text() -> bytes:
    """Three header lines, a good line, a bad line (line 5, in member 0), then 6000 good lines."""
    filler = "".join("f%d\t67\t1\t%d\t60\t4M\t=\t%d\t0\tACGT\tIIII\n" % (k, 12 + k, 12 + k) for k in range(6000))
    return (HEAD + GOOD + BAD + filler).encode()


def test_a_corrupt_block_is_reported_by_index(tmp_path):
    """The files of gw.corrupt_files, which tests/test_bgzf_inflate_cpu.py runs through the host build first. The
    corrupt block wins over the bad line 5 wherever it lies: the call is one range."""
    for how, k, raw in gw.corrupt_files(error_text()):
        path = tmp_path / ("c_%s_%d.sam.gz" % (how, k))
        path.write_bytes(raw)
        e = _err([str(path)])
        msg = str(e)
        assert e.code == -1 and msg.count("%s: BGZF block %d: " % (path, k)) == 1 and "line" not in msg, msg
        assert msg.endswith("inflate failed or ISIZE mismatch") or msg.endswith("CRC32 mismatch"), msg
        if how == "stored":
            assert msg.endswith("CRC32 mismatch")
        with pytest.raises(secedo_amd.SecedoError) as e2:
            secedo_amd.bgzf_inflate(str(path))
        assert str(e2.value) == msg


@pytest.mark.parametrize("damage", range(len(gw.LISTING_DAMAGE)))
def test_a_file_whose_members_cannot_be_listed(tmp_path, damage):
    """Member 0 (SAM text, which makes the file a .sam.gz) is whole; the list breaks at member 1."""
    name, data, tail = gw.listing_damage(gw.bgzf(error_text()[:20000], chunk=4096))[damage]
    path = tmp_path / (name + ".sam.gz")
    path.write_bytes(data)
    e = _err([str(path)])
    assert e.code == -1 and str(e) == gw.ERROR_PREFIX + str(path) + tail


def test_plain_gzip_is_still_refused_and_names_play_no_part(synth, tmp_path):
    import gzip
    _, _, bams, sams, gzs = synth
    path = tmp_path / "x.sam.gz"
    path.write_bytes(gzip.compress((HEAD + GOOD).encode()))
    e = _err([str(path)])
    assert e.code == -1 and "not BGZF" in str(e) and "decompress" in str(e)
    # a BAM named .sam.gz is a BAM, a .sam.gz named .bam is a .sam.gz
    as_gz, as_bam = str(tmp_path / "really_bam.sam.gz"), str(tmp_path / "really_samgz.bam")
    shutil.copy(bams[0], as_gz)
    shutil.copy(gzs["l6"][1], as_bam)
    same(bams[:2], [as_gz, as_bam], tmp_path)


def test_cli_on_sam_gz_directory(synth, tmp_path):
    _, _, bams, _, gzs = synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for kind, files in (("bam", bams), ("gz", gzs["l6"])):
        d = tmp_path / kind
        d.mkdir()
        for f in files[:4]:
            shutil.copy(f, d / os.path.basename(f))
        o = str(tmp_path / ("o_" + kind))
        r = subprocess.run([sys.executable, "-m", "secedo_amd.pileup_main", "-i", str(d), "-o", o, "--chromosomes",
                            "1,2", "--min_base_quality", "0", "--min_map_quality", "0", "--min_different", "0"],
                           cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append([open(o + s, "rb").read() for s in ("_1,2.map", "_1.pileup.bin", "_1.pileup.map",
                                                         "_1.pileup.txt", "_2.pileup.bin", "_2.pileup.txt")])
    assert outs[0] == outs[1] and len(outs[0][1]) > 0
