"""The tabix indexes built on the GPU: secedo_amd.tabix_build on the texts of tests/tabix_cases.py against the bytes
tests/tabix_expected.py gives and, through the spec's query (tests/tabix_reader.py), against the brute-force answer of
every listed region; the same file walked in many ranges; the refusals; and the bgzf writer under vcf_index="tbi"
against the stand-alone route and the expected bytes, from both entry points and the command line."""
import gzip
import os
import shutil

import numpy as np
import pytest

import secedo_amd
from secedo_amd import _lib, secedo_main, tabix_main, variant
from secedo_amd.pileup import FlatPileup
from tests import bgzf_deflate_cases as dc
from tests import bgzf_writer as gw
from tests import tabix_cases as tc
from tests import tabix_expected as te
from tests import tabix_reader as tr
from tests import variant_ref as vr
from tests.clone_tree_gen import clone_tree
from tests.test_gpu_variant import FEMALE, MALE, MALE_MAP, _fasta, _flat, _synthetic, _wrap

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


def _raw_index(path):
    """a written .tbi, checked as a BGZF file that ends in the EOF member -> its uncompressed bytes"""
    raw = open(path, "rb").read()
    assert raw.endswith(gw.EOF_MEMBER)
    data = te.inflate(raw)
    dc.check_file(raw, data, with_tokens=False)
    return data


def _build(tmp_path, name, text, **writer):
    path = str(tmp_path / (name + ".vcf.gz"))
    gz = gw.bgzf(text, **writer)
    with open(path, "wb") as f:
        f.write(gz)
    st = variant.tabix_build(path)
    return gz, _raw_index(path + ".tbi"), st


def _check_regions(gz, index, text):
    reader, recs = tr.Reader(gz, index), te.data_lines(text)
    regions = tc.regions(text)
    hits = 0
    for region in regions:  # every one, no sampling
        got = reader.query(*region)
        assert got == te.overlapping(text, *region, recs=recs), region
        hits += len(got)
    assert hits > 0 and not reader.query(b"absent", 0, 1 << 29)
    return len(regions)


@pytest.fixture(scope="module")
def formatter_text():
    return tc.formatter()


# --- 1. the stand-alone route against the expected bytes and the queries -----------------------------------------

def test_formatter_text(tmp_path, formatter_text):
    text = formatter_text
    gz, index, st = _build(tmp_path, "a", text)
    assert index == te.expected_bytes(gz)
    assert _check_regions(gz, index, text) > 500
    recs = te.data_lines(text)
    assert (st["files"], st["lines"], st["data_lines"], st["names"], st["ranges"]) == (1, te.count_lines(text), 3000, 3, 1)
    assert st["index_bytes"] == len(index) and st["compressed_bytes"] == os.path.getsize(tmp_path / "a.vcf.gz.tbi")
    parsed = tr.parse_index(index)
    assert st["bins"] == sum(len(b) for b, _l in parsed.values())
    assert st["chunks"] == sum(len(c) for b, _l in parsed.values() for c in b.values())
    assert st["windows"] == sum(len(l) for _b, l in parsed.values())
    assert len(recs) == 3000 and st["pass_ms"] > 0 and st["write_ms"] > 0
    # members of another size: other virtual offsets, the same lines
    gz2, index2, _ = _build(tmp_path, "a997", text, chunk=997, level=1)
    assert index2 == te.expected_bytes(gz2) and index2 != index


@pytest.mark.parametrize("name", ["spans", "cosmic"])
def test_spans_and_the_golden_extract(tmp_path, name):
    text = {"spans": tc.spans, "cosmic": tc.cosmic}[name]()
    for chunk in (0xFF00, 509):
        gz, index, st = _build(tmp_path, "%s%d" % (name, chunk), text, chunk=chunk)
        assert index == te.expected_bytes(gz), chunk
        assert _check_regions(gz, index, text) > 50
    assert st["data_lines"] == len(te.data_lines(text))


def test_small_files_and_300_files_in_one_call(tmp_path):
    texts = list(tc.SMALL.values()) + tc.tiny_files()
    paths = []
    for k, text in enumerate(texts):
        paths.append(str(tmp_path / ("f%03d.vcf.gz" % k)))
        with open(paths[-1], "wb") as f:
            f.write(gw.EOF_MEMBER if k == 1 else gw.bgzf(text, chunk=(0xFF00, 64, 7)[k % 3]))
    st = variant.tabix_build(paths)
    for path, text in zip(paths, texts):
        gz = open(path, "rb").read()
        assert _raw_index(path + ".tbi") == te.expected_bytes(gz), path
    assert st["files"] == len(texts) and st["ranges"] == 1
    assert st["lines"] == sum(te.count_lines(t) for t in texts)
    assert st["data_lines"] == sum(len(te.data_lines(t)) for t in texts)
    empty = _raw_index(paths[1] + ".tbi")
    assert len(empty) == 44 and empty[4:8] == bytes(4)
    # an index that exists: refused without overwrite, the files in front keep theirs
    os.remove(paths[0] + ".tbi")
    before = os.path.getmtime(paths[2] + ".tbi")
    with pytest.raises(_lib.SecedoError) as e:
        variant.tabix_build(paths[:3])
    assert "the index " + paths[1] + ".tbi exists; pass overwrite to replace it" in str(e.value)
    assert os.path.exists(paths[0] + ".tbi") and os.path.getmtime(paths[2] + ".tbi") == before
    assert variant.tabix_build(paths[:3], overwrite=True)["files"] == 3


def test_shrunken_budget_walks_ranges_to_the_same_bytes(tmp_path, formatter_text, monkeypatch):
    text = formatter_text
    gz, whole, _ = _build(tmp_path, "whole", text)
    for budget in (60000, 4099, 64):
        monkeypatch.setenv("SECEDO_TABIX_BATCH_BYTES", str(budget))
        _gz, index, st = _build(tmp_path, "b%d" % budget, text)
        assert st["ranges"] >= 3 and index == whole, budget
    # many files through small ranges: range starts inside files, at file starts and over files without lines
    monkeypatch.setenv("SECEDO_TABIX_BATCH_BYTES", "700")
    texts = [tc.spans()] + tc.tiny_files()[:40] + [tc.cosmic()]
    paths = []
    for k, t in enumerate(texts):
        paths.append(str(tmp_path / ("m%02d.vcf.gz" % k)))
        with open(paths[-1], "wb") as f:
            f.write(gw.bgzf(t, chunk=4096))
    st = variant.tabix_build(paths)
    assert st["ranges"] > 10
    for path in paths:
        assert _raw_index(path + ".tbi") == te.expected_bytes(open(path, "rb").read()), path


# --- 2. the refusals ---------------------------------------------------------------------------------------------

def _message(paths):
    with pytest.raises(_lib.SecedoError) as e:
        variant.tabix_build(paths)
    assert e.value.code == _lib.E_INVALID_ARG
    return str(e.value)


@pytest.mark.parametrize("name", sorted(tc.ERRORS))
def test_refused_lines_name_the_file_and_the_line(tmp_path, name, monkeypatch):
    text, line, words = tc.ERRORS[name]
    good, bad = str(tmp_path / "good.vcf.gz"), str(tmp_path / "bad.vcf.gz")
    for path, t in ((good, tc.SMALL["one-line"]), (bad, text)):
        with open(path, "wb") as f:
            f.write(gw.bgzf(t))
    assert "%s: line %d: %s" % (bad, line, words) in _message([good, bad])
    assert os.path.exists(good + ".tbi") and not os.path.exists(bad + ".tbi")
    # the same line when the file is walked in small ranges
    monkeypatch.setenv("SECEDO_TABIX_BATCH_BYTES", "64")
    os.remove(good + ".tbi")
    assert "%s: line %d: %s" % (bad, line, words) in _message([good, bad])


def test_refused_files(tmp_path):
    text = tc.spans()
    plain, crc, whole = (str(tmp_path / n) for n in ("plain.vcf.gz", "crc.vcf.gz", "whole.vcf.gz"))
    with open(plain, "wb") as f:
        f.write(gzip.compress(text))
    assert plain + ": a gzip file that is not BGZF; decompress it and compress it with bgzip" in _message(plain)
    raw = bytearray(gw.bgzf(text, chunk=8192))
    size = int.from_bytes(raw[16:18], "little") + 1  # member 1's CRC32 field
    size2 = int.from_bytes(raw[size + 16:size + 18], "little") + 1
    raw[size + size2 - 8] ^= 0x01
    with open(crc, "wb") as f:
        f.write(bytes(raw))
    assert crc + ": BGZF block 1: CRC32 mismatch" in _message(crc)
    with open(whole, "wb") as f:
        f.write(gw.bgzf(tc.cosmic_whole()))
    with pytest.raises(te.TabixError) as back:
        te.data_lines(tc.cosmic_whole())
    assert back.value.line > 30
    assert "%s: line %d: chromosome blocks not continuous (1 comes back)" % (whole, back.value.line) in _message(whole)
    with open(str(tmp_path / "text.vcf.gz"), "wb") as f:
        f.write(text)
    assert "not a bgzip-compressed file" in _message(str(tmp_path / "text.vcf.gz"))
    assert "Could not open" in _message(str(tmp_path / "missing.vcf.gz"))
    assert not [n for n in os.listdir(tmp_path) if n.endswith(".tbi")]


@pytest.mark.parametrize("damage", range(len(gw.LISTING_DAMAGE)))
def test_a_file_whose_members_cannot_be_listed(tmp_path, damage):
    name, data, tail = gw.listing_damage(gw.bgzf(tc.spans(), chunk=8192))[damage]
    path = str(tmp_path / (name + ".vcf.gz"))
    with open(path, "wb") as f:
        f.write(data)
    assert _message(path) == gw.ERROR_PREFIX + path + tail
    assert not os.path.exists(path + ".tbi")


def _spanning(n_names):
    """n_names lines, each under its own name and over all 32768 windows"""
    return b"".join(b"n%d\t1\t.\tA\t<DEL>\t.\t.\tEND=%d\n" % (k, 1 << 29) for k in range(n_names))


def test_window_total_is_held_against_a_cap_before_anything_is_emitted(tmp_path, monkeypatch):
    """Every (file, name) starts its windows anew, so few bytes ask for many windows: the total is counted in 64 bits
    and a range past the cap is refused. Under a lowered cap three names pass and four do not; under the real cap
    131073 names, whose 2^32 + 32768 windows would wrap a 32-bit sum to a small number, are refused as well."""
    monkeypatch.setenv("SECEDO_TABIX_MAX_WINDOWS", "100000")
    gz, index, st = _build(tmp_path, "three", _spanning(3))
    assert index == te.expected_bytes(gz) and st["windows"] == 3 * 32768
    four = str(tmp_path / "four.vcf.gz")
    with open(four, "wb") as f:
        f.write(gw.bgzf(_spanning(4)))
    with pytest.raises(_lib.SecedoError) as e:
        variant.tabix_build(four)
    assert e.value.code == _lib.E_LIMIT and four in str(e.value)
    assert "touch 131072 index windows, more than 100000" in str(e.value) and not os.path.exists(four + ".tbi")
    # spread over files of one batch the total is the same
    many = []
    for k in range(4):
        many.append(str(tmp_path / ("one%d.vcf.gz" % k)))
        with open(many[-1], "wb") as f:
            f.write(gw.bgzf(_spanning(1)))
    with pytest.raises(_lib.SecedoError) as e:
        variant.tabix_build(many)
    assert e.value.code == _lib.E_LIMIT
    monkeypatch.delenv("SECEDO_TABIX_MAX_WINDOWS")
    assert variant.tabix_build(four)["windows"] == 4 * 32768
    wrap = str(tmp_path / "wrap.vcf.gz")
    with open(wrap, "wb") as f:
        f.write(gw.bgzf(_spanning(131073), level=1))
    with pytest.raises(_lib.SecedoError) as e:
        variant.tabix_build(wrap)
    assert e.value.code == _lib.E_LIMIT and "touch %d index windows" % (131073 * 32768) in str(e.value)


# --- 3. the writer -----------------------------------------------------------------------------------------------

def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _check_written(tmp_path, name, with_index, without_index):
    """with_index: a directory written under vcf_index="tbi"; without_index: the same call without"""
    a, b = _files(with_index), _files(without_index)
    gz = sorted(n for n in a if n.endswith(".vcf.gz"))
    assert sorted(a) == sorted(list(b) + [n + ".tbi" for n in gz]) and len(gz) >= 2
    st = variant.tabix_stats()
    texts = {}
    for n in gz:
        texts[n] = gzip.decompress(a[n])
        assert vr.strip_date(texts[n].decode()) == vr.strip_date(gzip.decompress(b[n]).decode()), n
    for n in b:
        if not n.endswith(".vcf.gz"):
            assert a[n] == b[n], n
    # the writer's index against the stand-alone route's and the expected bytes
    alone = tmp_path / (name + "_alone")
    alone.mkdir()
    for n in gz:
        (alone / n).write_bytes(a[n])
    st_alone = variant.tabix_build([str(alone / n) for n in gz])
    for n in gz:
        written = _raw_index(os.path.join(with_index, n + ".tbi"))
        assert written == _raw_index(str(alone / n) + ".tbi"), n
        assert written == te.expected_bytes(a[n]), n
    for key in ("files", "lines", "data_lines", "names", "bins", "chunks", "windows", "index_bytes", "compressed_bytes"):
        assert st[key] == st_alone[key], key
    assert st["files"] == len(gz) and st["data_lines"] == sum(len(te.data_lines(t)) for t in texts.values())
    assert st["compressed_bytes"] == sum(len(a[n + ".tbi"]) for n in gz)
    return texts


@pytest.mark.parametrize("kind", ["diploid", "haploid", "mapped"])
def test_writer_on_synthetic_pileups(tmp_path, kind):
    rng = np.random.default_rng(["diploid", "haploid", "mapped"].index(kind) + 31)
    if kind == "mapped":
        fasta, mp, contigs, n_chr = MALE, MALE_MAP, [11, 7, 6], 3
    else:
        contigs = [400, 300, 250, 200]
        fasta, mp, n_chr = _fasta(str(tmp_path / "g.fa"), contigs, kind != "haploid", False, rng), "", 4
    chroms, clusters = _synthetic(rng, 300, 5, contigs, n_chr)
    p = _flat(chroms)
    d_tbi, d_none = str(tmp_path / "tbi"), str(tmp_path / "none")
    variant.variant_calling(p, clusters, fasta, mp, 1e-3, 0.01, d_none, vcf_output="bgzf")
    assert variant.tabix_stats()["files"] == 0
    variant.variant_calling(p, clusters, fasta, mp, 1e-3, 0.01, d_tbi, vcf_output="bgzf", vcf_index="tbi")
    assert variant.get_vcf_index() == "none"  # the keyword was a scoped override
    texts = _check_written(tmp_path, kind, d_tbi, d_none)
    assert sum(len(t) for t in texts.values()) > 1000
    # a query through a written index
    n = max(texts, key=lambda k: len(texts[k]))
    recs = te.data_lines(texts[n])
    reader = tr.Reader(open(os.path.join(d_tbi, n), "rb").read(), _raw_index(os.path.join(d_tbi, n + ".tbi")))
    for name, beg, end, _off, _line in recs[::7]:
        assert reader.query(name, beg, end) == te.overlapping(texts[n], name, beg, end, recs=recs)


def test_writer_on_the_clone_tree_host_and_resident(tmp_path):
    n = 300
    p0, truth = clone_tree(n, n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)
    p = FlatPileup(p0.chr_locus_off, p0.locus_pos + 1, p0.locus_entry_off, p0.read_ids, p0.id_base)
    fasta = str(tmp_path / "tree.fa")
    with open(fasta, "w") as f:
        f.write(">chr1\n" + _wrap("A" * p.n_loci) + "\n")
    clusters = (truth % 3).astype(np.uint16)
    d_tbi, d_none, d_res = (str(tmp_path / k) for k in ("tbi", "none", "resident"))
    variant.variant_calling(p, clusters, fasta, "", 1e-3, 0.01, d_none, vcf_output="bgzf")
    variant.variant_calling(p, clusters, fasta, "", 1e-3, 0.01, d_tbi, vcf_output="bgzf", vcf_index="tbi")
    texts = _check_written(tmp_path, "host", d_tbi, d_none)
    assert sum(len(t) for t in texts.values()) > 1000
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, np.arange(n, dtype=np.uint32), n)
        secedo_amd.variant_calling_resident(plan, res, clusters, fasta, "", 1e-3, 0.01, d_res, vcf_output="bgzf",
                                            vcf_index="tbi")
    _check_written(tmp_path, "resident", d_res, d_none)


def test_tbi_with_plain_output_raises_and_the_setting_routes_a_call(tmp_path):
    p = _flat([[(1, [i << 2 for i in range(10)])]])
    with pytest.raises(_lib.SecedoError) as e:
        variant.variant_calling(p, [1] * 10, FEMALE, "", 1e-3, 1e-3, str(tmp_path / "x"), vcf_index="tbi")
    assert e.value.code == _lib.E_INVALID_ARG and "add --vcf_output bgzf" in str(e.value)
    assert not [n for n in os.listdir(tmp_path / "x") if n.endswith(".vcf") or n.endswith(".tbi")]
    variant.set_vcf_index("tbi")
    try:
        variant.variant_calling(p, [1] * 10, FEMALE, "", 1e-3, 1e-3, str(tmp_path / "a"), vcf_output="bgzf")
    finally:
        variant.set_vcf_index("none")
    assert sorted(os.listdir(tmp_path / "a")) == [
        "cluster_0.vcf.gz", "cluster_0.vcf.gz.tbi", "cluster_1.vcf.gz", "cluster_1.vcf.gz.tbi", "common.vcf.gz",
        "common.vcf.gz.tbi", "scores", "variant"]
    for n in ("cluster_0", "cluster_1", "common"):
        gz = (tmp_path / "a" / (n + ".vcf.gz")).read_bytes()
        assert _raw_index(str(tmp_path / "a" / (n + ".vcf.gz.tbi"))) == te.expected_bytes(gz)


def test_writer_with_one_member_per_slice(tmp_path, monkeypatch):
    """The two-cluster call above with SECEDO_BGZF_SLICE_MEMBERS=1: every file border of the .vcf.gz files and of the
    index bodies is a slice border of the encoder's driver. The preamble holds the time to the second, so the pair of
    calls is made again should the second have changed between them."""
    p = _flat([[(1, [i << 2 for i in range(10)])]])
    for attempt in range(3):
        dirs = [tmp_path / ("%s%d" % (k, attempt)) for k in ("unset", "one")]
        variant.variant_calling(p, [1] * 10, FEMALE, "", 1e-3, 1e-3, str(dirs[0]), vcf_output="bgzf", vcf_index="tbi")
        with monkeypatch.context() as env:
            env.setenv("SECEDO_BGZF_SLICE_MEMBERS", "1")
            variant.variant_calling(p, [1] * 10, FEMALE, "", 1e-3, 1e-3, str(dirs[1]), vcf_output="bgzf",
                                    vcf_index="tbi")
        unset, one = _files(dirs[0]), _files(dirs[1])
        if all(unset[n] == one[n] for n in ("cluster_0.vcf.gz", "cluster_1.vcf.gz")):
            break
    assert sorted(one) == sorted(unset) and len([n for n in one if n.endswith(".tbi")]) == 3
    for n in ("cluster_0", "cluster_1", "common"):
        gz = one[n + ".vcf.gz"]
        assert gz == unset[n + ".vcf.gz"] and one[n + ".vcf.gz.tbi"] == unset[n + ".vcf.gz.tbi"], n
        assert _raw_index(str(dirs[1] / (n + ".vcf.gz.tbi"))) == te.expected_bytes(gz), n


# --- 4. the command lines ----------------------------------------------------------------------------------------

def test_cli_writes_the_index_files(tmp_path, capsys):
    d = tmp_path / "ten"
    d.mkdir()
    shutil.copy(os.path.join(DATA, "ten_rows.pileup.bin"), d / "s_22.pileup.bin")
    flags = ["-i", str(d), "--chromosomes=22", "--reference_genome=" + os.path.join(DATA, "genome_diploid_female.fa")]
    a, b = str(tmp_path / "tbi") + "/", str(tmp_path / "later") + "/"
    assert secedo_main.main(flags + ["-o", a, "--vcf_output", "bgzf", "--vcf_index", "tbi"]) == 0
    assert "tbi_pass_ms" in capsys.readouterr().out
    assert secedo_main.main(flags + ["-o", b, "--vcf_output", "bgzf"]) == 0
    assert "tbi" not in capsys.readouterr().out.split("times:")[1]
    gz = sorted(n for n in os.listdir(a) if n.endswith(".vcf.gz"))
    assert "common.vcf.gz" in gz and "cluster_0.vcf.gz" in gz
    assert not [n for n in os.listdir(b) if n.endswith(".tbi")]
    # the files written without an index get theirs from tabix_main
    assert tabix_main.main(["-i", b]) == 0
    for n in gz:
        assert _raw_index(a + n + ".tbi") == te.expected_bytes(open(a + n, "rb").read())
        assert _raw_index(b + n + ".tbi") == te.expected_bytes(open(b + n, "rb").read())
    with pytest.raises(SystemExit):
        tabix_main.main(["-i", b])
    assert tabix_main.main(["-i", b, "--overwrite"]) == 0
    assert secedo_main.main(flags + ["-o", a, "--vcf_index", "tbi"]) == 1
