"""``secedo_amd.genome_bins`` on the GPU against tests/gc_expected.py: every fetched array and every byte of the file,
over the input forms and range sizes of the device route, the line rule's quirks, random texts, the kernel's and the
host's edges, the selection and its refusals (by code and wording), both outputs, and the join with ``bin_depth``."""
import gzip
import os

import numpy as np
import pytest

import secedo_amd
from tests import bam_writer as bw
from tests import depth_expected as de
from tests import fasta_cases as fc
from tests import gc_expected as ge
from tests import split_expected as se

pytestmark = pytest.mark.gpu

FORMS = ("plain", "bgzf37", "bgzf", "gzip1")
KIND_OF = dict(plain="text", bgzf37="bgzf", bgzf="bgzf", gzip1="gzip")
BIN_SIZES = (1, 7, 16, 60, 61, 64, 1000)


def check(out, e, text=None):
    """The fetched arrays and the stats against the expected ones."""
    assert out["names"] == e.names
    assert out["contig_lengths"].dtype == np.uint64 and out["contig_lengths"].tolist() == e.contig_lengths
    bins = np.array(e.bins, np.int64).reshape(-1, 3)
    assert np.array_equal(out["bin_contig"], bins[:, 0]) and np.array_equal(out["bin_start"], bins[:, 1])
    assert np.array_equal(out["bin_end"], bins[:, 2])
    assert out["counts"].dtype == np.uint32 and out["counts"].shape == (len(e.bins), 6)
    assert np.array_equal(out["counts"], e.counts)
    assert np.array_equal(out["counts"][:, :5].sum(axis=1), bins[:, 2] - bins[:, 1])
    st = out["stats"]
    assert st == secedo_amd.genome_bins_stats()
    assert (st["contigs"], st["selected"], st["duplicate_names"], st["bins"], st["bases"]) == (
        e.contigs, len(e.names), e.duplicate_names, len(e.bins), sum(e.contig_lengths))
    if text is not None:
        assert st["fasta_bytes"] == len(text)


def read_file(path, bgzf):
    """The file's text; under BGZF every member within the cut and the EOF member present."""
    raw = open(str(path) + (".gz" if bgzf else ""), "rb").read()
    assert os.path.exists(str(path)) != bgzf
    if not bgzf:
        return raw
    assert raw.endswith(se.EOF) and all(isize <= se.CUT for isize, _ in se.member_sizes(raw))
    return gzip.decompress(raw)  # every CRC32 and ISIZE


def no_tmp(directory):
    return not [n for n in os.listdir(str(directory)) if ".tmp." in n]


def refused(e, *args, **kw):
    """The call must fail with the code and the words of ``e`` (a ge.Refused)."""
    with pytest.raises(secedo_amd.SecedoError) as r:
        secedo_amd.genome_bins(*args, **kw)
    assert r.value.code == e.code
    assert str(r.value) == "secedo_simmat error %d: %s" % (e.code, e.message)


def expect_refused(text, S, path, **kw):
    with pytest.raises(ge.Refused) as r:
        ge.expected(text, S, path=str(path), **kw)
    return r.value


@pytest.fixture
def batch(monkeypatch):
    def set_batch(value):
        if value is None:
            monkeypatch.delenv("SECEDO_FASTA_BATCH_BYTES", raising=False)
        else:
            monkeypatch.setenv("SECEDO_FASTA_BATCH_BYTES", str(value))
    return set_batch


@pytest.fixture(scope="module")
def kind_texts():
    rng = np.random.default_rng(31)
    return {kind: fc.kind_text(kind, rng) for kind in fc.KINDS}


@pytest.mark.parametrize("batch_bytes", [64, 4096, None])
@pytest.mark.parametrize("form", FORMS)
def test_kinds_by_form_and_range(tmp_path, kind_texts, batch, form, batch_bytes):
    batch(batch_bytes)
    for kind, text in kind_texts.items():
        path = fc.write_form(tmp_path / (kind + ".fa"), text, form)
        for S in BIN_SIZES:
            e = ge.expected(text, S)
            assert len(e.names) == (4 if kind == "haploid" else 6 if kind == "male" else 8)
            out = secedo_amd.genome_bins(path, S)
            check(out, e, text)
            st = out["stats"]
            assert st["kind"] == KIND_OF[form] and (st["device_members"] > 0) == form.startswith("bgzf")
            if batch_bytes == 64 and form != "bgzf":
                assert st["ranges"] >= len(text) // 64  # bins, chunks and headers straddle ranges
            if batch_bytes is None:
                assert st["ranges"] == 1


@pytest.mark.parametrize("batch_bytes", [64, None])
def test_quirks(tmp_path, batch, batch_bytes):
    batch(batch_bytes)
    for name, text in fc.QUIRKS.items():
        for form in ("plain", "bgzf37"):
            path = fc.write_form(tmp_path / (name + form), text, form)
            for S in (1, 3, 1000):
                if not text:
                    refused(expect_refused(text, S, path), path, S)
                else:
                    check(secedo_amd.genome_bins(path, S), ge.expected(text, S), text)


def test_random_texts(tmp_path, batch):
    rng = np.random.default_rng(2031)
    seen_dup = seen_gt = seen_multi = 0
    for i in range(200):
        text = fc.random_text(rng)
        form = ("plain", "bgzf37")[i % 2]
        batch((64, None)[(i // 2) % 2])
        path = fc.write_form(tmp_path / ("r%d" % i), text, form)
        for S in (1, 3):
            if not text:
                refused(expect_refused(text, S, path), path, S)
                continue
            e = ge.expected(text, S)
            seen_dup += e.duplicate_names > 0
            seen_gt += any(b">" in s for _, s in ge.contigs_of(text))
            seen_multi += e.contigs > 1
            check(secedo_amd.genome_bins(path, S), e, text)
    assert seen_dup >= 1 and seen_gt > 10 and seen_multi > 10  # the texts reach the rules they are here for


def seq_of(rng, n, alphabet=b"ACGTacgtNn"):
    return bytes(alphabet[i] for i in rng.integers(0, len(alphabet), n))


@pytest.mark.parametrize("width", [0, 60])
def test_one_long_contig(tmp_path, batch, width):
    batch(None)
    rng = np.random.default_rng(5)
    seq = seq_of(rng, 3 * 4096 + 5)
    body = seq if not width else b"\n".join(seq[i:i + width] for i in range(0, len(seq), width))
    text = b">long one\n" + body + b"\n"
    for form in ("plain", "bgzf"):
        path = fc.write_form(tmp_path / ("long" + form), text, form)
        for S in (16, 1024, 4096, 4097):
            e = ge.expected(text, S)
            assert e.contig_lengths == [3 * 4096 + 5] and len(e.bins) == -(-len(seq) // S)
            check(secedo_amd.genome_bins(path, S), e, text)


def test_wave_edges_and_classes(tmp_path, batch):
    batch(None)
    rng = np.random.default_rng(6)
    text = b"".join(b">c%d\n%s\n" % (n, seq_of(rng, n)) for n in (1023, 1024, 1025))
    text += b">lower\n" + seq_of(rng, 700, b"acgtn") + b"\n>allN\n" + b"N" * 333 + b"\n>rna\nACGUacguUUuu\n"
    path = fc.write_form(tmp_path / "edges.fa", text, "plain")
    for S in (1, 16, 64, 1000, 1024, 100000):
        e = ge.expected(text, S)
        check(secedo_amd.genome_bins(path, S), e, text)
    e = ge.expected(text, 100000)
    rows = dict(zip(e.names, e.counts.tolist()))
    assert rows["lower"][5] == 700 and rows["allN"] == [0, 0, 0, 0, 333, 0] and rows["rna"] == [2, 2, 2, 6, 0, 6]


def test_many_tiny_contigs_overflow_the_slots(tmp_path, batch):
    batch(None)
    rng = np.random.default_rng(7)
    text = b"".join(b">t%d some words\n%s\n" % (k, seq_of(rng, 1 + k % 5)) for k in range(300))
    for form in ("plain", "bgzf"):
        path = fc.write_form(tmp_path / ("tiny" + form), text, form)
        out = secedo_amd.genome_bins(path, 2)
        e = ge.expected(text, 2)
        assert out["stats"]["ranges"] == 1 and e.contigs == 300 and e.names[299] == "t299"
        check(out, e, text)
    # and a subset of them out of order
    pick = ["t299", "t0", "t150"]
    check(secedo_amd.genome_bins(path, 2, contigs=pick), ge.expected(text, 2, contigs=pick), text)


def test_headers_across_ranges_and_long_names(tmp_path, batch):
    batch(64)
    rng = np.random.default_rng(8)
    long_header = b">" + b"h" * 40 + b" " + b"d" * 58  # 100 bytes
    text = b">a\n" + seq_of(rng, 50) + b"\n" + long_header + b"\n" + seq_of(rng, 90) + b"\n>" + b"k" * 99 + b"\nAC"
    for form in ("plain", "bgzf37", "gzip1"):
        path = fc.write_form(tmp_path / ("hdr" + form), text, form)
        e = ge.expected(text, 7)
        assert e.names == ["a", "h" * 40, "k" * 99] and len(long_header) == 100
        check(secedo_amd.genome_bins(path, 7), e, text)
    ok = b">" + b"n" * 4096 + b" rest\nACGT\n"
    bad = b">first\nAC\n>" + b"n" * 4097 + b"\nACGT\n"
    for b in (64, None):
        batch(b)
        for form in ("plain", "bgzf"):
            path = fc.write_form(tmp_path / ("name%s%s" % (form, b)), ok, form)
            check(secedo_amd.genome_bins(path, 3), ge.expected(ok, 3), ok)
            path = fc.write_form(tmp_path / ("bad%s%s" % (form, b)), bad, form)
            e = expect_refused(bad, 3, path)
            assert e.message.endswith("contig 1: its name is longer than 4096 bytes")
            refused(e, path, 3)


def test_duplicate_names(tmp_path, batch):
    batch(None)
    text = b">x one\nACGT\n>y\nGG\n>x two\nTTTTTT\n>y\nA\n>z\nCC\n"
    path = fc.write_form(tmp_path / "dup.fa", text, "plain")
    e = ge.expected(text, 4)
    assert e.names == ["x", "y", "z"] and e.duplicate_names == 2 and e.contig_lengths == [4, 2, 2]
    check(secedo_amd.genome_bins(path, 4), e, text)
    e = ge.expected(text, 4, contigs=["z", "x"], lengths=[2, 4])
    check(secedo_amd.genome_bins(path, 4, contigs=["z", "x"], lengths=[2, 4]), e, text)


def test_selection_and_refusals(tmp_path, kind_texts, batch):
    batch(4096)
    text = kind_texts["haploid"]
    path = fc.write_form(tmp_path / "sel.fa", text, "bgzf")
    names = ["chr4", "chr3", "chr2", "chr1"]
    e = ge.expected(text, 64, contigs=names, lengths=[200, 250, 300, 400])
    assert e.names == names and [b[0] for b in e.bins] == sorted(b[0] for b in e.bins)
    check(secedo_amd.genome_bins(path, 64, contigs=names, lengths=[200, 250, 300, 400]), e, text)
    check(secedo_amd.genome_bins(path, 64, contigs=["chr3", "chr1"]), ge.expected(text, 64, contigs=["chr3", "chr1"]),
          text)
    for kw in (dict(contigs=["chr1", "3"]), dict(contigs=["chr2", "chr2"]), dict(contigs=[]),
               dict(contigs=["chr2", "chr1"], lengths=[300, 401])):
        e = expect_refused(text, 64, path, **kw)
        refused(e, path, 64, **kw)
    assert "no chr prefix" in expect_refused(text, 64, path, contigs=["1"]).message
    assert expect_refused(text, 64, path, contigs=["chr1"], lengths=[9]).message == \
        "chr1: the genome has 400 bases, expected 9"
    refused(expect_refused(text, 0, path), path, 0)
    for form in ("plain", "bgzf", "gzip1"):
        empty = fc.write_form(tmp_path / ("empty" + form), b"", form)
        refused(expect_refused(b"", 64, empty), empty, 64)
    with pytest.raises(secedo_amd.SecedoError) as r:
        secedo_amd.genome_bins(tmp_path / "missing.fa", 64)
    assert r.value.code == ge.INVALID_ARG and "does not exist" in str(r.value)
    # a failed call leaves no result to fetch and no file
    out_path = tmp_path / "never.tsv"
    with pytest.raises(secedo_amd.SecedoError):
        secedo_amd.genome_bins(path, 64, contigs=["nope"], out_path=out_path)
    assert not os.path.exists(str(out_path)) and no_tmp(tmp_path)


@pytest.mark.parametrize("output", ["plain", "bgzf"])
def test_output_file(tmp_path, kind_texts, batch, monkeypatch, output):
    batch(None)
    bgzf = output == "bgzf"
    text = kind_texts["male"]
    path = fc.write_form(tmp_path / "g.fa", text, "bgzf")
    e = ge.expected(text, 7)
    assert len(e.bins) > 200
    target = tmp_path / "out.tsv"
    out = secedo_amd.genome_bins(path, 7, out_path=target, output=output)
    check(out, e, text)
    assert read_file(target, bgzf) == e.file and no_tmp(tmp_path)
    st = out["stats"]
    assert st["text_bytes"] == len(e.file) and st["output"] == output
    assert (st["compressed_bytes"] > 0, st["members"] > 0) == (bgzf, bgzf)
    first = open(str(target) + (".gz" if bgzf else ""), "rb").read()
    # an existing file is refused, and left as it is; with overwrite it is replaced by the same bytes
    with pytest.raises(secedo_amd.SecedoError) as r:
        secedo_amd.genome_bins(path, 7, out_path=target, output=output)
    assert r.value.code == ge.INVALID_ARG and "exists; pass overwrite to replace it" in str(r.value)
    assert open(str(target) + (".gz" if bgzf else ""), "rb").read() == first and no_tmp(tmp_path)
    secedo_amd.genome_bins(path, 7, out_path=target, output=output, overwrite=True)
    assert open(str(target) + (".gz" if bgzf else ""), "rb").read() == first  # two runs, identical bytes
    # small text ranges and small encoder slices: no byte of text changes
    monkeypatch.setenv("SECEDO_GENOME_BINS_BATCH_BYTES", "1")
    monkeypatch.setenv("SECEDO_BGZF_SLICE_MEMBERS", "2")
    small = tmp_path / "small.tsv"
    secedo_amd.genome_bins(path, 7, out_path=small, output=output)
    assert read_file(small, bgzf) == e.file
    assert secedo_amd.genome_bins_stats()["members"] == (len(e.bins) + 1 if bgzf else 0)
    monkeypatch.setenv("SECEDO_GENOME_BINS_BATCH_BYTES", "1000")
    mid = tmp_path / "mid.tsv"
    secedo_amd.genome_bins(path, 7, contigs=["Y_paternal", "1_maternal"], out_path=mid, output=output)
    assert read_file(mid, bgzf) == ge.expected(text, 7, contigs=["Y_paternal", "1_maternal"]).file and no_tmp(tmp_path)
    # a target whose directory is missing: refused, nothing left
    with pytest.raises(secedo_amd.SecedoError):
        secedo_amd.genome_bins(path, 7, out_path=tmp_path / "nowhere" / "x.tsv", output=output)
    assert no_tmp(tmp_path)


# ---- bin_depth(reference_genome=...)

REFS = [("chr1", 5000), ("chr2", 3000), ("chrM", 777), ("chrX", 1234)]


def depth_record(k, ref_id, pos):
    return bw.Rec(name="r%04d" % k, ref=ref_id, pos=pos, cigar=[("M", 10)], seq="ACGTACGTAC", qual=[30] * 10, flag=0,
                  mapq=60)


@pytest.fixture(scope="module")
def depth_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gc_depth")
    rng = np.random.default_rng(9)
    cells = [[depth_record(10 * c + k, r, int(p)) for k, (r, p) in enumerate(
        sorted((int(r), int(rng.integers(0, REFS[int(r)][1] - 10))) for r in rng.integers(0, 4, 8)))] for c in range(3)]
    paths = []
    for c, recs in enumerate(cells):
        paths.append(os.path.join(str(d), "cell_%d.bam" % c))
        bw.write_bam(paths[-1], REFS, recs)
    seqs = {name: seq_of(rng, ln) for name, ln in REFS}
    order = ["chrX", "chr1", "extra", "chr2", "chrM"]  # the genome's own order, with a contig the BAMs do not have
    seqs["extra"] = seq_of(rng, 99)
    text = b"".join(b">%s desc\n%s\n" % (n.encode(), fc.wrap(seqs[n].decode(), 70).encode()) for n in order)
    genome = fc.write_form(os.path.join(str(d), "genome.fa.gz"), text, "bgzf")
    return dict(dir=d, cells=cells, paths=paths, text=text, genome=genome,
                names=[de.default_name(p) for p in paths])


@pytest.mark.parametrize("output", ["plain", "bgzf"])
def test_bin_depth_with_a_genome(depth_case, tmp_path, output):
    bgzf = output == "bgzf"
    chroms, S = [3, 0, 1], 700  # a subset, out of order: the bins run in ascending id
    ed = de.expected(depth_case["cells"], REFS, S, chroms, names=depth_case["names"])
    eg = ge.expected(depth_case["text"], S, contigs=["chr1", "chr2", "chrX"], lengths=[5000, 3000, 1234])
    got = secedo_amd.bin_depth(depth_case["paths"], S, chroms, out_dir=tmp_path, output=output,
                               reference_genome=depth_case["genome"])
    assert got["gc"].dtype == np.uint32 and np.array_equal(got["gc"], eg.counts)
    assert len(got["bin_start"]) == len(eg.bins) == 8 + 5 + 2
    assert np.array_equal(got["bin_start"], [b[1] for b in eg.bins])
    assert np.array_equal(got["bin_end"], [b[2] for b in eg.bins])
    assert [REFS[c][0] for c in got["bin_chrom"]] == [eg.names[b[0]] for b in eg.bins]
    text = read_file(tmp_path / "depth" / "depth.gc.tsv", bgzf)
    assert text == eg.file
    bed = open(str(tmp_path / "depth" / "depth.bins.bed"), "rb").read()
    assert bed == ed.files["depth.bins.bed"]
    assert [b"\t".join(l.split(b"\t")[:3]) for l in text.splitlines()[1:]] == bed.splitlines()
    assert sorted(os.listdir(str(tmp_path / "depth"))) == sorted(
        [n + (".gz" if bgzf and n in de.GZ_FILES else "") for n in ed.files] + ["depth.gc.tsv" + (".gz" if bgzf else "")])
    # an existing depth.gc.tsv is refused before anything runs
    before = {n: os.path.getmtime(str(tmp_path / "depth" / n)) for n in os.listdir(str(tmp_path / "depth"))}
    with pytest.raises(secedo_amd.SecedoError) as r:
        secedo_amd.bin_depth(depth_case["paths"], S, chroms, out_dir=tmp_path, output=output,
                             reference_genome=depth_case["genome"])
    assert "exists; pass overwrite" in str(r.value)
    assert before == {n: os.path.getmtime(str(tmp_path / "depth" / n)) for n in os.listdir(str(tmp_path / "depth"))}
    # without an out_dir the result still has gc
    got = secedo_amd.bin_depth(depth_case["paths"], S, chroms, reference_genome=depth_case["genome"])
    assert np.array_equal(got["gc"], eg.counts)


def test_bin_depth_refuses_a_wrong_genome(depth_case, tmp_path):
    text = depth_case["text"]
    short = text.replace(b">chr2 desc\n", b">chr2 desc\nA", 1)  # chr2 one base longer
    renamed = text.replace(b">chr2 ", b">2 ", 1)
    for name, wrong, words in (("short", short, "chr2: the genome has 3001 bases, expected 3000"),
                               ("renamed", renamed, "no contig named 'chr2' (names are matched exactly")):
        genome = fc.write_form(tmp_path / (name + ".fa"), wrong, "plain")
        out = tmp_path / (name + "_out")
        out.mkdir()
        with pytest.raises(secedo_amd.SecedoError) as r:
            secedo_amd.bin_depth(depth_case["paths"], 700, [0, 1], out_dir=out, reference_genome=genome)
        assert r.value.code == ge.INVALID_ARG and words in str(r.value) and "BAM header" in str(r.value)
        assert os.listdir(str(out)) == []  # no depth/ left behind
    # a depth/ that was there before stays, without this call's files
    out = tmp_path / "kept"
    (out / "depth").mkdir(parents=True)
    (out / "depth" / "notes.txt").write_text("mine")
    with pytest.raises(secedo_amd.SecedoError):
        secedo_amd.bin_depth(depth_case["paths"], 700, [0, 1], out_dir=out, reference_genome=genome)
    assert os.listdir(str(out / "depth")) == ["notes.txt"]


def test_bin_depth_without_a_genome_is_as_before(depth_case, tmp_path):
    ed = de.expected(depth_case["cells"], REFS, 700, [0, 2], names=depth_case["names"])
    got = secedo_amd.bin_depth(depth_case["paths"], 700, [0, 2], out_dir=tmp_path)
    assert "gc" not in got and sorted(os.listdir(str(tmp_path / "depth"))) == sorted(ed.files)
    for name, want in ed.files.items():
        assert open(str(tmp_path / "depth" / name), "rb").read() == want
    names, ln = secedo_amd.bam_pileup.depth_chromosomes()
    assert names == ["chr1", "chrM"] and ln.tolist() == [5000, 777]
