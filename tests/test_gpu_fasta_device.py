"""The device route of the reference genome (include/secedo_variant.h, fasta_kernels.hip): the FASTA parsed and the
per-locus reference genotypes gathered in HBM, from plain text, plain gzip and BGZF (inflated on the GPU). The
yardstick is always the host route of the same build on the plain file, which test_variant_cpu.py and
test_gpu_variant.py pin to the restatement; every comparison is exact, errors are compared as errors, word for word."""
import os

import numpy as np
import pytest

import secedo_amd
from secedo_amd import _lib, secedo_main, variant
from tests import bgzf_writer
from tests import fasta_cases as fc
from tests import variant_ref as vr
from tests.clone_tree_gen import clone_tree
from tests.pileup_file_writer import clone_tree_files

pytestmark = pytest.mark.gpu

FORMS = ("plain", "bgzf37", "bgzf", "gzip1")
BATCHES = ("64", "4096", "")  # "": the default, one range


def _set_batch(monkeypatch, batch):
    if batch:
        monkeypatch.setenv("SECEDO_FASTA_BATCH_BYTES", str(batch))
    else:
        monkeypatch.delenv("SECEDO_FASTA_BATCH_BYTES", raising=False)


def _outcome(path, off, pos, device, map_file="", where=None):
    """(locus_ref, chr_locus_end) as lists, or ("error", code, message with the file's directory taken out)."""
    try:
        if device:
            with variant._route("device"):
                ref, end = variant.reference_genotypes(path, off, pos, map_file, device=0)
        else:
            ref, end = variant.reference_genotypes(path, off, pos, map_file)
    except _lib.SecedoError as e:
        return ("error", e.code, str(e).replace(where or os.path.dirname(path), "<dir>"))
    return ref.tolist(), end.tolist()


def _write(tmp_path, text, form):
    d = tmp_path / form
    d.mkdir(exist_ok=True)
    return fc.write_form(d / "g.fa", text, form)


# --- device against host, every kind and form -------------------------------------------------------------------

@pytest.fixture(scope="module")
def kinds(tmp_path_factory):
    """kind -> (text, off, pos, the host route's outcome on the plain file)"""
    root = tmp_path_factory.mktemp("kinds")
    out = {}
    for i, kind in enumerate(fc.KINDS):
        rng = np.random.default_rng(300 + i)
        text = fc.kind_text(kind, rng)
        off, pos = fc.kind_loci(rng, kind)
        (root / kind).mkdir()
        out[kind] = (text, off, pos, _outcome(_write(root / kind, text, "plain"), off, pos, False))
    return out


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", fc.KINDS)
def test_device_equals_host(tmp_path, monkeypatch, kinds, kind, form, batch):
    text, off, pos, want = kinds[kind]
    _set_batch(monkeypatch, batch)
    got = _outcome(_write(tmp_path, text, form), off, pos, True)
    assert got == want and want[0] != "error"
    st = variant.fasta_stats()
    assert st["route"] == "device" and st["text_bytes"] == len(text) and st["fell_back_for_map"] == 0
    assert st["kind"] == {"plain": "text", "gzip1": "gzip"}.get(form, "bgzf")
    assert st["contigs"] == text.count(b">") and 0 < st["contigs_used"] <= st["contigs"]
    if not form.startswith("bgzf"):
        assert st["ranges"] == -(-len(text) // int(batch or 1 << 28)) and st["uploaded_bytes"] == len(text)
        assert st["device_members"] == 0


def test_the_setting_decides_for_text_and_bgzf_goes_to_the_device_anyway(tmp_path, kinds):
    text, off, pos, want = kinds["male"]
    plain, bg = _write(tmp_path, text, "plain"), _write(tmp_path, text, "bgzf37")
    with variant._route("host"):
        assert variant.reference_genotypes(plain, off, pos, device=0)[0].tolist() == want[0]
        assert variant.fasta_stats()["route"] == "host"
        assert variant.reference_genotypes(bg, off, pos, device=0)[0].tolist() == want[0]
        st = variant.fasta_stats()
    assert st["route"] == "device" and st["kind"] == "bgzf"
    assert st["device_members"] == -(-len(text) // 37) + 1  # and the end-of-file member
    assert st["host_inflated_bytes"] == 37  # the member that holds the first word, for the diploid test
    assert st["uploaded_bytes"] < os.path.getsize(bg)


# --- the quirks of the reference's stream calls ------------------------------------------------------------------

@pytest.mark.parametrize("batch", ("64", ""))
@pytest.mark.parametrize("form", ("plain", "bgzf37"))
@pytest.mark.parametrize("name", sorted(fc.QUIRKS))
def test_quirk_texts(tmp_path, monkeypatch, name, form, batch):
    text = fc.QUIRKS[name]
    off, pos = fc.quirk_loci(text)
    want = _outcome(_write(tmp_path, text, "plain"), off, pos, False)
    _set_batch(monkeypatch, batch)
    assert _outcome(_write(tmp_path, text, form), off, pos, True) == want
    assert variant.fasta_stats()["route"] == "device"
    if name in ("missing_paternal", "lengths_differ_by_one", "newline"):
        assert want[0] == "error"
    if name == "lengths_differ_by_one":
        assert want[2].endswith("Maternal and paternal chromosome sizes don't match (5 vs 4)")


@pytest.mark.parametrize("at", (64, 63, 62, 65, 128, 127))
@pytest.mark.parametrize("second", (b"Y_paternal", b"X_paternal", b""))
def test_a_header_at_a_range_edge(tmp_path, monkeypatch, at, second):
    """The second header's '>' is byte `at` of the text and ranges are 64 bytes: the first byte of a range, the last
    one (its byte 1, which decides whether X was a whole chromosome, in the next range), or one before."""
    first = b">X_maternal\n"
    text = first + b"ACGT" * 40
    text = text[:at - 1] + b"\n>" + second + b"\nGGTCA\n"
    assert text[at] == ord(">") and text[at - 1] == ord("\n")
    n = at - 1 - len(first)
    off = np.asarray([0, 6, 12], dtype=np.uint32)
    pos = np.asarray([1, 2, n, n + 1, 5, 6, 1, 2, 3, 5, 6, 0], dtype=np.uint32)
    want = _outcome(_write(tmp_path, text, "plain"), off, pos, False)
    monkeypatch.setenv("SECEDO_FASTA_BATCH_BYTES", "64")
    assert _outcome(_write(tmp_path, text, "plain"), off, pos, True) == want
    assert (want[0] == "error") == (second != b"Y_paternal")  # X then Y: haploid; else the lengths differ


# --- random texts -------------------------------------------------------------------------------------------------

def test_random_texts(tmp_path, monkeypatch):
    rng = np.random.default_rng(77)
    monkeypatch.setenv("SECEDO_FASTA_BATCH_BYTES", "64")
    path = str(tmp_path / "g.fa")
    errors = calls = 0
    for i in range(300):
        text = fc.random_text(rng, 2048 if i % 6 == 0 else 200) if i % 4 else fc.random_diploid_text(rng)
        with open(path, "wb") as f:
            f.write(text)
        for _ in range(5):
            off, pos = fc.random_loci(rng, max_pos=max(8, min(len(text), 300)))
            want = _outcome(path, off, pos, False)
            assert _outcome(path, off, pos, True) == want, (text, off, pos)
            errors += want[0] == "error"
            calls += 1
    assert 0 < errors <= calls // 4, (errors, calls)


# --- one larger case ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def large(tmp_path_factory):
    root = tmp_path_factory.mktemp("large")
    rng = np.random.default_rng(9)
    contigs = (200_000,) * 24  # 24 diploid chromosomes, a contig pair each: about 10 MB of text
    text = fc.kind_text("diploid", rng, contigs)
    off = np.append(np.arange(24, dtype=np.uint32) * 2084, 50_000).astype(np.uint32)
    pos = rng.integers(1, 200_001, 50_000).astype(np.uint32)
    pos[[10, 20_000, 49_999]] = [0, 200_001, 0xFFFFFFFF]
    paths = {form: fc.write_form(root / ("g_%s.fa" % form), text, form) for form in ("plain", "bgzf")}
    return text, off, pos, paths, _outcome(paths["plain"], off, pos, False, where=str(root))


@pytest.mark.parametrize("batch", (str(1 << 20), ""))
@pytest.mark.parametrize("form", ("plain", "bgzf"))
def test_a_larger_genome(monkeypatch, large, form, batch):
    text, off, pos, paths, want = large
    _set_batch(monkeypatch, batch)
    got = _outcome(paths[form], off, pos, True)
    assert want[0] != "error" and got == want
    st = variant.fasta_stats()
    assert st["text_bytes"] == len(text) and st["contigs"] == 48 and st["contigs_used"] == 48
    if form == "plain":
        assert st["ranges"] == -(-len(text) // int(batch or 1 << 28))
    else:
        assert st["device_members"] == -(-len(text) // 0xFF00) + 1 and st["host_inflated_bytes"] == 0xFF00
        assert st["ranges"] == (1 if not batch else -(-(st["device_members"] - 1) // ((1 << 20) // 0xFF00)))


# --- the map file, and errors -------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ("plain", "bgzf37"))
def test_a_map_file_sends_the_call_to_the_host_route(tmp_path, form):
    with open(fc.MALE, "rb") as f:
        text = f.read()
    off = np.asarray([0, 12, 20, 27], dtype=np.uint32)
    pos = np.asarray(list(range(1, 13)) + list(range(1, 9)) + list(range(1, 8)), dtype=np.uint32)
    want = _outcome(fc.MALE, off, pos, False, fc.MALE_MAP, where=fc.DATA)
    unmapped = _outcome(fc.MALE, off, pos, False, where=fc.DATA)
    assert want[0] != "error" and want != unmapped
    assert _outcome(_write(tmp_path, text, form), off, pos, True, fc.MALE_MAP) == want
    st = variant.fasta_stats()
    assert st["fell_back_for_map"] == 1 and st["route"] == "host"
    if form == "bgzf37":  # inflated on the GPU, downloaded
        assert st["device_members"] == -(-len(text) // 37) + 1 and st["host_inflated_bytes"] == 0


@pytest.mark.parametrize("batch", ("64", ""))
def test_corrupt_members_are_named_lowest_first(tmp_path, monkeypatch, batch):
    text = fc.kind_text("diploid", np.random.default_rng(12))
    off, pos = fc.kind_loci(np.random.default_rng(13), "diploid")
    raw = bgzf_writer.bgzf(text, chunk=37)
    _set_batch(monkeypatch, batch)
    path = tmp_path / "g.fa"
    for bad, lowest in (((9,), 9), ((30, 4), 4), ((1, 50), 1)):
        broken = raw
        for k in bad:
            broken = bgzf_writer.corrupt_member(broken, k)
        path.write_bytes(broken)
        got = _outcome(str(path), off, pos, True)
        assert got[0] == "error" and got[1] == _lib.E_INVALID_ARG
        head = "<dir>/g.fa: BGZF block %d: " % lowest
        assert got[2].endswith(head + "inflate failed or ISIZE mismatch") or got[2].endswith(head + "CRC32 mismatch")
    # a bad member is reported ahead of an error of the parse
    differ = bgzf_writer.corrupt_member(bgzf_writer.bgzf(fc.QUIRKS["lengths_differ_by_one"] * 3, chunk=37), 2)
    path.write_bytes(differ)
    got = _outcome(str(path), off, pos, True)
    assert got[0] == "error" and "BGZF block 2: " in got[2]


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("damage", range(len(bgzf_writer.LISTING_DAMAGE)))
def test_a_file_whose_members_cannot_be_listed(tmp_path, damage, device):
    """Member 0 is whole, which makes the file BGZF and not plain gzip; the list breaks at member 1, on either route."""
    text = fc.kind_text("diploid", np.random.default_rng(12))
    off, pos = fc.kind_loci(np.random.default_rng(13), "diploid")
    _name, data, tail = bgzf_writer.listing_damage(bgzf_writer.bgzf(text, chunk=37))[damage]
    path = tmp_path / "g.fa"
    path.write_bytes(data)
    assert _outcome(str(path), off, pos, device) == ("error", _lib.E_INVALID_ARG,
                                                     bgzf_writer.ERROR_PREFIX + "<dir>/g.fa" + tail)


# --- end to end ---------------------------------------------------------------------------------------------------

def _files(d):
    """{name: text} of a result directory without the lines that name the date and the reference's path."""
    out = {}
    for name, text in vr.read_dir(d).items():
        out[name] = "".join(l for l in text.splitlines(True) if not l.startswith("##reference="))
    return out


def _tree():
    """The planted clone tree with positions from 1 on (position 0 would end its chromosome at the first locus)."""
    p, truth = clone_tree(300, n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6, n_loci=2000)
    return secedo_amd.FlatPileup(p.chr_locus_off, p.locus_pos + 1, p.locus_entry_off, p.read_ids, p.id_base), truth


def test_variant_calling_end_to_end(tmp_path):
    p, truth = _tree()
    rng = np.random.default_rng(3)
    length = int(p.locus_pos.max()) + 10
    text = fc.kind_text("diploid", rng, (length,) * p.n_chr)
    fa = fc.write_form(tmp_path / "g.fa", text, "plain")
    gz = fc.write_form(tmp_path / "g.fa.gz", text, "bgzf")
    clusters = (truth % 3).astype(np.uint16)
    host, dev, res_dir = str(tmp_path / "host"), str(tmp_path / "dev"), str(tmp_path / "resident")
    variant.variant_calling(p, clusters, fa, "", 1e-3, 0.01, host)
    assert variant.fasta_stats()["route"] == "host"
    times = variant.variant_calling(p, clusters, gz, "", 1e-3, 0.01, dev, fasta_route="device")
    st = variant.fasta_stats()
    assert st["route"] == "device" and st["kind"] == "bgzf" and st["device_members"] > 0 and times["gather_ms"] == 0
    want = _files(host)
    assert sum(len(v) for v in want.values()) > 1000 and _files(dev) == want
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res = plan.upload(p, np.arange(300, dtype=np.uint32), 300)
        variant.variant_calling_resident(plan, res, clusters, gz, "", 1e-3, 0.01, res_dir)
        assert variant.fasta_stats()["route"] == "device"
        variant.variant_calling_resident(plan, res, clusters, fa, "", 1e-3, 0.01, res_dir + "_text",
                                         fasta_route="device")
        assert variant.fasta_stats()["route"] == "device" and variant.fasta_stats()["kind"] == "text"
    assert _files(res_dir) == want and _files(res_dir + "_text") == want
    assert variant.get_fasta_route() == "host"  # the keyword was a scoped override
    # the records alone
    a = variant.variant_calls(p, clusters, fa)
    b = variant.variant_calls(p, clusters, gz, fasta_route="device")
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) > 0


def test_the_cli_takes_a_compressed_genome(tmp_path):
    p, truth = _tree()
    names = ("1", "2", "X")
    clone_tree_files(str(tmp_path / "bin"), p, names)
    rng = np.random.default_rng(4)
    text = fc.kind_text("haploid", rng, (int(p.locus_pos.max()) + 10,) * 24)
    fa = fc.write_form(tmp_path / "g.fa", text, "plain")
    gz = fc.write_form(tmp_path / "g.fa.gz", text, "bgzf")
    labels = tmp_path / "labels"
    labels.write_text(",".join(str(int(t) % 2) for t in truth) + "\n")
    flags = ["-i", str(tmp_path / "bin"), "--chromosomes=1,2,X", "--clustering=" + str(labels)]
    a, b = str(tmp_path / "a") + "/", str(tmp_path / "b") + "/"
    assert secedo_main.main(flags + ["-o", a, "--reference_genome=" + fa]) == 0
    assert secedo_main.main(flags + ["-o", b, "--reference_genome=" + gz, "--fasta_route", "device"]) == 0
    assert variant.fasta_stats()["route"] == "device"
    want = {k: v for k, v in _files(a).items() if k.endswith(".vcf") or k in ("variant", "scores")}
    assert len(want) >= 4 and sum(len(v) for v in want.values()) > 1000
    assert {k: v for k, v in _files(b).items() if k in want} == want
    assert secedo_main.main(flags + ["-o", b, "--reference_genome=" + gz, "--fasta_route", "gpu"]) == 1
