"""Compressed reference genomes on the host functions of include/secedo_variant.h (no GPU): a FASTA written as
BGZF (whole members, and 37-byte members so that lines and headers span them) or as plain gzip (one member, three
members) gives what the plain file gives -- locus_ref, chr_locus_end, the diploid test, the contigs -- and a corrupt
or truncated file is an error that names it. The kind is told by content: every file here is called g.fa."""
import os
import subprocess
import sys

import numpy as np
import pytest

from secedo_amd import _lib, variant
from tests import bgzf_writer
from tests import fasta_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPRESSED = [f for f in fc.FORMS if f != "plain"]


def _texts():
    """name -> (text, map file, chr_locus_off, locus_pos)"""
    out = {}
    for i, kind in enumerate(fc.KINDS):
        rng = np.random.default_rng(100 + i)
        out[kind] = (fc.kind_text(kind, rng), "") + fc.kind_loci(rng, kind)
    with open(fc.MALE, "rb") as f:
        male = f.read()
    off = np.asarray([0, 12, 20, 27], dtype=np.uint32)
    pos = np.asarray(list(range(1, 13)) + list(range(1, 9)) + list(range(1, 8)), dtype=np.uint32)
    out["male_file"] = (male, "", off, pos)
    out["male_file_mapped"] = (male, fc.MALE_MAP, off, pos)
    for name, text in fc.QUIRKS.items():
        out["quirk_" + name] = (text, "") + fc.quirk_loci(text)
    return out


TEXTS = _texts()


def _outcome(f, *args, **kw):
    """The result, or the error's code and message with the file's directory taken out."""
    try:
        r = f(*args, **kw)
    except _lib.SecedoError as e:
        return ("error", e.code if hasattr(e, "code") else e.args[0], str(e))
    if isinstance(r, tuple):
        return tuple(np.asarray(x).tolist() for x in r)
    return np.asarray(r).tolist()


def _all(path, map_file, off, pos):
    return {
        "genotypes": _outcome(variant.reference_genotypes, path, off, pos, map_file),
        "diploid": _outcome(variant.is_diploid, path),
        "chromosomes": [_outcome(variant.read_chromosome, path, i, map_file) for i in range(len(off) - 1)],
    }


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The plain file's results, computed once per text."""
    root = tmp_path_factory.mktemp("plain")
    out = {}
    for name, (text, map_file, off, pos) in TEXTS.items():
        d = root / name
        d.mkdir()
        out[name] = _all(fc.write_form(d / "g.fa", text, "plain"), map_file, off, pos)
    return out


def _same(a, b, dir_a, dir_b):
    """Equal results; an error's message may differ only in the directory of the file it names."""
    def norm(x, d):
        if isinstance(x, tuple) and x and x[0] == "error":
            return (x[0], x[1], x[2].replace(d, "<dir>"))
        return x
    assert norm(a["genotypes"], dir_a) == norm(b["genotypes"], dir_b)
    assert norm(a["diploid"], dir_a) == norm(b["diploid"], dir_b)
    assert [norm(x, dir_a) for x in a["chromosomes"]] == [norm(x, dir_b) for x in b["chromosomes"]]


@pytest.mark.parametrize("form", COMPRESSED)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_compressed_equals_plain(tmp_path, plain, name, form):
    text, map_file, off, pos = TEXTS[name]
    path = fc.write_form(tmp_path / "g.fa", text, form)
    got = _all(path, map_file, off, pos)
    _same(got, plain[name], str(tmp_path), "<nowhere>")
    want = plain[name]["genotypes"]
    if not (isinstance(want, tuple) and want and want[0] == "error"):
        assert got["genotypes"] == want
    st = variant.fasta_stats()  # of the last call: read_chromosome, or reference_genotypes when there is no chromosome
    assert st["kind"] == ("bgzf" if form.startswith("bgzf") else "gzip") and st["route"] == "host"
    if len(text):
        assert st["host_inflated_bytes"] == len(text)


def test_plain_results_are_not_trivial(plain):
    ref, end = plain["diploid"]["genotypes"]
    assert len(set(ref)) > 8 and plain["diploid"]["diploid"] is True and plain["haploid"]["diploid"] is False
    assert plain["quirk_missing_paternal"]["genotypes"][0] == "error"
    assert "(5 vs 4)" in plain["quirk_lengths_differ_by_one"]["genotypes"][2]
    assert "empty line" in plain["quirk_newline"]["genotypes"][2]


@pytest.mark.parametrize("chunk,k", [(37, 0), (37, 5), (0xFF00, 1)])
def test_a_corrupt_bgzf_member_is_named(tmp_path, chunk, k):
    text = fc.kind_text("diploid", np.random.default_rng(5), contigs=(40000, 30000) if chunk > 37 else fc.CONTIGS)
    raw = bgzf_writer.corrupt_member(bgzf_writer.bgzf(text, chunk=chunk), k)
    path = tmp_path / "g.fa"
    path.write_bytes(raw)
    off, pos = np.asarray([0, 2], dtype=np.uint32), np.asarray([1, 2], dtype=np.uint32)
    for call in (lambda: variant.reference_genotypes(str(path), off, pos), lambda: variant.is_diploid(str(path)),
                 lambda: variant.read_chromosome(str(path), 0)):
        with pytest.raises(_lib.SecedoError) as e:
            call()
        message = str(e.value)
        assert "%s: BGZF block %d: " % (path, k) in message
        assert message.endswith("inflate failed or ISIZE mismatch") or message.endswith("CRC32 mismatch")


def test_the_lowest_of_two_corrupt_members_is_named(tmp_path):
    text = fc.kind_text("haploid", np.random.default_rng(6))
    raw = bgzf_writer.corrupt_member(bgzf_writer.corrupt_member(bgzf_writer.bgzf(text, chunk=37), 9), 4)
    path = tmp_path / "g.fa"
    path.write_bytes(raw)
    with pytest.raises(_lib.SecedoError, match="BGZF block 4: "):
        variant.is_diploid(str(path))


@pytest.mark.parametrize("form", ["gzip1", "gzip3"])
def test_a_cut_gzip_fails(tmp_path, form):
    text = fc.kind_text("diploid", np.random.default_rng(7))
    whole = fc.write_form(tmp_path / "whole.fa", text, form)
    raw = open(whole, "rb").read()
    path = tmp_path / "g.fa"
    off, pos = np.asarray([0, 1], dtype=np.uint32), np.asarray([1], dtype=np.uint32)
    for cut in (len(raw) // 2, len(raw) - 3):
        path.write_bytes(raw[:cut])
        with pytest.raises(_lib.SecedoError) as e:
            variant.reference_genotypes(str(path), off, pos)
        assert str(path) in str(e.value)
    flipped = bytearray(raw)
    flipped[-6] ^= 0x40  # the last member's CRC32
    path.write_bytes(bytes(flipped))
    with pytest.raises(_lib.SecedoError) as e:
        variant.is_diploid(str(path))
    assert str(path) in str(e.value)


def test_an_unknown_route_in_the_environment_fails_every_reader(tmp_path):
    path = fc.write_form(tmp_path / "g.fa", fc.QUIRKS["x_then_y"], "plain")
    code = ("import sys, numpy as np\n"
            "from secedo_amd import variant, _lib\n"
            "off, pos = np.asarray([0, 1], dtype=np.uint32), np.asarray([1], dtype=np.uint32)\n"
            "calls = [lambda: variant.reference_genotypes(sys.argv[1], off, pos), lambda: variant.is_diploid(sys.argv[1]),\n"
            "         lambda: variant.read_chromosome(sys.argv[1], 0), variant.get_fasta_route]\n"
            "for c in calls:\n"
            "    try:\n"
            "        c()\n"
            "    except _lib.SecedoError as e:\n"
            "        assert 'SECEDO_FASTA=bogus' in str(e), str(e)\n"
            "    else:\n"
            "        sys.exit(3)\n"
            "variant.set_fasta_route('host')\n"
            "assert variant.is_diploid(sys.argv[1]) is True and variant.get_fasta_route() == 'host'\n")
    env = dict(os.environ, SECEDO_FASTA="bogus", PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr.decode(errors="replace")[-2000:]
    for value, want in (("", "host"), ("host", "host"), ("device", "device")):
        env["SECEDO_FASTA"] = value
        res = subprocess.run([sys.executable, "-c", "from secedo_amd import variant; print(variant.get_fasta_route())"],
                             env=env, capture_output=True, timeout=120)
        assert res.returncode == 0 and res.stdout.decode().strip() == want, res.stderr.decode(errors="replace")[-2000:]
