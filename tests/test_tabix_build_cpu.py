"""The TBI writer (secedo_amd/csrc/tabix_build.hpp) and everything around the tabix indexes that needs no GPU: the host
builder under AddressSanitizer and UBSan (secedo_amd/csrc/build/tabix_build_test) on what the device's line pass would
hand it for the texts of tests/tabix_cases.py, whole and split at range boundaries, against tests/tabix_expected.py;
malformed and cut inputs; the oracle itself (tests/tabix_reader.py on expected indexes against the brute-force filter);
the setting, its environment variable and the command lines that are refused before torch is imported."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import bgzf_writer as gw
from tests import tabix_cases as tc
from tests import tabix_expected as te
from tests import tabix_reader as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "tabix_build_test")

TEXTS = {"formatter": tc.formatter, "spans": tc.spans, "cosmic": tc.cosmic,
         **{k: (lambda v=v: v) for k, v in tc.SMALL.items()}}


def program(*args):
    r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout


def built(tmp_path, text):
    """the builder's index for the input text -> (bytes, stats) or the rejection's reason"""
    (tmp_path / "in.txt").write_text(text)
    out = program("build", tmp_path / "in.txt", tmp_path / "out.tbi")
    if out.startswith("rejected: "):
        return out[len("rejected: "):].strip()
    words = out.split()
    return (tmp_path / "out.tbi").read_bytes(), dict(zip(words[0::2], (int(w) for w in words[1::2])))


# --- the oracle pinned ---------------------------------------------------------------------------------------------

def test_expected_bytes_of_a_hand_made_file():
    text = b"#h\n7\t5\t.\tAC\tG\n7\t16385\t.\tA\tC\n"
    gz = gw.bgzf(text)
    eof = len(gz) - 28
    line1, line2 = 3, 3 + len(b"7\t5\t.\tAC\tG\n")
    want = b"TBI\1" + struct.pack("<8i", 1, 2, 1, 2, 0, 35, 0, 2) + b"7\0" + struct.pack("<i", 3)
    want += struct.pack("<IiQQ", 4681, 1, line1, line2) + struct.pack("<IiQQ", 4682, 1, line2, eof << 16)
    want += struct.pack("<IiQQQQ", 37450, 2, line1, eof << 16, 2, 0) + struct.pack("<iQQ", 2, line1, line2)
    want += struct.pack("<Q", 0)
    assert te.expected_bytes(gz) == want
    assert te.expected_bytes(gw.bgzf(b"#only\n")) == b"TBI\1" + struct.pack("<8i", 0, 2, 1, 2, 0, 35, 0, 0) + bytes(8)
    assert te.expected_bytes(gw.EOF_MEMBER)[4:8] == bytes(4)


def test_the_parse_rules():
    tail = b"\t.\tA\tC\t.\t.\t"
    assert te.parse(b"1\t0" + tail + b"X=1")[2:] == (0, 1)
    assert te.parse(b"1\t10\t.\tACGT\tC")[2:] == (9, 13)
    assert te.parse(b"1\t10" + tail + b"END=50;A=1")[2:] == (9, 50)
    assert te.parse(b"1\t10" + tail + b"A=1;END=50\tGT")[2:] == (9, 50)
    for info in (b"XEND=50", b"END=.", b"END=9", b"END=5x", b"END", b"END=;A", b"A=1;END=7;END=99"):
        assert te.parse(b"1\t10" + tail + info)[2:] == (9, 10), info
    assert te.parse(b"1") == te.E_COLUMNS and te.parse(b"1\t1x") == te.E_POS and te.parse(b"1\t") == te.E_POS
    assert te.parse(b"1\t%d\t.\tAC" % (1 << 29)) == te.E_END and te.parse(b"1\t%d\t.\tA" % (1 << 29))[3] == 1 << 29


@pytest.mark.parametrize("name", sorted(tc.ERRORS))
def test_the_oracle_refuses_the_error_texts(name):
    text, line, words = tc.ERRORS[name]
    with pytest.raises(te.TabixError) as e:
        te.data_lines(text)
    assert (e.value.line, e.value.what) == (line, words)


def test_the_golden_extract_has_a_block_that_comes_back():
    with pytest.raises(te.TabixError) as e:
        te.data_lines(tc.cosmic_whole())
    assert e.value.what == te.E_BLOCKS
    assert len(te.data_lines(tc.cosmic())) > 10


@pytest.mark.parametrize("name", ["formatter", "spans", "cosmic", "no-last-newline", "comments-between"])
def test_reader_equals_the_brute_force_filter_on_expected_indexes(name):
    text = TEXTS[name]()
    recs = te.data_lines(text)
    for chunk in (0xFF00, 997):  # bgzip's cut, and many small members
        gz = gw.bgzf(text, chunk=chunk)
        reader = tr.Reader(gz, te.expected_bytes(gz))
        regions = tc.regions(text)
        hits = 0
        for region in regions[::1 if chunk == 0xFF00 else 5]:
            got = reader.query(*region)
            assert got == te.overlapping(text, *region, recs=recs), (name, chunk, region)
            hits += len(got)
        assert hits > 0
    # the reader does depend on the index: with the first chunk of the first name's lowest bin emptied, its line is lost
    index = bytearray(te.expected_bytes(gz))
    at = 36 + struct.unpack_from("<i", index, 32)[0] + 4
    lowest = struct.unpack_from("<I", index, at)[0]
    struct.pack_into("<Q", index, at + 8, struct.unpack_from("<Q", index, at + 16)[0])  # chunk_beg = chunk_end
    first = next(r for r in recs if te.reg2bin(r[1], r[2]) == lowest)
    assert first[0] == recs[0][0]
    assert tr.Reader(gz, bytes(index)).query(first[0], first[1], first[2]) != te.overlapping(text, *first[:3])


# --- the host builder ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(TEXTS))
def test_builder_gives_the_expected_bytes(name, tmp_path):
    text = TEXTS[name]()
    n = len(te.data_lines(text))
    rng = np.random.default_rng(5)
    for chunk in (0xFF00, 4096):
        gz = gw.bgzf(text, chunk=chunk)
        want = te.expected_bytes(gz)
        all_cuts = [(), range(0, n, 7), sorted(int(c) for c in rng.choice(max(n, 1), min(n, 40), replace=False))]
        for cuts in all_cuts if n else [()]:
            got, stats = built(tmp_path, te.builder_input(gz, cuts))
            assert got == want, (name, chunk, list(cuts)[:5])
            assert stats["bytes"] == len(want) and stats["joined"] == te.run_crossings(gz, cuts)
    if name == "formatter":
        assert stats["names"] == 3 and stats["chunks"] >= stats["bins"] >= 15


def test_builder_answers_malformed_input_with_a_reason(tmp_path):
    head = "N 1\nN 2\n"
    cases = {
        "H 0 4681 100 0\nH 0 4682 50 1\nE 200 2\n": "offsets do not ascend",
        "H 0 4681 100 0\nW 2 0 100\nE 200 1\n": "a window of an unknown name",
        "H 2 4681 100 0\nE 200 1\n": "a head of an unknown name",
        "H 0 37450 100 0\nE 200 1\n": "a bin past 37449",
        "H 0 4681 100 0\nH 0 4682 150 0\nE 200 2\n": "record ordinals do not ascend",
        "H 1 4681 100 0\nH 0 4681 150 1\nE 200 2\n": "RefIDs do not ascend",
        "H 0 4681 100 0\nW 0 40000 100\nE 200 1\n": "a window past 2^29",
        "W 1 3 100\nH 0 4681 100 0\nE 200 1\n": "windows of a reference without records",
        "H 0 4681 100 3\nE 200 3\n": "fewer records than the last head's ordinal",
        "H 0 4681 100 0\nE 50 1\n": "the end lies before the last head",
        "N 1\n": "chromosome blocks not continuous",
        "X 1\n": "a bad line",
        "H 0 4681 100 0\n": "no E line",
    }
    for body, why in cases.items():
        assert built(tmp_path, head + body) == why, body
    got, stats = built(tmp_path, "E 0 0\n")
    assert got == b"TBI\1" + struct.pack("<8i", 0, 2, 1, 2, 0, 35, 0, 0) + bytes(8) and stats["names"] == 0


def test_cut_inputs_are_refused_not_read_past(tmp_path):
    gz = gw.bgzf(tc.spans(), chunk=4096)
    (tmp_path / "in.txt").write_text(te.builder_input(gz, range(0, 14, 3)))
    out = program("cuts", tmp_path / "in.txt", 23).split()
    assert int(out[1]) == 1 and int(out[3]) > 20


# --- the setting and the command lines -----------------------------------------------------------------------------

def _child(code, env=None, args=()):
    return subprocess.run([sys.executable, "-c", code, *args], cwd=ROOT, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


def test_the_setting_and_its_environment_variable():
    get = "from secedo_amd import variant as v; print(v.get_vcf_index())"
    assert _child(get).stdout.strip() == "none"
    assert _child(get, {"SECEDO_VCF_INDEX": "tbi"}).stdout.strip() == "tbi"
    assert _child(get, {"SECEDO_VCF_INDEX": ""}).stdout.strip() == "none"
    bad = _child(get, {"SECEDO_VCF_INDEX": "csi"})
    assert bad.returncode != 0 and "SECEDO_VCF_INDEX=csi: expected none or tbi" in bad.stderr
    both = ("from secedo_amd import variant as v; v.set_vcf_index('tbi'); a = v.get_vcf_index(); "
            "v.set_vcf_index('none'); print(a, v.get_vcf_index(), v.tabix_stats()['files'])")
    assert _child(both, {"SECEDO_VCF_INDEX": "csi"}).stdout.split() == ["tbi", "none", "0"]
    from secedo_amd import variant
    with pytest.raises(ValueError):
        variant.set_vcf_index("csi")


def test_library_exports_the_tabix_functions():
    from secedo_amd import variant
    from tests.test_cluster_cpu import _declared, _exports
    names = {"secedo_variant_set_vcf_index", "secedo_variant_get_vcf_index", "secedo_variant_tabix_build",
             "secedo_variant_tabix_stats"}
    assert names <= _declared("secedo_variant.h") and names <= _exports(variant.LIB_PATH) and names <= set(variant.SIGNATURES)


def test_command_lines_refused_before_torch_is_imported(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    open(d / "s_1.pileup.bin", "wb").close()
    main = ("import sys; from secedo_amd import secedo_main as m; rc = m.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)")
    ok = ["-i", str(d), "--chromosomes=1"]
    for flags, env, words in ((["--vcf_index", "tbi"], {}, "add --vcf_output bgzf"),
                              (["--vcf_index=tbi", "--vcf_output=plain"], {"SECEDO_VCF": "bgzf"}, "add --vcf_output bgzf"),
                              (["--vcf_index", "csi", "--vcf_output", "bgzf"], {}, "Should be one of none, tbi")):
        p = _child(main, env, ok + flags)
        assert p.returncode == 1 and words in p.stderr and "torch imported" not in p.stderr, (flags, p.stderr)
    tabix = ("import sys; from secedo_amd import tabix_main as m\ntry:\n    rc = m.main(sys.argv[1:])\n"
             "except SystemExit as e:\n    print(e); rc = 3\nassert 'torch' not in sys.modules, 'torch imported'\n"
             "sys.exit(rc)")
    p = _child(tabix, args=["-i", str(tmp_path / "missing.vcf.gz")])
    assert p.returncode == 3 and "does not exist" in p.stdout
    p = _child(tabix, args=["-i", str(d)])
    assert p.returncode == 0 and "No .vcf.gz files found" in p.stdout
    (d / "a.vcf.gz").write_bytes(gw.bgzf(tc.SMALL["one-line"]))
    (d / "a.vcf.gz.tbi").write_bytes(b"x")
    p = _child(tabix, args=["-i", str(d)])
    assert p.returncode == 3 and "a.vcf.gz.tbi exists (1 of 1 files have an index); pass --overwrite" in p.stdout
