"""The secedo CLI (secedo_amd/secedo_main.py) and the binary pileup loader library without a GPU: flag parsing,
validators and exit codes before torch is imported, file discovery, --pos_file parsing, the test writers against
the host reader, and the loader library's exports."""
import os
import subprocess
import sys

import numpy as np
import pytest

import secedo_amd
from secedo_amd import pileup_load
from secedo_amd import secedo_main as sm
from secedo_amd.pileup import FlatPileup
from tests.pileup_file_writer import clone_tree_files, records, write_bin, write_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_spellings():
    f = sm.parse_flags(["-i", "in", "--o=out/", "--min_cluster_size", "40", "-max_coverage=50", "--seq_error_rate",
                        "0.02", "--expectation_maximization", "--noarma_kmeans", "--compute_read_stats=false",
                        "-clustering_type", "SPECTRAL2", "positional"])
    assert (f.i, f.o, f.min_cluster_size, f.max_coverage, f.seq_error_rate) == ("in", "out/", 40, 50, 0.02)
    assert f.expectation_maximization is True and f.arma_kmeans is False and f.compute_read_stats is False
    assert f.clustering_type == "SPECTRAL2"
    g = sm.parse_flags(["--arma_kmeans=true", "--noexpectation_maximization", "--compute_read_stats"])
    assert g.arma_kmeans is True and g.expectation_maximization is False and g.compute_read_stats is True
    d = sm.parse_flags([])
    assert d.chromosomes == ",".join([str(c) for c in range(1, 23)] + ["X"]) and d.tumor_purity == 5
    assert (d.min_cluster_size, d.max_cell_count, d.termination, d.normalization) == (100, 10000, "BIC", "ADD_MIN")
    for bad in (["--bogus=1"], ["--min_cluster_size=x"], ["--min_cluster_size"], ["--arma_kmeans=maybe"]):
        with pytest.raises(sm.UsageError):
            sm.parse_flags(bad)


def _run(args, cwd):
    """main(args) in a child process; asserts torch was never imported there. -> (exit code, output)."""
    code = ("import sys; from secedo_amd import secedo_main as m; rc = m.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch imported'; sys.exit(rc)")
    p = subprocess.run([sys.executable, "-c", code, *args], cwd=cwd, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert "torch imported" not in p.stderr, p.stderr
    return p.returncode, p.stdout + p.stderr


def _bins(d, names):
    os.makedirs(d, exist_ok=True)
    for n in names:
        open(os.path.join(d, n), "wb").close()


def test_validators_and_exit_codes(tmp_path):
    d = str(tmp_path / "in")
    _bins(d, ["s_1.pileup.bin", "s_2.pileup.bin"])
    ok = ["-i", d, "--chromosomes=1,2"]
    rc, out = _run([], tmp_path)
    assert rc == 1 and "secedo -i" in out
    for flag, text in (("--clustering_type=KMEANS", "clustering_type"), ("--termination=XIC", "termination"),
                       ("--normalization=NONE", "normalization"), ("--tumor_purity=6", "tumor_purity"),
                       ("--tumor_purity=0", "tumor_purity"), ("--arma_kmeans", "arma_kmeans"),
                       ("--chromosomes=1,2,3", "Chromosome 3"), ("--chromosomes=1,Z", "Invalid chromosome")):
        rc, out = _run(ok + [flag], tmp_path)
        assert rc == 1 and text in out, (flag, out)
    rc, out = _run(["-i", str(tmp_path / "none"), "--chromosomes=1"], tmp_path)
    assert rc == 1 and "Invalid pileup filename" in out
    _bins(str(tmp_path / "bad"), ["a_b_1.pileup.bin"])
    rc, out = _run(["-i", str(tmp_path / "bad"), "--chromosomes=1"], tmp_path)
    assert rc == 1 and "Invalid pileup filename" in out
    _bins(str(tmp_path / "dup" / "x"), ["s_1.pileup.bin"])
    _bins(str(tmp_path / "dup"), ["t_1.pileup.bin"])
    rc, out = _run(["-i", str(tmp_path / "dup"), "--chromosomes=1"], tmp_path)
    assert rc == 1 and "Two input files for chromosome 1" in out
    pos = tmp_path / "pos.txt"
    pos.write_text("1\t5\n")
    rc, out = _run(ok + ["--pos_file=" + str(pos)], tmp_path)
    assert rc == 1 and "does not match number of input files" in out
    rc, out = _run(ok + ["--pos_file=" + str(tmp_path / "missing.txt")], tmp_path)
    assert rc == 1 and "positions file" in out
    rc, out = _run(ok + ["--clustering=" + str(tmp_path / "missing")], tmp_path)
    assert rc == 1 and "clustering file" in out
    rc, out = _run(ok + ["--merge_file=" + str(tmp_path / "missing")], tmp_path)
    assert rc == 1 and "merge file" in out
    os.makedirs(tmp_path / "empty")
    rc, out = _run(["-i", str(tmp_path / "empty")], tmp_path)
    assert rc == 0 and "No input files" in out


def test_get_chromosome_and_discovery(tmp_path):
    assert sm.get_chromosome("/a/b/sample_X.pileup.bin") == 22
    assert sm.get_chromosome("sample_12.pileup") == 11
    assert sm.get_chromosome("dir_with_underscores/s_1.bin") == 0
    for bad in ("s.pileup.bin", "a_b_1.pileup.bin", "s_23.pileup.bin", "s_0.pileup.bin"):
        with pytest.raises(sm.UsageError):
            sm.get_chromosome(bad)
    d = tmp_path / "d"
    _bins(str(d / "sub"), ["s_2.pileup.bin", "s_1.pileup"])
    _bins(str(d), ["s_1.pileup.bin", "s_3.pileup", "notes.txt"])
    assert sm.input_files(str(d)) == sorted([str(d / "s_1.pileup.bin"), str(d / "sub" / "s_2.pileup.bin")])
    t = tmp_path / "t"
    _bins(str(t / "sub"), ["s_2.pileup"])
    _bins(str(t), ["s_1.pileup", "x.txt"])
    assert sm.input_files(str(t)) == [str(t / "s_1.pileup"), str(t / "sub" / "s_2.pileup")]
    assert sm.input_files(str(t / "s_1.pileup")) == [str(t / "s_1.pileup")]


def test_read_positions(tmp_path):
    f = tmp_path / "pos"
    f.write_text("# header\n2\t30\n2\t10\nX\t7\nMT\t5\n25\t1\n1\t4\n2\t20\n")
    got = sm.read_positions(str(f))
    assert len(got) == 23 and got[0] == [4] and got[1] == [10, 20, 30] and got[22] == [7]
    assert all(not v for v in got[2:22])


def test_writers_round_trip_through_the_host_reader(tmp_path):
    from tests.clone_tree_gen import clone_tree
    p, _ = clone_tree(40, n_loci=300, seed=4)
    parts = clone_tree_files(str(tmp_path), p, ("1", "7"))
    for name, part in parts.items():
        for path in (str(tmp_path / ("s_%s.pileup.bin" % name)),):
            got, nc, ml = secedo_amd.read_pileup(path, secedo_amd.get_grouping())
            assert np.array_equal(got.locus_pos, part.locus_pos) and got.locus_pos[0] == 1
            assert np.array_equal(got.locus_entry_off, part.locus_entry_off)
            assert np.array_equal(got.read_ids, part.read_ids) and np.array_equal(got.id_base, part.id_base)
        write_text(str(tmp_path / ("t_%s.pileup" % name)), part, name)
        got, nc2, ml2 = secedo_amd.read_pileup(str(tmp_path / ("t_%s.pileup" % name)), secedo_amd.get_grouping())
        assert np.array_equal(got.locus_pos, part.locus_pos) and np.array_equal(got.read_ids, part.read_ids)
        assert np.array_equal(got.id_base, part.id_base) and ml2 == ml
    assert len(records([5], [0], [], [])) == 6


def test_loader_library_exports_its_header():
    from tests.test_cluster_cpu import _declared, _exports
    assert _exports(pileup_load.LIB_PATH) == _declared("secedo_pileup.h") == set(pileup_load.SIGNATURES)


def test_loader_without_a_gpu_or_with_bad_slots(tmp_path):
    write_bin(str(tmp_path / "a.bin"), FlatPileup(
        np.asarray([0, 1], dtype=np.uint32), np.asarray([3], dtype=np.uint32), np.asarray([0, 1], dtype=np.uint64),
        np.asarray([0], dtype=np.uint32), np.asarray([4], dtype=np.uint32)))
    f = str(tmp_path / "a.bin")
    from secedo_amd import _lib
    with pytest.raises(_lib.SecedoError) as e:
        pileup_load.read_pileups([f, f], [1, 1], 24)
    assert e.value.code == _lib.E_INVALID_ARG and "slot" in str(e.value)
    with pytest.raises(_lib.SecedoError) as e:
        pileup_load.read_pileups([f], [24], 24)
    assert e.value.code == _lib.E_INVALID_ARG
