"""The GPU loader of binary pileup files (include/secedo_pileup.h) against the host reader secedo_pileup_read, bit
for bit: the reference's own .bin fixtures, synthetic files exercising every rule (coverage, position lists, the
stop rule, grouping, read spans dense and sparse, chunk boundaries, zero-coverage records, empty files, partial
headers), the errors, and the resident pileup feeding the filter and the divide_cluster recursion."""
import os
import shutil

import numpy as np
import pytest

import secedo_amd
from secedo_amd import _lib, pileup_load
from tests import golden_util as gu
from tests.pileup_file_writer import records

pytestmark = pytest.mark.gpu

DATA = os.path.join(gu.GOLDEN, "data")
VEC = np.load(os.path.join(gu.GOLDEN, "reader_vectors.npz"))
BIN_KEYS = sorted({k.rsplit("|", 1)[0] for k in VEC.files if "|bin|" in k})


@pytest.mark.parametrize("key", BIN_KEYS)
def test_loader_matches_reference_vectors(key, tmp_path):
    name, mc, mf, maxcov, _ = key.split("|")
    for f in os.listdir(DATA):
        shutil.copy(os.path.join(DATA, f), tmp_path)
    i2g = secedo_amd.get_grouping(int(mc), str(tmp_path / mf) if mf else "")
    per = {}
    p = pileup_load.read_pileups([str(tmp_path / (name + ".pileup.bin"))], [0], 1, i2g, int(maxcov),
                                 compute_read_stats=True, per_file=per)
    assert np.array_equal(p.locus_pos, VEC[key + "|pos"])
    assert np.array_equal(p.locus_entry_off, VEC[key + "|off"])
    assert np.array_equal(p.read_ids, VEC[key + "|rid"])
    assert np.array_equal(p.id_base, VEC[key + "|idb"])
    assert [per["num_cells"][0], per["max_read_length"][0]] == VEC[key + "|meta"].tolist()


def _random_file(path, rng, n_rec, n_cells=50, max_cov=40, sorted_pos=True, rid_range=None, zero_frac=0.1,
                 tail=b""):
    cov = rng.integers(1, max_cov + 1, n_rec)
    cov[rng.random(n_rec) < zero_frac] = 0
    pos = np.cumsum(rng.integers(1, 50, n_rec)).astype(np.uint32)
    if not sorted_pos:
        pos = rng.permutation(pos)
    e = int(cov.sum())
    rid = rng.integers(0, rid_range or max(4 * e // 3, 1), e).astype(np.uint32)
    if rid_range:  # a few hundred distinct ids spread over [0, rid_range): large ids that repeat
        pool = rng.integers(0, rid_range, 300).astype(np.uint32)
        rid = pool[rng.integers(0, len(pool), e)]
    packed = (rng.integers(0, n_cells, e) << 2 | rng.integers(0, 4, e)).astype(np.uint16)
    with open(path, "wb") as f:
        f.write(records(pos, cov, rid, packed) + tail)
    return pos


def _host(files, slots, n_slots, i2g, max_coverage, positions, stats):
    """read_pileup per file, concatenated in slot order -> (FlatPileup arrays, per-file num_cells / max length)."""
    chr_off, pos, off, rid, idb = [0], [], [np.zeros(1, np.uint64)], [], []
    nc, ml = [0] * len(files), [0] * len(files)
    base = 0
    by_slot = {s: i for i, s in enumerate(slots)}
    for s in range(n_slots):
        i = by_slot.get(s)
        n = 0
        if i is not None:
            pl = None if positions is None else positions[i]
            p, nc[i], ml[i] = secedo_amd.read_pileup(files[i], i2g, None, max_coverage, pl, stats)
            pos.append(p.locus_pos)
            off.append(np.asarray(p.locus_entry_off[1:], np.uint64) + np.uint64(base))
            rid.append(p.read_ids)
            idb.append(p.id_base)
            base += p.n_entries
            n = p.n_loci
        chr_off.append(chr_off[-1] + n)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return (np.asarray(chr_off, np.uint32), cat(pos, np.uint32), cat(off, np.uint64), cat(rid, np.uint32),
            cat(idb, np.uint32)), nc, ml


def _check(files, slots, n_slots=24, i2g=None, max_coverage=100, positions=None, stats=True, staging=0):
    i2g = secedo_amd.get_grouping() if i2g is None else i2g
    want, nc, ml = _host(files, slots, n_slots, i2g, max_coverage, positions, stats)
    per = {}
    got = pileup_load.read_pileups(files, slots, n_slots, i2g, max_coverage, positions, stats, staging,
                                   per_file=per)
    for a, b in zip((got.chr_locus_off, got.locus_pos, got.locus_entry_off, got.read_ids, got.id_base), want):
        assert np.array_equal(np.asarray(a), b)
    assert per["num_cells"] == nc and per["max_read_length"] == ml
    return got, per


def test_several_chromosomes_with_gaps(tmp_path):
    rng = np.random.default_rng(1)
    files = []
    for c in range(3):
        files.append(str(tmp_path / ("f%d.bin" % c)))
        _random_file(files[-1], rng, 400 + 100 * c)
    _check(files, [5, 0, 22])
    _check(files, [5, 0, 22], stats=False)
    _check(files, [5, 0, 22], max_coverage=20)  # coverage cut
    _check(files, [1, 2, 3], n_slots=4, staging=100)  # records straddle many chunks
    _check(files, [1, 2, 3], n_slots=4, staging=4099)


def test_position_lists(tmp_path):
    rng = np.random.default_rng(2)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    pa = _random_file(a, rng, 600)
    pb = _random_file(b, rng, 600, sorted_pos=False)
    some_a = np.sort(rng.choice(pa, 200, replace=False))
    mixed = np.sort(np.concatenate([rng.choice(pb, 100, replace=False), rng.integers(0, 40000, 50)])).astype(np.uint32)
    early = np.sort(pa[:150])  # the list ends early: the stop rule fires on record 150
    for plist in ([some_a, mixed], [early, None], [np.zeros(0, np.uint32), early], [early, mixed]):
        for staging in (0, 256):
            _check([a, b], [0, 1], 2, positions=plist, max_coverage=30, staging=staging)


def test_merge_grouping_and_read_span_branches(tmp_path):
    rng = np.random.default_rng(3)
    dense, sparse, unsorted = (str(tmp_path / n) for n in ("d.bin", "s.bin", "u.bin"))
    _random_file(dense, rng, 500)
    _random_file(sparse, rng, 500, rid_range=(1 << 32) - 1)  # ids far above the entry count: the sort branch
    _random_file(unsorted, rng, 500, sorted_pos=False)  # spans wrap in u32 as on the host
    i2g = secedo_amd.get_grouping(3)
    got, per = _check([dense, sparse, unsorted], [0, 1, 2], 3, i2g=i2g)
    assert min(per["max_read_length"]) > 0
    assert int(np.max(np.asarray(got.id_base) >> 2)) <= 50 // 3
    _check([dense, sparse, unsorted], [0, 1, 2], 3, i2g=i2g, stats=False)
    _check([sparse], [0], 1, staging=512)


def test_zero_coverage_empty_file_and_partial_header(tmp_path):
    rng = np.random.default_rng(4)
    zero, empty, partial = (str(tmp_path / n) for n in ("z.bin", "e.bin", "p.bin"))
    _random_file(zero, rng, 200, zero_frac=0.5)
    open(empty, "wb").close()
    _random_file(partial, rng, 200, tail=b"\x01\x02\x03\x04\x05")  # 5 bytes: ends the file silently
    got, per = _check([zero, empty, partial], [0, 1, 2], 3)
    assert per["num_cells"][1] == 1 and per["max_read_length"][1] == 0 and got.chr_locus_off[1] == got.chr_locus_off[2]
    only_zero = str(tmp_path / "oz.bin")
    with open(only_zero, "wb") as f:
        f.write(records([3, 9], [0, 0], [], []))
    got, per = _check([only_zero], [0], 1)
    assert got.n_loci == 2 and got.n_entries == 0 and per["num_cells"] == [1]


def _host_error(path, i2g, **kw):
    with pytest.raises(ValueError) as e:
        secedo_amd.read_pileup(path, i2g, None, **kw)
    return str(e.value)


def test_errors_match_the_host_reader(tmp_path):
    rng = np.random.default_rng(5)
    trunc = str(tmp_path / "t.bin")
    _random_file(trunc, rng, 50, tail=records([7], [3], [1, 2, 3], [4, 4, 4])[:-3])
    i2g = secedo_amd.get_grouping()
    msg = _host_error(trunc, i2g)
    with pytest.raises(_lib.SecedoError) as e:
        pileup_load.read_pileups([trunc], [0], 1, i2g)
    assert e.value.code == _lib.E_INVALID_ARG and str(e.value).endswith(msg) and "truncated" in msg
    small = str(tmp_path / "c.bin")
    _random_file(small, rng, 300, n_cells=60)
    i2g40 = np.arange(40, dtype=np.uint16)
    msg = _host_error(small, i2g40)
    with pytest.raises(_lib.SecedoError) as e:
        pileup_load.read_pileups([small], [0], 1, i2g40)
    assert e.value.code == _lib.E_INVALID_ARG and str(e.value).endswith(msg) and "Cell id" in msg
    with pytest.raises(_lib.SecedoError) as e:
        pileup_load.read_pileups([str(tmp_path / "missing.bin")], [0], 1)
    assert e.value.code == _lib.E_INVALID_ARG and "does not exist" in str(e.value)


def test_stop_rule_hides_a_truncated_tail(tmp_path):
    rng = np.random.default_rng(6)
    f = str(tmp_path / "s.bin")
    pos = _random_file(f, rng, 100, tail=records([10 ** 7], [3], [1, 2, 3], [4, 4, 4])[:-2])
    plist = np.sort(pos[:40])
    _check([f], [0], 1, positions=[plist])


def test_loaded_pileup_runs_the_pipeline(tmp_path):
    from secedo_amd import cluster
    from tests.clone_tree_gen import clone_tree
    from tests.pileup_file_writer import clone_tree_files
    p, truth = clone_tree(300, n_b=180, f_ab=0.35, f_a12=0.12, n_mixed=6)
    clone_tree_files(str(tmp_path), p, ("1", "2", "X"))
    files = [str(tmp_path / ("s_%s.pileup.bin" % c)) for c in ("1", "2", "X")]
    ident = np.arange(300)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        res, nc, ml = secedo_amd.read_pileups_resident(plan, files, [0, 1, 22], 24, ident.astype(np.uint16),
                                                       compute_read_stats=True)
        want, _, _ = _host(files, [0, 1, 22], 24, ident.astype(np.uint16), 100, None, True)
        host = secedo_amd.FlatPileup(*want)
        res2 = plan.upload(host, ident.astype(np.uint32), 300)
        assert nc == 300 and ml == 0
        f1, cov1 = secedo_amd.filter_resident(plan, res, ident, 0.01)
        f2, cov2 = secedo_amd.filter_resident(plan, res2, ident, 0.01)
        assert cov1 == cov2 and f1["n_loci"] == f2["n_loci"]
        assert np.array_equal(f1["pos"].cpu().numpy()[:f1["n_loci"]], f2["pos"].cpu().numpy()[:f2["n_loci"]])
        args = (ml, ident.astype(np.uint16), ident, ident, 0.01, 0.5, 0.01, "ADD_MIN", "BIC", "SPECTRAL6", False,
                True, 40)
        a = cluster.divide_cluster_resident(plan, res, *args)
        b = cluster.divide_cluster_resident(plan, res2, *args)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and len(a[2]) > 1
