"""CPU tests of the references and case tables that tests/test_gpu_spectral_kernels.py holds the spectral kernels
against (tests/spectral_ref.py, tests/spectral_cases.py): the references agree with each other and with
oracle/spectral_oracle.py, the Cholesky contract holds for numpy's own factorisation, and the case tables keep the
threshold margins and reach the code paths they claim."""
import numpy as np
import pytest

from oracle import spectral_oracle as so
from tests import spectral_cases as sc
from tests import spectral_ref as sr
from tests.test_gpu_spectral import planted

BW = sr.BW


@pytest.mark.parametrize("n,isolated", [(1, ()), (2, ()), (33, (4,)), (70, (0, 69))])
def test_the_two_halves_of_the_product_reproduce_the_oracle_laplacian(n, isolated):
    """T = the finished product applied to the identity's columns is (I + D^-1/2 A D^-1/2) / 2, so 2 (I - T) is the
    normalised Laplacian I - D^-1/2 A D^-1/2 (lambda_L = 2 (1 - tau), as the solver converts its Ritz values)."""
    a, _ = planted(n, 2, 90 + n, isolated=isolated)
    lap = 2 * (np.eye(n) - sr.operator_matrix(a))
    assert np.max(np.abs(lap - so.laplacian_fast(a))) <= 4e-16
    assert np.max(np.abs(lap - so.laplacian(a))) <= 4e-16
    for i in isolated:
        assert lap[i, i] == 1.0 and np.count_nonzero(lap[i]) == 1


def test_references_agree_with_each_other():
    rng = np.random.default_rng(5)
    n = 45
    a, _ = planted(n, 2, 6, isolated=(9,))
    sums, sums_bound = sr.row_sums(a)
    assert sr.ratio(a.sum(axis=1), sums, sums_bound) <= 1.0 and sums[9] == 0 and sums_bound[9] == 0
    s, root = sr.scale_from_sums(a.sum(axis=1))
    assert s[9] == 0.0 and root[9] == 0.0 and np.max(sr.ulp_distance(s * root, np.where(s > 0, 1.0, 0.0))) <= 2
    # the partials of any split of the rows add up to the full block's, and block_combine is the same sum
    x = rng.uniform(-1, 1, size=(n, BW))
    full, bound = sr.product_partial(a, s, x)
    parts = [sr.product_partial(a[lo:hi], s[lo:hi], x[lo:hi]) for lo, hi in ((0, 0), (0, 17), (17, 18), (18, 45))]
    assert sr.ratio(np.asarray(sum(p for p, _ in parts), dtype=np.float64), full, sum(b for _, b in parts)) <= 1.0
    assert np.all(parts[0][0] == 0) and np.all(parts[0][1] == 0)
    assert np.max(np.abs(np.asarray(full, dtype=np.float64) - a.T @ (s[:, None] * x))) <= float(np.max(bound))
    # gram(Q, W)[blk] == Q[blk]^T W == block_combine of the transposed roles
    q = sc.signed_blocks(n, 3, 8)
    w = rng.uniform(-1, 1, size=(n, BW))
    g, g_bound = sr.gram(q, w)
    for b in range(3):
        assert sr.ratio(q[b].T @ w, g[b], g_bound[b]) <= 1.0
    m = rng.uniform(-1, 1, size=(3, BW, BW))
    out0 = rng.uniform(-1, 1, size=(n, BW))
    val, vb = sr.block_combine(q, m, 0.5, 2.0, out0)
    assert sr.ratio(2.0 * out0 + 0.5 * np.einsum("bja,bac->jc", q, m), val, vb) <= 1.0
    val0, _ = sr.block_combine(q, m, 1.0, 0.0, np.full((n, BW), np.nan))
    assert np.all(np.isfinite(np.asarray(val0, dtype=np.float64)))
    # ratio() itself: a missed exact zero and a NaN are infinitely wrong
    assert sr.ratio(np.array([1e-300]), np.array([0.0]), np.array([0.0])) == float("inf")
    assert sr.ratio(np.array([np.nan]), np.array([0.0]), np.array([1.0])) == float("inf")
    assert sr.ratio(np.array([0.0, 1.5]), np.array([0.0, 1.0]), np.array([0.0, 1.0])) == 0.5


def test_write_vectors_reference_sign_and_tie_rule():
    y = np.zeros((6, 3))
    y[:, 0] = [1.0, -2.0, 0.5, 2.0, 0.0, 0.0]  # tie between index 1 (negative) and 3: index 1 decides -> flipped
    y[:, 2] = [3.0, 0.0, 0.0, 0.0, 0.0, -4.0]
    out = np.asarray(sr.write_vectors(y, 3), dtype=np.float64)
    assert out[1, 0] > 0 and out[3, 0] < 0 and np.all(out[:, 1] == 0) and out[5, 2] == 0.8 and out[0, 2] == -0.6
    assert np.allclose(np.linalg.norm(out, axis=0), [1, 0, 1])
    for n in sc.WRITE_N:
        yt, cols = sc.write_vectors_tie_block(n)
        assert (n >= 257) == any(hi == lo + 256 for _, lo, hi in cols) and (n == 1) == (not cols)
        for c, lo, hi in cols:
            assert abs(yt[lo, c]) == abs(yt[hi, c]) == 2.0 and yt[lo, c] == -yt[hi, c]
            assert np.count_nonzero(np.abs(yt[:, c]) >= 1.0) == 2


def _numpy_factor(g, alive):
    """numpy's Cholesky on the surviving set, laid out as cholesky_drop promises; a dropped column keeps its
    coefficients on the surviving columns before it."""
    S = np.flatnonzero(alive)
    r = np.zeros((BW, BW))
    rinv = np.zeros((BW, BW))
    if len(S):
        rs = np.linalg.cholesky(g[np.ix_(S, S)]).T
        r[np.ix_(S, S)] = rs
        rinv[np.ix_(S, S)] = np.linalg.inv(rs)
    for c in np.flatnonzero(~alive):
        b = S[S < c]
        if len(b) and g[c, c] > sr.NORM2_DROP:
            r[b, c] = np.linalg.solve(r[np.ix_(b, b)].T, g[b, c])
    return r, rinv


@pytest.mark.parametrize("name", sorted(sc.cholesky_cases()))
def test_cholesky_cases_keep_their_margins_and_numpy_keeps_the_contract(name):
    g, dropped = sc.cholesky_cases()[name]
    alive, margin = sr.cholesky_alive(g)
    assert sorted(np.flatnonzero(~alive)) == sorted(dropped)
    assert margin >= 100.0, margin  # every decision a factor of 100 clear of its threshold
    r, rinv = _numpy_factor(g, alive)
    ratios = sr.cholesky_contract(g, r, rinv, alive)
    print(name, "margin %.3g" % margin, ratios)
    assert max(ratios.values()) <= 1.0, ratios
    # the contract has teeth: one survivor too few, or a perturbed factor, breaks it
    if alive.any():
        k = int(np.flatnonzero(alive)[-1])
        fewer = alive.copy()
        fewer[k] = False
        with pytest.raises(AssertionError):
            sr.cholesky_contract(g, r, rinv, fewer)
        bent = r.copy()
        bent[k, k] *= 1.0 + 1e-12
        assert sr.cholesky_contract(g, bent, rinv, alive)["factor"] > 1.0
    r_prev = sc.r_prev_case()
    val, bound = sr.chained_factor(r, r_prev)
    assert sr.ratio(r @ r_prev, val, bound) <= 1.0 and np.all(np.tril(np.asarray(val, dtype=np.float64), -1) == 0)


def test_case_tables_reach_the_paths_they_claim():
    assert sc.PRODUCT_N == (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 191, 192, 256, 320, 513)
    segments, fast_odd_begin, slow_begin = set(), False, False
    for n in sc.PRODUCT_N:
        blocks = sc.product_blocks(n)
        assert blocks[0] == (0, n) and len(set(blocks)) == len(blocks)
        if n >= 2:
            assert {(0, 0), (n, 0), (n - 1, 1), (1, n - 1)} <= set(blocks)
        if n >= 130:
            assert (n - 64, 64) in blocks and (1, 64) in blocks and (3, 65) in blocks
        for lo, rows in blocks:
            assert 0 <= lo and lo + rows <= n
            segments.add(sc.product_segments(n, rows))
            # the straight-line path: even n, 32 columns and 64 rows inside the block
            fast = n % 2 == 0 and n >= 32 and rows >= 64
            fast_odd_begin |= fast and lo % 2 == 1
            slow_begin |= lo > 0 and not fast
    assert {1, 2, 3, 5} <= segments and fast_odd_begin and slow_begin
    assert (17, 128) in sc.product_blocks(192) and (5, 129) in sc.product_blocks(191)
    for n in sc.PARTITIONED_N:
        parts = sc.product_partitions(n)
        assert [len(p) for p in parts] == [3, 5]
        for p in parts:
            assert p[0][0] == 0 and sum(r for _, r in p) == n and all(a[0] + a[1] == b[0] for a, b in zip(p, p[1:]))
    assert sc.product_partitions(256) == []
    # isolated rows are in, and the cached inputs cannot be changed by a test
    a, s, x = sc.product_inputs(129)
    assert s[0] == 0.0 and s[64] == 0.0 and np.all(a[64] == 0) and x.min() < -0.9 and x.max() > 0.9
    with pytest.raises(ValueError):
        x[0, 0] = 1.0
    assert [sc.pad16(n) for n in (1, 15, 16, 17)] == [16, 16, 16, 32]
    assert [sc.gram_chunks(n) for n in (1, 128, 129, 257)] == [1, 1, 2, 3]
    assert sc.product_segments(16000, 16000) == 17 and sc.product_segments(4096, 8065) == 64
    assert sc.product_segments(4096, 8064) == 63 and sc.product_segments(300, 0) == 1
    assert sc.GRAM_WIDE_STRIDE[0] in sc.GRAM_N and sc.GRAM_WIDE_STRIDE[1] in sc.GRAM_NBLK
    v = sc.sums_case(600)
    assert np.count_nonzero(v == 0) > 50 and v.max() == 1e300 and 0 < v[v > 0].min() < 2.3e-308
    for n in sc.ROW_SUMS_N:
        assert all(lo + rows <= n and rows >= 1 for lo, rows in sc.row_sums_blocks(n))
