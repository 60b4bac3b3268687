"""spectral_cases.py -- TEST INFRASTRUCTURE ONLY: the shapes and inputs of tests/test_gpu_spectral_kernels.py and
tests/test_spectral_ref_cpu.py (the kernels of secedo_amd/csrc/spectral_kernels.hip one by one).

The similarity matrices have the planted structure of tests/test_gpu_spectral.planted, some with isolated
(all-zero) rows; block vectors carry signed values, so the sums cancel. The shapes sit on the rounding points of the
kernels: the 64-row LDS stage of the product, its 128-column workgroup and 32-column wave, the 128-row Gram chunk,
the 16 rows of a block_combine workgroup and pad16, the 256 threads of write_vectors.

The cap of 64 segments in product_segments needs more than 8064 local rows, far outside a test of seconds: it stays
with tests/test_gpu_fullsize.py.
"""
import functools

import numpy as np

from secedo_amd.distributed import row_range
from tests import spectral_ref as sr
from tests.test_gpu_spectral import planted

BW = sr.BW


# ---- the sizing functions of spectral_kernels.hpp restated (checked against the library on the GPU) ----

def pad16(n):
    return (n + 15) // 16 * 16


def gram_chunks(n):
    return (n + 127) // 128


def product_segments(n, n_rows):
    cols = (pad16(n) + 127) // 128  # workgroup columns; enough segments to fill the chip, 128 rows each at least
    return max(1, min((2048 + cols - 1) // cols, 64, max(1, (n_rows + 127) // 128)))


# ---- product_partial / product_finish ----

PRODUCT_N = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 191, 192, 256, 320, 513)
PARTITIONED_N = (320, 513)


def product_partitions(n):
    """The three-way and five-way even partitions of distributed.row_range, as lists of (row_begin, n_rows)."""
    if n not in PARTITIONED_N:
        return []
    return [[(lo, hi - lo) for lo, hi in (row_range(n, r, w) for r in range(w))] for w in (3, 5)]


def product_blocks(n):
    """Row blocks (row_begin, n_rows) of the product at n rows, the full block first."""
    blocks = [(0, n)]
    if n >= 2:
        blocks += [(0, 0), (n, 0), (n - 1, 1), (1, n - 1)]
    if n >= 130:
        blocks += [b for b in ((1, 64), (3, 65), (17, 128), (5, 129)) if b[0] + b[1] <= n] + [(n - 64, 64)]
    for part in product_partitions(n):
        blocks += part
    return list(dict.fromkeys(blocks))


@functools.lru_cache(maxsize=None)
def product_inputs(n):
    """(a, s, x): planted matrix (isolated rows from 16 rows on), D^-1/2 of its row sums, a signed block."""
    isolated = () if n < 16 else (0, n // 2) if n % 2 else (n - 1,)
    a, _ = planted(n, 1 + (n > 8) + (n > 100), 1000 + n, isolated=isolated)
    s, _ = sr.scale_from_sums(a.sum(axis=1))
    x = np.random.default_rng(2000 + n).uniform(-1.0, 1.0, size=(n, BW))
    for arr in (a, s, x):
        arr.setflags(write=False)
    return a, s, x


@functools.lru_cache(maxsize=None)
def product_reference(n, row_begin, n_rows):
    """(Ypart, bound) of the row block; computed once and shared (read-only)."""
    a, s, x = product_inputs(n)
    lo, hi = row_begin, row_begin + n_rows
    part, bound = sr.product_partial(a[lo:hi], s[lo:hi], x[lo:hi])
    part.setflags(write=False)
    bound.setflags(write=False)
    return part, bound


# ---- gram / block_combine / row_sums / write_vectors / scale_from_sums / init_block ----

GRAM_N = (1, 31, 127, 128, 129, 257, 300)
GRAM_NBLK = (1, 2, 7, 9)
GRAM_WIDE_STRIDE = (129, 7)  # the (n, nblk) whose blocks lie further apart than n * 32 doubles
COMBINE_N = (1, 15, 16, 17, 100, 257)
COMBINE_NBLK = (1, 6, 9)
COMBINE_ALPHA_BETA = ((1.0, 0.0), (-1.0, 1.0), (0.5, 2.0))
ROW_SUMS_N = (1, 63, 64, 65, 300)
WRITE_N = (1, 2, 255, 256, 257, 600)
WRITE_K = (1, 7, 32)
SCALE_N = (1, 255, 256, 257, 600)
INIT_N = (1, 33, 300, 1000)


def row_sums_blocks(n):
    blocks = [(0, n), (0, 1), (n - 1, 1)]
    if n >= 2:
        blocks += [(1, n - 1), (0, n - 1), (n // 3, n // 2)]
    return list(dict.fromkeys(blocks))


def signed_blocks(n, nblk, seed):
    """nblk blocks of n x 32 signed values."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nblk, n, BW))


def sums_case(n):
    """Row sums of every kind: zero (isolated cell), tiny, huge, ordinary."""
    v = np.random.default_rng(3000 + n).uniform(0.5, 3000.0, size=n)
    v[::7] = 0.0
    v[1::11] = 1e-300
    v[2::13] = 1e300
    v[3::17] = 2.0 ** -1060  # subnormal
    return v


# ties of write_vectors: (lower index, higher index) by what separates the two in the kernel -- the same thread's
# stride (j, j + 256), neighbouring threads, the two halves of each level of the 256-wide reduction tree
def write_ties(n):
    pairs = [(3, 259), (0, 256), (300, 556), (0, 1), (254, 255), (5, 133), (127, 128), (10, 74), (64, 96), (200, 216),
             (8, 12), (1, 3), (0, 255), (255, 256), (100, 399)]
    return [p for p in pairs if p[1] < n]


def write_vectors_tie_block(n):
    """(Y, [(column, lower, higher)]): per tie pair two columns, the lower index negative and the higher positive, then
    the reverse. The tied magnitude 2 is above every other entry."""
    y = np.random.default_rng(4000 + n).uniform(-1.0, 1.0, size=(n, BW))
    cols = []
    c = 0
    for lo, hi in write_ties(n):
        for sign in (-1.0, 1.0):
            y[lo, c], y[hi, c] = sign * 2.0, -sign * 2.0
            cols.append((c, lo, hi))
            c += 1
    assert c <= BW
    return y, cols


# ---- cholesky_drop ----

def _gram_of(w):
    return np.asarray(sr._mm(w.T, w), dtype=np.float64)


def _outside(w, c):
    """A unit vector orthogonal to every column of w but c."""
    others = np.delete(w, c, axis=1)
    q, _ = np.linalg.qr(others, mode="complete")
    return q[:, others.shape[1]]


def _nearly_dependent(w, c, on, part):
    """Column c := a combination of the columns `on` with the share `part` of its norm outside the span of all others."""
    v = w[:, on] @ np.array([0.5, -2.0, 1.0])
    v /= np.linalg.norm(v)
    w[:, c] = 3.0 * (np.sqrt(1.0 - part * part) * v + part * _outside(w, c))


@functools.lru_cache(maxsize=None)
def cholesky_cases():
    """name -> (G, dropped): the Gram matrix (W^T W summed in longdouble, rounded once) and the columns that the
    documented rule drops by construction."""
    def base(seed):
        return np.random.default_rng(seed).standard_normal((64, BW))

    cases = {"identity": (np.eye(BW), ())}
    cases["random"] = (_gram_of(base(1)), ())
    w = base(2) * np.random.default_rng(20).permutation(np.logspace(-6, 6, BW))[None, :]
    cases["scaled"] = (_gram_of(w), ())
    for name, zero in (("zero_one", (5,)), ("zero_five", (0, 3, 4, 17, 31)), ("zero_all", tuple(range(BW)))):
        w = base(3)
        w[:, list(zero)] = 0.0
        cases[name] = (_gram_of(w), zero)
    w = base(4)
    w[:, 9] = w[:, 2]
    cases["duplicate"] = (_gram_of(w), (9,))
    w = base(5)
    w[:, 20] = w[:, [1, 7, 11]] @ np.array([0.5, -2.0, 1.0])
    cases["combination"] = (_gram_of(w), (20,))
    w = base(6)
    _nearly_dependent(w, 12, [1, 7, 11], 1e-3)
    cases["nearly_dependent_kept"] = (_gram_of(w), ())
    w = base(7)
    _nearly_dependent(w, 12, [1, 7, 11], 1e-7)
    cases["nearly_dependent_dropped"] = (_gram_of(w), (12,))
    w = base(8)
    w[:, 0] *= 1e-16  # squared norm about 1e-30: exhausted, yet not zero
    cases["first_dropped"] = (_gram_of(w), (0,))
    w = base(9)
    w[:, 31] = w[:, [4, 15, 30]] @ np.array([0.5, -2.0, 1.0])
    cases["last_dropped"] = (_gram_of(w), (31,))
    for g, _ in cases.values():
        g.setflags(write=False)
    return cases


def r_prev_case():
    """An upper triangular factor of an earlier pass: signed, positive diagonal."""
    r = np.triu(np.random.default_rng(77).uniform(-1.0, 1.0, size=(BW, BW)))
    r[np.arange(BW), np.arange(BW)] = np.random.default_rng(78).uniform(0.5, 2.0, size=BW)
    return r
