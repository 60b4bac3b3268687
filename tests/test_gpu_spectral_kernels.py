"""The kernels of the spectral step (secedo_amd/csrc/spectral_kernels.hip) one by one, each against the plain
longdouble reference of its own operation (tests/spectral_ref.py) at the shapes of tests/spectral_cases.py, through
the test-only C ABI of tests/cpp/spectral_kernels_shim.cpp (secedo_amd/csrc/build/libspectral_kernels_test.so).

Every comparison uses the forward-error bound of the sum on the case's own data and prints the largest
error-to-bound ratio it saw; above 1 the kernel is at fault. Every device input and output is a slice from the middle
of a larger buffer with 64 KiB of NaN on both sides; scratch and outputs hold NaN before the call, so a read past an
edge that reaches a result, or scratch used before it is written, shows as NaN, and a write past an edge in the
guards.

The cap of 64 product segments needs more than 8064 local rows and stays with tests/test_gpu_fullsize.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import spectral_cases as sc
from tests import spectral_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW = sr.BW
GUARD = 8192  # doubles: 64 KiB
_vp, _u32, _u64, _f64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
_SIGNATURES = {
    "product_segments": (_u32, [_u32, _u32]),
    "gram_chunks": (_u32, [_u32]),
    "pad16": (_u32, [_u32]),
    "row_sums": (C.c_int, [_vp, _u32, _u32, _u32, _vp, _vp]),
    "scale_from_sums": (C.c_int, [_u32, _vp, _vp, _vp, _vp]),
    "laplacian": (C.c_int, [_vp, _vp, _u32, _vp, _vp]),
    "init_block": (C.c_int, [_u32, _vp, _vp, _vp]),
    "product_partial": (C.c_int, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "product_finish": (C.c_int, [_u32, _vp, _vp, _vp, _vp, _vp]),
    "gram": (C.c_int, [_u32, _vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    "block_combine": (C.c_int, [_u32, _vp, _u64, _u32, _vp, _f64, _f64, _vp, _vp]),
    "cholesky_drop": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "write_vectors": (C.c_int, [_u32, _vp, _u32, _vp, _vp]),
}
_shim = None


class Shim:
    """The shim's functions under their short names; a launch that fails raises."""

    def __init__(self):
        import torch  # noqa: F401  (one HIP runtime per process: torch's first, as in secedo_amd._lib)
        lib = C.CDLL(os.path.join(ROOT, "secedo_amd", "csrc", "build", "libspectral_kernels_test.so"))
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(lib, "spectral_shim_" + name)
            f.restype, f.argtypes = res, args
            setattr(self, name, f if res is _u32 else self._launcher(name, f))

    @staticmethod
    def _launcher(name, f):
        def call(*args):
            import torch
            rc = f(*args, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, "%s: hipError %d" % (name, rc)
            torch.cuda.synchronize()
        return call


def shim():
    global _shim
    if _shim is None:
        _shim = Shim()
    return _shim


class Dev:
    """`count` doubles in the middle of a larger device buffer, NaN on both sides; `data` fills the middle, else it
    holds `fill` (NaN: an output or scratch)."""

    def __init__(self, data=None, count=None, fill=float("nan")):
        import torch
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
            count = data.size
        self.count = int(count)
        self.buf = torch.full((2 * GUARD + self.count,), float("nan"), dtype=torch.float64, device="cuda")
        self.mid = self.buf[GUARD:GUARD + self.count]
        if data is not None:
            self.mid.copy_(torch.from_numpy(data))
        elif not np.isnan(fill):
            self.mid.fill_(fill)
        self.ptr = self.buf.data_ptr() + GUARD * 8

    def get(self, *shape):
        """The middle as a numpy array; the guards must still be NaN."""
        import torch
        assert bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.count:]).all()), \
            "a kernel wrote outside its buffer"
        out = self.mid.cpu().numpy()
        return out.reshape(shape) if shape else out


def test_sizing_functions_match_their_restatement():
    L = shim()
    for n in list(range(1, 700)) + [4095, 4096, 4097, 8000, 16000, 40000]:
        assert L.pad16(n) == sc.pad16(n) and L.gram_chunks(n) == sc.gram_chunks(n)
        for rows in {0, 1, 63, 64, 65, 127, 128, 129, 256, 257, n // 3, n // 2, n - 1, n}:
            if rows <= n:
                assert L.product_segments(n, rows) == sc.product_segments(n, rows), (n, rows)
    assert L.product_segments(40000, 8065) == 7 and L.product_segments(4096, 4096) == 32


# ---- row_sums, scale_from_sums, init_block ----

@pytest.mark.parametrize("n", sc.ROW_SUMS_N)
def test_row_sums(n):
    a, _, _ = sc.product_inputs(n) if n in sc.PRODUCT_N else (sc.planted(n, 3, 1000 + n, isolated=(0, 7, n - 1))[0], 0, 0)
    signed = a * np.where(np.random.default_rng(n).random(a.shape) < 0.5, -1.0, 1.0)  # sums that cancel as well
    worst = 0.0
    for mat in (a, signed):
        for lo, rows in sc.row_sums_blocks(n):
            ref, bound = sr.row_sums(mat[lo:lo + rows])
            sums, rows_in = Dev(count=n, fill=-7.25), Dev(mat[lo:lo + rows])
            shim().row_sums(rows_in.ptr, n, lo, rows, sums.ptr)
            got = sums.get()
            assert np.all(got[:lo] == -7.25) and np.all(got[lo + rows:] == -7.25), (lo, rows)
            worst = max(worst, sr.ratio(got[lo:lo + rows], ref, bound))
    print("row_sums n=%d: worst error/bound %.3g" % (n, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("n", sc.SCALE_N)
def test_scale_from_sums(n):
    sums = sc.sums_case(n)
    s_ref, root_ref = sr.scale_from_sums(sums)
    s, root, sums_in = Dev(count=n), Dev(count=n), Dev(sums)
    shim().scale_from_sums(n, sums_in.ptr, s.ptr, root.ptr)
    s, root = s.get(), root.get()
    zero = sums == 0
    assert np.all(s[zero] == 0.0) and np.all(root[zero] == 0.0) and not np.any(np.signbit(s[zero]))
    worst = max(np.max(sr.ulp_distance(s, s_ref)), np.max(sr.ulp_distance(root, root_ref)))
    print("scale_from_sums n=%d: worst distance %.3g ulp" % (n, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("n", sc.INIT_N)
def test_init_block(n):
    root = np.random.default_rng(n).uniform(0.0, 50.0, size=n)
    root[::5] = 0.0
    runs = []
    for _ in range(2):
        x, root_in = Dev(count=n * BW), Dev(root)
        shim().init_block(n, root_in.ptr, x.ptr)
        runs.append(x.get(n, BW))
    x = runs[0]
    assert np.array_equal(x[:, 0].view(np.uint64), root.view(np.uint64))  # column 0 is root, bit for bit
    assert np.array_equal(x.view(np.uint64), runs[1].view(np.uint64))  # a fixed fill: the same on every call
    assert np.all(np.abs(x[:, 1:]) < 1.0)
    cols = {x[:, c].tobytes() for c in range(1, BW)}
    assert len(cols) == BW - 1  # no two of the 31 random columns are equal
    if n >= 300:  # a fill, not a constant: both signs, spread over the interval
        assert x[:, 1:].min() < -0.99 and x[:, 1:].max() > 0.99 and abs(x[:, 1:].mean()) < 0.05


@pytest.mark.parametrize("n", (1, 65, 300))
def test_laplacian(n):
    """out = I - diag(s) A diag(s): two rounded products and one difference per element, so 3 EPS |s_r s_c a_rc| plus one
    ulp of the result; an isolated cell's row is the unit vector, exactly."""
    a, _ = sc.planted(n, 2, 1500 + n, isolated=(0, n // 2) if n > 1 else ())
    s, _ = sr.scale_from_sums(a.sum(axis=1))
    out, a_in, s_in = Dev(count=n * n), Dev(a), Dev(s)
    shim().laplacian(a_in.ptr, s_in.ptr, n, out.ptr)
    got = out.get(n, n)
    prod = s.astype(sr.LD)[:, None] * s.astype(sr.LD)[None, :] * a.astype(sr.LD)
    ref = np.eye(n, dtype=sr.LD) - prod
    worst = sr.ratio(got, ref, 3 * sr.EPS * np.abs(prod) + np.spacing(np.abs(ref.astype(np.float64))))
    print("laplacian n=%d: worst error/bound %.3g" % (n, worst))
    assert worst <= 1.0 and np.array_equal(got, got.T)
    assert got[0, 0] == 1.0 and np.count_nonzero(got[0]) == 1


# ---- the product ----

def _product(n, lo, rows, fused):
    """product_partial on the row block -> Ypart (split form) or the finished Y (fused form)."""
    L = shim()
    a, s, x = sc.product_inputs(n)
    z = Dev(count=(L.pad16(n) + 64) * BW)
    p = Dev(count=L.product_segments(n, rows) * L.pad16(n) * BW)
    out, rows_in, s_in, x_in = Dev(count=n * BW), Dev(a[lo:lo + rows]), Dev(s), Dev(x)
    L.product_partial(rows_in.ptr, n, lo, rows, s_in.ptr, x_in.ptr, z.ptr, p.ptr,
                      None if fused else out.ptr, out.ptr if fused else None)
    z.get(), p.get()  # the guards of the scratch
    return out.get(n, BW)


@pytest.mark.parametrize("n", sc.PRODUCT_N)
def test_product_partial_and_finish(n):
    a, s, x = sc.product_inputs(n)
    worst = {"partial": 0.0, "fused": 0.0, "finish": 0.0, "partition": 0.0}
    got = {}
    for lo, rows in sc.product_blocks(n):
        assert shim().product_segments(n, rows) == sc.product_segments(n, rows)
        ref, bound = sc.product_reference(n, lo, rows)
        got[lo, rows] = _product(n, lo, rows, fused=False)
        r = sr.ratio(got[lo, rows], ref, bound)
        assert r <= 1.0, "product_partial n=%d block (%d, %d): error/bound %.3g" % (n, lo, rows, r)
        worst["partial"] = max(worst["partial"], r)
    # the full block in both forms: finished in the last kernel, or by product_finish on the (one rank's) sum
    ref, bound = sc.product_reference(n, 0, n)
    y_ref, y_bound = sr.product_finish(s, x, ref, bound)
    worst["fused"] = sr.ratio(_product(n, 0, n, fused=True), y_ref, y_bound)
    y, s_in, x_in, sum_in = Dev(count=n * BW), Dev(s), Dev(x), Dev(got[0, n])
    shim().product_finish(n, s_in.ptr, x_in.ptr, sum_in.ptr, y.ptr)
    worst["finish"] = sr.ratio(y.get(n, BW), y_ref, y_bound)
    # product_finish on its own input: nothing but the two roundings of s * Ysum and of the sum
    f_ref, f_bound = sr.product_finish(s, x, got[0, n], 2 * sr.EPS * np.abs(got[0, n]))
    worst["finish"] = max(worst["finish"], sr.ratio(y.get(n, BW), f_ref, f_bound))
    for part in sc.product_partitions(n):
        total = sum(got[b].astype(sr.LD) for b in part)
        worst["partition"] = max(worst["partition"],
                                 sr.ratio(got[0, n], total, sum(sc.product_reference(n, *b)[1] for b in part)))
    print("product n=%d, %d row blocks: worst error/bound %s" % (
        n, len(got), ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


def test_product_cases_reach_one_two_three_and_five_segments():
    seen = {shim().product_segments(n, rows) for n in sc.PRODUCT_N for _, rows in sc.product_blocks(n)}
    assert {1, 2, 3, 5} <= seen, seen


# ---- gram, block_combine ----

@pytest.mark.parametrize("n", sc.GRAM_N)
def test_gram(n):
    L = shim()
    worst = 0.0
    for nblk in sc.GRAM_NBLK:
        stride = n * BW + (96 if (n, nblk) == sc.GRAM_WIDE_STRIDE else 0)
        q = sc.signed_blocks(n, nblk, 5000 + 10 * n + nblk)
        w = sc.signed_blocks(n, 1, 6000 + 10 * n + nblk)[0]
        laid = np.full((nblk - 1) * stride + n * BW, np.nan)  # NaN between blocks that lie apart
        for b in range(nblk):
            laid[b * stride:b * stride + n * BW] = q[b].reshape(-1)
        gp = Dev(count=L.gram_chunks(n) * nblk * BW * BW)
        g, q_in, w_in = Dev(count=nblk * BW * BW), Dev(laid), Dev(w)
        L.gram(n, q_in.ptr, stride, nblk, w_in.ptr, gp.ptr, g.ptr)
        gp.get()
        ref, bound = sr.gram(q, w)
        r = sr.ratio(g.get(nblk, BW, BW), ref, bound)
        assert r <= 1.0, "gram n=%d nblk=%d: error/bound %.3g" % (n, nblk, r)
        worst = max(worst, r)
    # W = Q[0]: the Gram matrix of a block with itself, as the orthonormalisation calls it (same buffer twice)
    q = sc.signed_blocks(n, 1, 7000 + n)
    qd, gp, g = Dev(q), Dev(count=L.gram_chunks(n) * BW * BW), Dev(count=BW * BW)
    L.gram(n, qd.ptr, n * BW, 1, qd.ptr, gp.ptr, g.ptr)
    ref, bound = sr.gram(q, q[0])
    got = g.get(BW, BW)
    worst = max(worst, sr.ratio(got, ref[0], bound[0]))
    print("gram n=%d: worst error/bound %.3g" % (n, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("n", sc.COMBINE_N)
def test_block_combine(n):
    worst = 0.0
    for nblk in sc.COMBINE_NBLK:
        q = sc.signed_blocks(n, nblk, 8000 + 10 * n + nblk)
        m = np.random.default_rng(8500 + 10 * n + nblk).uniform(-1.0, 1.0, size=(nblk, BW, BW))
        out0 = sc.signed_blocks(n, 1, 9000 + 10 * n + nblk)[0]
        for alpha, beta in sc.COMBINE_ALPHA_BETA:
            out = Dev(count=n * BW) if beta == 0.0 else Dev(out0)  # beta == 0: NaN on entry, never read
            q_in, m_in = Dev(q), Dev(m)
            shim().block_combine(n, q_in.ptr, n * BW, nblk, m_in.ptr, alpha, beta, out.ptr)
            got = out.get(n, BW)
            assert np.all(np.isfinite(got)), (n, nblk, alpha, beta)
            ref, bound = sr.block_combine(q, m, alpha, beta, out0)
            r = sr.ratio(got, ref, bound)
            assert r <= 1.0, "block_combine n=%d nblk=%d alpha=%g beta=%g: error/bound %.3g" % (n, nblk, alpha, beta, r)
            worst = max(worst, r)
    print("block_combine n=%d: worst error/bound %.3g" % (n, worst))


# ---- cholesky_drop ----

def _cholesky(g, r_prev):
    import torch
    rinv, r = Dev(count=BW * BW), Dev(count=BW * BW)
    alive = torch.full((4 * GUARD + BW,), -1, dtype=torch.int32, device="cuda")  # 64 KiB of -1 on both sides
    g_in, prev_in = Dev(g), None if r_prev is None else Dev(r_prev)
    shim().cholesky_drop(g_in.ptr, prev_in and prev_in.ptr, rinv.ptr, r.ptr,
                         alive.data_ptr() + 2 * GUARD * 4)
    alive = alive.cpu().numpy()
    assert np.all(alive[:2 * GUARD] == -1) and np.all(alive[2 * GUARD + BW:] == -1)
    alive = alive[2 * GUARD:2 * GUARD + BW]
    assert set(alive.tolist()) <= {0, 1}
    return r.get(BW, BW), rinv.get(BW, BW), alive.astype(bool)


@pytest.mark.parametrize("name", sorted(sc.cholesky_cases()))
def test_cholesky_drop(name):
    g, dropped = sc.cholesky_cases()[name]
    alive_ref, margin = sr.cholesky_alive(g)
    assert margin >= 100.0 and sorted(np.flatnonzero(~alive_ref)) == sorted(dropped)
    r, rinv, alive = _cholesky(g, None)
    assert np.array_equal(alive, alive_ref), (np.flatnonzero(~alive), dropped)
    ratios = sr.cholesky_contract(g, r, rinv, alive_ref)
    assert np.all(np.diag(r)[alive_ref] > 0)
    # with the factor of an earlier pass: the same survivors and inverse, and R * R_prev in place of R
    r_prev = sc.r_prev_case()
    r2, rinv2, alive2 = _cholesky(g, r_prev)
    assert np.array_equal(alive2, alive_ref)
    both = sr.cholesky_contract(g, r, rinv2, alive_ref)
    ratios["inverse"] = max(ratios["inverse"], both["inverse"])
    ref, bound = sr.chained_factor(r, r_prev)
    ratios["chained"] = sr.ratio(r2, ref, bound)
    assert np.all(r2[~alive_ref, :] == 0) and np.all(np.tril(r2, -1) == 0)
    # no alive pointer: allowed, the orthonormalisation's first pass calls it so
    rinv3, r3, g_in = Dev(count=BW * BW), Dev(count=BW * BW), Dev(g)
    shim().cholesky_drop(g_in.ptr, None, rinv3.ptr, r3.ptr, None)
    assert np.array_equal(r3.get(BW, BW), r) and np.array_equal(rinv3.get(BW, BW), rinv)
    print("cholesky_drop %s: margin %.3g, error/bound %s" % (name, margin, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0, ratios


# ---- write_vectors ----

def _write_vectors(y, k):
    n = y.shape[0]
    out, y_in = Dev(count=n * k), Dev(y)
    shim().write_vectors(n, y_in.ptr, k, out.ptr)
    return out.get(k, n).T  # column-major n x k


def _check_vectors(y, k, got):
    n = y.shape[0]
    ref = sr.write_vectors(y, k)
    r = sr.ratio(got, ref, 2 * np.spacing(np.abs(np.asarray(ref, dtype=np.float64))))
    norms = np.sqrt((got.astype(sr.LD) ** 2).sum(axis=0))
    zero = ~np.any(y[:, :k] != 0, axis=0)
    assert np.all(got[:, zero] == 0.0)  # a zero column gives zeros, not NaN
    rn = float(np.max(np.abs(norms[~zero] - 1) / ((n + 4) * sr.EPS))) if (~zero).any() else 0.0
    for c in np.flatnonzero(~zero):
        assert got[int(np.argmax(np.abs(y[:, c]))), c] > 0
    return r, rn


@pytest.mark.parametrize("n", sc.WRITE_N)
def test_write_vectors(n):
    worst = [0.0, 0.0]
    for k in sc.WRITE_K:
        y = sc.signed_blocks(n, 1, 9500 + 10 * n + k)[0] * np.logspace(-3, 3, BW)[None, :]
        y[:, k // 2] = 0.0
        r, rn = _check_vectors(y, k, _write_vectors(y, k))
        assert r <= 1.0 and rn <= 1.0, (n, k, r, rn)
        worst = [max(worst[0], r), max(worst[1], rn)]
    # exact ties: the lower index decides the sign
    y, cols = sc.write_vectors_tie_block(n)
    got = _write_vectors(y, BW)
    for c, lo, hi in cols:
        assert got[lo, c] > 0 and got[hi, c] < 0 and got[lo, c] == -got[hi, c], (n, c, lo, hi)
    r, rn = _check_vectors(y, BW, got)
    worst = [max(worst[0], r), max(worst[1], rn)]
    print("write_vectors n=%d: worst error/bound: values %.3g, unit norm %.3g (%d tie columns)" % (n, *worst, len(cols)))
    assert max(worst) <= 1.0
