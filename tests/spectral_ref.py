"""spectral_ref.py -- TEST INFRASTRUCTURE ONLY.

Plain numpy references of the kernels behind secedo_amd/csrc/spectral_kernels.hpp, one per launch wrapper, written
from the operation each header comment states (not from the kernel code). Sums are formed in np.longdouble. Every
reference returns, next to its value, the bound its comparison uses: the standard forward-error bound of the sum,
evaluated on the case's own data,

    |computed - exact| <= (terms + 4) * EPS * (|left|^T |right|)         EPS = 2^-53

with `terms` the number of products summed into the element (the 4 pays for the roundings of the operands that are
themselves rounded products, such as s[j] * X[j][c], and for alpha / beta). A zero bound means an exact zero is
owed. `ratio(got, ref, bound)` is the largest error-to-bound ratio; a test passes while it is at most 1.

cholesky_drop is not compared with a second factorisation's digits but through what the header promises
(`cholesky_contract`): see there.
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
BW = 32
NORM2_DROP = 1e-26  # a column whose squared norm is at most this is exhausted
PIVOT_DROP = 1e-10  # a pivot of the unit-diagonal matrix at most this: dependent on the columns before it


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def ratio(got, ref, bound):
    """Largest |got - ref| / bound over the elements (inf where a zero bound is missed or `got` is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    err = np.abs(got.astype(LD) - np.asarray(ref, dtype=LD))
    bound = np.asarray(bound, dtype=LD) + np.zeros_like(err)
    bad = ~np.isfinite(got) | ((bound == 0) & (err != 0))
    if bad.any():
        return float("inf")
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def _mm(a, b):
    """a @ b in longdouble (numpy has no BLAS for it: plain loops, exact to 2^-64 per operation)."""
    return np.matmul(np.asarray(a, dtype=LD), np.asarray(b, dtype=LD))


# ---- row_sums / scale_from_sums / init_block ----

def row_sums(a_rows):
    """sums[r] = sum_j a_rows[r][j] -> (sums, bound)."""
    a = np.asarray(a_rows, dtype=LD)
    n = a.shape[1]
    return a.sum(axis=1), (n + 4) * EPS * np.abs(a).sum(axis=1)


def scale_from_sums(sums):
    """s = 1 / sqrt(sum) (0 for a zero sum), root = sqrt(sum). No sum is formed here: the reference is the double
    expression the header states, and a kernel whose square root and division are correctly rounded reproduces it
    bit for bit; 1 ulp (np.spacing of the reference) is granted to a division that is not. -> (s, root)"""
    sums = np.asarray(sums, dtype=np.float64)
    pos = sums > 0
    safe = np.where(pos, sums, 1.0)
    return np.where(sums == 0, 0.0, 1.0 / np.sqrt(safe)), np.where(pos, np.sqrt(safe), 0.0)


def ulp_distance(got, ref):
    """|got - ref| in units of the spacing of ref (0 where both are the same value)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    return np.where(d == 0, 0.0, d / np.spacing(np.abs(ref)))


# ---- the product in two halves ----

def product_partial(a_rows, s_rows, x_rows):
    """Ypart[i][c] = sum over the local rows j of (s[j] X[j][c]) A[j][i]; a_rows (n_rows x n), s_rows (n_rows),
    x_rows (n_rows x 32) are the local rows' parts. -> (Ypart (n x 32), bound)"""
    a = np.asarray(a_rows, dtype=LD)
    z = np.asarray(s_rows, dtype=LD)[:, None] * np.asarray(x_rows, dtype=LD)
    n_rows = a.shape[0]
    return _mm(a.T, z), (n_rows + 4) * EPS * _mm(np.abs(a).T, np.abs(z))


def product_finish(s, x, ysum, ysum_bound):
    """Y = (X + s o Ysum) / 2 -> (Y, bound): the bound of the sum times |s_i| / 2, plus 2 ulp of the result."""
    s = np.asarray(s, dtype=LD)[:, None]
    y = (np.asarray(x, dtype=LD) + s * np.asarray(ysum, dtype=LD)) / 2
    return y, np.asarray(ysum_bound, dtype=LD) * np.abs(s) / 2 + 2 * np.spacing(np.abs(y.astype(np.float64)))


def operator_matrix(a):
    """The finished product applied to the identity's columns, T = (I + D^-1/2 A D^-1/2) / 2, through the two halves
    above (32 columns at a time) -- for the CPU cross-check against oracle/spectral_oracle.py."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    s, _ = scale_from_sums(row_sums(a)[0].astype(np.float64))
    out = np.zeros((n, 0), dtype=LD)
    for c0 in range(0, n, BW):
        x = np.zeros((n, BW))
        for c in range(c0, min(n, c0 + BW)):
            x[c, c - c0] = 1.0
        part, bound = product_partial(a, s, x)
        out = np.concatenate([out, product_finish(s, x, part, bound)[0][:, :min(BW, n - c0)]], axis=1)
    return out


# ---- gram / block_combine ----

def gram(q, w):
    """G[blk] = Q[blk]^T W; q (nblk x n x 32), w (n x 32) -> (G (nblk x 32 x 32), bound)"""
    q, w = np.asarray(q, dtype=LD), np.asarray(w, dtype=LD)
    n = w.shape[0]
    g = np.stack([_mm(b.T, w) for b in q])
    return g, (n + 4) * EPS * np.stack([_mm(np.abs(b).T, np.abs(w)) for b in q])


def block_combine(q, m, alpha, beta, out):
    """beta * out + alpha * sum_blk Q[blk] M[blk]; with beta == 0 `out` is not read -> (value, bound)"""
    q, m = np.asarray(q, dtype=LD), np.asarray(m, dtype=LD)
    acc = sum(_mm(q[b], m[b]) for b in range(q.shape[0]))
    mag = sum(_mm(np.abs(q[b]), np.abs(m[b])) for b in range(q.shape[0]))
    val, mag = LD(alpha) * acc, abs(alpha) * mag
    if beta != 0:
        val = val + LD(beta) * np.asarray(out, dtype=LD)
        mag = mag + abs(beta) * np.abs(np.asarray(out, dtype=LD))
    return val, (BW * q.shape[0] + 4) * EPS * mag


# ---- cholesky_drop ----

def cholesky_alive(g):
    """Who survives by the documented rule, in longdouble: a column is dropped when its squared norm is at most
    1e-26, or when its pivot in the matrix scaled to unit diagonal -- what is left of it outside the span of the
    surviving columns before it -- is at most 1e-10. -> (alive bool[32], margin): margin is the smallest factor
    by which any decision is clear of its threshold (inf for an exact zero)."""
    g = np.asarray(g, dtype=LD)
    n = g.shape[0]
    diag = np.diag(g).copy()
    alive = diag > NORM2_DROP
    margin = np.inf
    for v in diag:
        if v != 0:
            margin = min(margin, float(v / NORM2_DROP) if v > NORM2_DROP else float(NORM2_DROP / abs(v)))
    d = np.sqrt(np.where(alive, diag, 1))
    c = g / (d[:, None] * d[None, :])
    for k in range(n):
        if not alive[k]:
            continue
        piv = c[k, k]
        if piv != 0:
            margin = min(margin, float(piv / PIVOT_DROP) if piv > PIVOT_DROP else float(PIVOT_DROP / abs(piv)))
        if piv > PIVOT_DROP:
            row = c[k, :] / np.sqrt(piv)
            c = c - np.outer(row, row)
            c[k, :] = 0
            c[:, k] = 0
        else:
            alive[k] = False
    return alive, margin


def cholesky_contract(g, r, rinv, alive):
    """What cholesky_drop promises of (R, Rinv) for the Gram matrix g and the surviving set `alive`, as error-to-bound
    ratios (each must be at most 1) plus the exact structure (asserted here):
      structure   R upper triangular, its rows outside S zero; rows and columns of Rinv outside S zero
      factor      |R_SS^T R_SS - G_SS| <= 4 gamma_33 |R_SS^T| |R_SS|
      dropped     for a dropped column c, x = R[S before c, c] solves R_bb^T x = G[S before c, c] within
                  4 gamma_33 |R_bb^T| |x|: the column went through the same scaled elimination as the survivors', so
                  it gets their bound (the plain triangular-solve bound gamma_32 times the 4 of the scaling)
      inverse     |Rinv_SS R_SS - I| <= 4 gamma_32 |Rinv_SS| |R_SS|
    Works for any factorisation that keeps the contract (the CPU test feeds it numpy's)."""
    g, r, rinv = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(rinv, dtype=np.float64)
    alive = np.asarray(alive, dtype=bool)
    assert g.shape == r.shape == rinv.shape == (BW, BW) and alive.shape == (BW,)
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(rinv))
    assert np.all(np.tril(r, -1) == 0), "R is not upper triangular"
    assert np.all(r[~alive, :] == 0), "a dropped column keeps a row of R"
    assert np.all(rinv[~alive, :] == 0) and np.all(rinv[:, ~alive] == 0), "Rinv is not zero outside the survivors"
    S = np.flatnonzero(alive)
    out = {"factor": 0.0, "dropped": 0.0, "inverse": 0.0}
    if len(S):
        rs, ris = r[np.ix_(S, S)], rinv[np.ix_(S, S)]
        out["factor"] = ratio(_mm(rs.T, rs), g[np.ix_(S, S)], 4 * gamma(33) * _mm(np.abs(rs).T, np.abs(rs)))
        out["inverse"] = ratio(_mm(ris, rs), np.eye(len(S)), 4 * gamma(32) * _mm(np.abs(ris), np.abs(rs)))
    for c in np.flatnonzero(~alive):
        b = S[S < c]
        assert np.all(r[S[S > c], c] == 0)
        if len(b):
            rb, x = r[np.ix_(b, b)], r[b, c]
            out["dropped"] = max(out["dropped"], ratio(_mm(rb.T, x), g[b, c], 4 * gamma(33) * _mm(np.abs(rb).T, np.abs(x))))
    return out


def chained_factor(r, r_prev):
    """R * R_prev -> (value, bound): the product bound over 32 terms."""
    return _mm(r, r_prev), (BW + 4) * EPS * _mm(np.abs(r), np.abs(r_prev))


# ---- write_vectors ----

def write_vectors(y, k):
    """out[:, c] = Y[:, c] / ||Y[:, c]||, signed so that the component of largest magnitude (lowest index on ties) is
    positive; a zero column stays zero. -> out (n x k) in longdouble"""
    y = np.asarray(y, dtype=np.float64)[:, :k]
    n = y.shape[0]
    out = np.zeros((n, k), dtype=LD)
    for c in range(k):
        col = y[:, c].astype(LD)
        norm = np.sqrt((col * col).sum())
        if norm == 0:
            continue
        lead = int(np.argmax(np.abs(y[:, c])))  # numpy's argmax: the first maximum = the lowest index
        out[:, c] = (-col if y[lead, c] < 0 else col) / norm
    return out
