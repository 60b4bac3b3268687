"""The EM refinement in plain numpy with np.longdouble sums: a high-precision restatement of the reference's
expectation_maximization.cpp:19-161 as oracle/em_oracle.c states it, for the tests (tests/test_em_cpu.py).

The order of operations is the reference's where it matters: one maximisation step per chromosome, whose sums are
added to log-likelihoods that are never reset; the difference of the two clipped to +-100; the centres floored at
theta and then renormalised; a centre without weight is log 0.25 four times. The probability vector is float64
between iterations, as in the reference's signature; every sum, logarithm and exponential is np.longdouble.

em_ref returns (prob, iterations, margin). margin is the smallest | |new - old| - 1e-2 | over all cells and all
iterations: how far the run stayed from the edge of the reference's "nothing moved by 1e-2" test (:117). A case
whose margin is far above the kernels' error has an iteration count that no summation order can change.
"""
import numpy as np

LD = np.longdouble


def _log_centres(slot, weight, n_loci, theta):
    """cluster_center (:19-39) of every locus at once: (n_loci, 4) log compositions."""
    w = np.zeros(n_loci * 4, dtype=LD)
    np.add.at(w, slot, weight)  # :23-25
    w = w.reshape(n_loci, 4)
    s = w[:, 0] + w[:, 1] + w[:, 2] + w[:, 3]  # :27
    empty = s == 0
    frac = w / np.where(empty, LD(1), s)[:, None]
    frac = np.where(frac > theta, frac, LD(theta))  # :31-32
    s = frac[:, 0] + frac[:, 1] + frac[:, 2] + frac[:, 3]  # :34
    out = np.log(frac / s[:, None])  # :35-36
    out[empty] = np.log(LD(0.25))  # :28-30
    return out


def em_ref(p, id_to_pos, theta, prob_cluster_b, max_iterations=1000):
    i2p = np.asarray(id_to_pos, dtype=np.int64)
    prob_b = np.array(prob_cluster_b, dtype=np.float64)
    n_cells = len(prob_b)
    chr_off = np.asarray(p.chr_locus_off, dtype=np.int64)
    off = np.asarray(p.locus_entry_off, dtype=np.int64)
    n_loci = len(off) - 1
    idb = np.asarray(p.id_base, dtype=np.int64)
    group, base = idb >> 2, idb & 3
    if len(idb) and (group.max() >= n_cells or group.max() >= len(i2p) or i2p[group].max() >= n_cells):
        raise ValueError("a group id indexes past prob_cluster_b or id_to_pos")
    slot = np.repeat(np.arange(n_loci, dtype=np.int64), np.diff(off)) * 4 + base
    cell = i2p[group]
    ll_a, ll_b = np.zeros(n_cells, dtype=LD), np.zeros(n_cells, dtype=LD)  # :130-131, never reset
    margin, iterations = LD(np.inf), 0
    while True:
        if iterations == max_iterations:
            raise RuntimeError("em_ref did not settle within max_iterations")
        iterations += 1
        prob_a = 1 - prob_b  # :62-65, float64 like the reference's vector
        log_a = _log_centres(slot, prob_a[group].astype(LD), n_loci, theta).reshape(-1)
        log_b = _log_centres(slot, prob_b[group].astype(LD), n_loci, theta).reshape(-1)
        for c in range(len(chr_off) - 1):  # :135-147
            e = slice(off[chr_off[c]], off[chr_off[c + 1]])
            chr_a, chr_b = np.zeros(n_cells, dtype=LD), np.zeros(n_cells, dtype=LD)
            np.add.at(chr_a, cell[e], log_a[slot[e]])  # :77-80
            np.add.at(chr_b, cell[e], log_b[slot[e]])
            ll_a += chr_a  # :142-145
            ll_b += chr_b
        prior_b = prob_b.astype(LD).sum() / n_cells  # :109-110
        prior_a = 1 - prior_b
        odds = np.exp(np.clip(ll_b - ll_a, LD(-100), LD(100)))  # :115
        with np.errstate(divide="ignore"):  # prior_a == 0: odds / 0 = inf, and the probability is 1
            new = (1 - 1 / (1 + odds * prior_b / prior_a)).astype(np.float64)  # :116
        moved = np.abs(new.astype(LD) - prob_b.astype(LD))
        margin = min(margin, np.min(np.abs(moved - LD(1e-2))))
        prob_b = new
        if np.all(moved < 1e-2):  # :117
            return prob_b, iterations, float(margin)
