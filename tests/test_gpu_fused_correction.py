"""The sparse-loci path with the correction as accumulate_counts' epilogue (the default) against accumulate_counts +
correct_tiles (SECEDO_CORRECT_FUSED=0). The switch is read once per process: each side runs in a child process. Both
sides read the flagged entries' lists the packing built. Accumulators, matrices and work counters must be
bit-identical, and so must the flagged entries' lists."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Each case: (name, pileup expression, num_cells, max_fragment_length, block_cells, packing). 4100 cells in 128-cell
# blocks are 561 tiles, 3000 cells in 64-cell blocks 1128: a launch of all of them has one workgroup per tile, the
# shape of C3 and C5.
CASES = [
    ("c3_shape", "synth_pileup(4100, 20000, 4, 30000, 0.03, seed=11)", 4100, 1000, 128, "auto"),
    ("c5_shape", "synth_pileup(3000, 20000, 4, 30000, 0.01, seed=12)", 3000, 1000, 64, "auto"),
    # reads longer than max_fragment_length are split at flushes; many tail and multi-locus flags
    ("split_reads", "random_pileup(21, 4100, 2, 300, 40, 5, frag_min=30, frag_max=500, dup_frac=0.03)", 4100, 300, 128,
     "auto"),
    ("host_packing", "random_pileup(22, 4100, 2, 300, 40, 5, frag_min=30, frag_max=500, dup_frac=0.03)", 4100, 300,
     128, "host"),
    # reads that share more than 128 loci: the kernels note those pairs, the host adds their terms
    ("beyond_128", "random_pileup(23, 4100, 1, 700, 30, 1, frag_min=300, frag_max=650, dup_frac=0.0)", 4100, 1000, 128,
     "auto"),
]

SCRIPT = r'''
import ctypes as C, hashlib, sys
import numpy as np, torch
sys.path.insert(0, ROOT)
import secedo_amd
from secedo_amd import _lib
from secedo_amd.synth import synth_pileup
from tests.pileup_gen import random_pileup

RATES = (0.01, 0.5, 0.01)
out = {}

def digest(t):
    a = t.detach().cpu().numpy()
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)

def flag_lists(plan):
    L = _lib.lib()
    n = C.c_uint64()
    rc = L.secedo_simmat_debug_flag_lists(plan._h, C.byref(n), None, None, None)
    if rc != 0:
        return None
    nb = (plan.num_cells + plan.block_cells - 1) // plan.block_cells
    grp = np.zeros(nb * (plan.num_loci + 1), np.uint32)
    rec = np.zeros((max(n.value, 1), 4), np.uint32)
    idx = np.zeros(max(n.value, 1), np.uint32)
    _lib.check(L.secedo_simmat_debug_flag_lists(plan._h, C.byref(n), _lib.ptr(grp), _lib.ptr(rec), _lib.ptr(idx)))
    return grp, rec[:n.value], idx[:n.value]

def fused(plan):
    return _lib.lib().secedo_simmat_last_correction_fused(plan._h)

for name, expr, n, mfl, block, packing in CASES:
    p = eval(expr)
    with secedo_amd.SimilarityMatrixPlan(0) as plan:
        plan.set_packing(packing)
        plan.prepare(p, n, mfl, None, 2, block_cells=block)
        assert plan.pair_kernel == "accumulate_counts", (name, plan.pair_kernel)
        assert plan.block_cells == block, name
        T = plan.num_tiles
        lists = flag_lists(plan)  # (the packing's lists, before any accumulate)
        out[name + "/lists_after_prepare"] = np.array([lists is not None])
        r = {}
        acc = plan.new_acc()
        acc.fill_(-5)
        plan.accumulate(acc, *RATES, overwrite=True)                      # assign
        r["assign"] = (digest(acc), plan.last_counts(), fused(plan))
        grp, rec, idx = lists
        out[name + "/grp"], out[name + "/rec"], out[name + "/idx"] = grp, rec, idx
        plan.accumulate(acc, *RATES)                                      # += onto a non-zero accumulator
        r["accumulate"] = (digest(acc), plan.last_counts(), fused(plan))
        perm = np.random.default_rng(5).permutation(T).astype(np.uint32)
        acc2 = plan.new_acc()
        acc2.fill_(7)
        plan.accumulate_list(acc2, *RATES, perm, overwrite=True)          # assign_list
        r["assign_list"] = (digest(acc2), plan.last_counts(), fused(plan))
        plan.accumulate_list(acc2, *RATES, perm[: T // 2])                # accumulate_list
        r["accumulate_list"] = (digest(acc2), plan.last_counts(), fused(plan))
        acc3 = plan.new_acc()
        acc3.zero_()
        plan.accumulate(acc3, *RATES, 0, min(T, 36))                       # a launch of few tiles
        r["few_tiles"] = (digest(acc3), plan.last_counts(), fused(plan))
        for norm in ("ADD_MIN", "EXPONENTIATE", "SCALE_MAX_1"):
            m = plan.finalize(acc, norm)
            r["finalize_" + norm] = (digest(m), (0, 0), 0)
            acc4 = plan.new_acc()
            m = plan.assign_finalize(acc4, *RATES, norm)
            r["assign_finalize_" + norm] = (digest(m), plan.last_counts(), fused(plan))
        raw = plan.finalize_raw(acc).cpu().numpy()
        out[name + "/raw_nonzero"] = np.array([np.count_nonzero(raw)])
        out[name + "/max_read_entries"] = np.array([plan.max_read_entries])
        for op, (d, counts, f) in r.items():
            out[name + "/" + op + "/digest"] = d
            out[name + "/" + op + "/counts"] = np.asarray(counts, dtype=np.uint64)
            out[name + "/" + op + "/fused"] = np.array([f])
    torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
'''


def _run(tmp_path, tag, env):
    script = "ROOT = %r\nCASES = %r\n" % (ROOT, CASES) + SCRIPT
    out = str(tmp_path / (tag + ".npz"))
    subprocess.run([sys.executable, "-c", script, out], check=True, env=dict(os.environ, **env), timeout=900)
    return dict(np.load(out))


@pytest.mark.gpu
def test_fused_correction_matches_correct_tiles_on_the_packed_lists(tmp_path):
    new = _run(tmp_path, "fused", {})
    old = _run(tmp_path, "separate", {"SECEDO_CORRECT_FUSED": "0"})
    assert set(new) == set(old)
    for key in sorted(new):
        if key.endswith("/fused") or key.endswith("/lists_after_prepare"):
            continue
        assert np.array_equal(new[key], old[key]), key
    tails, multis = [], []
    for name, *_ in CASES:
        # the packing built the lists on both sides
        assert new[name + "/lists_after_prepare"][0] and old[name + "/lists_after_prepare"][0], name
        # which launches ran the epilogue: every launch with one workgroup per tile, never a launch of few tiles
        for op in ("assign", "accumulate", "assign_list", "assign_finalize_ADD_MIN"):
            assert new[name + "/" + op + "/fused"][0] == 1, (name, op)
        assert new[name + "/few_tiles/fused"][0] == 0, name
        assert not any(old[k][0] for k in old if k.endswith("/fused")), name
        # (beyond_128: every pair shares hundreds of loci, where the reference's wrapped sums give D = 0)
        assert name == "beyond_128" or new[name + "/raw_nonzero"][0] > 0, name
        # the lists hold both kinds of flag: never flushed (bit 18 of the record's first word) and multi-locus
        rec = new[name + "/rec"]
        assert len(rec) > 0, name
        tails.append(((rec[:, 0] >> 18) & 1).astype(bool))
        multis.append((rec[:, 1] != 0) | ((rec[:, 0] & (3 << 19)) != 0))
        idx = new[name + "/idx"]
        assert np.all(np.diff(idx.astype(np.int64)) > 0), name  # compact, in packed-entry order
    tail, multi = np.concatenate(tails), np.concatenate(multis)
    assert (tail & ~multi).any() and (tail & multi).any() and (multi & ~tail).any()
    assert new["beyond_128/max_read_entries"][0] > 128
