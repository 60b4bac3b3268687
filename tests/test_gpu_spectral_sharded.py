"""The row-sharded spectral solve (secedo_spectral_eigs_rows_device), every rank of a partition, in one process and
without a process group or threads.

include/secedo_spectral.h promises that everything but the partial products is replicated and deterministic. So:
  1. world size 1 with a callback that records every buffer it is handed (the row sums, then one n x 32 partial per
     block product) and leaves it unchanged must return what secedo_spectral_eigs_device returns, bit for bit: the two
     routes do the same arithmetic in the same order (the segments' sum, then (X + s o sum) / 2, in one kernel or two);
  2. each rank of a partition, run alone, whose callback answers call k with recording k -- what a correct all-reduce
     would have returned -- must make the same number of calls and return the same eigenpairs, bit for bit;
  3. the buffers the ranks handed in must add up to the recording: the row sums exactly (each row is summed by the one
     rank that holds it, in the same order), product k within 4 n eps max(s) ||A[:, i]||_2 for element (i, c) -- the
     multiplied blocks have orthonormal columns, so ||s o x_c|| <= max(s)."""
import ctypes as C

import numpy as np
import pytest

from secedo_amd import _lib
from secedo_amd.distributed import _DevicePointer, row_range
from tests import spectral_ref as sr
from tests.test_gpu_spectral import planted

pytestmark = pytest.mark.gpu
BW = sr.BW
N_VALUES, N_VECTORS = 20, 7


def _solve_rows(a, lo, rows, on_buffer):
    """The raw ABI on rows [lo, lo + rows) of `a` (a CUDA tensor), on a stream of its own; on_buffer(k, buf) is the
    all-reduce of call k (buf: the device buffer as a tensor, changed in place) -> (rc, vals, vecs, info, calls)."""
    import torch
    n = a.shape[0]
    stream = torch.cuda.Stream()
    calls, failure = [0], []

    def allreduce(_ctx, ptr, count, st):
        try:
            assert (st or 0) == stream.cuda_stream
            with torch.cuda.stream(stream):
                on_buffer(calls[0], torch.as_tensor(_DevicePointer(ptr, count), device=a.device))
            calls[0] += 1
            return 0
        except Exception as e:  # an exception must not cross the C frames above
            failure.append(e)
            return 1

    hook = _lib.ALLREDUCE_SUM_FN(allreduce)
    vals, info = np.full(N_VALUES, np.nan), _lib.SpectralInfo()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        block = a[lo:lo + rows].contiguous()
        vecs = torch.full((N_VECTORS, n), float("nan"), dtype=torch.float64, device=a.device)
        rc = _lib.lib().secedo_spectral_eigs_rows_device(
            0, block.data_ptr() if rows else None, lo, rows, n, N_VALUES, N_VECTORS, 0.0, 0, _lib.ptr(vals),
            vecs.data_ptr(), C.byref(info), hook, None, stream.cuda_stream)
    stream.synchronize()
    return rc, vals, vecs.cpu().numpy(), info, calls[0], failure


def _recorded(a_host):
    """Step 1 -> (the device matrix, the recording, eigenvalues, eigenvectors)."""
    import torch
    n = a_host.shape[0]
    a = torch.from_numpy(a_host).cuda()
    recording = []
    rc, vals, vecs, info, calls, failure = _solve_rows(a, 0, n, lambda k, buf: recording.append(buf.clone()))
    assert rc == 0 and not failure and info.converged
    assert calls == len(recording) == 1 + info.block_products
    assert recording[0].numel() == n and all(r.numel() == n * BW for r in recording[1:])
    # the plain single-device entry on the same matrix: the same bits
    vals1, info1 = np.full(N_VALUES, np.nan), _lib.SpectralInfo()
    vecs1 = torch.full((N_VECTORS, n), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().secedo_spectral_eigs_device(0, a.data_ptr(), n, N_VALUES, N_VECTORS, 0.0, 0, _lib.ptr(vals1),
                                                      vecs1.data_ptr(), C.byref(info1),
                                                      torch.cuda.current_stream().cuda_stream))
    assert (info1.cycles, info1.block_products) == (info.cycles, info.block_products)
    assert np.array_equal(vals.view(np.uint64), vals1.view(np.uint64))
    assert np.array_equal(vecs.view(np.uint64), vecs1.cpu().numpy().view(np.uint64))
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(vecs))
    return a, recording, vals, vecs


def _thirds(n):
    return [(lo, hi - lo) for lo, hi in (row_range(n, r, 3) for r in range(3))]


PARTITIONS = [
    (300, [(0, 150), (150, 150)]),
    (300, [(0, 1), (1, 298), (299, 1)]),
    (300, [(0, 0), (0, 300), (300, 0)]),
    (300, [(0, 64), (64, 65), (129, 171)]),
    (257, _thirds(257)),  # odd: every rank on the clamped and masked path
    (640, [(0, 129), (129, 383), (512, 128)]),  # several segments and the straight-line path at odd row_begin
]
_cache = {}


def _case(n):
    if n not in _cache:
        a_host, _ = planted(n, 3, 700 + n, isolated=(5,))
        _cache[n] = (a_host,) + _recorded(a_host)
    return _cache[n]


@pytest.mark.parametrize("n,partition", PARTITIONS, ids=lambda v: str(v).replace(" ", "") if isinstance(v, list) else str(v))
def test_every_rank_alone_reproduces_the_whole(n, partition):
    assert partition[0][0] == 0 and sum(r for _, r in partition) == n
    assert all(p[0] + p[1] == q[0] for p, q in zip(partition, partition[1:]))
    a_host, a, recording, vals, vecs = _case(n)
    own = []
    for lo, rows in partition:
        mine = []

        def exchange(k, buf):
            assert k < len(recording) and buf.numel() == recording[k].numel()
            mine.append(buf.clone())
            buf.copy_(recording[k])

        rc, r_vals, r_vecs, info, calls, failure = _solve_rows(a, lo, rows, exchange)
        assert rc == 0 and not failure, failure
        assert calls == len(recording), "rank (%d, %d) made %d all-reduce calls, the whole matrix %d" % (
            lo, rows, calls, len(recording))
        assert np.array_equal(r_vals.view(np.uint64), vals.view(np.uint64)), (lo, rows)
        assert np.array_equal(r_vecs.view(np.uint64), vecs.view(np.uint64)), (lo, rows)
        own.append([m.cpu().numpy() for m in mine])
    rec = [r.cpu().numpy() for r in recording]
    # the row sums: the rank's rows bit for bit, zero elsewhere
    for (lo, rows), bufs in zip(partition, own):
        inside = np.zeros(n, dtype=bool)
        inside[lo:lo + rows] = True
        assert np.array_equal(bufs[0][inside].view(np.uint64), rec[0][inside].view(np.uint64)), (lo, rows)
        assert np.all(bufs[0][~inside] == 0.0), (lo, rows)
    # the products: the ranks' partials add up to the whole matrix's
    s, _ = sr.scale_from_sums(rec[0])
    bound = (4 * n * sr.EPS * s.max() * np.linalg.norm(a_host, axis=0))[:, None]
    worst = 0.0
    for k in range(1, len(rec)):
        total = sum(bufs[k].astype(sr.LD) for bufs in own).reshape(n, BW)
        worst = max(worst, sr.ratio(rec[k].reshape(n, BW), total, bound))
    print("sharded n=%d %s: %d products, worst |sum of partials - whole| / bound %.3g" % (
        n, partition, len(rec) - 1, worst))
    assert worst <= 1.0


def test_a_recording_cut_short_fails_the_solve():
    """An all-reduce that fails (here: asked for more buffers than the recording holds) must surface as an error."""
    a_host, a, recording, vals, vecs = _case(300)
    short = recording[:len(recording) // 2]

    def exchange(k, buf):
        assert k < len(short)
        buf.copy_(short[k])

    rc, _, _, _, calls, failure = _solve_rows(a, 0, 150, exchange)
    assert calls == len(short) and len(failure) == 1 and rc != 0
    with pytest.raises(_lib.SecedoError):
        _lib.check(rc)
