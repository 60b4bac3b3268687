"""The four kernels of the SAM parse (secedo_amd/csrc/sam_kernels.hip) one by one on every case of tests/sam_cases.py,
each against tests/sam_ref.py byte for byte, through the test-only C ABI of tests/cpp/sam_kernels_shim.cpp
(secedo_amd/csrc/build/libsam_kernels_test.so): sam_newline_count against a count per vector, sam_line_starts against
``split_lines``, sam_size against ``parse_range`` (RefID, POS, sizes, the error word), sam_encode against the records.
The two scans between them are ``torch.cumsum``.

Every device input and output is a slice from the middle of a larger buffer. Outputs and what surrounds them hold 0xA5
before a call, and the surroundings must still hold it afterwards. The text is padded with zeros as the contract says,
to whole 16-byte vectors plus one; directly behind the padding, and in front of the text, lie tabs, digits and
newlines, so a read beyond either end changes a result. When a case has a bad line, the encode pass runs on the lines
below it, as parse_sam_range does, and nothing may be written at or after that line's offset."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import sam_cases as sc
from tests import sam_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "secedo_amd", "csrc", "build", "libsam_kernels_test.so")
GUARD = 4096  # bytes on each side
FILL = 0xA5
_vp, _u32, _u64, _int = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
_REFS = [_vp, _vp, _vp, _vp, _vp, _u32]
_SIGNATURES = {
    "newline_count": [_vp, _u64, _vp, _vp],
    "line_starts": [_vp, _u64, _vp, _u32, _u32, _int, _vp, _vp],
    "size": [_vp, _vp, _u32, _u64, _int] + _REFS + [_vp, _vp, _vp, _vp, _vp],
    "encode": [_vp, _vp, _u32] + _REFS + [_vp, _vp, _vp],
}
_shim = None


class Shim:
    """The shim's functions under their short names; a launch that fails raises."""

    def __init__(self):
        import torch  # noqa: F401  (one HIP runtime per process: torch's first, as in secedo_amd._lib)
        lib = C.CDLL(LIB)
        for name, args in _SIGNATURES.items():
            f = getattr(lib, "sam_shim_" + name)
            f.restype, f.argtypes = C.c_int, args
            setattr(self, name, self._launcher(name, f))

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
    """``nbytes`` in the middle of a larger device buffer that holds ``around`` (0xA5, or the bytes given) on both
    sides; ``data`` fills the middle (an input), else it holds 0xA5 (an output)."""

    def __init__(self, data=None, nbytes=None, dtype=np.uint8, around=None):
        import torch
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            nbytes = data.size
        self.nbytes, self.dtype = int(nbytes), dtype
        side = np.full(GUARD, FILL, np.uint8) if around is None else np.resize(np.frombuffer(around, np.uint8), GUARD)
        self.side = side
        host = np.concatenate([side, np.full(self.nbytes, FILL, np.uint8) if data is None else data, side])
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def get(self):
        """The middle as a numpy array of the buffer's type; both sides must hold what they held."""
        host = self.buf.cpu().numpy()
        assert np.array_equal(host[:GUARD], self.side) and np.array_equal(host[GUARD + self.nbytes:], self.side), \
            "a kernel wrote outside its buffer"
        return host[GUARD:GUARD + self.nbytes].view(self.dtype)


JUNK = b"\t12\t3\n4\t\n\n567\t8\n9\t0\t"  # what lies in front of the text and behind its zero padding


def text_on_device(text: bytes) -> Dev:
    n16 = (len(text) + 15) // 16
    return Dev(np.frombuffer(text + b"\0" * (n16 * 16 + 16 - len(text)), np.uint8), around=JUNK)


class Refs:
    def __init__(self, names, selected):
        raw, off, hashes, ids = sc.ref_tables(names)
        self.n = len(names)
        self.parts = [Dev(np.frombuffer(raw, np.uint8)), Dev(np.asarray(off, np.uint32)),
                      Dev(np.asarray(hashes, np.uint64)), Dev(np.asarray(ids, np.uint32)),
                      Dev(np.asarray(list(selected) or [0], np.uint8))]

    def args(self):
        return [p.ptr for p in self.parts] + [self.n]


def exclusive(values, dtype):
    """The exclusive scan of a device vector with one more entry for the total, by torch.cumsum."""
    import torch
    v = torch.from_numpy(np.ascontiguousarray(values).astype(np.int64)).cuda()
    out = torch.zeros(v.numel() + 1, dtype=torch.int64, device="cuda")
    out[1:] = torch.cumsum(v, 0)
    return out.cpu().numpy().astype(dtype)


def expected(c: sc.Case):
    text = c.text
    padded = text + b"\0" * (-len(text) % 16)
    cnt = [padded[i:i + 16].count(b"\n") for i in range(0, len(padded), 16)]
    start = sr.split_lines(text, text.endswith(b"\n"))
    info, records, err = sr.parse_range(text, list(c.names), c.selected, c.line_base, c.ends_file)
    return cnt, start, info, records, err


def run_passes(c: sc.Case, want=None):
    """The four kernels on a case, each checked against the restatement before its output feeds the next
    -> (sizes, the bytes sam_encode wrote, the lines it ran on)."""
    L = shim()
    cnt_w, start_w, info_w, records_w, err_w = want or expected(c)
    text, n16 = text_on_device(c.text), (len(c.text) + 15) // 16
    trailing = c.text.endswith(b"\n")
    n_lines = len(start_w) - 1

    cnt = Dev(nbytes=4 * n16, dtype=np.uint32)
    L.newline_count(text.ptr, n16, cnt.ptr)
    cnt = cnt.get()
    assert cnt.tolist() == cnt_w, "sam_newline_count"

    scan = Dev(exclusive(cnt, np.uint32), dtype=np.uint32)
    assert int(scan.get()[-1]) + (0 if trailing else 1) == n_lines
    start = Dev(nbytes=4 * (n_lines + 1), dtype=np.uint32)
    L.line_starts(text.ptr, n16, scan.ptr, n_lines, len(c.text), int(not trailing), start.ptr)
    assert start.get().tolist() == start_w, "sam_line_starts"

    refs = Refs(c.names, c.selected)
    size, ref, pos = Dev(nbytes=8 * n_lines, dtype=np.uint64), Dev(nbytes=4 * n_lines, dtype=np.int32), \
        Dev(nbytes=4 * n_lines, dtype=np.int32)
    err = Dev(np.full(1, sr.NO_ERROR, np.uint64), dtype=np.uint64)
    L.size(text.ptr, start.ptr, n_lines, c.line_base, int(c.ends_file), *refs.args(), size.ptr, ref.ptr, pos.ptr,
           err.ptr)
    size, err = size.get(), int(err.get()[0])
    got = list(zip(ref.get().tolist(), pos.get().tolist(), size.tolist()))
    for k, (g, w) in enumerate(zip(got, info_w)):
        assert g == w, "sam_size, line %d: (RefID, POS, size) %r, expected %r: %r" % (
            k, g, w, c.text[start_w[k]:start_w[k + 1] - 1][:200])
    assert err == err_w, "sam_size: line %d code %d, expected line %d code %d" % (err >> 8, err & 0xFF, err_w >> 8,
                                                                                err_w & 0xFF)

    limit = n_lines if err == sr.NO_ERROR else (err >> 8) - c.line_base
    off = exclusive(size, np.uint64)
    off, out = Dev(off, dtype=np.uint64), Dev(nbytes=int(off[-1]))
    L.encode(text.ptr, start.ptr, limit, *refs.args(), off.ptr, out.ptr)
    for p in [text, scan, start, off] + refs.parts:
        p.get()  # the inputs' surroundings as well
    return size, out.get().tobytes(), limit


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_kernels_equal_the_restatement(name):
    c = sc.BY_NAME[name]
    want = expected(c)
    _, start_w, info_w, records_w, err_w = want
    if c.error is not None:
        assert err_w == c.error
    size, out, limit = run_passes(c, want)
    o, r = 0, 0
    for k in range(limit):
        n = int(size[k])
        if n:
            assert out[o:o + n] == records_w[r], "sam_encode, line %d (%s): %r" % (
                k, c.why, c.text[start_w[k]:start_w[k + 1] - 1][:200])
            o, r = o + n, r + 1
    assert out[o:] == bytes([FILL]) * (len(out) - o), "sam_encode wrote at or after the first bad line's offset"
    if err_w != sr.NO_ERROR:
        assert limit < len(info_w)
        if c.name.startswith("error_"):
            assert o > 0 and len(out) > o  # records on both sides of the bad line: the check above saw bytes to keep
