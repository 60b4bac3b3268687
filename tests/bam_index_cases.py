"""The BAMs and indexes of tests/test_gpu_pileup_bam_index.py that are corrupt or do not fit each other, built here so
that tests/test_bam_index_cpu.py can put the same bytes through the host programs under the sanitizers
(secedo_amd/csrc/build/bgzf_inflate_test, bam_walk_test, bam_index_test) before a GPU sees them, as
tests/bam_device_cases.py does for the device route's tests. Everything is seeded: two calls give the same bytes."""
from __future__ import annotations

import struct

import numpy as np

from tests import bai_writer as bi
from tests import bam_device_cases as cases
from tests import bam_writer as bw
from tests import bgzf_writer as gw

REFS = [("1", 200000), ("2", 200000), ("3", 200000), ("4", 200000)]  # the last has no records


def reads(n=300, seed=5, long_every=0):
    """n records on each of three references, CB-tagged for three cells, and an unmapped tail"""
    rng = np.random.default_rng(seed)
    out = []
    for ref in range(3):
        pos = np.sort(rng.integers(1000, 3000, n))
        for k in range(n):
            length = 2500 if long_every and k % long_every == 7 else int(rng.integers(30, 70))
            seq = "".join(rng.choice(list("ACGT"), length))
            out.append(bw.Rec("q%d_%d" % (ref, k), ref, int(pos[k]), [("M", length)], seq,
                              qual=[int(q) for q in rng.integers(25, 41, length)], mapq=int(rng.integers(0, 60)),
                              tags=[("AS", "C", int(rng.integers(0, 100))), ("CB", "Z", "cell%d" % (k % 3))]))
    out += [bw.Rec("un%d" % k, -1, -1, [], "ACGT", qual=[30] * 4, flag=0x4) for k in range(5)]
    return out


def raw_bam(records, refs=REFS) -> bytes:
    return gw.inflate_all(bw.bam_bytes(refs, records))


def htslib_members(raw: bytes, limit=4096) -> bytes:
    """htslib's layout: the header in members of its own, then a member is flushed before a record that would not fit"""
    spans = bi.record_spans(raw)
    first = spans[0][0] if spans else len(raw)
    cuts, at = [0, first], first
    for s, e in spans:
        if e - at > limit and s > at:
            cuts.append(s)
            at = s
    cuts.append(len(raw))
    return b"".join(gw.bgzf(raw[a:b], chunk=0xFF00, eof=False) for a, b in zip(cuts, cuts[1:]) if b > a) + gw.EOF_MEMBER


def three_bam() -> bytes:
    return htslib_members(raw_bam(reads()))


def put(directory, name, data: bytes, index=True, pseudo_bin=True) -> str:
    path = str(directory / name)
    open(path, "wb").write(data)
    if index:
        bi.write_bai(path, pseudo_bin=pseudo_bin)
    return path


def rewritten_index(recs, move_start=None, move_end=None, pseudo_bin=True) -> bytes:
    """A minimal index of bai_writer.layout's records over REFS, one chunk per reference; reference 1's chunk begins
    at move_start and ends at move_end where given"""
    out = bytearray(b"BAI\1" + struct.pack("<i", len(REFS)))
    for ref in range(len(REFS)):
        rs = [r for r in recs if r[0] == ref]
        if not rs:
            out += struct.pack("<ii", 0, 0)
            continue
        b, e = rs[0][3], rs[-1][4]
        if ref == 1:
            b, e = move_start or b, move_end or e
        out += struct.pack("<i", 2 if pseudo_bin else 1) + struct.pack("<IiQQ", 4681, 1, b, e)
        if pseudo_bin:
            out += struct.pack("<IiQQQQ", bi.PSEUDO_BIN, 2, b, e, len(rs), 0)
        out += struct.pack("<i", 0)
    return bytes(out)


def moved_indexes(path):
    """Indexes of the BAM at ``path`` (three_bam's layout) whose reference 1 is off by a record or lands inside one
    -> ({name: index bytes}, reference 1's layout records). "good" is the untouched one."""
    _table, recs, _n = bi.layout(path)
    mine = [r for r in recs if r[0] == 1]
    assert mine[-1][3] & 0xFFFF  # the moved end lies inside a member: the record at it is read
    return {
        "start-later": rewritten_index(recs, move_start=mine[1][3]),
        "end-earlier-no-pseudo-bin": rewritten_index(recs, move_end=mine[-1][3], pseudo_bin=False),
        "end-earlier": rewritten_index(recs, move_end=mine[-1][3]),
        "start-inside-a-record": rewritten_index(recs, move_start=mine[1][3] + 9),
        "good": rewritten_index(recs),
    }, mine


def other_bam_pair():
    """Two BAMs with the same header and the same members (stored, fixed size): one record of reference 0 is 10 bytes
    longer in the second and reference 1's last record 10 bytes shorter, so reference 1 starts elsewhere and ends at
    the same byte -> (the BAM under test, the BAM whose index it is given)"""
    def padded(first, second):
        recs = reads()
        k0 = [k for k, r in enumerate(recs) if r.ref == 0][5]
        k1 = max(k for k, r in enumerate(recs) if r.ref == 1)
        recs[k0].tags = recs[k0].tags + [("XP", "Z", "x" * first)]
        recs[k1].tags = recs[k1].tags + [("XP", "Z", "x" * second)]
        return gw.bgzf(raw_bam(recs), chunk=4096, level=0)
    return padded(0, 10), padded(10, 0)


DEFECT_REFS = [("1", 3_000_000), ("2", 3_000_000)]
DEFECT_MEMBER, DEFECT_RECORD = 3, 700


def defect_bams():
    """3000 small records on reference 0 and 200 on reference 1 in stored 16 KiB members (stored, so that a changed
    byte moves no member and the good file's index still passes the file-level checks) -> dict(good, member: member 3's
    middle payload byte flipped, size: block_size 31 in record 700); both defects lie in reference 0's span only"""
    raw = gw.inflate_all(bw.bam_bytes(DEFECT_REFS, cases.many(3000) + cases.many(200, ref=1)))
    at = cases.record_start(raw, DEFECT_RECORD)
    good = gw.bgzf(raw, chunk=16384, level=0)
    return dict(good=good, member=gw.corrupt_member(good, DEFECT_MEMBER),
                size=gw.bgzf(raw[:at] + struct.pack("<I", 31) + raw[at + 4:], chunk=16384, level=0))


def span_of(bam: bytes, index: bytes, chromosome: int):
    """What the index makes the readers walk for one chromosome, restated: the inflated bytes of the members from the
    start's coffset through the end's (left out when its uoffset is 0), the entry and the limit inside them, and the
    offset of each member's first byte -> (bytes, entry, limit, [member starts])"""
    import zlib
    beg, end, _count = bi.parse_ranges(index)[chromosome]
    out, starts = bytearray(), []
    for coff, n, _isize, _lin in bi.member_table(bam):
        if beg >> 16 <= coff and (coff < end >> 16 or (coff == end >> 16 and end & 0xFFFF)):
            starts.append(len(out))
            out += zlib.decompress(bam[coff + 18:coff + n - 8], -15)
    limit = len(out) if not end & 0xFFFF else starts[-1] + (end & 0xFFFF)
    return bytes(out), beg & 0xFFFF, limit, starts
