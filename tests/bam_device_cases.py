"""The corrupt BAM files of tests/test_gpu_pileup_bam_device.py, built here so that tests/test_bam_walk_cpu.py can put
the same members through the decoder on the host (secedo_amd/csrc/build/bgzf_inflate_test) before a GPU sees them."""
from __future__ import annotations

import struct

from tests import bam_writer as bw
from tests import bgzf_writer as gw

BAD_MEMBERS = (0, 3, 5)


def many(n=400, ref=0):
    return [bw.Rec("f%d" % k, ref, 12 + k, [("M", 4)], "ACGT", qual=[40] * 4) for k in range(n)]


def block_error_bytes() -> bytes:
    """inflated BAM bytes: 3000 small records on one reference"""
    return gw.inflate_all(bw.bam_bytes([("1", 3_000_000)], many(3000)))


def corrupt_bams():
    """-> [(writer name, member, BGZF bytes)]: 16 KiB members, the middle payload byte of one member flipped"""
    raw = block_error_bytes()
    out = []
    for how, kw in gw.ERROR_WRITERS.items():
        data = gw.bgzf(raw, chunk=16384, **kw)
        out += [(how, k, gw.corrupt_member(data, k)) for k in BAD_MEMBERS]
    return out


def record_start(raw: bytes, k: int) -> int:
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    for _ in range(k):
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    return o


def corrupt_with_record_error(record: int) -> bytes:
    """member 3 corrupt and block_size 31 in the given record"""
    raw = block_error_bytes()
    at = record_start(raw, record)
    return gw.corrupt_member(gw.bgzf(raw[:at] + struct.pack("<I", 31) + raw[at + 4:], chunk=16384), 3)
