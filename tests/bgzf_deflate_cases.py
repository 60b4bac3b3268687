"""Inputs and checks shared by tests/test_bgzf_deflate_cpu.py (the encoder of bgzf_deflate.hpp as a host program) and
tests/test_gpu_bgzf_deflate.py (the same encoder as a kernel): what a BGZF file made from `data` must look like,
whoever made it. zlib is the reference of every comparison."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np

from tests import bgzf_writer as gw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "secedo_amd", "csrc", "build", "bgzf_deflate_test")
CUT = 0xFF00
CASE_TIMEOUT = 120  # seconds per run of the executable; 130 KB take well under one

# Our payload bytes over zlib level 1's (dynamic codes) on the same 0xFF00 blocks. The encoder has the fixed codes
# only, and that is where it loses: zlib itself with Z_FIXED at level 1 is at 1.283 (vcf_like_text) and 1.301
# (sam_like_text(4000)) of its own dynamic level 1. Measured quotients of ours: 1.2088 and 1.3001. The bound is the
# measured quotient plus 5 %: the output is deterministic, the margin only leaves room for harmless tie-break changes.
RATIO_VCF_MEASURED, RATIO_SAM_MEASURED = 1.2088, 1.3001
RATIO_VCF_BOUND, RATIO_SAM_BOUND = RATIO_VCF_MEASURED * 1.05, RATIO_SAM_MEASURED * 1.05

PHRASE = b"The quick brown fox jumps over the lazy!"  # 40 bytes


def vcf_like_text(n_lines=20000, seed=5) -> bytes:
    """Lines with the shape of the project's VCF output: ascending positions, few distinct REF/ALT/GT columns,
    small counts."""
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(1, 400, n_lines))
    out = []
    for k in range(n_lines):
        c = rng.integers(0, 60, 4)
        out.append("%d\t%d\t.\t%s\t%s\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t%s\t%d %d %d %d \n" % (
            1 + k * 22 // n_lines, pos[k] % 250_000_000 + 1, "ACGT"[rng.integers(4)], "ACGT"[rng.integers(4)],
            "1/1" if rng.random() < 0.8 else "0/1", c[0], c[1], c[2], c[3]))
    return "".join(out).encode()


def cases():
    """name -> input bytes (the table of the encoder's edge inputs)."""
    rng = np.random.default_rng(17)
    sam = gw.sam_like_text(1200)
    assert len(sam) >= 2 * CUT + 1 and len(PHRASE) == 40
    out = {"empty": b"", "one": b"a", "two": b"ab"}
    for n in (258, 259, 260, 600):
        out["run_%d" % n] = b"x" * n  # distance 1, maximum length
    out["all_bytes"] = bytes(range(256)) * 2  # 9-bit fixed codes from 144 on; once alone they would be stored
    # the phrase again at distance exactly 32768 (taken) and 32769 (must not be); zeros in between leave the hash
    # table's entries for the phrase alone
    out["phrase_at_32768"] = PHRASE + bytes(32768 - 40) + PHRASE
    out["phrase_at_32769"] = PHRASE + bytes(32769 - 40) + PHRASE
    for n in (CUT - 1, CUT, CUT + 1, 2 * CUT + 1):
        out["sam_%d" % n] = sam[:n]  # the cut; a match must not cross it
    out["random_65280"] = rng.integers(0, 256, CUT, dtype=np.uint8).tobytes()  # stored fallback
    # 3 header bits + 6 literals of 9 bits + 7 bits of end-of-block = 64 bits; 7 literals of 8 bits give 66
    out["flush_aligned"] = bytes([150, 160, 170, 180, 190, 200])
    out["flush_unaligned"] = b"abcdefg"
    return out


def host_encode(data: bytes, tmp_path, tag="x") -> bytes:
    src, dst = tmp_path / ("%s.in" % tag), tmp_path / ("%s.gz" % tag)
    src.write_bytes(data)
    r = subprocess.run([EXE, str(src), str(dst)], capture_output=True, text=True, timeout=CASE_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return dst.read_bytes()


def split_members(raw: bytes):
    """-> [(member bytes, payload, crc, isize)] by following BSIZE; every header checked on the way."""
    out, o = [], 0
    while o < len(raw):
        assert len(raw) - o >= 28
        magic = struct.unpack_from("<BBBBIBBH", raw, o)
        assert magic == (31, 139, 8, 4, 0, 0, 255, 6), magic
        si1, si2, slen, bsize = struct.unpack_from("<BBHH", raw, o + 12)
        assert (si1, si2, slen) == (66, 67, 2)
        size = bsize + 1
        assert o + size <= len(raw) and size <= 65536
        crc, isize = struct.unpack_from("<II", raw, o + size - 8)
        out.append((raw[o:o + size], raw[o + 18:o + size - 8], crc, isize))
        o += size
    return out


def tokens(payload: bytes):
    """The (length, distance) of every match of a BTYPE 1 payload, [] for a stored one."""
    bits = np.unpackbits(np.frombuffer(payload, dtype=np.uint8), bitorder="little").tolist()
    at = 0

    def take(n):  # an integer field, least significant bit first
        nonlocal at
        v = 0
        for k in range(n):
            v |= bits[at + k] << k
        at += n
        return v

    def huff(n, v=0):  # n more bits of a Huffman code, most significant first
        nonlocal at
        for k in range(n):
            v = v << 1 | bits[at + k]
        at += n
        return v

    assert take(1) == 1  # BFINAL
    btype = take(2)
    if btype == 0:
        return []
    assert btype == 1
    out = []
    while True:
        c = huff(7)
        if c <= 0b0010111:
            sym = 256 + c
        else:
            c = huff(1, c)
            if 0b00110000 <= c <= 0b10111111:
                sym = c - 0b00110000
            elif 0b11000000 <= c <= 0b11000111:
                sym = 280 + c - 0b11000000
            else:
                sym = 144 + huff(1, c) - 0b110010000
        if sym == 256:
            assert (at + 7) // 8 == len(payload)
            return out
        if sym < 256:
            continue
        s = sym - 257
        assert s <= 28
        length = 258 if s == 28 else 3 + s if s < 8 else ((4 + (s & 3)) << ((s >> 2) - 1)) + 3 + take((s >> 2) - 1)
        d = huff(5)
        assert d <= 29
        dist = 1 + d if d < 4 else ((2 + (d & 1)) << ((d >> 1) - 1)) + 1 + take((d >> 1) - 1)
        out.append((length, dist))


def check_file(raw: bytes, data: bytes, with_tokens=True):
    """Everything a BGZF file made from `data` owes, whoever made it -> its members (without the EOF member).
    with_tokens: also walk every match of every member (slow in Python: off for the long ratio texts, where zlib's own
    check of the distances has to do)."""
    assert gzip.decompress(raw) == data
    assert gw.inflate_all(raw) == data
    assert raw.endswith(gw.EOF_MEMBER)
    members = split_members(raw)
    assert members[-1][0] == gw.EOF_MEMBER
    members = members[:-1]
    assert len(members) == -(-len(data) // CUT)  # bgzip's cut: every member but the last is full
    o = 0
    for k, (member, payload, crc, isize) in enumerate(members):
        piece = data[o:o + isize]
        assert isize == min(CUT, len(data) - o), k
        assert crc == zlib.crc32(piece) and len(member) <= 65536, k
        assert len(payload) <= isize + 5, k  # never larger than its stored form
        d = zlib.decompressobj(-15)  # the member on its own: nothing reaches into the member before
        assert d.decompress(payload) == piece and d.eof and not d.unused_data, k
        for length, dist in tokens(payload) if with_tokens else ():
            assert 3 <= length <= 258 and 1 <= dist <= 32768, (k, length, dist)
        o += isize
    assert o == len(data)
    return members


def zlib_sizes(data: bytes):
    """Payload bytes of zlib at level 1 and 6 over the same 0xFF00 blocks."""
    return tuple(sum(len(gw.deflate(data[o:o + CUT], level)) for o in range(0, len(data), CUT)) for level in (1, 6))


def payload_bytes(raw: bytes) -> int:
    return sum(len(m[1]) for m in split_members(raw)[:-1])
