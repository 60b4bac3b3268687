"""BGZF written with chosen zlib settings, for the inflate tests (the plain writer is bam_writer.bgzf): a level, a
strategy, a chunk size, and optionally a Z_FULL_FLUSH inside each member, which puts several DEFLATE blocks in it."""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE}
LEVELS = (0, 1, 6, 9)
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def deflate(chunk: bytes, level=6, strategy="default", flush_at=None) -> bytes:
    """Raw DEFLATE of chunk; flush_at: a Z_FULL_FLUSH after that many bytes (a block boundary inside the stream)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, STRATEGIES[strategy])
    if flush_at is None:
        return c.compress(chunk) + c.flush()
    return c.compress(chunk[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(chunk[flush_at:]) + c.flush()


def member(payload: bytes, crc: int, isize: int) -> bytes:
    """One BGZF member around a raw DEFLATE payload."""
    bsize = len(payload) + 25
    assert bsize <= 65535
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize) + payload +
            struct.pack("<II", crc & 0xFFFFFFFF, isize))


def members(data: bytes, level=6, strategy="default", chunk=0xFF00, flush=False):
    """-> [(payload, crc, isize)] of data cut into chunks (level 0 needs room for the stored headers)."""
    if level == 0:
        chunk = min(chunk, 0xFF00 - 64)
    out = []
    for o in range(0, len(data), chunk):
        piece = data[o:o + chunk]
        out.append((deflate(piece, level, strategy, len(piece) // 3 if flush else None), zlib.crc32(piece),
                    len(piece)))
    return out


def bgzf(data: bytes, level=6, strategy="default", chunk=0xFF00, flush=False, eof=True) -> bytes:
    return b"".join(member(*m) for m in members(data, level, strategy, chunk, flush)) + (EOF_MEMBER if eof else b"")


def fixed_huffman(tokens) -> bytes:
    """A one-block fixed-Huffman DEFLATE stream of tokens: an int is a literal, (length, distance) a match. zlib
    never emits a distance above 32506, so the longest distances are written by hand."""
    bits = []

    def put(value, n, msb_first=False):
        order = range(n - 1, -1, -1) if msb_first else range(n)
        bits.extend((value >> k) & 1 for k in order)

    def symbol(s):
        if s < 144:
            put(0x30 + s, 8, True)
        elif s < 256:
            put(0x190 + s - 144, 9, True)
        elif s < 280:
            put(s - 256, 7, True)
        else:
            put(0xC0 + s - 280, 8, True)

    len_base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163,
                195, 227, 258]
    len_extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dist_base = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049,
                 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    put(1, 1)
    put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            symbol(t)
            continue
        length, dist = t
        k = max(i for i in range(29) if len_base[i] <= length and (i == 28 or length < 258))
        symbol(257 + k)
        put(length - len_base[k], len_extra[k])
        d = max(i for i in range(30) if dist_base[i] <= dist)
        put(d, 5, True)
        put(dist - dist_base[d], max(0, d // 2 - 1))
    symbol(256)
    bits.extend([0] * (-len(bits) % 8))
    return np.packbits(np.array(bits, dtype=np.uint8), bitorder="little").tobytes()


def max_distance_member():
    """-> (payload, crc, isize, bytes): 32768 random literals, then matches of 258 at distance 32768 up to 65280."""
    rng = np.random.default_rng(9)
    head = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    n_match = (65280 - 32768) // 258
    data = (head * 2)[:32768 + 258 * n_match]
    payload = fixed_huffman(list(head) + [(258, 32768)] * n_match)
    assert zlib.decompress(payload, -15) == data
    return payload, zlib.crc32(data), len(data), data


def sam_like_text(n_lines=4000, seed=3) -> bytes:
    """Text with the statistics of SAM lines: repeated field shapes, bases, qualities."""
    rng = np.random.default_rng(seed)
    lines = []
    for k in range(n_lines):
        seq = "".join("ACGT"[b] for b in rng.integers(0, 4, 60))
        qual = "".join(chr(33 + int(q)) for q in rng.integers(20, 41, 60))
        lines.append("read%06d\t%d\t1\t%d\t60\t60M\t=\t%d\t%d\t%s\t%s\tAS:i:%d\tCB:Z:AAC%02d-1\n"
                     % (k // 2, 99 if k % 2 == 0 else 147, 1000 + 7 * k, 1100 + 7 * k, 160, seq, qual,
                        int(rng.integers(0, 120)), k % 8))
    return "".join(lines).encode()


def round_trip_cases():
    """-> [(name, data, writer keywords)]: every level x strategy on text, and the shapes that stress the decoder."""
    rng = np.random.default_rng(7)
    text = sam_like_text()
    cases = [("text-l%d-%s" % (level, s), text, dict(level=level, strategy=s)) for level in LEVELS for s in STRATEGIES]
    period = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    cases += [
        ("random", rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes(), dict(level=6, chunk=60000)),
        ("zeros-65280", bytes(65280), dict(level=9)),
        ("period-32768", period * 2, dict(level=9, chunk=65536 - 256)),
        ("empty", b"", dict(level=6)),
        ("multi-block", text, dict(level=6, flush=True)),
        ("multi-block-stored", text[:100_000], dict(level=0, flush=True)),
        ("chunks-4k", text, dict(level=6, chunk=4096)),
        ("chunks-1", text[:300], dict(level=6, chunk=1)),
    ]
    return cases


def round_trip_files(directory):
    """Writes every round-trip case, the text of a synthetic SAM set and the hand-written maximum-distance member:
    -> [(name, path of the BGZF file, expected bytes)], the golden BAMs (written by htslib) included."""
    out = []
    for name, data, kw in round_trip_cases():
        path = os.path.join(str(directory), name + ".gz")
        with open(path, "wb") as f:
            f.write(bgzf(data, **kw))
        out.append((name, path, data))
    from tests import multiplex_bam as mb
    from tests import sam_writer as sw
    refs, cells = mb.synthetic_cells(os.path.join(str(directory), "raw"), n_cells=3, pairs_per_cell=60, n_refs=2, seed=11)
    recs = sorted((r for c in cells for r in c), key=bw_sort_key())
    for name, kw in (("synthetic-sam", dict(level=6)), ("synthetic-sam-l1-4k", dict(level=1, chunk=4096))):
        data = sw.sam_text(refs, recs).encode()
        path = os.path.join(str(directory), name + ".gz")
        with open(path, "wb") as f:
            f.write(bgzf(data, **kw))
        out.append((name, path, data))
    payload, crc, isize, data = max_distance_member()
    path = os.path.join(str(directory), "distance-32768.gz")
    with open(path, "wb") as f:
        f.write(member(payload, crc, isize) + EOF_MEMBER)
    out.append(("distance-32768", path, data))
    for bam in golden_bams():
        out.append((os.path.basename(bam), bam, inflate_all(open(bam, "rb").read())))
    return out


def bw_sort_key():
    from tests import bam_writer as bw
    return bw.sort_key


def golden_bams():
    from tests.golden_util import GOLDEN
    d = os.path.join(GOLDEN, "bam")
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".bam"))


def inflate_all(raw: bytes) -> bytes:
    """What zlib makes of a BGZF file: the reference of every comparison."""
    out, o = [], 0
    while o < len(raw):
        d = zlib.decompressobj(31)
        out.append(d.decompress(raw[o:]))
        o = len(raw) - len(d.unused_data)
    return b"".join(out)


def corruptions(n_flips=240, n_cuts=120, seed=5):
    """-> [(payload, crc, isize, original bytes)]: single-bit flips and truncations of valid members, seeded."""
    rng = np.random.default_rng(seed)
    text = sam_like_text(600)
    base = []
    for kw in (dict(level=0), dict(level=1), dict(level=6), dict(level=9), dict(level=6, strategy="fixed"),
               dict(level=6, strategy="huffman"), dict(level=6, strategy="rle"), dict(level=6, flush=True)):
        piece = text[:20_000]
        (payload, crc, isize), = members(piece, chunk=0xFF00, **kw)
        base.append((payload, crc, isize, piece))
    out = []
    for k in range(n_flips):
        payload, crc, isize, piece = base[k % len(base)]
        # half of the flips in the first 64 bytes, where the block headers and code lengths are
        bit = int(rng.integers(0, (64 if k % 2 else len(payload)) * 8))
        p = bytearray(payload)
        p[bit // 8] ^= 1 << (bit % 8)
        out.append((bytes(p), crc, isize, piece))
    for k in range(n_cuts):
        payload, crc, isize, piece = base[k % len(base)]
        out.append((payload[:int(rng.integers(0, len(payload)))], crc, isize, piece))
    return out


def corrupt_member(raw: bytes, k: int) -> bytes:
    """raw BGZF with one payload byte of member k flipped (the middle one)."""
    o = 0
    for _ in range(k):
        o += int.from_bytes(raw[o + 16:o + 18], "little") + 1
    size = int.from_bytes(raw[o + 16:o + 18], "little") + 1
    at = o + 18 + (size - 26) // 2
    return raw[:at] + bytes([raw[at] ^ 0x10]) + raw[at + 1:]


def listing_damage(raw: bytes):
    """The three files whose member list no reader gets past member 0, made of a valid BGZF file of two members or
    more (18-byte headers): -> [(name, bytes, the message behind the file's name)]. A valid first member, then 40
    bytes that are no gzip header; a second member whose BSIZE is less than its header and trailer; a second member
    whose ISIZE field says 65537."""
    n0 = int.from_bytes(raw[16:18], "little") + 1
    n1 = int.from_bytes(raw[n0 + 16:n0 + 18], "little") + 1
    assert n0 + n1 <= len(raw) and raw[n0:n0 + 4] == raw[:4]
    small, big = bytearray(raw), bytearray(raw)
    small[n0 + 16:n0 + 18] = struct.pack("<H", 24)  # 25 bytes: 18 of header and 8 of trailer do not fit
    big[n0 + n1 - 4:n0 + n1] = struct.pack("<I", 65537)
    return [("not-bgzf", raw[:n0] + bytes(range(1, 41)), ": not a BGZF block at byte %d" % n0),
            ("bad-bsize", bytes(small), ": bad BGZF block size at byte %d" % n0),
            ("big-isize", bytes(big), ": BGZF ISIZE above 64 KiB")]


LISTING_DAMAGE = ("not-bgzf", "bad-bsize", "big-isize")
ERROR_PREFIX = "secedo_simmat error -1: "  # SecedoError's words in front of an E_INVALID_ARG message

ERROR_WRITERS = {"stored": dict(level=0), "l6": dict(level=6), "fixed": dict(level=6, strategy="fixed")}
ERROR_MEMBERS = (0, 3, 9)


def corrupt_files(text: bytes):
    """The corrupt .sam.gz files of the GPU error tests: text in 16 KiB members, one member's middle payload byte
    flipped -> [(writer name, member, bytes)], and one file with two bad members (2 and 7) as ("two", 2, bytes)."""
    out = []
    for how, kw in ERROR_WRITERS.items():
        raw = bgzf(text, chunk=16384, **kw)
        out += [(how, k, corrupt_member(raw, k)) for k in ERROR_MEMBERS]
    out.append(("two", 2, corrupt_member(corrupt_member(bgzf(text, chunk=16384), 7), 2)))
    return out


def zlib_verdict(payload: bytes, piece: bytes) -> bool:
    """zlib inflates the payload, whole, to exactly piece."""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(payload)
    except zlib.error:
        return False
    return d.eof and got == piece
