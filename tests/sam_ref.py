"""The SAM -> BAM record conversion of include/secedo_bam.h and secedo_amd/csrc/sam_kernels.hpp restated in plain
Python, written from those two contracts and the SAM specification, not from the parser's code: one line -> the bytes
of its BAM record or the ``SamErr`` code that refuses it, the line starts of a range of text, and what the size and
encode passes give for a range.

Text is handled as latin-1, one character per byte, and every class of character is spelled out in ASCII, so that
Python's wider notions of digit, letter and upper case do not leak in.

``f`` values are ``struct.pack("<f", float(text))``: the decimal text correctly rounded to double, then to float32. With
at most 9 significant digits that is the correctly rounded float32 except in cases no input of the tests comes near,
and an exact tie between two floats stays an exact tie in double and rounds to even."""
import re
import struct

from tests import bam_writer as bw
from tests import sam_writer as sw

NT16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
B_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
B_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1),
           "I": (0, 2 ** 32 - 1)}

# SamErr of sam_kernels.hpp
FIELDS, NAME, FLAG, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN, QUAL, CIGAR_SEQ, AUX, HEADER, EMPTY, MANY_OPS, \
    TOO_LONG = range(1, 18)
NO_RECORD = -2 ** 31  # the RefID reported for a line that is no record
NO_ERROR = 2 ** 64 - 1

_INT = re.compile(r"-?[0-9]+\Z")
_FLOAT = re.compile(r"[-+]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][-+]?[0-9]+)?\Z")
_DIGITS = "0123456789"
_LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"


class SamError(Exception):
    """``code``: the SamErr the line is refused with."""

    def __init__(self, code, what=""):
        super().__init__("%s (code %d)" % (what, code))
        self.code = code


def _int(s, lo, hi, code):
    """A decimal integer in [lo, hi]; a '-' only where the range goes below zero."""
    if not _INT.match(s) or (s.startswith("-") and lo >= 0) or not lo <= int(s) <= hi:
        raise SamError(code, "integer %r" % s[:40])
    return int(s)


def _float(s):
    if not _FLOAT.match(s):
        raise SamError(AUX, "float %r" % s[:40])
    return struct.pack("<f", float(s))


def parse_aux(f: str) -> bytes:
    if len(f) < 5 or f[2] != ":" or f[4] != ":" or f[0] not in _LETTERS or f[1] not in _LETTERS + _DIGITS:
        raise SamError(AUX, "aux")
    tag, typ, v = f[:2], f[3], f[5:]
    out = tag.encode("latin-1")
    if typ == "A":
        if len(v) != 1 or not "!" <= v <= "~":
            raise SamError(AUX, "aux")
        return out + b"A" + v.encode("latin-1")
    if typ == "i":
        x = _int(v, -2 ** 31, 2 ** 32 - 1, AUX)
        t = sw.smallest_int_type(x)
        return out + t.encode() + struct.pack(B_FMT[t], x)
    if typ == "f":
        return out + b"f" + _float(v)
    if typ in ("Z", "H"):
        return out + typ.encode() + v.encode("latin-1") + b"\0"
    if typ == "B":
        if not v or v[0] not in B_FMT or (len(v) > 1 and v[1] != ","):
            raise SamError(AUX, "aux")
        vals = v[2:].split(",") if len(v) > 1 else []
        sub = v[0]
        body = b"".join(_float(x) if sub == "f" else struct.pack(B_FMT[sub], _int(x, *B_RANGE[sub], AUX)) for x in vals)
        return out + b"B" + sub.encode() + struct.pack("<I", len(vals)) + body
    raise SamError(AUX, "aux")


def parse_line(line: str, names) -> bytes:
    """One SAM alignment line -> the BAM record (block_size first) under the rules of include/secedo_bam.h. The checks
    run in the documented order, so a line with two defects raises the code of the one checked first."""
    if line == "":
        raise SamError(EMPTY, "empty")
    if line[0] == "@":
        raise SamError(HEADER, "header")
    f = line.split("\t")
    if len(f) < 11 or any(not x for x in f[:11]):
        raise SamError(FIELDS, "fields")
    ids = {}
    for i, n in enumerate(names):
        ids.setdefault(n, i)
    qname = f[0]
    if len(qname) > 254:
        raise SamError(NAME, "qname")
    flag = _int(f[1], 0, 65535, FLAG)
    if f[2] != "*" and f[2] not in ids:
        raise SamError(RNAME, "rname")
    ref = -1 if f[2] == "*" else ids[f[2]]
    pos = _int(f[3], 0, 2 ** 31 - 1, POS) - 1
    mapq = _int(f[4], 0, 255, MAPQ)
    cigar = []
    if f[5] != "*":
        num = ""
        for c in f[5]:
            if c in _DIGITS:
                num += c
                continue
            if not num or c not in bw.CIGAR_OPS or not 1 <= int(num) < 2 ** 28:
                raise SamError(CIGAR, "cigar")
            cigar.append((c, int(num)))
            num = ""
        if num:
            raise SamError(CIGAR, "cigar")
        if len(cigar) > 65535:
            raise SamError(MANY_OPS, "cigar ops")
    if f[6] == "=":
        nref = ref
    elif f[6] == "*":
        nref = -1
    elif f[6] in ids:
        nref = ids[f[6]]
    else:
        raise SamError(RNEXT, "rnext")
    pnext = _int(f[7], 0, 2 ** 31 - 1, PNEXT) - 1
    tlen = _int(f[8], -(2 ** 31 - 1), 2 ** 31 - 1, TLEN)
    seq = "" if f[9] == "*" else f[9]
    if f[10] == "*":
        qual = b"\xff" * len(seq)
    else:
        if len(f[10]) != len(seq) or any(not "!" <= c <= "~" for c in f[10]):
            raise SamError(QUAL, "qual")
        qual = bytes(ord(c) - 33 for c in f[10])
    if cigar and seq and sum(n for op, n in cigar if op in "MIS=X") != len(seq):
        raise SamError(CIGAR_SEQ, "cigar/seq")
    rlen = max(bw.ref_length(cigar), 1)
    upper = lambda c: chr(ord(c) - 32) if "a" <= c <= "z" else c  # noqa: E731
    codes = [NT16.get(upper(c), 15) for c in seq] + ([0] if len(seq) % 2 else [])
    # bin is a 16-bit field: past 2^29 the bin number is kept modulo 2^16, as htslib's uint16_t does
    core = struct.pack("<iiBBHHHIiii", ref, pos, len(qname) + 1, mapq,
                       bw.reg2bin(max(pos, 0), max(pos + rlen, 1)) & 0xFFFF, len(cigar), flag, len(seq), nref, pnext,
                       tlen)
    body = (core + qname.encode("latin-1") + b"\0" + b"".join(struct.pack("<I", n << 4 | bw.CIGAR_OPS.index(op))
                                                                for op, n in cigar)
            + bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2)) + qual
            + b"".join(parse_aux(x) for x in f[11:]))
    if len(body) >= 2 ** 31:
        raise SamError(TOO_LONG, "record")
    return struct.pack("<i", len(body)) + body


def split_lines(text: bytes, trailing: bool):
    """The line starts of a range as sam_kernels.hpp defines them: line k spans [start[k], start[k + 1] - 1).
    ``trailing``: the range's last byte is a newline; without one, start[n_lines] = len + 1 closes the last line."""
    assert trailing == text.endswith(b"\n")
    start = [0] + [i + 1 for i, c in enumerate(text) if c == 10]
    if not trailing:
        start.append(len(text) + 1)
    return start


def parse_range(text: bytes, names, selected, line_base: int, ends_file: bool):
    """What the size and encode passes give for a range: ([(RefID, POS, record bytes or 0) per line], the records of
    the selected references concatenated (every good line's, whatever comes before it), the error word)."""
    start = split_lines(text, text.endswith(b"\n"))
    n_lines = len(start) - 1
    info, records, err = [], [], NO_ERROR
    for k in range(n_lines):
        line = text[start[k]:start[k + 1] - 1].decode("latin-1")
        if line == "" and ends_file and k + 1 == n_lines:
            info.append((NO_RECORD, 0, 0))
            continue
        try:
            rec = parse_line(line, names)
        except SamError as e:
            err = min(err, (line_base + k) << 8 | e.code)
            info.append((NO_RECORD, 0, 0))
            continue
        ref, pos = struct.unpack_from("<ii", rec, 4)
        keep = ref >= 0 and bool(selected[ref])
        info.append((ref, pos, len(rec) if keep else 0))
        if keep:
            records.append(rec)
    return info, records, err
