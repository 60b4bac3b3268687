"""What ``secedo_amd.genome_bins`` must return and write, computed on the CPU in plain Python from the contract of
include/secedo_variant.h alone: ``expected``. Nothing here looks at the library.

The rules, restated. The text is cut into lines at '\\n'; a last line without '\\n' counts, a trailing '\\n' adds no
line. Line 0 is a header; line i >= 1 is a header iff it starts with '>' and line i - 1 is not a header; every other
line is sequence. Every header starts a contig whose sequence is the bytes of the sequence lines up to the next header.
Its name is the header's bytes after the first, up to the first space, tab or '\\r'; longer than 4096 bytes is refused.
Of two contigs with one name the first is taken. Without ``contigs`` all are selected in file order, else the listed
names in the listed order. Selected contig k of length L has ceil(L / S) bins [bS, min((b + 1)S, L)), numbered in
selection order. Per bin: a (A a), c (C c), g (G g), t (T t U u), other (every other byte), masked ('a'..'z', in
addition to the class). The file: a header line, then a line per bin, tab-separated, 0-based half-open.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

COLUMNS = ("a", "c", "g", "t", "other", "masked")
HEADER = b"chrom\tstart\tend\ta\tc\tg\tt\tother\tmasked\n"
MAX_NAME = 4096
INVALID_ARG, LIMIT = -1, -6  # SECEDO_E_INVALID_ARG, SECEDO_E_LIMIT (include/secedo_simmat.h)
CLASS = {}
for _letters, _k in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)):
    for _ch in _letters:
        CLASS[ord(_ch)] = _k


class Refused(Exception):
    """The call must fail with this code and this message."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code, self.message = code, message


def contigs_of(text: bytes) -> List[Tuple[bytes, bytes]]:
    """(header line without its '\\n', sequence bytes) of every contig, in file order."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # a trailing '\n' adds no line (and an empty text has none)
    out: List[Tuple[bytes, bytearray]] = []
    before_is_header = False
    for i, line in enumerate(lines):
        header = i == 0 or (line.startswith(b">") and not before_is_header)
        if header:
            out.append((line, bytearray()))
        else:
            out[-1][1].extend(line)
        before_is_header = header
    return [(h, bytes(s)) for h, s in out]


def name_of(header: bytes) -> bytes:
    rest = header[1:]
    for i, b in enumerate(rest):
        if b in b" \t\r":
            return rest[:i]
    return rest


def row_of(seq: bytes) -> List[int]:
    row = [0] * 6
    for b in seq:
        row[CLASS.get(b, 4)] += 1
        row[5] += 0x61 <= b <= 0x7A
    return row


class Expected:
    def __init__(self):
        self.names: List[str] = []
        self.contig_lengths: List[int] = []
        self.bins: List[Tuple[int, int, int]] = []  # (position in the selection, start, end) per global bin
        self.counts = np.zeros((0, 6), np.uint32)
        self.contigs = 0
        self.duplicate_names = 0
        self.file = b""


def expected(text: bytes, S: int, contigs: Optional[Sequence] = None, lengths: Optional[Sequence[int]] = None,
             path: str = "") -> Expected:
    """The result for a FASTA ``text`` at bin size ``S``, or raises ``Refused``. ``path``: the FASTA's, for the
    messages that name it."""
    if S == 0:
        raise Refused(INVALID_ARG, "secedo_variant_genome_bins: bin_size is 0, at least 1 is needed")
    if not text:
        raise Refused(INVALID_ARG, "%s: the genome is empty" % path)
    all_contigs = contigs_of(text)
    names = []
    for k, (header, _) in enumerate(all_contigs):
        names.append(name_of(header))
        if len(names[-1]) > MAX_NAME:
            raise Refused(INVALID_ARG, "%s: contig %d: its name is longer than 4096 bytes" % (path, k))
    first = {}
    for k, n in enumerate(names):
        first.setdefault(n, k)
    e = Expected()
    e.contigs = len(all_contigs)
    e.duplicate_names = len(names) - len(first)
    if contigs is None:
        chosen = [k for k, n in enumerate(names) if first[n] == k]
    else:
        listed = [c if isinstance(c, bytes) else str(c).encode() for c in contigs]
        if not listed:
            raise Refused(INVALID_ARG, "no contig is selected: the list of names is empty")
        chosen = []
        for i, n in enumerate(listed):
            if n in listed[:i]:
                raise Refused(INVALID_ARG, "contig name '%s' is listed twice" % n.decode())
            if n not in first:
                raise Refused(INVALID_ARG, "the genome has no contig named '%s' (names are matched exactly: no chr "
                                           "prefix is added or removed)" % n.decode())
            chosen.append(first[n])
        if lengths is not None:
            for i, k in enumerate(chosen):
                if len(all_contigs[k][1]) != int(lengths[i]):
                    raise Refused(INVALID_ARG, "%s: the genome has %d bases, expected %d"
                                  % (listed[i].decode(), len(all_contigs[k][1]), int(lengths[i])))
    rows, lines = [], [HEADER]
    for i, k in enumerate(chosen):
        seq = all_contigs[k][1]
        e.names.append(names[k].decode("utf-8", "surrogateescape"))
        e.contig_lengths.append(len(seq))
        for start in range(0, len(seq), S):
            end = min(start + S, len(seq))
            row = row_of(seq[start:end])
            assert sum(row[:5]) == end - start
            e.bins.append((i, start, end))
            rows.append(row)
            lines.append(names[k] + b"\t" + b"\t".join(str(v).encode() for v in [start, end] + row) + b"\n")
    e.counts = np.array(rows, np.uint32).reshape(-1, 6)
    e.file = b"".join(lines)
    return e


def hand_example():
    """A small FASTA worked by hand -> (text, S, names, lengths, bins, rows, file bytes).

    Line 0 ``>one first`` is a header, name ``one``. ``ACGTN`` and ``acgtn`` are its sequence, 10 bases. ``>two`` starts
    contig ``two``; the line after it, ``>GG``, directly follows a header and so is sequence: '>' counts as other.
    ``uU\\r`` is sequence too: u and U are t, '\\r' is other. ``two`` has 3 + 3 = 6 bases. ``>one again`` is a third
    contig with a name seen before: counted in duplicate_names, left out."""
    text = b">one first\nACGTN\nacgtn\n>two\n>GG\nuU\r\n>one again\nTTTT\n"
    names, lengths = ["one", "two"], [10, 6]
    # S = 4: one -> [0,4) ACGT, [4,8) Nacg, [8,10) tn; two -> [0,4) >GGu, [4,6) U\r
    bins = [(0, 0, 4), (0, 4, 8), (0, 8, 10), (1, 0, 4), (1, 4, 6)]
    rows = [[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 1, 3], [0, 0, 0, 1, 1, 2], [0, 0, 2, 1, 1, 1], [0, 0, 0, 1, 1, 0]]
    file = (b"chrom\tstart\tend\ta\tc\tg\tt\tother\tmasked\n"
            b"one\t0\t4\t1\t1\t1\t1\t0\t0\none\t4\t8\t1\t1\t1\t0\t1\t3\none\t8\t10\t0\t0\t0\t1\t1\t2\n"
            b"two\t0\t4\t0\t0\t2\t1\t1\t1\ntwo\t4\t6\t0\t0\t0\t1\t1\t0\n")
    return text, 4, names, lengths, bins, rows, file
