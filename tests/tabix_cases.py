"""The VCF texts of the tabix tests, each the smallest that reaches its edges, and the regions queried on them.

  formatter()   3000 lines of the bgzf writer's shape over chromosomes 1, 2 and X, about 150 KB: lines straddle the
                0xFF00 member cut and one starts exactly on it (the preamble is padded to make that so); positions on
                both sides of 16384, 32768, 131072 and 2^20; a cluster five windows past the last one (backward fill)
  spans()       multi-base REF and END= lines that span windows and bin levels; END= first in INFO, behind ';', as
                the key XEND= (which must not count), END=. and an END not above beg; POS 0; a line that ends in INFO
  SMALL         preamble only, empty, one data line, a last line without '\\n', no preamble; tiny_files(): 300 tiny files, some
                without data lines
  ERRORS        one text per refusal, with the line and the words of the message
  cosmic()      the head of a COSMIC extract (tests/golden/vcf/cosmic_small.vcf, 16 data lines, long INFO columns); the
                whole file has chromosome 1 coming back after MT and is an error case
"""
from __future__ import annotations

import os

import numpy as np

from tests import tabix_expected as te

CUT = 0xFF00
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcf", "cosmic_small.vcf")

PREAMBLE = (b"##fileformat=VCFv4.2\n##source=SVC (Somatic Variant Caller)\n##reference=genome.fa\n##cluster=0\n"
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tcluster-0\n")


def _line(chrom, pos, rng):
    ref, alt = rng.choice(4, 2, replace=False)
    counts = " ".join(str(int(c)) for c in rng.integers(0, 40, 4))
    return ("%s\t%d\t.\t%s\t%s\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t%s\t%s \n"
            % (chrom, pos, "ACGT"[ref], "ACGT"[alt], ("1/1", "0/1")[pos % 2], counts)).encode()


def formatter() -> bytes:
    rng = np.random.default_rng(12)
    edges = [b + d for b in (16384, 32768, 131072, 1 << 20) for d in (-1, 0, 1, 2)]  # POS b + 1 is beg b
    far = [(((1 << 20) >> 14) + 6) * 16384 + 11 * j for j in range(12)]
    pos1 = sorted(set(range(100, 100 + 37 * 1200, 37)) | set(edges) | set(far))
    body = [_line("1", p, rng) for p in pos1]
    body += [_line("2", p, rng) for p in range(5, 5 + 131 * 1000, 131)]
    body += [_line("X", p, rng) for p in range(16000, 16000 + 3 * (3000 - len(body)), 3)]
    assert len(body) == 3000
    starts = np.cumsum([len(PREAMBLE)] + [len(b) for b in body])
    k = int(np.searchsorted(starts, CUT - 8, side="right")) - 1  # the last line that a pad line can push onto the cut
    pad = CUT - int(starts[k])
    text = PREAMBLE[:PREAMBLE.index(b"#CHROM")] + b"##pad=" + b"x" * (pad - 7) + b"\n" + \
        PREAMBLE[PREAMBLE.index(b"#CHROM"):] + b"".join(body)
    assert text[CUT - 1:CUT] == b"\n" and text[2 * CUT - 1:2 * CUT] != b"\n" and 140_000 < len(text) < 200_000
    return text


def spans() -> bytes:
    tail = b"\t.\t.\t"
    lines = [
        b"1\t0\t.\tA\tC" + tail + b"DP=3\n",                                       # POS 0: beg 0
        b"1\t100\t.\t" + b"ACGT" * 5000 + b"\tA" + tail + b"DP=1\n",               # REF of 20000: windows 0-1
        b"1\t16000\t.\tA\t<DEL>" + tail + b"END=50000;SVTYPE=DEL\n",               # END first: windows 0-3
        b"1\t16100\t.\tA\t<DEL>" + tail + b"SVTYPE=DEL;END=140000\tGT\t0/1\n",     # END behind ';': a 1 Mb bin
        b"1\t16200\t.\tA\t<DEL>" + tail + b"XEND=999999;SVTYPE=DEL\n",             # not the key END
        b"1\t16300\t.\tA\tC" + tail + b"END=.\n",                                  # not a number
        b"1\t16385\t.\tA\tC" + tail + b"END=100;DP=2\n",                           # not above beg
        b"1\t16500\t.\tA\tC" + tail + b"SVTYPE=X;XEND=5;END=70000;END=5\n",        # the first END= key decides
        b"1\t16600\t.\tA\tC" + tail + b"ENDX=9;END=9x\n",                          # not a number
        b"1\t20000\t.\t" + b"AC" * 8200 + b"\tA" + tail + b".\n",                  # REF of 16400: three windows
        b"1\t131000\t.\tA\tC" + tail + b"END=1200000\n",                           # across 2^20: bin level 2
        b"1\t8000000\t.\tA\tC" + tail + b"END=80000000\n",                         # bin 0 or level 1
        b"2\t5\t.\tAC\tG\n",                                                       # five columns
        b"2\t70001\t.\tA\tC" + tail + b"END=1200000",                              # ends in INFO, no '\n'
    ]
    return PREAMBLE + b"".join(lines)


SMALL = {
    "preamble-only": PREAMBLE,
    "empty": b"",
    "one-line": PREAMBLE + b"7\t12345\t.\tA\tC\t.\t.\tDP=1\n",
    "no-last-newline": PREAMBLE + b"7\t5\t.\tA\tC\t.\t.\tDP=1\n7\t16384\t.\tAC\tC\t.\t.\tDP=1",
    "no-preamble": b"5\t7\t.\tA\tC\n5\t40000\t.\tA\tC\n",  # the first line at virtual offset 0
    "comments-between": b"##a\n3\t5\t.\tA\tC\n\n#x\n3\t9\t.\tA\tC\n##y\n4\t1\t.\tA\tC\n\n",
}


def tiny_files():
    rng = np.random.default_rng(4)
    out = []
    for k in range(300):
        if k % 7 == 3:
            out.append(PREAMBLE if k % 2 else b"")
            continue
        n = int(rng.integers(1, 6))
        pos = np.sort(rng.integers(1, 40000, n))
        text = (PREAMBLE if k % 3 else b"") + b"".join(_line("%d" % (1 + k % 5), int(p), rng) for p in pos)
        out.append(text[:-1] if k % 11 == 0 else text)
    return out


_OK = b"1\t10\t.\tA\tC\t.\t.\tDP=1\n"
ERRORS = {  # name: (text, line, words)
    "one-column": (PREAMBLE + _OK + b"1 20 . A C\n", 7, te.E_COLUMNS),
    "pos-12x": (PREAMBLE + _OK + b"1\t12x\t.\tA\tC\n", 7, te.E_POS),
    "pos-empty": (_OK + b"1\t\t.\tA\tC\n", 2, te.E_POS),
    "end-past-2^29": (PREAMBLE + _OK + b"1\t20\t.\tA\tC\t.\t.\tEND=%d\n" % ((1 << 29) + 1), 7, te.E_END),
    "position-down": (PREAMBLE + _OK + b"1\t30\t.\tA\tC\n1\t29\t.\tA\tC\n2\t1\t.\tA\tC\n", 8, te.E_ORDER),
    "one-comes-back": (PREAMBLE + _OK + b"2\t5\t.\tA\tC\n2\t6\t.\tA\tC\n1\t50\t.\tA\tC\n", 9, te.E_BLOCKS),
}


def cosmic_whole() -> bytes:
    return open(GOLDEN, "rb").read()


def cosmic() -> bytes:
    """the file up to its last sorted block: chromosome 1 comes back after MT"""
    text = cosmic_whole()
    recs = []
    o = 0
    while o < len(text):
        e = text.index(b"\n", o) + 1
        recs.append(text[o:e])
        o = e
    mt = max(i for i, r in enumerate(recs) if r.startswith(b"MT\t"))
    return b"".join(recs[:mt + 1])


def regions(text: bytes):
    """The fixed list of regions of a text: per name the whole chromosome, every data line's own span and the single
    positions around its ends, every window and bin edge near a line, ranges across each member cut, a range past the
    last line; and an absent chromosome."""
    recs = te.data_lines(text)
    names = []
    for r in recs:
        if r[0] not in names:
            names.append(r[0])
    out = [(b"absent", 0, 1 << 29), (b"", 0, 100)]
    for name in names:
        mine = [r for r in recs if r[0] == name]
        out.append((name, 0, 1 << 29))
        out.append((name, mine[-1][2], mine[-1][2] + 100000))  # past the last line
        out.append((name, mine[-1][2] + (6 << 14), 1 << 29))
        edges = set()
        for _n, beg, end, _off, _line in mine[::max(1, len(mine) // 20)] + mine[-3:]:
            for p in (beg, end - 1):
                edges.update({p, p + 1, (p >> 14) << 14, ((p >> 14) + 1) << 14})
        for p in (16384, 32768, 131072, 1 << 20):
            edges.update({p - 1, p})
        for p in sorted(edges):
            if 0 <= p < (1 << 29):
                out.append((name, p, p + 1))                   # a single position
                out.append((name, max(p - 1, 0), p + 1))       # across the edge
                out.append((name, p, min(p + 40000, 1 << 29)))
        # ranges whose lines lie around each member cut
        for cut in range(CUT, len(text), CUT):
            near = [r for r in mine if cut - 300 <= r[3] <= cut + 300]
            if near:
                out.append((name, near[0][1], near[-1][2]))
                out.append((name, near[0][1], near[0][1] + 1))
    return out
