"""SAM input without a GPU: tests/sam_writer.py writes the records ``bw.encode_record`` encodes (checked with a small
SAM -> BAM record parser that follows the rules of include/secedo_bam.h), the golden .sam fixtures hold their .bam's
records, and ``pileup_main`` finds SAM files in a directory that holds no BAM."""
import os
import struct

import pytest

from secedo_amd import pileup_main
from tests import bam_writer as bw
from tests import sam_writer as sw
from tests.golden_util import GOLDEN

NT16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
B_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
B_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1),
           "I": (0, 2 ** 32 - 1)}


class SamError(Exception):
    pass


def _int(s, lo, hi, what):
    if not s or not s.lstrip("-").isdigit() or (s.startswith("-") and lo >= 0) or not lo <= int(s) <= hi:
        raise SamError(what)
    return int(s)


def parse_aux(f: str) -> bytes:
    if len(f) < 5 or f[2] != ":" or f[4] != ":" or not f[0].isalpha() or not f[1].isalnum():
        raise SamError("aux")
    tag, typ, v = f[:2], f[3], f[5:]
    out = tag.encode()
    if typ == "A":
        if len(v) != 1 or not "!" <= v <= "~":
            raise SamError("aux")
        return out + b"A" + v.encode()
    if typ == "i":
        x = _int(v, -2 ** 31, 2 ** 32 - 1, "aux")
        t = sw.smallest_int_type(x)
        return out + t.encode() + struct.pack(B_FMT[t], x)
    if typ == "f":
        return out + b"f" + struct.pack("<f", float(v))
    if typ in "ZH":
        return out + typ.encode() + v.encode() + b"\0"
    if typ == "B":
        if not v or v[0] not in B_FMT or (len(v) > 1 and v[1] != ","):
            raise SamError("aux")
        vals = v[2:].split(",") if len(v) > 1 else []
        sub = v[0]
        body = b"".join(struct.pack("<f", float(x)) if sub == "f" else struct.pack(B_FMT[sub], _int(x, *B_RANGE[sub], "aux"))
                        for x in vals)
        return out + b"B" + sub.encode() + struct.pack("<I", len(vals)) + body
    raise SamError("aux")


def parse_line(line: str, names) -> bytes:
    """One SAM alignment line -> the BAM record (block_size first) under the rules of include/secedo_bam.h."""
    f = line.split("\t")
    if len(f) < 11 or any(not x for x in f[:11]):
        raise SamError("fields")
    ids = {n: i for i, n in enumerate(names)}
    qname, flag = f[0], _int(f[1], 0, 65535, "flag")
    if f[2] != "*" and f[2] not in ids:
        raise SamError("rname")
    ref = -1 if f[2] == "*" else ids[f[2]]
    pos = _int(f[3], 0, 2 ** 31 - 1, "pos") - 1
    mapq = _int(f[4], 0, 255, "mapq")
    cigar = []
    if f[5] != "*":
        num = ""
        for c in f[5]:
            if c.isdigit():
                num += c
                continue
            if not num or c not in bw.CIGAR_OPS or not 1 <= int(num) < 2 ** 28:
                raise SamError("cigar")
            cigar.append((c, int(num)))
            num = ""
        if num:
            raise SamError("cigar")
    if f[6] == "=":
        nref = ref
    elif f[6] == "*":
        nref = -1
    elif f[6] in ids:
        nref = ids[f[6]]
    else:
        raise SamError("rnext")
    pnext = _int(f[7], 0, 2 ** 31 - 1, "pnext") - 1
    tlen = _int(f[8], -(2 ** 31 - 1), 2 ** 31 - 1, "tlen")
    seq = "" if f[9] == "*" else f[9]
    if f[10] == "*":
        qual = b"\xff" * len(seq)
    else:
        if len(f[10]) != len(seq) or any(not "!" <= c <= "~" for c in f[10]):
            raise SamError("qual")
        qual = bytes(ord(c) - 33 for c in f[10])
    if cigar and seq and sum(n for op, n in cigar if op in "MIS=X") != len(seq):
        raise SamError("cigar/seq")
    rlen = max(bw.ref_length(cigar), 1)
    codes = [NT16.get(c.upper(), 15) for c in seq] + ([0] if len(seq) % 2 else [])
    core = struct.pack("<iiBBHHHIiii", ref, pos, len(qname) + 1, mapq, bw.reg2bin(max(pos, 0), max(pos + rlen, 1)),
                       len(cigar), flag, len(seq), nref, pnext, tlen)
    body = (core + qname.encode() + b"\0" + b"".join(struct.pack("<I", n << 4 | bw.CIGAR_OPS.index(op))
                                                        for op, n in cigar)
            + bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2)) + qual
            + b"".join(parse_aux(x) for x in f[11:]))
    return struct.pack("<i", len(body)) + body


REFS = [("chr1", 5000), ("chr2", 4000)]


def covering_records():
    q = lambda n: [(7 * k) % 60 for k in range(n)]  # noqa: E731
    return [
        bw.Rec("all_ops", 0, 99, [("H", 2), ("S", 3), ("M", 5), ("I", 2), ("D", 1), ("N", 3), ("P", 1), ("=", 4),
                                  ("X", 1), ("S", 1)], "ACGTNACGTACGTAGC", qual=q(16),
               tags=[("AS", "i", 79), ("XN", "i", -27), ("GP", "i", 698303082), ("XS", "S", 300), ("XT", "s", -300),
                     ("XU", "I", 70000), ("XI", "i", -70000), ("XA", "A", "q"), ("XF", "f", 1.5),
                     ("XZ", "Z", "a b:c"), ("XH", "H", "1AE301"), ("XB", "B", ("c", [-1, 2, -128])),
                     ("YB", "B", ("C", [255])), ("ZB", "B", ("s", [-300, 300])), ("ZC", "B", ("S", [65535])),
                     ("ZI", "B", ("i", [-2 ** 31])), ("ZJ", "B", ("I", [2 ** 32 - 1])),
                     ("ZF", "B", ("f", [0.25, -3.0])), ("ZE", "B", ("c", []))],
               next_ref=0, next_pos=400, tlen=-317),
        bw.Rec("noseq", 0, 200, [("M", 20)], "*", tags=[("AS", "C", 3)], next_ref=1, next_pos=10, tlen=0),
        bw.Rec("noqual", 1, 0, [("M", 4)], "RYKM", qual=None),
        bw.Rec("nocigar", 1, 30, [], "ACGT", qual=[30] * 4),
        bw.Rec("unmapped", -1, -1, [], "ACGTA", qual=[20] * 5, flag=0x4),
        bw.Rec("iupac", 1, 3000, [("M", 16)], "=ACMGRSVTWYHKDBN", qual=[93] * 16),
        bw.Rec("odd.x-y", 1, 3100, [("S", 1), ("M", 2)], "ZAC", qual=[0, 1, 2]),
    ]


def test_writer_lines_parse_to_encode_record():
    names = [n for n, _ in REFS]
    recs = sw.canonical(covering_records())
    text = sw.sam_text(REFS, recs)
    lines = text.splitlines()
    assert lines[0].startswith("@HD") and lines[1:3] == ["@SQ\tSN:chr1\tLN:5000", "@SQ\tSN:chr2\tLN:4000"]
    for line, r in zip(lines[3:], recs):
        assert parse_line(line, names) == bw.encode_record(r), r.name
    # lowercase bases give the upper-case codes
    low = sw.record_line(recs[0], REFS).split("\t")
    low[9] = low[9].lower()
    assert parse_line("\t".join(low), names) == bw.encode_record(recs[0])


def test_canonical_types():
    r = sw.canonical([bw.Rec("x", 0, 1, [("M", 1)], "A", tags=[("AS", "S", 79), ("XS", "i", -27), ("GP", "i", 698303082),
                                                               ("ZZ", "I", 300), ("ZS", "Z", "v")])])[0]
    assert [t[1] for t in r.tags] == ["C", "c", "I", "S", "Z"]


@pytest.mark.parametrize("line", [
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA\tI\tAS:i-90",      # the second ':' missing
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA",                  # ten fields
    "r\t0\tchr3\t1\t60\t1M\t*\t0\t0\tA\tI",               # RNAME not in @SQ
    "r\t0\tchr1\t1\t60\t2M\t*\t0\t0\tA\tI",               # CIGAR against SEQ
    "r\t0\tchr1\t1\t60\t0M\t*\t0\t0\tA\tI",               # a zero-length op
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA\tII",              # QUAL length
    "r\t65536\tchr1\t1\t60\t1M\t*\t0\t0\tA\tI",           # FLAG range
    "r\t0\tchr1\t1\t60\t1M\t*\t0\t0\tA\tI\tXX:i:4294967296",
])
def test_reference_parser_refuses(line):
    with pytest.raises(SamError):
        parse_line(line, ["chr1"])


@pytest.mark.parametrize("name", ["hard_clipping", "soft_clipping", "insert_at_end", "test2", "test3"])
def test_golden_sam_holds_its_bam(name):
    """Each golden .sam parses to its .bam's records (the bin field aside: the fixtures' writer computes it)."""
    refs, _ = bw.read_bam(os.path.join(GOLDEN, "bam", name + ".bam"))
    raw = bw.gzip.decompress(open(os.path.join(GOLDEN, "bam", name + ".bam"), "rb").read())
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    want = []
    while o < len(raw):
        bs = struct.unpack_from("<i", raw, o)[0]
        want.append(raw[o:o + 4 + bs])
        o += 4 + bs
    lines = [l for l in open(os.path.join(GOLDEN, "bam", name + ".sam")).read().split("\n") if l and l[0] != "@"]
    got = [parse_line(l, [n for n, _ in refs]) for l in lines]
    strip = lambda b: b[:14] + b[16:]  # noqa: E731
    assert [strip(g) for g in got] == [strip(w) for w in want]


def test_input_files_falls_back_to_sam(tmp_path):
    d = tmp_path / "sams"
    (d / "sub").mkdir(parents=True)
    for p in ("b_1.sam", "sub/a_2.sam", "notes.txt"):
        (d / p).write_text("")
    assert pileup_main.input_files(str(d)) == sorted([str(d / "b_1.sam"), str(d / "sub" / "a_2.sam")])
    single = str(d / "b_1.sam")
    assert pileup_main.input_files(single) == [single]


def test_input_files_prefers_bam(tmp_path):
    for p in ("x_1.bam", "x_2.sam", "y_3.bam"):
        (tmp_path / p).write_text("")
    assert pileup_main.input_files(str(tmp_path)) == [str(tmp_path / "x_1.bam"), str(tmp_path / "y_3.bam")]


def test_help_names_sam(capsys):
    with pytest.raises(SystemExit):
        pileup_main.parse_args(["--help"])
    assert "SAM" in capsys.readouterr().out
