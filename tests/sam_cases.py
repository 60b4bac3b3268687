"""The inputs of the SAM parser's tests, one table for the host program (tests/test_sam_parse_cpu.py), the four
kernels (tests/test_gpu_sam_kernels.py) and the product (tests/test_gpu_sam_records.py). A case is one range of text
as the kernels see it, with its @SQ names, the selected references, the line index of its first line and whether it
ends the file; ``why`` names the edge it is there for, and a record's QNAME names the edge of that line.

Left out, and why:
 - code 17 (a record of 2^31 bytes or more) needs 2 GiB of text;
 - no case holds two reference names with the same 64-bit FNV-1a hash: none is known, so the walk over a run of equal
   hashes is never taken past its first entry.
The largest case is the line with 65535 CIGAR ops, about 130 KB of text."""
import struct
from typing import List, NamedTuple, Optional, Sequence, Tuple

from tests import bam_writer as bw
from tests import sam_ref as sr
from tests import sam_writer as sw

# the reference list of most cases; the third one is not selected
REFS = [("chr1", 2 ** 31 - 1), ("chr2", 2 ** 31 - 1), ("chrU", 1000)]
NAMES = [n for n, _ in REFS]
SELECTED = [1, 1, 0]


class Case(NamedTuple):
    name: str
    why: str
    text: bytes
    names: Sequence[str] = tuple(NAMES)
    selected: Sequence[int] = tuple(SELECTED)
    line_base: int = 0
    ends_file: bool = True
    product: bool = False  # its good lines on selected references also go through split_clusters
    error: Optional[int] = None  # the error word the case is built to give, where it is built to give one


def fnv1a(name: bytes) -> int:
    h = 1469598103934665603
    for c in name:
        h = ((h ^ c) * 1099511628211) & (2 ** 64 - 1)
    return h


def ref_tables(names: Sequence[str]):
    """The @SQ names as the passes take them: (packed bytes, off[n + 1], hashes ascending, the RefID of each hash)."""
    raw = [n.encode("latin-1") for n in names]
    off = [0]
    for n in raw:
        off.append(off[-1] + len(n))
    order = sorted((fnv1a(n), i) for i, n in enumerate(raw))
    return b"".join(raw), off, [h for h, _ in order], [i for _, i in order]


def line(qname="r", flag=0, rname="chr1", pos=1, mapq=60, cigar="1M", rnext="*", pnext=0, tlen=0, seq="A", qual="I",
         aux=()) -> bytes:
    return "\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual]
                     + list(aux)).encode("latin-1")


def text_of(lines: Sequence[bytes], last_newline=True) -> bytes:
    return b"\n".join(lines) + (b"\n" if last_newline and lines else b"")


GOOD = line("good", pos=7, cigar="4M", seq="ACGT", qual="IIII", aux=["AS:i:5"])


def fitted(length: int) -> bytes:
    """A record line of ``length`` bytes."""
    out = line("f" * (length - len(line("", pos=3))), pos=3)
    assert len(out) == length
    return out


def padded_to(total: int, last_newline=True) -> bytes:
    """GOOD lines and one more record whose QNAME is as long as it takes to make the text ``total`` bytes."""
    stem = len(line("pad_", pos=9)) + (1 if last_newline else 0)
    lines = [GOOD] * ((total - stem - 100) // (len(GOOD) + 1))
    rest = total - len(text_of(lines)) - stem
    assert 0 <= rest <= 250
    out = text_of(lines + [line("pad_" + "p" * rest, pos=9)], last_newline)
    assert len(out) == total
    return out


# ---- line splitting

def _splitting() -> List[Case]:
    junk = (b"ab\tc\n" * 8)
    out = [Case("len_%d" % n, "a text of %d bytes" % n, junk[:n], ends_file=False) for n in (0, 1, 15, 16, 17, 31, 32)]
    out += [
        Case("one_newline", "a text that is one newline", b"\n"),
        Case("len_0_ends_file", "no text at the end of a file: one empty line, no record, no error", b""),
        Case("nl_at_byte_15", "a newline as byte 15 of a vector: the next line starts on a multiple of 16",
             text_of([fitted(31), GOOD])),
        Case("nl_at_byte_0", "a newline as byte 0 of a vector", text_of([fitted(32), GOOD])),
        Case("vector_of_newlines", "a vector of 16 newlines between two records: fifteen empty lines in the file",
             fitted(31) + b"\n" * 17 + GOOD + b"\n", ends_file=False),
        Case("one_workgroup", "4096 bytes: 256 vectors, exactly one workgroup of the newline passes",
             padded_to(4096)),
        Case("second_workgroup", "4112 bytes: one vector in the second workgroup", padded_to(4112)),
        Case("no_last_newline_x16", "a last line without newline, the length a multiple of 16",
             padded_to(256, last_newline=False)),
        Case("no_last_newline_odd", "a last line without newline, the length no multiple of 16",
             padded_to(251, last_newline=False)),
        Case("600_lines", "600 short records: the third workgroup of the size and encode passes",
             text_of([line("s%d" % k, pos=1 + k, rname=NAMES[k % 3]) for k in range(600)])),
    ]
    by = {c.name: c.text for c in out}
    assert by["nl_at_byte_15"][31:32] == b"\n" and by["nl_at_byte_0"][32:33] == b"\n"
    assert by["vector_of_newlines"][32:48] == b"\n" * 16 and by["vector_of_newlines"][48:49] != b"\n"
    return out


# ---- records

def mandatory_lines() -> List[bytes]:
    return [
        line("q"),                                                   # QNAME of one character
        line("n" * 254, pos=2),                                      # QNAME of 254 characters
        line("flag_0", flag=0, pos=3),
        line("flag_65535", flag=65535, pos=4),
        line("pos_0_pnext_0", pos=0, pnext=0),                       # stored as -1
        line("pos_max_pnext_max", pos=2147483647, pnext=2147483647),
        line("tlen_min", tlen=-2147483647, pos=5),
        line("tlen_minus_0", tlen="-0", pos=6),
        line("tlen_max", tlen=2147483647, pos=7),
        line("mapq_0", mapq=0, pos=8),
        line("mapq_255", mapq=255, pos=9),
        line("rnext_same", rnext="=", pnext=100, pos=10),
        line("rnext_none", rnext="*", pos=11),
        line("rnext_other", rnext="chr2", pnext=5, pos=12),
        line("rnext_unselected", rnext="chrU", pnext=5, pos=13),
        line("rnext_same_on_chr2", rname="chr2", rnext="=", pos=14),
        line("rname_none", rname="*", pos=0, flag=4),                # RefID -1, size 0
        line("rname_none_rnext_same", rname="*", rnext="=", pos=0, flag=4),  # '=' of no reference: -1
        line("unselected", rname="chrU", pos=15),                    # RefID and POS reported, size 0
    ]


def bin_lines() -> List[bytes]:
    out = []
    for k in (14, 17, 20, 23, 26, 29):
        for rlen in (1, 2):
            # 0-based start 2^k - 1: the last position of its bin at that level; length 2 crosses into the next
            out.append(line("bin_2p%d_len%d" % (k, rlen), pos=2 ** k, cigar="%dM" % rlen, seq="*", qual="*"))
            out.append(line("bin_2p%d_del%d" % (k, rlen), pos=2 ** k, cigar="1M%dD" % rlen, seq="A", qual="I"))
    out += [
        line("bin_pos0_len1", pos=0, cigar="1M"),
        line("bin_pos0_len2", pos=0, cigar="2M", seq="AC", qual="II"),
        line("bin_pos0_len16385", pos=0, cigar="16385M", seq="*", qual="*"),  # [-1, 16384): clamped to start 0
        line("bin_pos0_len16386", pos=0, cigar="16386M", seq="*", qual="*"),  # and one more crosses into the next bin
        line("bin_no_cigar", pos=2 ** 14, cigar="*"),                # reference length 0 counts as 1
        line("bin_insert_only", pos=2 ** 14, cigar="1I"),
        line("bin_clip_only_end_of_bin", pos=2 ** 17, cigar="1S1H", seq="A", qual="I"),
        line("bin_past_2p29", pos=2 ** 30, cigar="1M"),              # bin numbers past 65535 keep their low 16 bits
    ]
    return out


def cigar_lines() -> List[bytes]:
    return [
        line("all_nine_ops", pos=20, cigar="2H3S5M2I1D3N1P4=1X1S", seq="ACGTNACGTACGTAGC", qual="I" * 16),
        line("op_length_max", pos=21, cigar="%dM" % (2 ** 28 - 1), seq="*", qual="*"),
        line("op_length_max_twice", pos=22, cigar="%dN%dD" % (2 ** 28 - 1, 2 ** 28 - 1), seq="*", qual="*"),
        line("op_leading_zeros", pos=23, cigar="0001M"),
    ]


def many_ops_line(n=65535, qname="ops_65535") -> bytes:
    return line(qname, pos=24, cigar="1M" * n, seq="*", qual="*")


def seq_qual_lines() -> List[bytes]:
    letters = "=ACMGRSVTWYHKDBN"
    rest = "EFIJLOPQUXZ"  # the letters that are no IUPAC code
    return [
        line("codes_upper", pos=30, cigar="16M", seq=letters, qual="~" * 16),
        line("codes_lower", pos=31, cigar="16M", seq=letters.lower(), qual="!" * 16),
        line("other_letters", pos=32, cigar="22M", seq=rest + rest.lower(), qual="5" * 22),
        line("non_letters", pos=33, cigar="8M", seq=".5-[`{@\x7f", qual="I" * 8),  # code 15 each
        # a kept departure (include/secedo_bam.h): htslib reads the digits 0..3 as A, C, G, T; here they are code 15
        line("digits_0_to_3", pos=33, cigar="4M", seq="0123", qual="IIII"),
        line("high_bytes", pos=33, cigar="4M", seq="\xe1\xc1\xff\x80", qual="IIII"),  # 'A' | 0x80 is no 'A'
        line("seq_1", pos=34, cigar="1M", seq="C", qual="!"),
        line("seq_2", pos=35, cigar="2M", seq="CG", qual="!~"),
        line("seq_3", pos=36, cigar="3M", seq="CGT", qual="~!~"),    # an odd length: the last nibble is zero
        line("seq_3_n", pos=36, cigar="3M", seq="NNN", qual="*"),    # and stays zero behind a code 15
        line("no_qual", pos=37, cigar="5M", seq="ACGTA", qual="*"),  # 0xFF each
        line("no_seq_no_qual", pos=38, cigar="5M", seq="*", qual="*"),
        line("seq_without_cigar", pos=39, cigar="*", seq="ACG", qual="III"),
        line("qual_is_a_star_of_length_1", pos=40, cigar="1M", seq="A", qual="*"),
    ]


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


def covering_lines() -> List[bytes]:
    recs = sw.canonical(covering_records())
    return [sw.record_line(r, REFS).encode("latin-1") for r in recs]


AUX_INTS = [-129, -128, -1, 0, 255, 256, 65535, 65536, -32768, -32769, -2147483648, 4294967295, 127, 128, 32767, 32768,
            2147483647, 2147483648, -2147483647]


def f32_text(bits: int) -> str:
    return "%.9g" % struct.unpack("<f", struct.pack("<I", bits))[0]


def float_texts() -> List[Tuple[str, str]]:
    """(what, text): at most 9 significant digits each."""
    out = [("largest_finite", f32_text(0x7F7FFFFF)), ("largest_finite_negative", "-" + f32_text(0x7F7FFFFF)),
           ("smallest_normal", f32_text(0x00800000)), ("smallest_denormal", f32_text(0x00000001)),
           ("largest_denormal", f32_text(0x007FFFFF)), ("one_and_an_ulp", f32_text(0x3F800001)),
           ("below_one", f32_text(0x3F7FFFFF))]
    bits = 0x9E3779B9
    for k in range(40):  # float32 values all over the exponent range, printed with %.9g
        bits = (bits * 1664525 + 1013904223) & 0xFFFFFFFF
        if (bits >> 23) & 0xFF != 0xFF:
            out.append(("nine_digits_%d" % k, f32_text(bits)))
    # exact ties between two floats, which round to even; each of these came out one float too high with a power of
    # ten that is off in its last place
    out += [("tie_g_%d" % k, t) for k, t in enumerate(("2.65189e+08", "7.12013e+07", "6.43428e+08", "265189000",
                                                       "16777217"))]
    # an exact tie at every power of ten that can make one: m * 5^k odd and of 25 bits, so m * 10^k lies half way
    # between two floats and is exact in double; m and m + 2 round to even in opposite directions. A power of ten that
    # is off in its last place moves one of each pair off its tie, to the wrong side. (5^11 has more than 25 bits.)
    for k in range(11):
        m = -(-2 ** 24 // 5 ** k) | 1
        assert 2 ** 24 < m * 5 ** k < 2 ** 25 and m + 2 < 10 ** 9
        out.append(("tie_e%d_a" % k, "%de%d" % (m, k)))
        if (m + 2) * 5 ** k < 2 ** 25:  # all but 10^10, where only 3e10 fits
            out.append(("tie_e%d_b" % k, "%de+%d" % (m + 2, k)))
    out += [("tenth", "0.1"), ("exponent_minus_3", "1e-3"), ("minus_zero", "-0"), ("no_fraction_digits", "5."),
            ("no_integer_digits", ".5"), ("capital_e_plus", "1E+2"), ("plus_sign", "+2.5"), ("zero", "0"),
            ("zero_with_exponent", "0e5"), ("leading_zeros", "000.250")]
    return out


def aux_lines() -> List[bytes]:
    out = [line("i_%d" % k, pos=50, aux=["XI:i:%d" % v]) for k, v in enumerate(AUX_INTS)]
    out += [
        line("i_minus_0", pos=51, aux=["XI:i:-0"]),                  # zero: the unsigned byte
        line("i_leading_zeros", pos=51, aux=["XI:i:000256"]),
        line("A_first", pos=52, aux=["XA:A:!"]),
        line("A_last", pos=52, aux=["XA:A:~"]),
        line("Z_empty", pos=53, aux=["XZ:Z:"]),
        line("H_empty", pos=53, aux=["XH:H:"]),
        line("Z_with_colons_and_spaces", pos=53, aux=["XZ:Z:a b:c:", "X1:Z::"]),
        line("tag_with_digit_lower", pos=53, aux=["a9:i:1", "zZ:A:z"]),
        line("Z_empty_then_more", pos=53, aux=["XZ:Z:", "XY:i:1"]),
    ]
    for sub, (lo, hi) in sr.B_RANGE.items():
        out += [
            line("B_%s_none" % sub, pos=54, aux=["XB:B:%s" % sub]),
            line("B_%s_one_low" % sub, pos=54, aux=["XB:B:%s,%d" % (sub, lo)]),
            line("B_%s_one_high" % sub, pos=54, aux=["XB:B:%s,%d" % (sub, hi)]),
            line("B_%s_300" % sub, pos=54,
                 aux=["XB:B:%s" % sub + "".join(",%d" % (lo if k % 2 else hi) for k in range(300)), "XE:i:1"]),
        ]
    big = f32_text(0x7F7FFFFF)
    out += [
        line("B_f_none", pos=55, aux=["XB:B:f"]),
        line("B_f_one_low", pos=55, aux=["XB:B:f,-" + big]),
        line("B_f_one_high", pos=55, aux=["XB:B:f," + big]),
        line("B_f_300", pos=55, aux=["XB:B:f" + "".join("," + ("-" + big if k % 2 else big) for k in range(300))]),
        line("B_f_every_text", pos=55, aux=["XB:B:f" + "".join("," + t for _, t in float_texts()), "XE:i:1"]),
    ]
    out += [line("f_" + what, pos=56, aux=["XF:f:" + t]) for what, t in float_texts()]
    twenty = ["T%s:%s" % (chr(65 + k), ("i:%d" % (k * 1000 - 7000), "A:%s" % chr(40 + k), "Z:v%d" % k, "f:%d.5" % k,
                                "B:s,%d,-%d" % (k, k), "H:%02X" % k)[k % 6]) for k in range(20)]
    out.append(line("twenty_fields", pos=57, aux=twenty))
    return out


def _records() -> List[Case]:
    many = ["c"] + ["c%d" % k for k in range(1, 300)]
    _, _, hashes, ids = ref_tables(many)
    picked = [ids[0], ids[1], ids[149], ids[150], ids[298], ids[299], many.index("c"), many.index("c1"),
              many.index("c10"), many.index("c100"), many.index("c29"), many.index("c299")]
    sel_many = [k % 2 for k in range(300)]
    return [
        Case("mandatory", "the ends of every mandatory field's range, RNEXT in its three forms, RNAME '*', a reference "
             "that is not selected", text_of(mandatory_lines()), product=True),
        Case("bins", "reg2bin at the last position of a bin at every level, for reference lengths 1 and 2, at POS 0 "
             "and for a reference length of 0", text_of(bin_lines()), product=True),
        Case("cigar", "all nine ops, the largest op length", text_of(cigar_lines()), product=True),
        Case("ops_65535", "the largest number of ops, with SEQ '*'", text_of([many_ops_line()]), product=True),
        Case("seq_qual", "all 16 codes in both cases, code 15 for everything else, SEQ of 1, 2, 3, QUAL '*', '!', '~'",
             text_of(seq_qual_lines()), product=True),
        Case("covering", "covering_records(): every op, aux type and subtype", text_of(covering_lines()), product=True),
        Case("aux", "integers at every type boundary, A, empty Z and H, B arrays of 0, 1 and 300 values at both ends "
             "of each subtype, floats, twenty fields", text_of(aux_lines()), product=True),
        Case("one_sq", "a single @SQ line", text_of([line("a", rname="only", rnext="only"), line("b", rname="only",
                                                                                                  rnext="=")]),
             names=("only",), selected=(1,)),
        Case("one_sq_unselected", "a single @SQ line that is not selected: nothing is written",
             text_of([line("a", rname="only")]), names=("only",), selected=(0,)),
        Case("300_sq", "300 names that share prefixes and differ in length; those whose hashes sort first, last and in "
             "the middle", text_of([line("n%d" % i, rname=many[i], rnext=many[picked[(k + 1) % len(picked)]], pos=1 + k)
                                    for k, i in enumerate(picked)]), names=tuple(many), selected=tuple(sel_many)),
    ]


# ---- errors

def error_lines() -> List[Tuple[int, str, bytes]]:
    """(code, what, line): the first line of every code is the one the product test sends through pileup_bams."""
    E = sr
    long_name = "n" * 255
    return [
        (E.FIELDS, "ten fields", b"\t".join(GOOD.split(b"\t")[:10])),
        (E.FIELDS, "an empty field", line(rnext="")),
        (E.FIELDS, "a line of one tab", b"\t"),
        (E.FIELDS, "an empty QUAL", line(qual="")),
        (E.NAME, "QNAME of 255", line(long_name)),
        (E.FLAG, "FLAG 65536", line(flag=65536)),
        (E.FLAG, "FLAG with a sign", line(flag="-0")),
        (E.FLAG, "FLAG in hex", line(flag="0x10")),
        (E.FLAG, "FLAG with a plus", line(flag="+1")),
        (E.RNAME, "RNAME unknown", line(rname="chr3")),
        (E.RNAME, "RNAME a prefix of a name", line(rname="chr")),
        (E.RNAME, "RNAME '=' ", line(rname="=")),
        (E.POS, "POS 2^31", line(pos=2147483648)),
        (E.POS, "POS negative", line(pos=-1)),
        (E.POS, "POS of 30 digits", line(pos="1" * 30)),
        (E.MAPQ, "MAPQ 256", line(mapq=256)),
        (E.CIGAR, "a zero-length op", line(cigar="0M")),
        (E.CIGAR, "an op of 2^28", line(cigar="%dM" % 2 ** 28, seq="*", qual="*")),
        (E.CIGAR, "an unknown op", line(cigar="1Q")),
        (E.CIGAR, "a lower-case op", line(cigar="1m")),
        (E.CIGAR, "digits without an op", line(cigar="1M2")),
        (E.CIGAR, "an op without digits", line(cigar="M")),
        (E.CIGAR, "an op of 20 digits", line(cigar="%dM" % 10 ** 19, seq="*", qual="*")),
        (E.RNEXT, "RNEXT unknown", line(rnext="chr9")),
        (E.PNEXT, "PNEXT 2^31", line(pnext=2147483648)),
        (E.TLEN, "TLEN -2^31", line(tlen=-2147483648)),
        (E.TLEN, "TLEN 2^31", line(tlen=2147483648)),
        (E.TLEN, "TLEN only a sign", line(tlen="-")),
        (E.TLEN, "TLEN two signs", line(tlen="--1")),
        (E.QUAL, "a CRLF line: the carriage return is a QUAL character", line() + b"\r"),
        (E.QUAL, "QUAL longer than SEQ", line(qual="II")),
        (E.QUAL, "QUAL with a space", line(cigar="2M", seq="AC", qual="I ")),
        (E.QUAL, "QUAL with 0x7F", line(cigar="2M", seq="AC", qual="I\x7f")),
        (E.QUAL, "QUAL for SEQ '*'", line(seq="*", qual="I")),
        (E.CIGAR_SEQ, "CIGAR of 2 against SEQ of 1", line(cigar="2M")),
        (E.CIGAR_SEQ, "H does not count", line(cigar="1M1H", seq="AC", qual="II")),
        (E.AUX, "no second colon", line(aux=["AS:i-90"])),
        (E.AUX, "a trailing tab", line() + b"\t"),
        (E.AUX, "an empty field between two", line(aux=["XA:A:a", "", "XB:A:b"])),
        (E.AUX, "B with no value behind its comma", line(aux=["XB:B:c,"])),
        (E.AUX, "B value out of range", line(aux=["XB:B:c,200"])),
        (E.AUX, "B value with a sign in an unsigned array", line(aux=["XB:B:C,-0"])),
        (E.AUX, "B without a subtype", line(aux=["XB:B:"])),
        (E.AUX, "B with an unknown subtype", line(aux=["XB:B:d,1"])),
        (E.AUX, "B with no comma behind the subtype", line(aux=["XB:B:c1"])),
        (E.AUX, "i of 2^32", line(aux=["XX:i:4294967296"])),
        (E.AUX, "i of -2^31 - 1", line(aux=["XX:i:-2147483649"])),
        (E.AUX, "i empty", line(aux=["XX:i:"])),
        (E.AUX, "i with a plus", line(aux=["XX:i:+1"])),
        (E.AUX, "f with an empty exponent", line(aux=["XX:f:1e"])),
        (E.AUX, "f inf", line(aux=["XX:f:inf"])),
        (E.AUX, "f nan", line(aux=["XX:f:nan"])),
        (E.AUX, "f of only a point", line(aux=["XX:f:."])),
        (E.AUX, "f empty", line(aux=["XX:f:"])),
        (E.AUX, "f with a signed empty exponent", line(aux=["XX:f:1e+"])),
        (E.AUX, "f in hex", line(aux=["XX:f:0x1p3"])),
        (E.AUX, "B:f with a bad value", line(aux=["XX:B:f,1.5,x"])),
        (E.AUX, "A of two characters", line(aux=["XX:A:ab"])),
        (E.AUX, "A empty", line(aux=["XX:A:"])),
        (E.AUX, "A of a space", line(aux=["XX:A: "])),
        (E.AUX, "an unknown type", line(aux=["XX:Q:1"])),
        (E.AUX, "a tag that starts with a digit", line(aux=["1X:i:1"])),
        (E.AUX, "a tag with a punctuation character", line(aux=["X_:i:1"])),
        (E.AUX, "a field of four characters", line(aux=["XX:i"])),
        (E.AUX, "the second of two fields", line(aux=["XA:i:1", "XB:i:x"])),
        (E.HEADER, "a header line", b"@CO\tlate"),
        (E.HEADER, "a lone '@'", b"@"),
        (E.EMPTY, "an empty line inside the file", b""),
        (E.MANY_OPS, "65536 ops", many_ops_line(65536, "ops_65536")),
    ]


def two_defect_lines() -> List[Tuple[int, str, bytes]]:
    """Lines with two defects: the code of the one checked first."""
    E = sr
    return [
        (E.NAME, "QNAME before FLAG", line("n" * 255, flag=65536)),
        (E.FLAG, "FLAG before RNAME", line(flag=65536, rname="chr3")),
        (E.RNAME, "RNAME before POS", line(rname="chr3", pos=-1)),
        (E.POS, "POS before MAPQ", line(pos=-1, mapq=256)),
        (E.MAPQ, "MAPQ before CIGAR", line(mapq=256, cigar="0M")),
        (E.CIGAR, "CIGAR before RNEXT", line(cigar="0M", rnext="chr9")),
        (E.CIGAR, "a bad op before the count of ops", many_ops_line(65536).replace(b"1M\t*", b"0M\t*")),
        (E.MANY_OPS, "the count of ops before RNEXT", many_ops_line(65536).replace(b"\t*\t0\t0\t", b"\tchr9\t0\t0\t")),
        (E.RNEXT, "RNEXT before PNEXT", line(rnext="chr9", pnext=-1)),
        (E.PNEXT, "PNEXT before TLEN", line(pnext=-1, tlen="x")),
        (E.TLEN, "TLEN before QUAL", line(tlen="x", qual="II")),
        (E.QUAL, "QUAL before CIGAR against SEQ", line(cigar="2M", qual="II")),
        (E.CIGAR_SEQ, "CIGAR against SEQ before the optional fields", line(cigar="2M", aux=["XX:i:x"])),
        (E.FIELDS, "the fields before everything", line("n" * 255, flag=65536, qual="")),
        (E.HEADER, "'@' before the fields", b"@\t\t"),
    ]


def _errors() -> List[Case]:
    out = []
    for k, (code, what, bad) in enumerate(error_lines() + two_defect_lines()):
        out.append(Case("error_%d_code_%d" % (k, code), what,
                        text_of([GOOD, line("g2", rname="chr2", pos=3), bad, GOOD]), error=2 << 8 | code))
    short = [line("s%d" % k, pos=1 + k) for k in range(600)]
    bad3_400 = list(short)
    bad3_400[3] = line("bad3", mapq=256)
    bad3_400[400] = line("bad400", flag=65536)
    bad_late = list(short)
    bad_late[598] = line("bad598", tlen="x")
    out += [
        Case("bad_3_and_400", "bad lines in two workgroups: the lower line is reported", text_of(bad3_400),
             error=3 << 8 | sr.MAPQ),
        Case("bad_598", "a bad line in the third workgroup", text_of(bad_late), error=598 << 8 | sr.TLEN),
        Case("line_base_2p33", "the error word is composed in 64 bits", text_of([GOOD, line(mapq=256)]),
             line_base=2 ** 33, error=(2 ** 33 + 1) << 8 | sr.MAPQ),
        Case("line_base_2p33_good", "no error at a large line_base", text_of([GOOD, GOOD]), line_base=2 ** 33,
             error=sr.NO_ERROR),
        Case("empty_last_line_ends_file", "an empty last line at the end of the file is no record and no error",
             text_of([GOOD, GOOD]) + b"\n", ends_file=True, error=sr.NO_ERROR),
        Case("empty_last_line_inside", "an empty last line of a range inside the file is code 15",
             text_of([GOOD, GOOD]) + b"\n", ends_file=False, error=2 << 8 | sr.EMPTY),
        Case("two_empty_last_lines", "of two empty lines at the end of the file the first is code 15",
             text_of([GOOD]) + b"\n\n", ends_file=True, error=1 << 8 | sr.EMPTY),
        Case("good_last_line_no_newline", "the last line without newline is a record like any other",
             text_of([GOOD, line("last", pos=9, aux=["XZ:Z:end"])], last_newline=False), error=sr.NO_ERROR),
        Case("bad_last_line_no_newline", "a defect in the last field of a last line without newline",
             text_of([GOOD, line("last", pos=9, aux=["XB:B:c,"])], last_newline=False), error=1 << 8 | sr.AUX),
    ]
    return out


def _build() -> List[Case]:
    cases = _splitting() + _records() + _errors()
    cases = [c._replace(error=sr.NO_ERROR) if c.product else c for c in cases]
    assert len({c.name for c in cases}) == len(cases)
    assert max(len(c.text) for c in cases) < 140_000 and all(c.text.count(b"\n") <= 601 for c in cases)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def product_lines() -> List[bytes]:
    """The good lines of the product cases on selected references, in (RefID, POS) order (stable). Lines with POS 0 stay
    with the parser's own tests: the input layer refuses a record of a requested chromosome with a negative position
    (bam_walk.hpp, kErrNegative)."""
    keyed = []
    for c in CASES:
        if not c.product:
            continue
        for ln in c.text.split(b"\n")[:-1]:
            rec = sr.parse_line(ln.decode("latin-1"), NAMES)
            ref, pos = struct.unpack_from("<ii", rec, 4)
            if ref >= 0 and SELECTED[ref] and pos >= 0:
                keyed.append((ref, pos, len(keyed), ln))
    return [ln for _, _, _, ln in sorted(keyed)]
