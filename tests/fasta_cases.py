"""Reference-genome texts for the compressed-FASTA and device-route tests: the kinds of test_gpu_variant.py rebuilt
here, the quirk texts, seeded random texts, the written forms (plain, BGZF, plain gzip) and loci to ask for."""
import gzip
import os

import numpy as np

from tests import bgzf_writer
from tests import variant_ref as vr

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
MALE = os.path.join(DATA, "genome_diploid_male.fa")
MALE_MAP = os.path.join(DATA, "genome_diploid_male.map")

KINDS = ("diploid", "haploid", "male", "fewer_contigs")
CONTIGS = (400, 300, 250, 200)
ALPHABET = b">\nACgtN\rXYm"


def wrap(s, w=60):
    return "\n".join(s[i:i + w] for i in range(0, len(s), w))


def kind_text(kind, rng, contigs=CONTIGS, width=60) -> bytes:
    """The FASTA of one of test_gpu_variant.py's kinds: contig (pairs) of the given lengths, `width`-column lines."""
    diploid, male = kind != "haploid", kind == "male"
    names = [str(i + 1) for i in range(len(contigs))]
    if male:
        names[-2:] = ["X", "Y"]
    out = []
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    for name, n in zip(names, contigs):
        m = bases[rng.integers(0, 4, n)]
        mat = m.tobytes().decode()
        if diploid and not (male and name in "XY"):
            p = np.where(rng.random(n) < 0.9, m, bases[rng.integers(0, 4, n)])
            out.append(">%s_maternal\n%s\n>%s_paternal\n%s\n" % (name, wrap(mat, width), name,
                                                                 wrap(p.tobytes().decode(), width)))
        elif diploid:
            out.append(">%s_%s\n%s\n" % (name, "maternal" if name == "X" else "paternal", wrap(mat, width)))
        else:
            out.append(">chr%s\n%s\n" % (name, wrap(mat, width)))
    return "".join(out).encode()


def kind_n_chr(kind):
    return 6 if kind == "fewer_contigs" else 4


def kind_loci(rng, kind, contigs=CONTIGS, per_chr=150):
    """Loci as test_gpu_variant.py's _synthetic makes them: sorted positions inside the contig, position 0 in front of
    chromosome 1, a position past the end and a small one after it on chromosome 0. -> (chr_locus_off, locus_pos)."""
    off, pos = [0], []
    for c in range(kind_n_chr(kind)):
        length = contigs[min(c, len(contigs) - 1)]
        p = np.sort(rng.choice(np.arange(1, length + 1), min(length, per_chr), replace=False)).tolist()
        if c == 1:
            p = [0] + p
        if c == 0:
            p = p + [length + 5, 3]
        pos += p
        off.append(len(pos))
    return np.asarray(off, dtype=np.uint32), np.asarray(pos, dtype=np.uint32)


QUIRKS = {
    "empty": b"",
    "newline": b"\n",
    "header_only": b">chr1",
    "header_only_newline": b">chr1\n",
    "alternating_run": b">a\n>b\n>c\nACGT\n",
    "sequence_starts_with_gt": b">a\n>ACGT\nACGT\n>b\nGG\n",
    "no_trailing_newline": b">a\nACGT\n>b\nTTGA",
    "crlf": b">a\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",
    "empty_lines": b">a\nAC\n\nGT\n\n\n>b\n\nA\n",
    "one_long_line": b">a\n" + bytes(b"ACGT"[(i * 7 + i // 5) % 4] for i in range(5000)) + b"\n>b\nACGT\n",
    "lower_u_n": b">a\nacgtuUNnxACGT\n>b\nnnnn\n",
    "x_then_y": b">X_maternal\nACGTAC\n>Y_paternal\nGGT\n",
    "x_last": b">1_maternal\nAC\n>1_paternal\nAG\n>X_maternal\n",
    "missing_paternal": b">1_maternal\nACGT\n",
    "lengths_differ_by_one": b">1_maternal\nACGTA\n>1_paternal\nACGT\n",
    "first_line_not_a_header": b"ACGT\nGGCC\n>b\nTT\n",
    "leading_blank_word": b"\n>1_maternal\nAC\n",
}
QUIRK_N_CHR = 3


def quirk_loci(text: bytes):
    """Every position from 0 to a little past the longest line count, on each of QUIRK_N_CHR chromosomes, unsorted
    on the last one."""
    top = min(len(text), 12) + 3
    one = list(range(0, top))
    last = [5, 1, top + 100, 2, 0xFFFFFFFF, 3]
    pos = one + one[::-1] + last
    off = [0, len(one), 2 * len(one), len(pos)]
    return np.asarray(off, dtype=np.uint32), np.asarray(pos, dtype=np.uint32)


def random_text(rng, max_len=60) -> bytes:
    n = int(rng.integers(0, max_len + 1))
    return bytes(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), n))


def random_diploid_text(rng) -> bytes:
    """`>1_maternal` in front, then contigs in pairs of equal length (one pair in ten differs by a base)."""
    out = b""
    seq_alphabet = b"ACgtN\rm"
    for k in range(int(rng.integers(1, 4))):
        n = int(rng.integers(0, 12))
        name = [b"1", b"2", b"X", b"Y"][int(rng.integers(0, 4))]
        halves = 1 if name == b"Y" else 2
        for h in range(halves):
            m = n + (1 if h == 1 and rng.random() < 0.1 else 0)
            seq = bytes(seq_alphabet[i] for i in rng.integers(0, len(seq_alphabet), m))
            cut = int(rng.integers(0, m + 1))
            body = seq[:cut] + b"\n" + seq[cut:] if rng.random() < 0.5 else seq
            head = b">" + (b"1" if k == 0 and h == 0 else name) + (b"_maternal" if h == 0 else b"_paternal")
            out += head + b"\n" + body + (b"\n" if rng.random() < 0.9 else b"")
            if not out.endswith(b"\n"):
                return out
    return out


def random_loci(rng, max_pos=70):
    n_chr = int(rng.integers(0, 5))
    off, pos = [0], []
    for _ in range(n_chr):
        k = int(rng.integers(0, 9))
        p = rng.integers(0, max_pos, k).tolist()
        if k and rng.random() < 0.2:
            p[int(rng.integers(0, k))] = int(rng.choice([0, 0xFFFFFFFF, 1 << 31]))
        pos += p
        off.append(len(pos))
    return np.asarray(off, dtype=np.uint32), np.asarray(pos, dtype=np.uint32)


FORMS = ("plain", "bgzf", "bgzf37", "gzip1", "gzip3")


def write_form(path, text: bytes, form: str) -> str:
    """The text written in one of FORMS; the name never says which."""
    if form == "plain":
        raw = text
    elif form == "bgzf":
        raw = bgzf_writer.bgzf(text, chunk=0xFF00)
    elif form == "bgzf37":
        raw = bgzf_writer.bgzf(text, chunk=37)
    elif form == "gzip1":
        raw = gzip.compress(text, mtime=0)
    elif form == "gzip3":
        a, b = len(text) // 3, 2 * len(text) // 3
        raw = b"".join(gzip.compress(t, mtime=0) for t in (text[:a], text[a:b], text[b:]))
    else:
        raise ValueError(form)
    with open(path, "wb") as f:
        f.write(raw)
    return str(path)


def restated(text: bytes, n_chr: int):
    """The chromosomes the restatement reads from the text -> list of genotype lists, or the error's message."""
    f, diploid, chr_data, out = vr.Stream(text), vr.check_is_diploid(text), [], []
    for c in range(n_chr):
        line0_empty = c == 0 and text[:1] == b"\n"
        if line0_empty:
            return "empty line"
        try:
            chr_data = vr.get_next_chromosome(f, {}, diploid, chr_data)
        except ValueError as e:
            return str(e)
        out.append(list(chr_data))
    return out
