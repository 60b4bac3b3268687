"""Edge inputs for pileup creation from BAM files, one family per rule of the reference's pileup_bams() that the seeded
synthetic sets meet only by chance: CIGAR shapes, the wrapping u16 coverage counter, the signed-char quality compare,
the second 2^24-position device window, the 1,000,000-position chunks and MAX_INSERT_SIZE, every threshold at and one
below its value, the aux layouts GetTag("AS", uint32_t&) walks, SEQ codes, and the batch slots of the read-name maps.

No random numbers: bases and qualities are arithmetic on the record index, so the expectations committed in
tests/golden/pileup_edges.npz (recorded from the compiled reference by oracle/gen_golden.py pileup_edges) cannot drift.
Every record has flag 0x3 and a SEQ as long as its CIGAR's M/I/S/=/X ops, so every file is a structurally valid BAM.
Importable without torch.

``build(family, directory)`` writes the family's files (with a .bai each, which the reference needs) and returns its
cases as ``Case(name, files, params, kind)``: ``params`` = (max_coverage, min_base_quality, min_map_quality,
min_alignment_score, min_different) at chromosome 0, ``kind`` one of CLEAN, ABORT (an assert of the reference) and
UNDEFINED (the reference reads past the quality string there: an error here, nothing recorded).
"""
from __future__ import annotations

import contextlib
import functools
import itertools
import os
import struct
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from tests import bai_writer
from tests import bam_writer as bw
from tests import pileup_bam_ref as ref

CLEAN, ABORT, UNDEFINED = "clean", "abort", "undefined"
FAMILIES = ("cigars", "wrap", "quality", "window", "chunks", "thresholds", "tags", "seq", "slots")
SMALL_FAMILIES = tuple(f for f in FAMILIES if f != "cigars")  # their .txt lines are recorded too
WINDOW = 1 << 24  # positions per device window
FLAG = 0x3
OPEN = (100, 0, 0, 0, 0)  # max_coverage 100, every other threshold 0


class Case(NamedTuple):
    name: str
    files: Tuple[str, ...]
    params: Tuple[int, int, int, int, int]
    kind: str


def case_name(family: str, what: str, params) -> str:
    return "%s/%s@%s" % (family, what, ",".join(str(p) for p in params))


def family_of(name: str) -> str:
    return name.split("/", 1)[0]


def seq_len(cigar) -> int:
    return sum(n for op, n in cigar if op in "MIS=X")


def read(name, pos, cigar, idx, **kw) -> bw.Rec:
    """A record whose k-th base is ACGT[(idx + k) % 4] with quality 30 + (idx + k) % 10."""
    n = seq_len(cigar)
    kw.setdefault("seq", "".join("ACGT"[(idx + k) % 4] for k in range(n)) if n else "*")
    kw.setdefault("qual", [30 + (idx + k) % 10 for k in range(n)])
    kw.setdefault("flag", FLAG)
    return bw.Rec(name, 0, pos, list(cigar), **kw)


def write(directory, name, records: Sequence[bw.Rec], ref_len=3_000_000) -> str:
    path = os.path.join(str(directory), name + ".bam")
    bw.write_bam(path, [("1", ref_len)], sorted(records, key=bw.sort_key))
    bai_writer.write_bai(path)
    return path


# ------------------------------------------------------------------------------------------------------------
# cigars

CIGAR_LENGTHS = (2, 1, 3, 2)
INSERT_NOT_LAST, DELETION, QUALITY_INDEX = "insert not last", "deletion", "quality index"
ABORT_CLASSES = (INSERT_NOT_LAST, DELETION, QUALITY_INDEX)
SLOT = 40  # positions per CIGAR in the one file
PER_CLASS = 8


def all_cigars() -> List[List[Tuple[str, int]]]:
    """Every op sequence of length 1 to 3 over MIDNSHP=X, and the four-op ones that start with S, H or M and hold at
    least three distinct ops; the op at position p has length CIGAR_LENGTHS[p]. 2,835 in all."""
    out = []
    for n in (1, 2, 3):
        out.extend(itertools.product(bw.CIGAR_OPS, repeat=n))
    out.extend(s for s in itertools.product(bw.CIGAR_OPS, repeat=4) if s[0] in "SHM" and len(set(s)) >= 3)
    return [[(op, CIGAR_LENGTHS[p]) for p, op in enumerate(s)] for s in out]


def cigar_text(cigar) -> str:
    return "".join("%d%s" % (n, op) for op, n in cigar)


def abort_class(message: str) -> str:
    """The class of a RefAbort raised by the restatement's walk."""
    if message.startswith("quality index"):
        return QUALITY_INDEX
    if message == "deletion":
        return DELETION
    return INSERT_NOT_LAST  # the asserts on cigar_idx when AlignedBases ends inside the CIGAR


def classify_cigars():
    """-> (walked, aborting): [(index, cigar)] of the CIGARs the restatement walks, {class: [(index, cigar)]} of the
    others, at thresholds 0."""
    walked, aborting = [], {c: [] for c in ABORT_CLASSES}
    for idx, cigar in enumerate(all_cigars()):
        r = read("c%04d" % idx, 100 + SLOT * idx, cigar, idx)
        d = dict(name=r.name.encode(), ref=0, pos=r.pos, mapq=r.mapq, flag=r.flag, cigar=r.cigar,
                 seq="" if r.seq == "*" else r.seq, qual=bytes(r.qual), aux=b"")
        try:
            ref.walk(d, 0, ref.CHUNK_SIZE, 0, 0, 0)
            walked.append((idx, cigar))
        except ref.RefAbort as e:
            aborting[abort_class(str(e))].append((idx, cigar))
    return walked, aborting


def evenly(items, count=PER_CLASS):
    return [items[i * (len(items) - 1) // (count - 1)] for i in range(count)]


def cigars(directory) -> List[Case]:
    walked, aborting = classify_cigars()
    path = write(directory, "cigars", [read("c%04d" % idx, 100 + SLOT * idx, cigar, idx) for idx, cigar in walked])
    out = [Case(case_name("cigars", "all", OPEN), (path, path), OPEN, CLEAN)]
    good = read("good", 10, [("M", 4)], 0)
    for cls in ABORT_CLASSES:
        for idx, cigar in evenly(aborting[cls]):
            p = write(directory, "cigar_%s" % cigar_text(cigar).replace("=", "E"),
                      [good, read("c%04d" % idx, 100, cigar, idx)])
            out.append(Case(case_name("cigars", cls.replace(" ", "_") + ":" + cigar_text(cigar), OPEN), (p,), OPEN,
                            UNDEFINED if cls == QUALITY_INDEX else ABORT))
    return out


# ------------------------------------------------------------------------------------------------------------
# wrap

WRAP_K = (0, 1, 2, 5)
WRAP_PARAMS = ((100, 0, 0, 0, 0), (100, 0, 0, 0, 3), (100, 0, 0, 0, 4), (3, 0, 0, 0, 0))
WRAP_POS = 5000


def wrap_bam(path, n_reads: int) -> str:
    """n_reads one-base reads (1M, base ACGT[i % 4], quality 40, named w<i>) at WRAP_POS, built with numpy as
    bw.uniform_cell_bam builds its records."""
    dt = np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("lname", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                   ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<u4"), ("nref", "<i4"), ("npos", "<i4"),
                   ("tlen", "<i4"), ("name", "S7"), ("cig", "<u4"), ("seq", "u1"), ("qual", "u1")])
    rec = np.zeros(n_reads, dtype=dt)
    i = np.arange(n_reads)
    rec["bs"] = dt.itemsize - 4
    rec["pos"] = WRAP_POS
    rec["lname"] = 7
    rec["mapq"] = 60
    rec["bin"] = bw.reg2bin(WRAP_POS, WRAP_POS + 1)
    rec["ncig"] = 1
    rec["flag"] = FLAG
    rec["lseq"] = 1
    rec["nref"] = -1
    rec["npos"] = -1
    rec["name"] = np.char.encode(np.char.add("w", np.char.zfill(i.astype(str), 5)))  # 6 characters and the NUL
    rec["cig"] = 1 << 4
    rec["seq"] = bw.BASE_CODE[i % 4] << 4
    rec["qual"] = 40
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:1\tLN:3000000\n"
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + \
        struct.pack("<i", 2) + b"1\0" + struct.pack("<i", 3_000_000) + rec.tobytes()
    with open(path, "wb") as f:
        f.write(bw.bgzf(raw))
    return path


def wrap(directory, ks=WRAP_K) -> List[Case]:
    out = []
    for k in ks:
        path = wrap_bam(os.path.join(str(directory), "wrap_%d.bam" % k), 65536 + k)
        bai_writer.write_bai(path)
        out.extend(Case(case_name("wrap", "k%d" % k, p), (path,), p, CLEAN) for p in WRAP_PARAMS)
    return out


# ------------------------------------------------------------------------------------------------------------
# quality

QUALITY_Q = (0, 1, 19, 20, 21, 93, 94, 95, 100, 222, 223, 254)
QUALITY_MIN = (0, 1, 20, 21, 94, 95, 96, 200)  # past 95 only the signed compare lets q >= 95 through


def quality_records(q_values=QUALITY_Q, odd_ones=True) -> List[bw.Rec]:
    recs = [read("q%03d" % q, 100 + 10 * k, [("M", 3)], k, qual=[q, 40, q]) for k, q in enumerate(q_values)]
    if odd_ones:
        k = len(q_values)
        recs.append(read("qff00", 100 + 10 * k, [("M", 3)], k, qual=[255, 0, 0]))
        recs.append(read("qnone", 110 + 10 * k, [("M", 3)], k + 1, qual=None))
    return recs


def quality(directory) -> List[Case]:
    path = write(directory, "quality", quality_records())
    return [Case(case_name("quality", "all", p), (path, path), p, CLEAN)
            for p in ((100, q, 0, 0, 0) for q in QUALITY_MIN)]


# ------------------------------------------------------------------------------------------------------------
# window

WINDOW_PARAMS = (OPEN, (100, 35, 0, 0, 1))


def window_records(cell: int) -> List[bw.Rec]:
    """Twelve 20M3D10M reads stepping by 5 from 2^24 - 30, one 30M read at 2^24 - 1 and one at 2^24, and two 30M reads
    whose last bases lie at 2^24 - 1 and at 2^24: the last and the first position of a window. Cell 1 differs from cell
    0 in every second base."""
    def rd(name, pos, cigar, idx):
        n = seq_len(cigar)
        return read(name, pos, cigar, idx, seq="".join("ACGT"[(idx + k + cell * (k % 2)) % 4] for k in range(n)))
    recs = [rd("win%02d" % i, WINDOW - 30 + 5 * i, [("M", 20), ("D", 3), ("M", 10)], i) for i in range(12)]
    recs.append(rd("below", WINDOW - 1, [("M", 30)], 12))
    recs.append(rd("at", WINDOW, [("M", 30)], 13))
    recs.append(rd("ends_below", WINDOW - 30, [("M", 30)], 14))
    recs.append(rd("ends_at", WINDOW - 29, [("M", 30)], 15))
    return recs


def window(directory) -> List[Case]:
    files = tuple(write(directory, "window_%d" % c, window_records(c), ref_len=30_000_000) for c in (0, 1))
    return [Case(case_name("window", "two_cells", p), files, p, CLEAN) for p in WINDOW_PARAMS]


# ------------------------------------------------------------------------------------------------------------
# chunks

def chunks(directory) -> List[Case]:
    good = read("good", 10, [("M", 4)], 0)
    edge = write(directory, "chunk_edge", [read("edge", 999_990, [("M", 30)], 1)])
    nxt = write(directory, "chunk_next", [read("next", 1_000_100, [("M", 4)], 2)])
    # the last base of a read at 999,000 with a reference length of 2,000 lies 999 past the chunk's end
    fine = write(directory, "chunk_999", [good, read("far", 999_000, [("M", 10), ("D", 1980), ("M", 10)], 3)])
    far = write(directory, "chunk_1000", [good, read("far", 999_000, [("M", 10), ("D", 1981), ("M", 10)], 3, mapq=5)])
    mq = (100, 0, 6, 0, 0)
    return [Case(case_name("chunks", "cut_off", OPEN), (edge, edge), OPEN, CLEAN),
            Case(case_name("chunks", "carried_over", OPEN), (edge, edge, nxt), OPEN, CLEAN),
            Case(case_name("chunks", "999_past", OPEN), (fine, fine, nxt), OPEN, CLEAN),
            Case(case_name("chunks", "1000_past", OPEN), (far, far, nxt), OPEN, ABORT),
            Case(case_name("chunks", "1000_past_low_mapq", mq), (far, far, nxt), mq, CLEAN)]


# ------------------------------------------------------------------------------------------------------------
# thresholds

THRESHOLD_PARAMS = ((6, 0, 0, 0, 0), (100, 0, 0, 0, 2), (100, 0, 10, 0, 0), (100, 0, 0, 50, 0), (6, 0, 10, 50, 2),
                    (7, 0, 9, 49, 1))


def thresholds(directory) -> List[Case]:
    """Eight cells of one-base reads. At max_coverage 6, min_different 2, min_map_quality 10, min_alignment_score 50:
    position -> (cell: base [, mapq, AS])"""
    loci = {
        1000: "ACGTA",  # coverage max_coverage - 1
        1010: "ACGTAC",  # coverage max_coverage
        1020: "A",  # coverage 1
        1030: "AC",  # coverage 2
        1040: "AAAAC",  # coverage - max(count) = min_different - 1
        1050: "AAACC",  # coverage - max(count) = min_different
        1060: "ACGTACG",  # coverage max_coverage + 1
        1070: "ACGTACGT",  # every cell
    }
    per_cell = [[] for _ in range(8)]
    for pos, bases in loci.items():
        for c, b in enumerate(bases):
            per_cell[c].append(read("t%d_%d" % (c, pos), pos, [("M", 1)], 0, seq=b, tags=[("AS", "C", 60)]))
    for c in range(5):  # 1080: mapq at and one below min_map_quality; 1090: AS at and one below min_alignment_score
        per_cell[c].append(read("t%d_1080" % c, 1080, [("M", 1)], c, mapq=9 + c % 2, tags=[("AS", "C", 60)]))
        per_cell[c].append(read("t%d_1090" % c, 1090, [("M", 1)], c, tags=[("AS", "C", 49 + c % 2)]))
    files = tuple(write(directory, "thr_%d" % c, recs) for c, recs in enumerate(per_cell))
    return [Case(case_name("thresholds", "eight_cells", p), files, p, CLEAN) for p in THRESHOLD_PARAMS]


# ------------------------------------------------------------------------------------------------------------
# tags

def _t(tag, typ, value) -> bytes:
    return bw._tag(tag, typ, value)


TAG_LAYOUTS = (
    ("AS_A", _t("AS", "A", "2")),  # the character '2' is 50
    ("AS_C50", _t("AS", "C", 50)),
    ("AS_C49", _t("AS", "C", 49)),
    ("AS_S50", _t("AS", "S", 50)),
    ("AS_I50", _t("AS", "I", 50)),
    ("AS_s", _t("AS", "s", 50)),
    ("AS_i", _t("AS", "i", 50)),
    ("AS_c", _t("AS", "c", 50)),
    ("B_then_AS", _t("XB", "B", ("s", [1, 2, 3])) + _t("AS", "C", 50)),
    ("H_then_AS", _t("XH", "H", "AB") + _t("AS", "C", 50)),
    ("AS_c_then_AS_C", _t("AS", "c", 60) + _t("AS", "C", 60)),
    ("empty_Z_then_AS", _t("XZ", "Z", "") + _t("AS", "C", 50)),
    ("f_then_AS_S300", _t("XF", "f", 1.5) + _t("AS", "S", 300)),
    ("no_aux", b""),
    ("AS_last_bytes", _t("NM", "C", 1) + _t("AS", "I", 50)),
    ("cut_aux", _t("XX", "C", 1) + b"AS"),  # parsed + 3 > len at the second field
    ("no_AS", _t("NM", "C", 1) + _t("XS", "Z", "x")),  # the walk ends where the next field would start
    ("unknown_type_then_AS", b"XQq\x01" + _t("AS", "C", 60)),  # FindTag gives up at a type it does not know
    ("NUL_then_AS", _t("XX", "C", 1) + b"\0" + _t("AS", "C", 60)),  # a NUL where the next field would start
)
TAG_MIN_AS = (0, 50, 51)


def tag_records(layouts=TAG_LAYOUTS) -> List[bw.Rec]:
    return [read("tag_" + name, 100 + 10 * k, [("M", 3)], k, aux=aux) for k, (name, aux) in enumerate(layouts)]


def tags(directory) -> List[Case]:
    path = write(directory, "tags", tag_records())
    return [Case(case_name("tags", "all", p), (path, path), p, CLEAN) for p in ((100, 0, 0, a, 0) for a in TAG_MIN_AS)]


# ------------------------------------------------------------------------------------------------------------
# seq

def seq_records() -> List[bw.Rec]:
    codes = bw.SEQ_CODES + "A"  # all sixteen 4-bit codes, odd length
    return [read("codes", 100, [("M", len(codes))], 0, seq=codes, qual=[40] * len(codes)),
            read("one", 200, [("M", 1)], 1),
            read("star", 300, [("M", 5)], 2, seq="*", qual=[])]


def seq(directory) -> List[Case]:
    path = write(directory, "seq", seq_records())
    return [Case(case_name("seq", "all", OPEN), (path, path), OPEN, CLEAN)]


# ------------------------------------------------------------------------------------------------------------
# slots

SLOTS_PARAMS = (110, 0, 0, 0, 0)


def slots(directory) -> List[Case]:
    """102 files: files 0 and 100, and 1 and 101, share a read-name map (MAX_OPEN_FILES = 100)."""
    files = []
    for f in range(102):
        files.append(write(directory, "slot_%03d" % f, [
            read("shared", 100, [("M", 8)], 0, seq="ACGTACGT"),
            read("own%d" % f, 104, [("M", 8)], 0, seq="CCGTACGT" if f % 2 else "ACGTACGT")], ref_len=1000))
    return [Case(case_name("slots", "102_files", SLOTS_PARAMS), tuple(files), SLOTS_PARAMS, CLEAN)]


BUILDERS = dict(cigars=cigars, wrap=wrap, quality=quality, window=window, chunks=chunks, thresholds=thresholds,
                tags=tags, seq=seq, slots=slots)


def build(family: str, directory, **kw) -> List[Case]:
    d = os.path.join(str(directory), family)
    os.makedirs(d, exist_ok=True)
    return BUILDERS[family](d, **kw)


def build_all(directory) -> List[Case]:
    return [c for f in FAMILIES for c in build(f, directory)]


# ------------------------------------------------------------------------------------------------------------
# running a case: the restatement, the compiled reference, and what is recorded of either

REF_PILEUP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_pileup")
ABORT_STATUS = 134  # 128 + SIGABRT, what a shell reports for a failed assert


def have_reference() -> bool:
    return os.access(REF_PILEUP, os.X_OK)


def run_reference(case: Case, out: str, timeout: float = 120) -> int:
    """oracle/_ref/ref_pileup on the case -> its exit status (128 + the signal when one ended it); <out>.bin, .map
    and .txt are what it wrote."""
    import subprocess
    r = subprocess.run([REF_PILEUP, out, "0"] + [str(p) for p in case.params] + list(case.files),
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout)
    return r.returncode if r.returncode >= 0 else 128 - r.returncode


def run_restatement(case: Case) -> ref.Pileup:
    return ref.pileup_bams(list(case.files), 0, *case.params)


def txt_upto16(text: str) -> str:
    return "".join(l + "\n" for l in text.splitlines() if int(l.split("\t")[2]) <= 16)


def summary(bin_bytes: bytes, map_bytes: bytes, txt_text: str) -> dict:
    """What tests/golden/pileup_edges.npz keeps of a clean run."""
    import hashlib
    n_loci = n_entries = o = 0
    while o < len(bin_bytes):
        cov = struct.unpack_from("<H", bin_bytes, o + 4)[0]
        o += 6 + 6 * cov
        n_loci += 1
        n_entries += cov
    return dict(bin_sha=hashlib.sha256(bin_bytes).hexdigest(), map_sha=hashlib.sha256(map_bytes).hexdigest(),
                n_loci=n_loci, n_entries=n_entries, txt=txt_upto16(txt_text))


def summary_of_files(out: str) -> dict:
    return summary(open(out + ".bin", "rb").read(), open(out + ".map", "rb").read(), open(out + ".txt").read())


def summary_of_restatement(p: ref.Pileup) -> dict:
    return summary(p.bin_bytes(), p.map_text().encode(), p.txt_text())


@contextlib.contextmanager
def cached_records():
    """Within the block the restatement decodes each (file, chromosome) once: for files that are written once."""
    plain = ref.chromosome_records
    ref.chromosome_records = functools.lru_cache(maxsize=None)(plain)
    try:
        yield
    finally:
        ref.chromosome_records = plain
